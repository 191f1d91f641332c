"""MI355X: ``delta_tensor_results`` end to end, each argument a store and then a hit."""

import asyncio
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

B = 4096
NBYTES = 2 << 20
CASES = {  # name: (executor options, what the electron changes, changed blocks or None = whole)
    "row": ({}, "row", 1),
    "nothing": ({}, "none", 0),
    "everything": ({}, "all", None),  # beyond the cap of half the blocks
    "packed-state-dict": ({}, "dict", 64),
    "retained": ({"retain_tensor_results": True}, "row", 1),
    "flipped-byte": ({}, "row", 1),
    "option-off": ({"delta_tensor_results": False}, "row", None),
}


def _electron():  # a local function, so cloudpickle ships it by value
    def touch(state, how):
        if how == "row":
            state["w3"][7] += 1  # one block
        elif how != "none":
            state["w3"] += 1  # the large tensor, or one 256 KiB tensor of eight
        return state

    return touch


_touch = _electron()


@pytest.mark.parametrize("case", CASES)
def test_delta_results_end_to_end(tmp_path, monkeypatch, case):
    from covalent_ssh_plugin_amd import SSHExecutor
    from covalent_ssh_plugin_amd.remote import workers as worker_pool
    from covalent_ssh_plugin_amd.transport import native_io
    from covalent_ssh_plugin_amd.transport.channel import Channel

    assert torch.cuda.is_available() and native_io.load() is not None, "no MI355X or libcsp_io.so"
    monkeypatch.setattr(Channel, "large_frame_threshold", 1 << 20)
    options, how, changed = CASES[case]
    ex = SSHExecutor(**{
        **dict(transport="local", local_home=str(tmp_path), cache_dir=str(tmp_path / "cache"),
               python_path=sys.executable, gpu_slots=1, persistent_workers=True,
               device_tensor_args=True, cache_tensor_args=True, arg_cache_min_bytes=1_100_000, arg_cache_bytes=64 << 20,
               pack_tensor_results=True, pack_results_min_bytes=0, pack_tensor_args=True,
               pack_args_min_bytes=0, delta_tensor_results=True, fixed_gpu=0,
               pinned_staging_threshold_bytes=3 << 19, hip_visible_devices_policy="fixed"),
        **options,
    })
    gen = torch.Generator().manual_seed(5)
    if how == "dict":  # small tensors: one packed arena each way
        state = {"w%d" % i: torch.randn(256, 256, generator=gen) for i in range(8)}
    else:
        state = {"w3": torch.randn(NBYTES // B, B // 4, generator=gen)}
    want = _touch({k: v.clone() for k, v in state.items()}, how)
    real = worker_pool.apply_result_delta

    def flipped(info, frame, base_view):
        frame = bytearray(frame)
        frame[100] ^= 0x20  # inside the one changed block, on the way
        return real(info, frame, base_view)

    async def run():
        rounds = []
        if case == "flipped-byte":
            with monkeypatch.context() as patch:
                patch.setattr(worker_pool, "apply_result_delta", flipped)
                with pytest.raises(RuntimeError, match="result buffer 0, rebuilt from a delta "
                                   "against argument 0, failed its integrity check"):
                    await ex.execute(_touch, [state, how], {}, dispatch_id="d", node_id=0)
        sends = [(state, how), (state, how)]  # the argument is a store, then a hit
        for node, args in enumerate(sends, 1):
            value = await ex.execute(_touch, list(args), {}, dispatch_id="d", node_id=node)
            rounds.append((value, ex.last_task_record.remote_meta))
            if case == "retained" and node == 2:
                sends.append((value, "none"))  # the retained result as the next argument
        await ex.close_pool()
        return rounds

    rounds = asyncio.run(run())
    for i, (value, meta) in enumerate(rounds):
        (info,), staging = meta["buffers"], meta["staging"]
        assert all(torch.equal(value[k], want[k]) for k in want) and len(value) == len(want)
        assert "delta_fallback" not in staging, staging
        if case == "option-off":
            assert "delta" not in info and not any(k.startswith("delta") for k in staging)
            continue
        assert len(info["sum"]) == 2 and meta["result_integrity"]["verified"] == 1
        count = 0 if i == 2 else changed  # the third round hands back what it got
        if count is None:
            assert "delta" not in info and staging["delta_buffers"] == 0
            continue
        assert info["delta"] == {"arg": 0, "block": B, "changed": count, "nbytes": NBYTES}
        assert staging["delta_buffers"] == 1 and staging["delta_full_bytes"] == NBYTES
        assert staging["delta_bytes"] == count * (B + 4) and staging["delta_ms"] >= 0.0
    assert len(rounds[1][1]["arg_cache"]["hits"]) == 1, "the second argument was not a hit"
    assert rounds[1][1]["served"] == (3 if case == "flipped-byte" else 2), "worker replaced"
    # the corrupted frame was rebuilt, and counted, before its checksum failed
    assert ex.counters["result_deltas"] == (
        0 if changed is None else len(rounds) + (case == "flipped-byte"))
    assert case != "packed-state-dict" or len(rounds[0][1]["buffers"][0]["packed"]) == 8
    if case == "retained":
        name = rounds[1][1]["buffers"][0]["retained"]
        assert rounds[2][1]["arg_cache"]["hits"] == [name]  # and no argument byte travelled
        assert rounds[2][1]["arg_staging"]["bytes"] == 0
