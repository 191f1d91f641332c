"""MI355X tests for ``narrow_tensor_args`` end to end through a loopback worker, just above a
lowered staging threshold: what narrows, to which width, what travels whole, what the cache does."""

import asyncio
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

STAGING = 256 << 10
N = STAGING // 4 + 63  # float32 elements just above the threshold, no multiple of a vector


def _make_electron():
    """A local function, so cloudpickle ships it by value."""

    def echo(t):
        # what arrived on the GPU, for a bitwise comparison on the other side
        return {"cuda": t.is_cuda, "dtype": str(t.dtype), "shape": list(t.shape),
                "bytes": t.cpu().numpy().tobytes()}

    return echo


_echo = _make_electron()


def _tensor(kind):
    i = torch.arange(N)
    if kind == "bf16":
        return ((i % 251 - 125).float() / 8).to(torch.bfloat16).float()
    if kind == "f32":
        return (i.float() / 3).double()
    if kind == "thirds":
        return i.float() / 3
    return i * 7919 % int(kind) - (5 if int(kind) > 256 else 0)  # int64 ids


def _make_executor(tmp_path, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor

    options = dict(
        transport="local", local_home=str(tmp_path), cache_dir=str(tmp_path / "cache"),
        python_path=sys.executable, gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True, device_tensor_args=True, narrow_tensor_args=True,
        pinned_staging_threshold_bytes=STAGING, hip_visible_devices_policy="fixed", fixed_gpu=0,
    )
    return SSHExecutor(**{**options, **overrides})


def _run(ex, tensors):
    """One electron per tensor on one worker; [(what it saw, the worker's meta)]."""

    async def run():
        try:
            out = []
            for node, t in enumerate(tensors):
                seen = await ex.execute(_echo, [t], {}, dispatch_id="a", node_id=node)
                out.append((seen, ex.last_task_record.remote_meta))
            return out
        finally:
            await ex.close_pool()

    return asyncio.run(run())


def _same(seen, t):
    return (seen["cuda"] and seen["dtype"] == str(t.dtype) and seen["shape"] == list(t.shape)
            and seen["bytes"] == t.numpy().tobytes())


@pytest.mark.parametrize("isolate", [False, True])
@pytest.mark.parametrize("kind, size", [("256", 1), ("32768", 2), ("70000", 4), ("bf16", 2),
                                        ("f32", 4)])
def test_an_exact_argument_arrives_bit_equal_from_a_fraction_of_the_bytes(tmp_path, kind, size,
                                                                          isolate):
    t = _tensor(kind)
    ex = _make_executor(tmp_path, **({"isolate_tasks": True} if isolate else {}))
    ((seen, meta),) = _run(ex, [t])
    stage = meta["arg_staging"]
    assert _same(seen, t) and stage["verified"] == 1
    assert stage["widened"] == 1 and stage["wire_bytes"] == N * size and stage["widen_ms"] > 0
    assert ex.counters["arg_narrowed"] == 1
    assert ex.counters["arg_narrow_saved_bytes"] == N * (t.element_size() - size)


@pytest.mark.parametrize("on", [True, False])
def test_an_inexact_argument_and_the_option_off_travel_whole(tmp_path, on):
    t = _tensor("thirds" if on else "bf16")
    ex = _make_executor(tmp_path, narrow_tensor_args=on)
    ((seen, meta),) = _run(ex, [t])
    assert _same(seen, t)
    assert meta["arg_staging"] == {**meta["arg_staging"], "mode": "pinned-h2d", "tensors": 1,
                                   "bytes": 4 * N, "verified": 1}
    assert set(meta["arg_staging"]) == {"mode", "tensors", "bytes", "verified", "read_ms", "h2d_ms"}
    assert ex.counters["arg_narrowed"] == 0 and (ex.counters["arg_narrow_ms"] > 0) is on


def test_the_cache_stores_narrow_hits_without_narrowing_and_resends_narrow_once(tmp_path):
    a, b = _tensor("256"), _tensor("32768")
    ex = _make_executor(tmp_path, cache_tensor_args=True, arg_cache_min_bytes=STAGING,
                        arg_cache_bytes=8 * N + 4096)  # room for one master
    (s1, m1), (s2, m2), (s3, m3), (s4, m4) = _run(ex, [a, a, b, a])
    assert all(_same(s, t) for s, t in ((s1, a), (s2, a), (s3, b), (s4, a)))
    key_a, key_b = m1["arg_cache"]["stored"][0], m3["arg_cache"]["stored"][0]
    # a store that arrives narrow: the master and the private tensor from one launch
    assert m1["arg_staging"]["widened"] == 1 and m1["arg_staging"]["wire_bytes"] == N
    # the hit: nothing travels, nothing is narrowed, the copy is private
    assert m2["arg_cache"]["hits"] == [key_a] and "widened" not in m2["arg_staging"]
    assert m2["arg_staging"]["mode"] == "cached"
    # b evicts a; a again is a miss and travels narrow exactly once more
    assert m3["arg_cache"]["evicted"] == [key_a] and m3["arg_staging"]["wire_bytes"] == 2 * N
    assert m4["arg_cache"].get("resent") and m4["arg_cache"]["stored"] == [key_a]
    assert m4["arg_cache"]["evicted"] == [key_b] and m4["arg_staging"]["widened"] == 1
    assert ex.counters["arg_narrowed"] == 3 and ex.counters["arg_cache_hits"] == 1


def test_a_corrupted_narrow_frame_fails_its_integrity_check_and_leaves_no_master(tmp_path,
                                                                                  monkeypatch):
    from covalent_ssh_plugin_amd.remote import workers

    real = workers.narrow_arg

    def damaged(*args, **kwargs):
        wire, data = real(*args, **kwargs)
        data[len(data) // 2] ^= 0x04  # one bit of one narrow element
        return wire, data

    monkeypatch.setattr(workers, "narrow_arg", damaged)
    ex = _make_executor(tmp_path, cache_tensor_args=True, arg_cache_min_bytes=STAGING,
                        arg_cache_bytes=64 << 20)

    async def run():
        try:
            with pytest.raises(RuntimeError, match="argument buffer 0 failed its integrity check"):
                await ex.execute(_echo, [_tensor("32768")], {}, dispatch_id="a", node_id=0)
            return ex.last_task_record.remote_meta
        finally:
            await ex.close_pool()

    meta = asyncio.run(run())
    assert meta["arg_cache"]["stored"] == [] and meta["arg_cache"]["entries"] == 0
