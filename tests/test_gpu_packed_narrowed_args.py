"""MI355X tests for ``pack_tensor_args`` with ``narrow_tensor_args`` end to end through a loopback
worker with a lowered staging threshold: what narrows inside the arena, what the cache holds."""

import asyncio
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

STAGING = 64 << 10  # every tensor below is smaller: all of them share the arena
CACHE_MIN = 16 << 10  # above every tensor, below the arena
N = 1001


def _make_electron():
    """A local function, so cloudpickle ships it by value."""

    def echo(state):
        # what arrived on the GPU, for a bitwise comparison on the other side
        return {k: (t.is_cuda, str(t.dtype), list(t.shape), t.cpu().numpy().tobytes())
                for k, t in state.items()}

    return echo


_echo = _make_electron()


def _state():
    """int64 ids that take uint8, int16 and int32, a bf16-valued and an inexact float32, bytes."""
    i = torch.arange(N)
    return {"u8": i % 256, "i16": i * 61 - 30000, "i32": i * 70001 - 9,
            "bf16": (i % 251 - 125).float() / 8, "thirds": i.float() / 3,
            "bytes": torch.arange(77, dtype=torch.uint8)}


ROWS = [(N, "uint8", "int64"), (N, "int16", "int64"), (N, "int32", "int64"),
        (N, "bfloat16", "float32"), (4 * N, "", ""), (77, "", "")]


def _narrow_total():
    from covalent_ssh_plugin_amd.gpu.probe import unpack_widen_layout

    return unpack_widen_layout(ROWS)[1]


def _make_executor(tmp_path, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor

    options = dict(
        transport="local", local_home=str(tmp_path), cache_dir=str(tmp_path / "cache"),
        python_path=sys.executable, gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True, device_tensor_args=True, narrow_tensor_args=True,
        pack_tensor_args=True, pack_args_min_bytes=0, pinned_staging_threshold_bytes=STAGING,
        hip_visible_devices_policy="fixed", fixed_gpu=0,
    )
    return SSHExecutor(**{**options, **overrides})


def _run(ex, states, error=None):
    """One electron per state on one worker; [(what it saw, the worker's meta)]."""

    async def run():
        try:
            out = []
            for node, state in enumerate(states):
                if error:
                    with pytest.raises(RuntimeError, match=error):
                        await ex.execute(_echo, [state], {}, dispatch_id="a", node_id=node)
                    seen = None
                else:
                    seen = await ex.execute(_echo, [state], {}, dispatch_id="a", node_id=node)
                out.append((seen, ex.last_task_record.remote_meta))
            return out
        finally:
            await ex.close_pool()

    return asyncio.run(run())


def _same(seen, state):
    return seen == {k: (True, str(t.dtype), list(t.shape), t.numpy().tobytes())
                    for k, t in state.items()}


@pytest.mark.parametrize("isolate", [False, True])
def test_a_mixed_dict_arrives_bit_equal_from_the_narrow_arena(tmp_path, isolate):
    state = _state()
    ex = _make_executor(tmp_path, **({"isolate_tasks": True} if isolate else {}))
    ((seen, meta),) = _run(ex, [state])
    stage = meta["arg_staging"]
    assert _same(seen, state) and stage["verified"] == 1 and stage["packed_tensors"] == 6
    assert stage["widened"] == 4 and stage["wire_bytes"] == _narrow_total()
    assert stage["widen_ms"] > 0 and ex.counters["arg_narrowed"] == 4
    wide = sum((t.numel() * t.element_size() + 15) // 16 * 16 for t in state.values())
    assert stage["bytes"] == wide == stage["wire_bytes"] + ex.counters["arg_narrow_saved_bytes"]


def test_a_store_arrives_narrow_then_hits_and_patches_find_the_wide_master(tmp_path):
    state = _state()
    changed = dict(state, i16=state["i16"] + 1)
    ex = _make_executor(tmp_path, cache_tensor_args=True, arg_cache_min_bytes=CACHE_MIN,
                        arg_cache_bytes=64 << 20, patch_tensor_args=True)
    (s1, m1), (s2, m2), (s3, m3) = _run(ex, [state, state, changed])
    assert _same(s1, state) and _same(s2, state) and _same(s3, changed)
    (key_a,), (key_b,) = m1["arg_cache"]["stored"], m3["arg_cache"]["stored"]
    assert m1["arg_staging"]["widened"] == 4 and m1["arg_staging"]["wire_bytes"] == _narrow_total()
    # the hit: nothing travels, nothing is narrowed or widened
    assert m2["arg_cache"]["hits"] == [key_a] and "widened" not in m2["arg_staging"]
    assert m2["arg_staging"]["mode"] == "cached" and ex.counters["arg_narrowed"] == 4
    # one changed tensor travels wide as a patch of the master that arrived narrow
    assert m3["arg_cache"]["patched"] == [[key_a, key_b]] and "widened" not in m3["arg_staging"]
    assert m3["arg_staging"]["patched_bytes"] == 8 * N + 8


def test_a_corrupted_narrow_frame_fails_its_integrity_check_and_leaves_no_master(tmp_path,
                                                                                  monkeypatch):
    from covalent_ssh_plugin_amd.remote import workers

    real = workers.narrow_arg

    def damaged(view, dtype, **kwargs):
        got = real(view, dtype, **kwargs)
        if got is not None and got[0] == "int16":
            got[1][len(got[1]) // 2] ^= 0x04  # one bit of one narrow element
        return got

    monkeypatch.setattr(workers, "narrow_arg", damaged)
    ex = _make_executor(tmp_path, cache_tensor_args=True, arg_cache_min_bytes=CACHE_MIN,
                        arg_cache_bytes=64 << 20)
    ((_, meta),) = _run(ex, [_state()], error="argument buffer 0 failed its integrity check")
    assert meta["arg_cache"]["stored"] == [] and meta["arg_cache"]["entries"] == 0


def test_with_the_option_off_the_entry_is_unchanged(tmp_path):
    state = _state()
    ex = _make_executor(tmp_path, narrow_tensor_args=False)
    ((seen, meta),) = _run(ex, [state])
    assert _same(seen, state) and ex.counters["arg_narrowed"] == 0
    assert not {"widened", "wire_bytes", "widen_ms"} & set(meta["arg_staging"])
    assert meta["arg_staging"]["unpack_ms"] >= 0 and meta["arg_staging"]["packed_tensors"] == 6
