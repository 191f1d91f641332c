"""MI355X tests for bool tensors as ``"bits"`` end to end through a loopback worker, under
``narrow_tensor_results`` and ``narrow_tensor_args``, just above the staging threshold."""

import asyncio
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

OPTIONS = dict(pinned_staging_threshold_bytes=256 << 10)


def _n(ex):
    """The smallest odd bool tensor on the large-tensor path, read from the executor's gate."""
    return int(ex.pinned_staging_threshold_bytes) + 61


def _make_electrons():
    """Local functions, so cloudpickle ships them by value."""

    def produce(kind, n):
        import torch

        out = torch.rand(n, device="cuda") > 0.5
        if kind == "poisoned":  # a uint8 tensor viewed as bool, one byte of 2
            out = out.view(torch.uint8)
            out[n // 2] = 2
            out = out.view(torch.bool)
        # what left the GPU, for a bitwise comparison on the other side
        return {"out": out, "bytes": out.view(torch.uint8).cpu().numpy().tobytes()}

    def echo(t):
        import torch

        return {"cuda": t.is_cuda, "dtype": str(t.dtype), "shape": list(t.shape),
                "bytes": t.view(torch.uint8).cpu().numpy().tobytes()}

    return produce, echo


_produce, _echo = _make_electrons()


def _make_executor(tmp_path, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor

    options = dict(
        transport="local", local_home=str(tmp_path), cache_dir=str(tmp_path / "cache"),
        python_path=sys.executable, gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True, device_tensor_args=True, narrow_tensor_results=True,
        narrow_tensor_args=True, hip_visible_devices_policy="fixed", fixed_gpu=0, **OPTIONS,
    )
    return SSHExecutor(**{**options, **overrides})


def _run(ex, function, arg_lists):
    """One electron per argument list on one worker; [(its value, the worker's meta)]."""

    async def run():
        try:
            out = []
            for node, args in enumerate(arg_lists):
                value = await ex.execute(function, args, {}, dispatch_id="b", node_id=node)
                out.append((value, ex.last_task_record.remote_meta))
            return out
        finally:
            await ex.close_pool()

    return asyncio.run(run())


def _mask(n):
    mask = torch.arange(n) * 7919 % 5 < 2
    mask[0] = mask[-1] = True
    return mask


def _same(seen, t):
    return (seen["cuda"] and seen["dtype"] == "torch.bool" and seen["shape"] == list(t.shape)
            and seen["bytes"] == t.view(torch.uint8).numpy().tobytes())


def test_a_bool_result_arrives_bit_equal_as_an_eighth_of_the_bytes(tmp_path):
    ex = _make_executor(tmp_path)
    n = _n(ex)
    ((value, meta),) = _run(ex, _produce, [["random", n]])
    out = value["out"]
    assert out.dtype == torch.bool and out.shape == (n,) and not out.is_cuda
    assert out.view(torch.uint8).numpy().tobytes() == value["bytes"]
    (info,) = meta["buffers"]
    assert info["wire"] == "bits" and info["dtype"] == "bool"
    staging = meta["staging"]
    assert staging["narrowed"] == 1 and staging["narrow_saved_bytes"] == n - (n + 7) // 8
    assert "narrow_fallback" not in staging and meta["result_integrity"]["verified"] == 1


@pytest.mark.parametrize("kind, on", [("poisoned", True), ("random", False)])
def test_a_poisoned_bool_result_and_the_option_off_travel_whole(tmp_path, kind, on):
    ex = _make_executor(tmp_path, narrow_tensor_results=on)
    n = _n(ex)
    ((value, meta),) = _run(ex, _produce, [[kind, n]])
    assert value["out"].view(torch.uint8).numpy().tobytes() == value["bytes"]
    assert meta["buffers"] == [{"dtype": "bool", "shape": [n]}]
    assert "narrowed" not in meta["staging"] and meta["staging"]["pinned_tensors"] == 1
    assert ("not exact as bits" in meta["staging"].get("narrow_fallback", "")) is on


@pytest.mark.parametrize("isolate", [False, True])
def test_a_bool_argument_is_unpacked_on_the_gpu_from_its_bits(tmp_path, isolate):
    ex = _make_executor(tmp_path, **({"isolate_tasks": True} if isolate else {}))
    t = _mask(_n(ex))
    ((seen, meta),) = _run(ex, _echo, [[t]])
    stage = meta["arg_staging"]
    assert _same(seen, t) and stage["verified"] == 1
    assert stage["widened"] == 1 and stage["wire_bytes"] == (t.numel() + 7) // 8
    assert ex.counters["arg_narrowed"] == 1


def test_the_cache_stores_a_bool_argument_from_bits_and_hits_without_a_frame(tmp_path):
    ex = _make_executor(tmp_path, cache_tensor_args=True, arg_cache_bytes=64 << 20,
                        arg_cache_min_bytes=OPTIONS["pinned_staging_threshold_bytes"])
    t = _mask(_n(ex))
    (s1, m1), (s2, m2) = _run(ex, _echo, [[t], [t]])
    assert _same(s1, t) and _same(s2, t)
    # the store arrives as bits: the master and the private tensor from one launch
    assert m1["arg_staging"]["widened"] == 1
    assert m1["arg_staging"]["wire_bytes"] == (t.numel() + 7) // 8
    assert m2["arg_cache"]["hits"] == m1["arg_cache"]["stored"]
    assert "widened" not in m2["arg_staging"] and m2["arg_staging"]["mode"] == "cached"


def test_a_corrupted_frame_of_bits_fails_its_integrity_check(tmp_path, monkeypatch):
    from covalent_ssh_plugin_amd.remote import workers

    real = workers.narrow_arg

    def damaged(*args, **kwargs):
        wire, data = real(*args, **kwargs)
        data[len(data) // 2] ^= 0x04  # one element
        return wire, data

    monkeypatch.setattr(workers, "narrow_arg", damaged)
    ex = _make_executor(tmp_path)
    with pytest.raises(RuntimeError, match="argument buffer 0 failed its integrity check"):
        _run(ex, _echo, [[_mask(_n(ex))]])
