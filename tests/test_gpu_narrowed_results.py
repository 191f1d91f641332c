"""MI355X tests for ``narrow_tensor_results`` end to end through a loopback worker, just above a
lowered staging threshold: what narrows, to which width, what travels whole, what is retained."""

import asyncio
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

STAGING = 256 << 10
N = STAGING // 4 + 64  # float32 elements just above the threshold, int64 well above


def _make_electrons():
    """Local functions, so cloudpickle ships them by value."""

    def produce(kind, n):
        import torch

        i = torch.arange(n, device="cuda")
        if kind == "logits":  # a bf16 matmul upcast at the end
            a = (i % 13 - 6).to(torch.bfloat16).reshape(-1, 8) / 3
            out = (a @ a[:8].t()).float().reshape(-1)
        elif kind == "thirds":
            out = i.float() / 3
        else:  # ids below int(kind)
            out = i * 7919 % int(kind)
        # what left the GPU, for a bitwise comparison on the other side
        return {"out": out, "bytes": out.cpu().numpy().tobytes()}

    def consume(value):
        return value["out"].is_cuda

    return produce, consume


_produce, _consume = _make_electrons()


def _make_executor(tmp_path, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor

    options = dict(
        transport="local", local_home=str(tmp_path), cache_dir=str(tmp_path / "cache"),
        python_path=sys.executable, gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True, device_tensor_args=True, narrow_tensor_results=True,
        pinned_staging_threshold_bytes=STAGING, hip_visible_devices_policy="fixed", fixed_gpu=0,
    )
    return SSHExecutor(**{**options, **overrides})


def _run(ex, kind, take=False):
    async def run():
        try:
            value = await ex.execute(_produce, [kind, N], {}, dispatch_id="n", node_id=1)
            meta = ex.last_task_record.remote_meta
            meta_b = None
            if take:
                await ex.execute(_consume, [value], {}, dispatch_id="n", node_id=2)
                meta_b = ex.last_task_record.remote_meta
            return value, meta, meta_b
        finally:
            await ex.close_pool()

    return asyncio.run(run())


@pytest.mark.parametrize("kind, dtype, wire, ratio", [
    ("logits", torch.float32, "bfloat16", 2), ("256", torch.int64, "uint8", 8),
    ("32768", torch.int64, "int16", 4), ("70000", torch.int64, "int32", 2),
])
def test_an_exact_result_arrives_bit_equal_at_a_fraction_of_the_bytes(tmp_path, kind, dtype,
                                                                       wire, ratio):
    value, meta, _ = _run(_make_executor(tmp_path), kind)
    out = value["out"]
    assert out.dtype == dtype and out.shape == (N,) and not out.is_cuda
    assert out.numpy().tobytes() == value["bytes"]
    (info,) = meta["buffers"]
    assert info["wire"] == wire and info["dtype"] == str(dtype).replace("torch.", "")
    staging, nbytes = meta["staging"], N * out.element_size()
    assert staging["narrowed"] == 1 and staging["narrow_saved_bytes"] == nbytes - nbytes // ratio
    assert "narrow_fallback" not in staging and meta["result_integrity"]["verified"] == 1


@pytest.mark.parametrize("on", [True, False])
def test_an_inexact_result_and_the_option_off_travel_whole(tmp_path, on):
    value, meta, _ = _run(_make_executor(tmp_path, narrow_tensor_results=on),
                          "thirds" if on else "logits")
    assert value["out"].numpy().tobytes() == value["bytes"]
    assert meta["buffers"] == [{"dtype": "float32", "shape": [N]}]
    assert "narrowed" not in meta["staging"] and meta["staging"]["pinned_tensors"] == 1
    assert ("not exact as bfloat16" in meta["staging"].get("narrow_fallback", "")) is on


def test_a_retained_result_keeps_its_full_bytes_and_is_a_hit_later(tmp_path):
    ex = _make_executor(tmp_path, cache_tensor_args=True, arg_cache_min_bytes=200_000,
                        arg_cache_bytes=64 << 20, retain_tensor_results=True)
    value, meta, meta_b = _run(ex, "logits", take=True)
    (info,) = meta["buffers"]
    assert value["out"].numpy().tobytes() == value["bytes"] and "wire" not in info
    assert info["retained"] == meta["retained"]["stored"][0]
    hits = meta_b["arg_cache"]["hits"]
    assert "narrowed" not in meta["staging"] and hits == [info["retained"]]


def test_a_corrupted_narrow_frame_fails_its_integrity_check(tmp_path, monkeypatch):
    from covalent_ssh_plugin_amd.transport import native_io

    real = native_io.checksum  # the two sums swapped: what a damaged frame would give
    monkeypatch.setattr(native_io, "checksum", lambda *a, **k: tuple(reversed(real(*a, **k))))
    with pytest.raises(RuntimeError, match="result buffer 0 failed its integrity check"):
        _run(_make_executor(tmp_path), "256")
