"""MI355X tests for ``narrow_tensor_results`` inside the packed result arena, end to end through a
loopback worker: a dict of small tensors just below the staging threshold, each at the narrowest
exact width, filled and summed by csp_pack_narrow_checksum_dev."""

import asyncio
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

STAGING = 256 << 10
N = 20000  # 160 000 bytes as int64: every tensor is below the threshold
WIRES = {"logits": "bfloat16", "bytes": "uint8", "ids": "int16"}
WIDE = {"thirds": "float32", "half": "float16", "empty": "float32"}


def _make_electrons():
    """Local functions, so cloudpickle ships them by value."""

    def build(device, transposed=False):
        import torch

        i = torch.arange(N, device=device)
        out = {
            "logits": (i % 251 - 125).to(torch.bfloat16).float() / 4,
            "bytes": i * 7919 % 200,
            "ids": i * 7919 % 30000 - 100,
            "thirds": (torch.arange(N).float() / 3).to(device),  # divided on the CPU both times
            "half": (i % 1024).to(torch.float16),
            "empty": torch.empty(0, 3, device=device),
        }
        if transposed:
            out["t"] = out["bytes"].reshape(100, 200).t()
        return out

    def produce(transposed=False):
        return build("cuda", transposed)

    def consume(value):
        return all(v.is_cuda for v in value.values())

    return build, produce, consume


_build, _produce, _consume = _make_electrons()


def _run(tmp_path, take=False, transposed=False, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor

    options = dict(
        transport="local", local_home=str(tmp_path), cache_dir=str(tmp_path / "cache"),
        python_path=sys.executable, gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True, pack_tensor_results=True, pack_results_min_bytes=4096,
        narrow_tensor_results=True, pinned_staging_threshold_bytes=STAGING,
        hip_visible_devices_policy="fixed", fixed_gpu=0,
    )
    ex = SSHExecutor(**{**options, **overrides})

    async def run():
        try:
            value = await ex.execute(_produce, [transposed], {}, dispatch_id="p", node_id=1)
            meta, meta_b = ex.last_task_record.remote_meta, None
            if take:
                await ex.execute(_consume, [value], {}, dispatch_id="p", node_id=2)
                meta_b = ex.last_task_record.remote_meta
            return value, meta, meta_b
        finally:
            await ex.close_pool()

    value, meta, meta_b = asyncio.run(run())
    want = _build("cpu", transposed)  # integer and exactly rounded arithmetic: the GPU's bits
    assert list(value) == list(want)
    for key, w in want.items():
        assert value[key].dtype == w.dtype and value[key].shape == w.shape, key
        assert torch.equal(value[key], w), key
    return want, meta, meta_b


def test_a_mixed_dict_travels_at_the_narrow_widths(tmp_path):
    want, meta, _ = _run(tmp_path)
    (info,) = meta["buffers"]
    entries = dict(zip(want, info["packed"]))
    assert {k: e.get("wire") for k, e in entries.items()} == {**WIRES, **dict.fromkeys(WIDE)}
    sizes = {k: v.numel() * (torch.empty(0, dtype=getattr(torch, WIRES[k])).element_size()
                             if k in WIRES else v.element_size()) for k, v in want.items()}
    assert {k: e["nbytes"] for k, e in entries.items()} == sizes
    assert info["nbytes"] == sum((n + 15) // 16 * 16 for n in sizes.values())
    staging = meta["staging"]
    wide = sum(v.numel() * v.element_size() for v in want.values())
    assert staging["narrowed"] == 3 and staging["narrow_saved_bytes"] == wide - sum(sizes.values())
    assert "narrow_fallback" not in staging and "pack_fallback" not in staging
    assert meta["result_integrity"]["verified"] == 1


def test_the_option_off_leaves_the_meta_as_it_is(tmp_path):
    want, meta, _ = _run(tmp_path, narrow_tensor_results=False)
    (info,) = meta["buffers"]
    assert sorted(info) == ["nbytes", "packed", "sum"]
    assert all(sorted(e) == ["dtype", "nbytes", "offset", "shape"] for e in info["packed"])
    assert [e["nbytes"] for e in info["packed"]] == [
        v.numel() * v.element_size() for v in want.values()]
    assert "narrowed" not in meta["staging"] and "narrow_ms" not in meta["staging"]


def test_a_retained_arena_keeps_its_full_bytes_and_is_a_hit_later(tmp_path):
    _, meta, meta_b = _run(
        tmp_path, take=True, device_tensor_args=True, pack_tensor_args=True,
        pack_args_min_bytes=0, cache_tensor_args=True, arg_cache_bytes=64 << 20,
        arg_cache_min_bytes=STAGING, retain_tensor_results=True,
    )
    (info,) = meta["buffers"]
    assert not any("wire" in e for e in info["packed"]) and "narrowed" not in meta["staging"]
    assert meta_b["arg_cache"]["hits"] == [info["retained"]]


def test_an_arena_with_a_strided_tensor_is_not_narrowed(tmp_path):
    _, meta, _ = _run(tmp_path, transposed=True, gather_tensor_results=True)
    (info,) = meta["buffers"]
    assert not any("wire" in e for e in info["packed"]) and "narrowed" not in meta["staging"]
    assert meta["staging"]["gathered_tensors"] == 1


def test_a_corrupted_narrow_arena_fails_its_integrity_check(tmp_path, monkeypatch):
    from covalent_ssh_plugin_amd.transport import native_io

    real = native_io.checksum  # the two sums swapped: what a damaged frame would give
    monkeypatch.setattr(native_io, "checksum", lambda *a, **k: tuple(reversed(real(*a, **k))))
    with pytest.raises(RuntimeError, match="result buffer 0 failed its integrity check"):
        _run(tmp_path)
