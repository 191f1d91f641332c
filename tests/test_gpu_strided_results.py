"""MI355X tests for ``gather_tensor_results`` end to end through a loopback
worker: a transposed CUDA result laid out by csp_gather_checksum_dev, retained
and on the pinned path, and a tensor the kernel refuses.  The thresholds are
low so that 3 MiB and 512 KiB tensors count as large."""

import asyncio
import hashlib
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

STAGING = 256 << 10
CACHE_MIN = 200_000
NBYTES = 1024 * 768 * 4


def _make_electrons():
    """Local functions, so cloudpickle ships them by value."""

    def source(kind):
        import torch

        gen = torch.Generator().manual_seed(11)
        if kind == "transpose":
            return torch.randn(1024, 768, generator=gen)
        return torch.randn(32, 32, 16, 16, 16, generator=gen)

    def view_of(x, kind):
        return x.t() if kind == "transpose" else x[::2, ::2, ::2, ::2, ::2]

    def produce(kind):
        out = view_of(source(kind).cuda(), kind)
        assert not out.is_contiguous()
        return out

    def consume(value):
        import hashlib

        data = value.cpu().numpy().tobytes()
        return {"cuda": value.is_cuda, "digest": hashlib.blake2b(data, digest_size=16).hexdigest()}

    return source, view_of, produce, consume


_source, _view_of, _produce, _consume = _make_electrons()


def _make_executor(tmp_path, retain, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor

    home = tmp_path / "home"
    home.mkdir()
    options = dict(
        transport="local",
        local_home=str(home),
        cache_dir=str(tmp_path / "cache"),
        python_path=sys.executable,
        gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True,
        device_tensor_args=True,
        cache_tensor_args=retain,
        arg_cache_min_bytes=CACHE_MIN,
        arg_cache_bytes=64 << 20,
        retain_tensor_results=retain,
        gather_tensor_results=True,
        pinned_staging_threshold_bytes=STAGING,
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
    )
    options.update(overrides)
    return SSHExecutor(**options)


def _run_chain(ex, kind, take=False):
    async def run():
        value = await ex.execute(_produce, [kind], {}, dispatch_id="s", node_id=1)
        meta = ex.last_task_record.remote_meta
        out = None
        if take:
            out = await ex.execute(_consume, [value], {}, dispatch_id="s", node_id=2)
            out = (out, ex.last_task_record.remote_meta, dict(ex.counters))
        await ex.close_pool()
        return value, meta, out

    return asyncio.run(run())


def test_retained_transpose_is_gathered_verified_and_a_hit_later(tmp_path):
    ex = _make_executor(tmp_path, retain=True)
    value, meta, (out, meta_b, counters) = _run_chain(ex, "transpose", take=True)
    want = _view_of(_source("transpose"), "transpose")
    assert not value.is_cuda and value.shape == (768, 1024) and torch.equal(value, want)
    staging = meta["staging"]
    assert staging["gathered_tensors"] == 1 and staging["gathered_bytes"] == NBYTES
    assert "gather_fallback" not in staging and "retain_fallback" not in staging
    assert meta["result_integrity"]["verified"] >= 1
    (info,) = meta["buffers"]
    assert info["retained"] == meta["retained"]["stored"][0] and len(info["sum"]) == 2
    digest = hashlib.blake2b(want.contiguous().numpy().tobytes(), digest_size=16).hexdigest()
    assert out["cuda"] is True and out["digest"] == digest
    assert meta_b["arg_cache"]["hits"] == [info["retained"]]
    assert counters["arg_cache_hits"] == 1 and counters["arg_cache_bytes_saved"] == NBYTES


@pytest.mark.parametrize("retain, gather", [(False, True), (True, False)])
def test_the_large_pinned_path_and_the_option_off(tmp_path, retain, gather):
    ex = _make_executor(tmp_path, retain=retain, gather_tensor_results=gather)
    value, meta, _ = _run_chain(ex, "transpose")
    assert torch.equal(value, _view_of(_source("transpose"), "transpose"))
    staging = meta["staging"]
    assert staging["pinned_tensors"] == 1 and "gather_fallback" not in staging
    if gather:  # one buffer filled by the gather, streamed, and no sum attached
        assert staging["gathered_tensors"] == 1 and staging["gathered_bytes"] == NBYTES
        assert meta["buffers"] == [{"dtype": "float32", "shape": [768, 1024]}]
    else:
        assert "gathered_tensors" not in staging and staging["retained_buffers"] == 1


@pytest.mark.parametrize("retain", [True, False])
def test_a_refused_tensor_falls_back_to_contiguous(tmp_path, retain):
    ex = _make_executor(tmp_path, retain=retain)
    value, meta, _ = _run_chain(ex, "five")
    assert torch.equal(value, _view_of(_source("five"), "five"))
    staging = meta["staging"]
    assert "5 dimensions are left" in staging["gather_fallback"]
    assert "gathered_tensors" not in staging and staging["pinned_tensors"] == 1
    assert ("retained" in meta["buffers"][0]) is retain
