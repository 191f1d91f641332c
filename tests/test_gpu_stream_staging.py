"""MI355X tests for the streaming result path: csp_d2h_stream_fd on its
own (ring wrap, odd sizes, unaligned source, reader gone mid-frame) and
end to end through the worker's deferred CUDA buffers and the channel's
native large-frame receive."""

import asyncio
import os
import struct
import sys
import threading
import time

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CHUNK = 64 * 1024  # tiny, so the two-chunk ring wraps on tiny data
SIZES = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17, 3 * CHUNK]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests require a visible MI355X (torch.cuda unavailable)")


@pytest.fixture(scope="module")
def probe():
    from covalent_ssh_plugin_amd.gpu import probe as gpu_probe

    gpu_probe.load()  # GpuLibError if the extension was not built/shipped
    return gpu_probe


@pytest.fixture(scope="module")
def source():
    """Seeded random bytes on the GPU plus their host copy, shared by every
    case (3 bytes of slack in front for the unaligned case)."""
    gen = torch.Generator().manual_seed(20240607)
    host = torch.randint(0, 256, (3 + max(SIZES),), dtype=torch.uint8, generator=gen)
    dev = host.cuda()
    torch.cuda.synchronize()
    return dev, dev.cpu().numpy().tobytes()


def _stream_through_pipe(probe, ptr, nbytes, chunk):
    """Run csp_d2h_stream_fd into an os.pipe drained by a thread; returns
    (call report, everything the reader got)."""
    r, w = os.pipe()
    got = bytearray()

    def drain():
        while True:
            piece = os.read(r, 1 << 16)
            if not piece:
                return
            got.extend(piece)

    t = threading.Thread(target=drain)
    t.start()
    try:
        report = probe.stream_d2h_to_fd(w, ptr, nbytes, chunk)
    finally:
        os.close(w)
        t.join()
        os.close(r)
    return report, bytes(got)


@pytest.mark.parametrize("offset", [0, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("nbytes", SIZES)
def test_stream_frame_is_exact(probe, source, nbytes, offset):
    dev, host = source
    report, got = _stream_through_pipe(probe, dev.data_ptr() + offset, nbytes, CHUNK)
    assert report["rc"] == probe.STREAM_OK, report
    assert got[:8] == struct.pack(">Q", nbytes)
    assert len(got) == 8 + nbytes
    assert got[8:] == host[offset : offset + nbytes]


def test_stream_default_chunk(probe, source):
    dev, host = source
    n = len(host)
    report, got = _stream_through_pipe(probe, dev.data_ptr(), n, 0)
    assert report["rc"] == probe.STREAM_OK, report
    assert got == struct.pack(">Q", n) + host


def test_reader_gone_mid_frame_then_clean_call(probe, source):
    """A host-side pipe error: the reader takes the header and the first
    chunk, then closes.  The call must come back promptly with the
    mid-frame code, and the next call must work (ring returned clean)."""
    dev, host = source
    nbytes = 3 * CHUNK  # more than the 64 KiB pipe can swallow
    r, w = os.pipe()

    def take_first_chunk_and_leave():
        want = 8 + CHUNK
        while want:
            piece = os.read(r, want)
            if not piece:
                break
            want -= len(piece)
        os.close(r)

    t = threading.Thread(target=take_first_chunk_and_leave)
    t.start()
    t0 = time.monotonic()
    try:
        report = probe.stream_d2h_to_fd(w, dev.data_ptr(), nbytes, CHUNK)
    finally:
        os.close(w)
        t.join()
    assert time.monotonic() - t0 < 5.0
    assert report["rc"] == probe.STREAM_FAILED_MID_FRAME, report

    report, got = _stream_through_pipe(probe, dev.data_ptr(), 2 * CHUNK + 17, CHUNK)
    assert report["rc"] == probe.STREAM_OK, report
    assert got == struct.pack(">Q", 2 * CHUNK + 17) + host[: 2 * CHUNK + 17]


def test_closed_fd_fails_before_header(probe, source):
    dev, _host = source
    r, w = os.pipe()
    os.close(r)
    os.close(w)
    report = probe.stream_d2h_to_fd(w, dev.data_ptr(), CHUNK, CHUNK)
    assert report["rc"] == probe.STREAM_FAILED_BEFORE_HEADER, report


# -- end to end ------------------------------------------------------------

BIG_CUDA_BYTES = (3 << 20) + 10  # bf16: an odd number of 2-byte elements' worth


def _electron_pair():
    """(payload, electron), both local functions so cloudpickle ships them
    by value.  ``payload(seed)`` is what the electron returns, built on
    the CPU from a seed so the test can build the same thing."""
    big_cuda_elems = BIG_CUDA_BYTES // 2

    def payload(seed):
        import torch

        gen = torch.Generator().manual_seed(seed)
        return {
            "big_cuda": torch.randn(big_cuda_elems, generator=gen).to(torch.bfloat16),
            "small_cuda": torch.randn(1000, generator=gen),
            "big_cpu": torch.randn((2 << 20) // 4 + 3, generator=gen),
            "seed": seed,
        }

    def electron(seed, make):
        out = make(seed)
        out["big_cuda"] = out["big_cuda"].cuda()
        out["small_cuda"] = out["small_cuda"].cuda()
        return out

    return payload, electron


def _make_executor(kind, tmp_path, sshim, monkeypatch):
    from covalent_ssh_plugin_amd import SSHExecutor

    common = dict(
        cache_dir=str(tmp_path / "cache"),
        python_path=sys.executable,
        gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True,
        # one slot, so both electrons meet the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
        pinned_staging_threshold_bytes=1 << 20,
    )
    if kind == "local":
        home = tmp_path / "home"
        home.mkdir()
        return SSHExecutor(transport="local", local_home=str(home), **common)
    monkeypatch.setenv(
        "SSHIM_PASS_ENV",
        "HSA_ENABLE_IPC_MODE_LEGACY,LD_LIBRARY_PATH,HIP_VISIBLE_DEVICES,"
        "ROCR_VISIBLE_DEVICES,PYTORCH_ROCM_ARCH,TMPDIR",
    )
    return SSHExecutor(
        transport="ssh", hostname=sshim.hostname, username="mi355x",
        ssh_key_file=str(sshim.key), **common,
    )


@pytest.mark.parametrize("kind", ["local", "sshim"])
def test_end_to_end_streamed_result(kind, tmp_path, sshim, monkeypatch):
    from covalent_ssh_plugin_amd.transport import native_io
    from covalent_ssh_plugin_amd.transport.channel import Channel

    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    # 1 MiB on both sides: the worker streams the big CUDA tensor, and the
    # dispatcher takes both out-of-band frames through the native receive
    monkeypatch.setattr(Channel, "large_frame_threshold", 1 << 20)
    ex = _make_executor(kind, tmp_path, sshim, monkeypatch)
    _payload, _electron = _electron_pair()

    async def run():
        first = await ex.execute(_electron, [11, _payload], {}, dispatch_id="s", node_id=0)
        meta1 = ex.last_task_record.remote_meta
        # same worker again: the stream must still be aligned
        second = await ex.execute(_electron, [12, _payload], {}, dispatch_id="s", node_id=1)
        meta2 = ex.last_task_record.remote_meta
        await ex.close_pool()
        return first, meta1, second, meta2

    first, meta1, second, meta2 = asyncio.run(run())
    for out, meta, seed in ((first, meta1, 11), (second, meta2, 12)):
        want = _payload(seed)
        assert set(out) == set(want)
        assert out["seed"] == seed
        for key in ("big_cuda", "small_cuda", "big_cpu"):
            assert not out[key].is_cuda
            assert out[key].dtype == want[key].dtype
            assert torch.equal(out[key], want[key]), key
        assert out["big_cuda"].numel() * 2 == BIG_CUDA_BYTES
        assert meta["staging"]["mode"] == "pinned", meta
        assert meta["staging"]["pinned_tensors"] == 1, meta
        assert len(meta["buffers"]) == 2, meta
    assert meta1["pid"] == meta2["pid"], "second electron ran on another worker"
    assert meta2["served"] == meta1["served"] + 1
