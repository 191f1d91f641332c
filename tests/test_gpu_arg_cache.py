"""MI355X tests for ``cache_tensor_args``: csp_copy_checksum_dev on its own
(exact copy, guard bytes, the checksum against numpy and csp_checksum_dev,
refused calls), and the argument cache end to end through a loopback
persistent worker: store then hit, private copies, one master for two views,
eviction with its single resend, a wrong checksum on a reference, the size
threshold, and a fresh worker that knows nothing."""

import asyncio
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

# the shipped grid is at most 1024 blocks of 256 lanes, 16 bytes a lane and
# four vectors a trip: 16 MiB.  The last size takes one such trip, then the
# one-vector loop, then the byte tail.
ONE_TRIP = 1024 * 256 * 16 * 4
SIZES = [0, 1, 3, 4, 15, 16, 17, 65535, 256 * 16 * 3 + 5, ONE_TRIP + 256 * 16 * 3 + 7]
SRC_OFF, DST_OFF = 16, 48
GUARD = 64


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
    """Seeded random bytes at offset SRC_OFF of a larger device buffer, with
    their host copy; shared by every case and never written to."""
    gen = torch.Generator().manual_seed(20241103)
    host = torch.randint(0, 256, (SRC_OFF + max(SIZES) + GUARD,), dtype=torch.uint8, generator=gen)
    dev = host.cuda()
    torch.cuda.synchronize()
    return dev, host.numpy()


def reference(data: bytes):
    """(s0, s1) as the protocol defines them: pad to 4 bytes, view as
    little-endian u32, widen to u64, wrapping sums."""
    words = np.frombuffer(data + b"\0" * (-len(data) % 4), dtype="<u4").astype(np.uint64)
    weight = (np.arange(len(words), dtype=np.uint64) % np.uint64(1 << 32)) + np.uint64(1)
    with np.errstate(over="ignore"):
        return (
            int(words.sum(dtype=np.uint64)),
            int((words * weight).sum(dtype=np.uint64)),
        )


def _guarded(nbytes):
    """nbytes of destination at DST_OFF inside a buffer of 0xA5."""
    buf = torch.full((DST_OFF + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf


# -- csp_copy_checksum_dev ---------------------------------------------------


@pytest.mark.parametrize("n", SIZES)
def test_copy_is_exact_and_sum_matches(probe, source, n):
    dev, host = source
    want = host[SRC_OFF : SRC_OFF + n].tobytes()
    buf = _guarded(n)
    src_ptr = dev.data_ptr() + SRC_OFF
    dst_ptr = buf.data_ptr() + DST_OFF
    assert src_ptr % 16 == 0 and dst_ptr % 16 == 0
    got = probe.copy_checksum_device(dst_ptr, src_ptr, n)
    after = buf.cpu().numpy()
    assert after[DST_OFF : DST_OFF + n].tobytes() == want
    assert after[:DST_OFF].tobytes() == b"\xa5" * DST_OFF, "wrote before the destination"
    assert after[DST_OFF + n :].tobytes() == b"\xa5" * GUARD, "wrote past the destination"
    assert got == reference(want)
    assert got == probe.checksum_device(src_ptr, n)
    if n == max(SIZES):
        assert np.array_equal(dev.cpu().numpy(), host), "the source changed"


def test_source_is_unchanged_by_the_small_sizes(probe, source):
    """After the cases above (whatever their order, this is idempotent): one
    more copy, then the whole source buffer against its host copy."""
    dev, host = source
    buf = _guarded(65535)
    probe.copy_checksum_device(buf.data_ptr() + DST_OFF, dev.data_ptr() + SRC_OFF, 65535)
    assert np.array_equal(dev[: SRC_OFF + 65535 + GUARD].cpu().numpy(),
                          host[: SRC_OFF + 65535 + GUARD])


@pytest.mark.parametrize("which", ["src", "dst"])
def test_misaligned_pointer_is_refused(probe, source, which):
    dev, host = source
    buf = _guarded(1024)
    src_ptr = dev.data_ptr() + SRC_OFF + (4 if which == "src" else 0)
    dst_ptr = buf.data_ptr() + DST_OFF + (8 if which == "dst" else 0)
    with pytest.raises(probe.GpuLibError, match="16-byte aligned"):
        probe.copy_checksum_device(dst_ptr, src_ptr, 1024)
    assert buf.cpu().numpy().tobytes() == b"\xa5" * (DST_OFF + 1024 + GUARD)
    # nothing was launched, the library is fine
    want = host[SRC_OFF : SRC_OFF + 1024].tobytes()
    assert probe.copy_checksum_device(
        buf.data_ptr() + DST_OFF, dev.data_ptr() + SRC_OFF, 1024
    ) == reference(want)


@pytest.mark.parametrize("shift", [0, 16, 1008, -1008])
def test_overlapping_ranges_are_refused(probe, shift):
    n = 1024
    buf = torch.arange(4096, dtype=torch.int32, device="cuda").to(torch.uint8)
    torch.cuda.synchronize()
    before = buf.cpu().numpy().copy()
    src_ptr = buf.data_ptr() + 2048
    with pytest.raises(probe.GpuLibError, match="overlap"):
        probe.copy_checksum_device(src_ptr + shift, src_ptr, n)
    assert np.array_equal(buf.cpu().numpy(), before), "dst was touched"
    # ranges that only touch are fine
    probe.copy_checksum_device(src_ptr + n, src_ptr, n)
    after = buf.cpu().numpy()
    assert np.array_equal(after[2048 + n : 2048 + 2 * n], before[2048 : 2048 + n])


# -- end to end --------------------------------------------------------------

ELEMS = 16385  # float32: 65540 bytes, 4 more than a multiple of 16
NBYTES = ELEMS * 4


def _tensor(seed, elems=ELEMS):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(elems, generator=gen)


def _make_electron():
    """A local function, so cloudpickle ships it by value."""

    def electron(t, log=None, bump=False):
        import os

        if log is not None:
            with open(log, "a") as f:
                f.write("ran\n")
        seen = t.cpu().clone()
        if bump:
            t.add_(1)
        return {"cuda": t.is_cuda, "seen": seen, "pid": os.getpid()}

    return electron


_electron = _make_electron()


def _make_executor(tmp_path, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor
    from covalent_ssh_plugin_amd.transport import native_io

    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
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
        cache_tensor_args=True,
        arg_cache_min_bytes=4096,
        # one slot, so every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
    )
    options.update(overrides)
    return SSHExecutor(**options)


async def _send(ex, tensor, node, **kwargs):
    out = await ex.execute(_electron, [tensor], kwargs, dispatch_id="c", node_id=node)
    return out, ex.last_task_record.remote_meta


def _delivered(out, want):
    assert out["cuda"] is True
    assert out["seen"].dtype == want.dtype and out["seen"].shape == want.shape
    assert torch.equal(out["seen"], want)


def test_second_dispatch_of_equal_bytes_is_a_hit(tmp_path):
    ex = _make_executor(tmp_path)

    async def run():
        first = await _send(ex, _tensor(1), 0)
        second = await _send(ex, _tensor(1), 1)  # equal, another object
        await ex.close_pool()
        return first, second

    (out1, meta1), (out2, meta2) = asyncio.run(run())
    _delivered(out1, _tensor(1))
    _delivered(out2, _tensor(1))
    assert meta1["pid"] == meta2["pid"]
    assert meta1["arg_staging"]["bytes"] == NBYTES and meta1["arg_staging"]["mode"] == "pinned-h2d"
    assert len(meta1["arg_cache"]["stored"]) == 1 and meta1["arg_cache"]["hits"] == []
    assert meta1["arg_cache"]["entries"] == 1
    assert meta1["arg_cache"]["resident_bytes"] == NBYTES
    assert meta2["arg_staging"]["bytes"] == 0 and meta2["arg_staging"]["mode"] == "cached"
    assert meta2["arg_staging"]["verified"] == 1
    assert meta2["arg_cache"]["hits"] == meta1["arg_cache"]["stored"]
    assert meta2["arg_cache"]["stored"] == [] and meta2["arg_cache"]["miss"] == []
    assert ex.counters["arg_cache_hits"] == 1
    assert ex.counters["arg_cache_misses"] == 0
    assert ex.counters["arg_cache_bytes_saved"] == NBYTES


def test_electrons_get_private_copies(tmp_path):
    ex = _make_executor(tmp_path)

    async def run():
        a = await _send(ex, _tensor(2), 0, bump=True)  # store, then t.add_(1)
        b = await _send(ex, _tensor(2), 1, bump=True)  # hit, then t.add_(1)
        c = await _send(ex, _tensor(2), 2)
        await ex.close_pool()
        return a, b, c

    results = asyncio.run(run())
    for out, _meta in results:
        _delivered(out, _tensor(2))
    assert [len(meta["arg_cache"]["hits"]) for _out, meta in results] == [0, 1, 1]
    assert results[2][1]["arg_staging"]["bytes"] == 0
    assert ex.counters["arg_cache_hits"] == 2


def test_same_bytes_as_two_views_share_one_master(tmp_path):
    ex = _make_executor(tmp_path)
    as_float = _tensor(3, 4 * 4096).reshape(4, 4096)
    as_int = as_float.clone().view(torch.int32).reshape(16384)

    async def run():
        a = await _send(ex, as_float, 0)
        b = await _send(ex, as_int, 1)
        await ex.close_pool()
        return a, b

    (out_a, meta_a), (out_b, meta_b) = asyncio.run(run())
    _delivered(out_a, as_float)
    _delivered(out_b, as_int)
    assert len(meta_a["arg_cache"]["stored"]) == 1
    assert meta_b["arg_cache"]["hits"] == meta_a["arg_cache"]["stored"]
    assert meta_b["arg_cache"]["stored"] == [] and meta_b["arg_cache"]["entries"] == 1
    assert meta_b["arg_staging"]["bytes"] == 0


def test_eviction_costs_one_miss_and_one_resend(tmp_path):
    ex = _make_executor(tmp_path, arg_cache_bytes=3 * NBYTES)
    log = tmp_path / "ran.log"

    async def run():
        metas = []
        for node, seed in enumerate((10, 11, 12, 13)):  # A, B, C, D
            out, meta = await _send(ex, _tensor(seed), node)
            _delivered(out, _tensor(seed))
            metas.append(meta)
        out, meta = await _send(ex, _tensor(10), 4, log=str(log))  # A again
        await ex.close_pool()
        return metas, out, meta

    metas, out, meta = asyncio.run(run())
    keys = [m["arg_cache"]["stored"][0] for m in metas]
    assert len(set(keys)) == 4
    assert [m["arg_cache"]["evicted"] for m in metas] == [[], [], [], [keys[0]]]
    assert metas[3]["arg_cache"]["entries"] == 3
    _delivered(out, _tensor(10))
    # the reference missed; the reply here is the resend's: A stored again,
    # B (the least recently used by then) evicted for it
    assert ex.counters["arg_cache_misses"] == 1
    assert ex.counters["arg_cache_hits"] == 0
    assert meta["arg_cache"]["resent"] is True
    assert meta["arg_cache"]["stored"] == [keys[0]]
    assert meta["arg_cache"]["evicted"] == [keys[1]]
    assert meta["arg_cache"]["miss"] == []
    assert meta["arg_staging"]["bytes"] == NBYTES
    assert meta["served"] == metas[3]["served"] + 2, "not exactly one resend"
    assert log.read_text() == "ran\n", "the user function did not run exactly once"


def test_wrong_sum_on_a_reference(tmp_path, monkeypatch):
    from covalent_ssh_plugin_amd.transport import native_io

    ex = _make_executor(tmp_path)
    real = native_io.checksum

    def off_by_one(*args, **kwargs):
        s0, s1 = real(*args, **kwargs)
        return s0, (s1 + 1) % (1 << 64)

    async def run():
        _out, meta0 = await _send(ex, _tensor(20), 0)
        with monkeypatch.context() as patch:
            patch.setattr(native_io, "checksum", off_by_one)
            with pytest.raises(RuntimeError, match="integrity") as failure:
                await _send(ex, _tensor(20), 1)
        bad_meta = ex.last_task_record.remote_meta
        out, good_meta = await _send(ex, _tensor(20), 2)
        await ex.close_pool()
        return meta0, str(failure.value), bad_meta, out, good_meta

    meta0, message, bad_meta, out, good_meta = asyncio.run(run())
    assert "argument buffer 0" in message, message
    assert ex.counters["arg_cache_misses"] == 1
    assert bad_meta["arg_cache"]["resent"] is True
    assert bad_meta["arg_cache"]["stored"] == [] and bad_meta["arg_cache"]["entries"] == 0
    assert "user_fn" not in bad_meta["phases_ms"], "user code ran on unverified data"
    assert bad_meta["served"] == meta0["served"] + 2
    _delivered(out, _tensor(20))
    assert good_meta["pid"] == meta0["pid"] == bad_meta["pid"]
    # the bad reference cost the entry: this one stored it again
    assert good_meta["arg_cache"]["stored"] == meta0["arg_cache"]["stored"]
    assert good_meta["served"] == bad_meta["served"] + 1


def test_below_the_threshold_nothing_is_cached(tmp_path):
    from covalent_ssh_plugin_amd.remote import workers as worker_pool

    ex = _make_executor(tmp_path)
    small = _tensor(30, 1000)  # 4000 bytes, under arg_cache_min_bytes=4096

    async def run():
        a = await _send(ex, small, 0)
        b = await _send(ex, small, 1)
        residents = [set(h.resident) for h in worker_pool._workers.values()]
        await ex.close_pool()
        return a, b, residents

    (out_a, meta_a), (out_b, meta_b), residents = asyncio.run(run())
    _delivered(out_a, small)
    _delivered(out_b, small)
    for meta in (meta_a, meta_b):
        assert "arg_cache" not in meta
        assert meta["arg_staging"]["bytes"] == 4000
        assert meta["arg_staging"]["mode"] == "pinned-h2d"
    assert residents == [set()]
    assert ex.counters["arg_cache_hits"] == 0


def test_fresh_worker_starts_with_an_empty_cache(tmp_path):
    ex = _make_executor(tmp_path)

    def leave():
        import os

        os._exit(7)

    async def run():
        first = await _send(ex, _tensor(40), 0)
        with pytest.raises(Exception):  # the worker died under this task
            await ex.execute(leave, [], {}, dispatch_id="c", node_id=1)
        second = await _send(ex, _tensor(40), 2)
        await ex.close_pool()
        return first, second

    (out1, meta1), (out2, meta2) = asyncio.run(run())
    _delivered(out1, _tensor(40))
    _delivered(out2, _tensor(40))
    assert meta2["pid"] != meta1["pid"], "the worker was not replaced"
    assert meta2["arg_staging"]["bytes"] == NBYTES
    assert meta2["arg_cache"]["stored"] == meta1["arg_cache"]["stored"]
    assert meta2["arg_cache"]["miss"] == [] and "resent" not in meta2["arg_cache"]
    assert ex.counters["arg_cache_misses"] == 0
    assert ex.counters["arg_cache_hits"] == 0
