"""MI355X tests for the edges of the two checksum kernels that ordinary
sizes do not reach: the 2^32-word boundary where the weight of ``s1`` wraps
(16 GiB, against the closed form and against the host routine), and, through
the tools-only grid caps, every hand-off between the unrolled loop, the
single-vector loop and the byte tail on a few KiB."""

import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from checksum_closed_form import (  # noqa: E402
    BOUNDARY_BYTES,
    expected,
    sparse_mapping,
    vector_sentinels,
)

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_BYTE = 0xA5
SLICE = 1 << 30  # device comparisons go in slices of this many bytes

# -- the 2^32-word boundary ---------------------------------------------------

N_BIG = BOUNDARY_BYTES + 7  # 16 GiB + 64 KiB and a 7-byte end: two tail words

# -- loop edges through grid caps ----------------------------------------------

CAPS = [1, 2, 3]  # blocks: strides of 256, 512 and 768 vectors
TAILS = [0, 1, 3, 4, 15]
UNROLL = 4  # kChecksumUnroll


def edge_vector_counts(stride):
    """n16 at which 0, 1, 2 or 3 strides remain after the unrolled loop, one
    less and one more than each, and more than one unrolled trip."""
    return [
        0, 1, stride - 1, stride, stride + 1, 3 * stride, 4 * stride - 1, 4 * stride,
        4 * stride + 1, 5 * stride, 6 * stride + 5, 7 * stride + stride - 1, 8 * stride,
        9 * stride + 1,
    ]


MAX_EDGE_BYTES = 16 * max(edge_vector_counts(256 * max(CAPS))) + max(TAILS)
# the shipped grid (1024 blocks of 256 lanes) enters the unrolled loop once
# more than three strides of vectors exist: 12 MiB.  Here 769 lanes take one
# unrolled trip, every lane then takes single-vector trips, then 5 tail bytes.
UNROLLED_AT_DEFAULT = (12 << 20) + 16 * (3 * 256 + 1) + 5


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests require a visible MI355X (torch.cuda unavailable)")


@pytest.fixture(scope="module")
def probe():
    from covalent_ssh_plugin_amd.gpu import probe as gpu_probe

    gpu_probe.load()  # GpuLibError if the extension was not built/shipped
    return gpu_probe


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


# -- the 2^32-word boundary ---------------------------------------------------


@pytest.fixture(scope="module")
def big(probe):
    """One source of N_BIG bytes and one guarded destination (GUARD bytes of
    0xA5 on each side of a 16-byte aligned payload), both only ever on the
    device: about 32 GiB of HBM, given back when the module ends."""
    bufs = {}
    try:
        bufs["src"] = torch.empty(N_BIG, dtype=torch.uint8, device="cuda")
        bufs["dst"] = torch.empty(GUARD + N_BIG + GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
    except RuntimeError as err:  # torch.OutOfMemoryError is one
        bufs.clear()
        torch.cuda.empty_cache()
        pytest.fail(
            f"could not allocate 2 x {N_BIG} bytes of HBM for the 2^32-word boundary "
            f"tests: {probe.mem_info()} ({err})"
        )
    assert bufs["src"].data_ptr() % 16 == 0 and (bufs["dst"].data_ptr() + GUARD) % 16 == 0
    yield bufs
    bufs.clear()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def host_sparse_pair():
    """``native_io.checksum`` of the sparse pattern's content, from a private
    mapping of zeros on the host: the pair the dispatcher would send."""
    from covalent_ssh_plugin_amd.transport import native_io

    assert native_io.load() is not None, "libcsp_io.so was not built"
    buf = sparse_mapping(N_BIG, vector_sentinels(N_BIG))
    pair = native_io.checksum(buf)
    gc.collect()
    try:
        buf.close()
    except BufferError:
        pass
    return pair


def _write_sparse(dev, sparse):
    """Write ``{offset: byte}`` into the device buffer, one small copy per
    run of adjacent offsets."""
    offsets = sorted(sparse)
    start = 0
    for k in range(1, len(offsets) + 1):
        if k == len(offsets) or offsets[k] != offsets[k - 1] + 1:
            run = offsets[start:k]
            values = torch.tensor([sparse[o] for o in run], dtype=torch.uint8)
            dev[run[0] : run[-1] + 1].copy_(values)
            start = k


def _first_difference(a, b):
    """Offset of the first byte at which two equally long device buffers
    differ, or None; compared in slices so the temporary stays small."""
    for lo in range(0, a.numel(), SLICE):
        hi = min(lo + SLICE, a.numel())
        if not torch.equal(a[lo:hi], b[lo:hi]):
            return lo + int((a[lo:hi] != b[lo:hi]).nonzero()[0])
    return None


def _all_equal_to(buf, byte):
    for lo in range(0, buf.numel(), SLICE):
        if not bool((buf[lo : lo + SLICE] == byte).all()):
            return False
    return True


@pytest.mark.parametrize("pattern", ["dense", "sparse"])
def test_both_kernels_wrap_at_2_to_32_words(probe, big, host_sparse_pair, pattern):
    """dense: every byte 0xFF, so s0 itself wraps modulo 2^64, every product
    is as large as it gets and a vector counted twice or not at all shifts
    the pair.  sparse: zeros with sentinels in every word position of the
    two vectors at the boundary, which pins the wrap to the exact word."""
    src, dst = big["src"], big["dst"]
    if pattern == "dense":
        src.fill_(0xFF)
        want = expected(N_BIG, 0xFF)
    else:
        sparse = vector_sentinels(N_BIG)
        src.zero_()
        _write_sparse(src, sparse)
        want = expected(N_BIG, 0x00, sparse)
    dst.fill_(GUARD_BYTE)
    torch.cuda.synchronize()
    payload = dst[GUARD : GUARD + N_BIG]

    got = probe.checksum_device(src.data_ptr(), N_BIG)
    print(f"{pattern}: csp_checksum_dev {got}, closed form {want}")
    assert got == want, "csp_checksum_dev against the closed form"

    copied = probe.copy_checksum_device(payload.data_ptr(), src.data_ptr(), N_BIG)
    print(f"{pattern}: csp_copy_checksum_dev {copied}")
    assert copied == want, "csp_copy_checksum_dev against the closed form"

    assert _first_difference(payload, src) is None, "the copy differs from the source"
    assert _all_equal_to(dst[:GUARD], GUARD_BYTE), "wrote before the destination"
    assert _all_equal_to(dst[GUARD + N_BIG :], GUARD_BYTE), "wrote past the destination"
    if pattern == "dense":
        assert _all_equal_to(src, 0xFF), "the source changed"
    else:
        print(f"sparse: native_io.checksum {host_sparse_pair}")
        assert got == host_sparse_pair, "device and host disagree on the same content"
        assert probe.checksum_device(payload.data_ptr(), N_BIG) == host_sparse_pair
        assert probe.checksum_device(src.data_ptr(), N_BIG) == want, "the source changed"


# -- loop edges through grid caps ----------------------------------------------


@pytest.fixture
def caps(probe):
    """Setter for both grid caps; the shipped defaults are back afterwards,
    whatever happened."""

    def set_caps(cap):
        assert probe.checksum_grid_cap(cap) == cap
        assert probe.copy_checksum_grid_cap(cap) == cap

    try:
        yield set_caps
    finally:
        assert probe.checksum_grid_cap(0) == 1024
        assert probe.copy_checksum_grid_cap(0) == 1024


@pytest.fixture(scope="module")
def edge_sources():
    """Seeded random bytes and all-0xFF bytes on the device, with the host
    copy of the former; shared and never written to."""
    gen = torch.Generator().manual_seed(20250117)
    host = torch.randint(0, 256, (MAX_EDGE_BYTES,), dtype=torch.uint8, generator=gen)
    dev = {"random": host.cuda(), "dense": torch.full_like(host, 0xFF).cuda()}
    pristine = {name: t.clone() for name, t in dev.items()}
    torch.cuda.synchronize()
    return dev, pristine, host.numpy().tobytes()


def _edge_cases():
    for cap in CAPS:
        for n16 in edge_vector_counts(256 * cap):
            for tail in TAILS:
                yield cap, n16, tail


def _want(pattern, host, nbytes):
    return reference(host[:nbytes]) if pattern == "random" else expected(nbytes, 0xFF)


def test_grid_caps_default_to_1024_blocks(probe, caps):
    caps(3)
    assert probe.checksum_grid_cap(0) == 1024
    assert probe.copy_checksum_grid_cap(0) == 1024


@pytest.mark.parametrize("pattern", ["random", "dense"])
def test_checksum_kernel_loop_edges(probe, caps, edge_sources, pattern):
    dev, pristine, host = edge_sources
    src = dev[pattern]
    failures = []
    for cap, n16, tail in _edge_cases():
        caps(cap)
        nbytes = 16 * n16 + tail
        got = probe.checksum_device(src.data_ptr(), nbytes)
        want = _want(pattern, host, nbytes)
        if got != want:
            failures.append(((cap, n16, tail), got, want))
    assert torch.equal(src, pristine[pattern]), "the source changed"
    assert not failures, f"{len(failures)} (cap, n16, tail) differ, first: {failures[0]}"


@pytest.mark.parametrize("pattern", ["random", "dense"])
def test_copy_checksum_kernel_loop_edges(probe, caps, edge_sources, pattern):
    dev, pristine, host = edge_sources
    src = dev[pattern]
    buf = torch.empty(GUARD + MAX_EDGE_BYTES + GUARD, dtype=torch.uint8, device="cuda")
    image = torch.empty_like(buf)  # what buf must hold after the call
    dst_ptr = buf.data_ptr() + GUARD
    assert src.data_ptr() % 16 == 0 and dst_ptr % 16 == 0
    failures = []
    for cap, n16, tail in _edge_cases():
        caps(cap)
        nbytes = 16 * n16 + tail
        buf.fill_(GUARD_BYTE)
        image.fill_(GUARD_BYTE)
        image[GUARD : GUARD + nbytes] = src[:nbytes]
        torch.cuda.synchronize()
        got = probe.copy_checksum_device(dst_ptr, src.data_ptr(), nbytes)
        want = _want(pattern, host, nbytes)
        if got != want:
            failures.append(((cap, n16, tail), "sums", got, want))
        elif not torch.equal(buf, image):
            at = int((buf != image).nonzero()[0]) - GUARD
            failures.append(((cap, n16, tail), f"first wrong byte at payload offset {at}"))
        elif not torch.equal(src, pristine[pattern]):
            failures.append(((cap, n16, tail), "the source changed"))
    assert not failures, f"{len(failures)} (cap, n16, tail) differ, first: {failures[0]}"


def test_checksum_kernel_unrolled_loop_at_the_default_cap(probe):
    assert probe.checksum_grid_cap(0) == 1024
    n = UNROLLED_AT_DEFAULT
    assert n // 16 > (UNROLL - 1) * 1024 * 256  # some lane passes the unrolled loop's test
    gen = torch.Generator().manual_seed(20250118)
    host = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=gen)
    dev = host.cuda()
    torch.cuda.synchronize()
    want = reference(host.numpy().tobytes())
    assert probe.checksum_device(dev.data_ptr(), n) == want
    dst = torch.full((GUARD + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert probe.copy_checksum_device(dst.data_ptr() + GUARD, dev.data_ptr(), n) == want
    assert torch.equal(dst[GUARD : GUARD + n], dev)
    assert _all_equal_to(dst[:GUARD], GUARD_BYTE) and _all_equal_to(dst[GUARD + n :], GUARD_BYTE)
