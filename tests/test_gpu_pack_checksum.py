"""MI355X tests for csp_pack_checksum_dev: the pack kernel's gather with the
arena's checksum from the same pass.  Every size class at every source byte
offset, together and alone; the arena against a numpy model and against
csp_pack_dev's; the sum against numpy, csp_checksum_dev and the host
library; one segment past 64 MiB (the large-tensor case); the per-block tile
loop under small grid caps and the default one; every refusal."""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5  # the arena before the call
HOLDER = 0x3C  # what surrounds the arena
OFFSETS = list(range(16))  # source start, from a 16-byte aligned base
DEFAULT_CAP = 1024


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
def native_io():
    from covalent_ssh_plugin_amd.transport import native_io as io

    assert io.load() is not None, "libcsp_io.so was not built/shipped"
    return io


def _sizes(tile):
    return [0, 1, 15, 16, 17, 4095, tile, tile + 1, 3 * tile + 5, (1 << 20) + 3]


@pytest.fixture(scope="module")
def cases(probe):
    """Every size at every source offset, as (start, nbytes) slices of one
    seeded random device tensor that is shared and never written to.  Each
    source starts ``offset`` bytes after a 16-byte boundary."""
    tile = probe.pack_tile_bytes()
    spans = []
    cursor = 0
    for nbytes in _sizes(tile):
        for offset in OFFSETS:
            start = (cursor + 15) // 16 * 16 + offset
            spans.append((start, nbytes))
            cursor = start + nbytes
    gen = torch.Generator().manual_seed(20261021)
    host = torch.randint(0, 256, (cursor,), dtype=torch.uint8, generator=gen)
    dev = host.cuda()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    for (start, _), offset in zip(spans, OFFSETS * len(_sizes(tile))):
        assert (dev.data_ptr() + start) % 16 == offset
    return dev, host.numpy(), spans


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


def _expected(host, spans, offsets, total):
    """The arena assembled on the host from the same layout rule; bytes no
    segment owns are zero."""
    want = np.zeros(total, dtype=np.uint8)
    for (start, nbytes), off in zip(spans, offsets):
        want[off : off + nbytes] = host[start : start + nbytes]
    return want


def _holder(total):
    """A 0x3C holder with a 16-byte aligned, 0xA5-filled arena of ``total``
    bytes GUARD bytes into it."""
    outer = torch.full((GUARD + total + GUARD,), HOLDER, dtype=torch.uint8, device="cuda")
    outer[GUARD : GUARD + total] = FILL
    torch.cuda.synchronize()
    assert (outer.data_ptr() + GUARD) % 16 == 0
    return outer


def _pack_checksum_and_check(probe, native_io, dev, host, spans, check_sources=True):
    """One csp_pack_checksum_dev call on ``spans`` of ``dev`` and every
    property the kernel promises.  Returns (arena bytes, sum)."""
    offsets, total = probe.pack_layout([n for _, n in spans])
    outer = _holder(total)
    arena_ptr = outer.data_ptr() + GUARD
    segments = [
        (dev.data_ptr() + start, off, nbytes)
        for (start, nbytes), off in zip(spans, offsets)
    ]
    report = probe.pack_checksum_device(segments, arena_ptr, total)
    assert report["kernel_ms"] >= 0.0
    got = outer.cpu().numpy()
    arena = got[GUARD : GUARD + total]
    want = _expected(host, spans, offsets, total)
    assert np.array_equal(arena, want), "arena differs from the numpy model"
    for (_, nbytes), off in zip(spans, offsets):
        pad_end = off + (nbytes + 15) // 16 * 16
        assert not arena[off + nbytes : pad_end].any(), "padding is not zero"
    assert (got[:GUARD] == HOLDER).all(), "wrote before the arena"
    assert (got[GUARD + total :] == HOLDER).all(), "wrote past the arena"
    if check_sources:
        assert np.array_equal(dev.cpu().numpy(), host), "a source was written to"
    ref = reference(want.tobytes())
    assert report["sum"] == ref, "sum differs from the numpy reference"
    assert report["sum"] == probe.checksum_device(arena_ptr, total)
    assert report["sum"] == tuple(native_io.checksum(want.tobytes()) if total else (0, 0))
    other = _holder(total)
    probe.pack_device(segments, other.data_ptr() + GUARD, total)
    assert torch.equal(other, outer), "arena differs from csp_pack_dev's"
    return arena, report["sum"]


# -- sizes, offsets, sums ----------------------------------------------------


def test_every_size_at_every_offset_in_one_call(probe, native_io, cases):
    dev, host, spans = cases
    assert len(spans) == 160
    _pack_checksum_and_check(probe, native_io, dev, host, spans)


def test_every_size_at_every_offset_alone(probe, native_io, cases):
    dev, host, spans = cases
    for span in spans:
        _pack_checksum_and_check(probe, native_io, dev, host, [span], check_sources=False)
    # nothing restores the sources: one look after all the calls sees any write
    assert np.array_equal(dev.cpu().numpy(), host), "a source was written to"


@pytest.fixture(scope="module")
def large():
    """64 MiB + 5 bytes + 1: the one-segment large-tensor source."""
    nbytes = (64 << 20) + 5
    rng = np.random.default_rng(64)
    host = rng.integers(0, 256, size=nbytes + 1, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    return dev, host, nbytes


@pytest.mark.parametrize("offset", [0, 1])
def test_one_segment_past_64_mib(probe, native_io, large, offset):
    dev, host, nbytes = large
    total = (nbytes + 15) // 16 * 16
    outer = _holder(total)
    arena_ptr = outer.data_ptr() + GUARD
    report = probe.pack_checksum_device([(dev.data_ptr() + offset, 0, nbytes)], arena_ptr, total)
    got = outer.cpu().numpy()
    want = np.zeros(total, dtype=np.uint8)
    want[:nbytes] = host[offset : offset + nbytes]
    assert np.array_equal(got[GUARD : GUARD + total], want)
    assert (got[:GUARD] == HOLDER).all() and (got[GUARD + total :] == HOLDER).all()
    assert report["sum"] == reference(want.tobytes())
    assert report["sum"] == probe.checksum_device(arena_ptr, total)
    # the frame that leaves is the nbytes without the padding: the same sum
    assert report["sum"] == tuple(native_io.checksum(want[:nbytes].tobytes()))
    assert np.array_equal(dev.cpu().numpy(), host), "the source was written to"


def test_one_flipped_source_bit_changes_the_sum(probe, native_io, cases):
    dev, host, spans = cases
    picked = [s for s in spans if s[1] in (17, 4095)][::5]
    assert len(picked) == 7
    _, clean = _pack_checksum_and_check(probe, native_io, dev, host, picked)
    flipped_dev = dev.clone()
    flipped_host = host.copy()
    start, nbytes = picked[3]
    where = start + nbytes - 1  # the last byte of a segment: in a tail vector
    flipped_host[where] ^= 0x10
    flipped_dev[where] = int(flipped_host[where])
    torch.cuda.synchronize()
    _, dirty = _pack_checksum_and_check(probe, native_io, flipped_dev, flipped_host, picked)
    assert dirty != clean
    assert dirty[0] != clean[0] and dirty[1] != clean[1]


# -- the per-block tile loop -------------------------------------------------


def _tiles(probe, spans):
    tile = probe.pack_tile_bytes()
    return sum(-(-((n + 15) // 16 * 16) // tile) for _, n in spans)


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_small_grid_caps(probe, native_io, cases, cap):
    dev, host, spans = cases
    picked = [s for s in spans if s[1] >= 4095][::3]  # every size class, mixed offsets
    assert _tiles(probe, picked) > cap * 4
    assert probe.pack_checksum_grid_cap(cap) == cap
    try:
        _pack_checksum_and_check(probe, native_io, dev, host, picked)
    finally:
        assert probe.pack_checksum_grid_cap(0) == DEFAULT_CAP


def test_more_tiles_than_blocks_at_the_default_cap(probe, native_io, cases):
    dev, host, _ = cases
    assert probe.pack_checksum_grid_cap(0) == DEFAULT_CAP
    rng = np.random.default_rng(5)
    sizes = rng.integers(0, 5001, size=3000).tolist()
    assert sum(1 for n in sizes if n) > 2 * DEFAULT_CAP  # one tile each: a third trip
    spans = []
    cursor = 0
    for nbytes in sizes:  # back to back: the sources land on every alignment
        if cursor + nbytes > len(host):
            cursor = 0  # sources may share bytes, nothing writes to them
        spans.append((cursor, nbytes))
        cursor += nbytes
    assert len({start % 16 for start, _ in spans}) == 16
    _pack_checksum_and_check(probe, native_io, dev, host, spans)


# -- refusals ----------------------------------------------------------------


def test_every_refusal_launches_nothing(probe, native_io, cases):
    dev, host, _ = cases
    spans = [(0, 100), (128, 33), (256, 4096)]
    offsets, total = probe.pack_layout([n for _, n in spans])
    assert offsets == [0, 112, 160] and total == 160 + 4096
    outer = _holder(total + 16)  # room for the calls that declare 16 more
    arena_ptr = outer.data_ptr() + GUARD
    before = outer.cpu().numpy().copy()
    base = dev.data_ptr()

    def segments(offs, sizes=None, srcs=None):
        sizes = sizes or [n for _, n in spans]
        srcs = srcs or [base + s for s, _ in spans]
        return list(zip(srcs, offs, sizes))

    refused = probe.GpuLibError
    # what csp_pack_dev refuses
    with pytest.raises(refused, match="layout rule"):
        probe.pack_checksum_device(segments([0, 100, 160]), arena_ptr, total)
    with pytest.raises(refused, match="layout rule"):
        probe.pack_checksum_device(segments([16, 128, 176]), arena_ptr, total + 16)
    with pytest.raises(refused, match="arena_bytes"):
        probe.pack_checksum_device(segments(offsets), arena_ptr, total + 16)
    with pytest.raises(refused, match="16-byte aligned"):
        probe.pack_checksum_device(segments(offsets), arena_ptr + 4, total)
    with pytest.raises(refused, match="null pointer"):
        probe.pack_checksum_device(
            segments(offsets, srcs=[base, 0, base + 256]), arena_ptr, total
        )
    with pytest.raises(refused, match="null arena"):
        probe.pack_checksum_device(segments(offsets), 0, total)
    with pytest.raises(refused, match="overflows"):
        probe.pack_checksum_device(
            segments([0, 112], sizes=[100, (1 << 64) - 8], srcs=[base, 16]), arena_ptr, total
        )
    lib = probe.load()
    one = (ctypes.c_void_p * 1)(base)
    zero = (ctypes.c_uint64 * 1)(0)
    size = (ctypes.c_uint64 * 1)(16)
    out = (ctypes.c_uint64 * 2)(7, 7)
    rc = lib.csp_pack_checksum_dev(
        one, zero, size, 1 << 31, ctypes.c_void_p(arena_ptr), 16, out, None
    )
    assert rc == -1 and b"too many" in lib.csp_last_error()
    assert (out[0], out[1]) == (0, 0)
    # its own: a source that overlaps the arena, at either end and inside
    for src in (arena_ptr - 50, arena_ptr + total - 1, arena_ptr + 200, arena_ptr - 16):
        with pytest.raises(refused, match="overlap the arena"):
            probe.pack_checksum_device(
                segments(offsets, srcs=[src, base + 128, base + 256]), arena_ptr, total
            )
    # its own: more than 16 GiB, declared on small real buffers
    huge = (16 << 30) + 16
    with pytest.raises(refused, match="above 16 GiB"):
        probe.pack_checksum_device([(base, 0, huge)], arena_ptr, huge)
    with pytest.raises(refused, match="above 16 GiB"):
        probe.pack_checksum_device(segments(offsets), arena_ptr, huge)
    torch.cuda.synchronize()
    assert np.array_equal(outer.cpu().numpy(), before), "a refused call launched something"
    assert np.array_equal(dev.cpu().numpy(), host)
    # the library is fine
    _pack_checksum_and_check(probe, native_io, dev, host, spans)


def test_touching_ranges_are_accepted(probe):
    """A source that ends where the arena begins, and one that begins where
    it ends."""
    n = 4096 + 7
    rounded = (n + 15) // 16 * 16
    total = 2 * rounded
    gen = torch.Generator().manual_seed(7)
    buf_host = torch.randint(0, 256, (rounded + total + n,), dtype=torch.uint8, generator=gen)
    buf = buf_host.cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    arena_ptr = buf.data_ptr() + rounded
    first = buf.data_ptr() + rounded - n  # ends at the arena's first byte
    second = arena_ptr + total  # begins at the first byte after the arena
    report = probe.pack_checksum_device(
        [(first, 0, n), (second, rounded, n)], arena_ptr, total
    )
    got = buf.cpu().numpy()
    src = buf_host.numpy()
    want = np.zeros(total, dtype=np.uint8)
    want[:n] = src[rounded - n : rounded]
    want[rounded : rounded + n] = src[rounded + total :]
    assert np.array_equal(got[rounded : rounded + total], want)
    assert np.array_equal(got[:rounded], src[:rounded])
    assert np.array_equal(got[rounded + total :], src[rounded + total :])
    assert report["sum"] == reference(want.tobytes())
