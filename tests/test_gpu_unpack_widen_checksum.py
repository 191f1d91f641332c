"""MI355X tests for csp_unpack_widen_checksum_dev against numpy integer arithmetic on the bits:
copies and widened segments of one narrow arena, the private tensors, the wide master, the sum
with wide-arena word indices, grid caps, the two kernels it generalises and every refusal; no
tolerance."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_narrow_checksum import (  # noqa: E402
    PAIRS, _narrow_values, _sizes, _widen_bits, probe,  # noqa: F401  (probe: a fixture)
)
from test_gpu_pack_checksum import FILL, GUARD, HOLDER, _holder, reference  # noqa: E402

pytestmark = pytest.mark.gpu

RAW = np.random.default_rng(20261126).integers(0, 256, 40 << 10, dtype=np.uint8)


def _unpack(probe, rows, pieces, master=True, cap=0):
    """One call on ``rows``, (count, narrow, wide) each, whose wire bytes are ``pieces``; the pad
    bytes after a narrowed segment are 0xFF.  Returns (sum, [dst bytes], master bytes or None)
    after the guards around every destination and the master were checked."""
    src_off, narrow_total, dst_off, wide_total = probe.unpack_widen_layout(rows)
    host = np.zeros(narrow_total, dtype=np.uint8)
    for off, piece, row in zip(src_off, pieces, rows):
        if row[1]:
            host[off: off + (len(piece) + 15) // 16 * 16] = 0xFF
        host[off: off + len(piece)] = piece
    arena = torch.from_numpy(host).cuda()
    sizes = [n * probe.NARROW_ELEM_SIZE[wide] if narrow else n for n, narrow, wide in rows]
    outs = [_holder(n) for n in sizes] + ([_holder(wide_total)] if master else [])
    try:
        probe.unpack_widen_checksum_grid_cap(cap)
        report = probe.unpack_widen_checksum_device(
            [(o.data_ptr() + GUARD, s, d) + r for o, s, d, r in zip(outs, src_off, dst_off, rows)],
            arena.data_ptr(), narrow_total, outs[-1].data_ptr() + GUARD if master else 0,
            wide_total)
    finally:
        probe.unpack_widen_checksum_grid_cap(0)
    assert np.array_equal(arena.cpu().numpy(), host), "the narrow arena changed"
    got = []
    for outer, n in zip(outs, sizes + [wide_total]):
        raw = outer.cpu().numpy()
        assert (raw[:GUARD] == HOLDER).all() and (raw[GUARD + n:] == HOLDER).all(), "guards"
        got.append(raw[GUARD: GUARD + n])
    if master:
        assert report["sum"] == probe.checksum_device(outs[-1].data_ptr() + GUARD, wide_total)
    return report["sum"], got[: len(rows)], got[-1] if master else None


def _mixed(probe, pair, n, master, cap=0):
    """A 17-byte copy, a widened segment, a copy of 16 KiB + 1 bytes and the widened segment
    again, each checked against the model; returns (sum, wide arena)."""
    wide, wire = pair
    narrow = _narrow_values(wire, n)
    rows = [(17, "", ""), (n, wire, wide), ((16 << 10) + 1, "", ""), (n, wire, wide)]
    pieces = [RAW[1:18], narrow.view(np.uint8), RAW[32: 32 + (16 << 10) + 1], narrow.view(np.uint8)]
    full = _widen_bits(narrow, wide).view(np.uint8)
    sums, dsts, held = _unpack(probe, rows, pieces, master, cap)
    _, _, dst_off, wide_total = probe.unpack_widen_layout(rows)
    want = np.zeros(wide_total, dtype=np.uint8)
    for off, got, piece in zip(dst_off, dsts, [pieces[0], full, pieces[2], full]):
        assert np.array_equal(got, piece), "a destination differs from the model"
        want[off: off + len(piece)] = piece
    assert sums == reference(want.tobytes())
    assert held is None or np.array_equal(held, want), "the master is not the wide arena"
    return sums, want


@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("pair, n", [
    (p, n) for p in PAIRS for e, w, t in [_sizes(p[1])]
    for n in (1, e - 1, e, e + 1, w - 1, w + 1, t - 1, t + 1, 2 * t + 1)])
def test_a_mixed_arena_equals_the_model(probe, pair, n, master):
    _mixed(probe, pair, n, master)


@pytest.mark.parametrize("pair", PAIRS)
def test_grid_caps_and_a_lone_segment(probe, pair):
    wide, wire = pair
    n = 2 * _sizes(wire)[2] + 1  # nine units in the mixed arena
    sums, arena = _mixed(probe, pair, n, True)
    for cap in (1, 2, 3):
        again, same = _mixed(probe, pair, n, cap != 2, cap)
        assert again == sums and np.array_equal(same, arena)
    narrow = _narrow_values(wire, n)
    lone, (got,), _ = _unpack(probe, [(n, wire, wide)], [narrow.view(np.uint8)], False)
    dev = torch.from_numpy(np.resize(narrow.view(np.uint8), probe.narrow_bytes(n, wire))).cuda()
    other = _holder(len(got))
    alone = probe.widen_checksum_device(dev.data_ptr(), n, wire, wide, other.data_ptr() + GUARD)
    assert lone == alone["sum"]
    assert np.array_equal(got, other.cpu().numpy()[GUARD: GUARD + len(got)])


def test_only_copies_equal_the_unpack_kernel(probe):
    spans = [(1, 17), (32, (16 << 10) + 1), (20000, 5), (20011, 0), (20016, 4096)]
    pieces = [RAW[s: s + n] for s, n in spans]
    sums, dsts, held = _unpack(probe, [(n, "", "") for _, n in spans], pieces)
    offsets, total = probe.pack_layout([n for _, n in spans])
    outs = [_holder(n) for _, n in spans]
    wide = torch.from_numpy(held).cuda()
    plain = probe.unpack_checksum_device(
        wide.data_ptr(), total,
        [(o.data_ptr() + GUARD if n else 0, off, n) for o, off, (_, n) in zip(outs, offsets, spans)])
    assert sums == plain["sum"]
    for got, outer, piece in zip(dsts, outs, pieces):
        assert np.array_equal(got, piece)
        assert np.array_equal(outer.cpu().numpy()[GUARD: GUARD + len(piece)], piece)


REFUSALS = [  # (segment, field, value) or (buffer, field, value), and the message
    ((1, 0, 0), "segment 1 has 4096 bytes and a null dst"),
    ((1, 0, "+4"), "segment 1: dst .* is not 16-byte aligned"),
    ((1, 4, "float32"), "segment 1: no widening from kind 0 to kind 0"),
    ((1, 1, 16), "segment 1: src_off is 16, the narrow layout gives 32"),
    ((2, 2, 4112), "segment 2: dst_off is 4112, the wide layout gives 4128"),
    ((2, 3, 113), "segment 2: .* end past wide_bytes"),
    ((2, 3, 96), "the segments need"),
    (("narrow", "bytes", 16), "the segments need"),
    (("wide", "bytes", -16), "segment 2: .* end past wide_bytes"),
    (("wide", "bytes", 4 << 30), "above 4 GiB"),
    (("narrow", "ptr", "+8"), "narrow arena pointer .* is not 16-byte aligned"),
    (("wide", "ptr", "+8"), "master pointer .* is not 16-byte aligned"),
    (("narrow", "ptr", 0), "null narrow arena"),
    ((0, 0, "narrow"), "segment 0: .* overlap the narrow arena"),
    ((1, 0, "wide"), "segment 1: .* overlap the narrow arena .* or the master"),
    (("wide", "ptr", "narrow"), "narrow arena .* overlap .* master"),
]


@pytest.mark.parametrize("change, text", REFUSALS)
def test_refusals_name_the_segment_and_launch_nothing(probe, change, text):
    rows = [(17, "", ""), (1024, "bfloat16", "float32"), (100, "", "")]
    src_off, narrow_total, dst_off, wide_total = probe.unpack_widen_layout(rows)
    outs = [_holder(n) for n in (17, 4096, 100, wide_total)]
    arena = torch.zeros(narrow_total, dtype=torch.uint8, device="cuda")
    bufs = {"narrow": {"ptr": arena.data_ptr(), "bytes": narrow_total},
            "wide": {"ptr": outs[-1].data_ptr() + GUARD, "bytes": wide_total}}
    segs = [[o.data_ptr() + GUARD, s, d, *r] for o, s, d, r in zip(outs, src_off, dst_off, rows)]

    def call():
        return probe.unpack_widen_checksum_device(
            segs, bufs["narrow"]["ptr"], bufs["narrow"]["bytes"], bufs["wide"]["ptr"],
            bufs["wide"]["bytes"])

    assert call()["sum"] == (0, 0)  # the unchanged call is served: zeros, widened
    for outer, n in zip(outs, (17, 4096, 100, wide_total)):
        outer[GUARD: GUARD + n] = FILL
    torch.cuda.synchronize()
    where, field, value = change
    target = bufs[where] if isinstance(where, str) else segs[where]
    if value in ("narrow", "wide"):
        target[field] = bufs[value]["ptr"]
    elif field == "bytes" or str(value)[0] == "+":
        target[field] += int(value)
    else:
        target[field] = value
    with pytest.raises(probe.GpuLibError, match=text):
        call()
    for outer, n in zip(outs, (17, 4096, 100, wide_total)):
        assert (outer.cpu().numpy()[GUARD: GUARD + n] == FILL).all(), "something was written"
