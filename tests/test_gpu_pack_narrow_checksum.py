"""MI355X tests for csp_pack_narrow_probe_dev and csp_pack_narrow_checksum_dev against numpy
integer arithmetic on the bits: narrowed segments and plain copies in one arena, its sum with
arena-global word indices, per-segment verdicts, grid caps and every refusal; no tolerance."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_narrow_checksum import (  # noqa: E402
    BITS, PAIRS, POISONS, _narrow_values, _sizes, _widen_bits,
)
from test_gpu_pack_checksum import FILL, GUARD, HOLDER, _holder, reference  # noqa: E402

pytestmark = pytest.mark.gpu

RAW = 40 << 10  # bytes of the copied segments' source


@pytest.fixture(scope="module")
def probe():
    from covalent_ssh_plugin_amd.gpu import probe as gpu_probe

    gpu_probe.load()  # GpuLibError if the extension was not built/shipped
    return gpu_probe


@pytest.fixture(scope="module")
def raw():
    host = np.random.default_rng(20261126).integers(0, 256, RAW, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), host


def _dev(bits):
    dev = torch.from_numpy(bits.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return dev


def _pack(probe, rows, cap=0):
    """One pack call on ``rows``, (ptr, numel, src, dst) each, into a guarded arena."""
    offsets, total = probe.pack_narrow_layout(rows)
    outer = _holder(total)
    try:
        probe.pack_narrow_checksum_grid_cap(cap)
        report = probe.pack_narrow_checksum_device(
            [r + (off,) for r, off in zip(rows, offsets)], outer.data_ptr() + GUARD, total)
    finally:
        probe.pack_narrow_checksum_grid_cap(0)
    got = outer.cpu().numpy()
    assert (got[:GUARD] == HOLDER).all() and (got[GUARD + total:] == HOLDER).all(), "guards"
    assert report["sum"] == probe.checksum_device(outer.data_ptr() + GUARD, total)
    return report, got[GUARD: GUARD + total], offsets


def _mixed(probe, raw, pair, n, cap=0):
    """A 17-byte copy one byte off alignment, a narrowed segment, a copy of 16 KiB + 1 bytes and
    the narrowed source again; returns the report and the arena after the model was checked."""
    src, dst = pair
    narrow = _narrow_values(dst, n)
    wide = _dev(_widen_bits(narrow, src))
    dev, host = raw
    rows = [(dev.data_ptr() + 1, 17, "", ""), (wide.data_ptr(), n, src, dst),
            (dev.data_ptr() + 32, (16 << 10) + 1, "", ""), (wide.data_ptr(), n, src, dst)]
    report, arena, offsets = _pack(probe, rows, cap)
    want = np.zeros(len(arena), dtype=np.uint8)
    for off, piece in zip(offsets, [host[1:18], narrow.view(np.uint8),
                                    host[32: 32 + (16 << 10) + 1], narrow.view(np.uint8)]):
        want[off: off + len(piece)] = piece
    assert np.array_equal(arena, want), "arena differs from the numpy model, padding included"
    assert report["sum"] == reference(want.tobytes())
    assert report["fits"][0] is None and dst in report["fits"][1] and dst in report["fits"][3]
    return report, arena


@pytest.mark.parametrize("pair, n", [
    (p, n) for p in PAIRS for e, w, t in [_sizes(p[1])]
    for n in (1, e - 1, e, e + 1, w - 1, w + 1, t - 1, t + 1, 2 * t + 1)])
def test_a_mixed_arena_equals_the_model(probe, raw, pair, n):
    _mixed(probe, raw, pair, n)


@pytest.mark.parametrize("pair", PAIRS)
def test_grid_caps_and_a_lone_segment(probe, raw, pair):
    src, dst = pair
    n = 2 * _sizes(dst)[2] + 1  # nine units in the mixed arena
    report, arena = _mixed(probe, raw, pair, n)
    for cap in (1, 2, 3):
        capped, again = _mixed(probe, raw, pair, n, cap)
        assert capped["sum"] == report["sum"] and np.array_equal(again, arena)
    wide = _dev(_widen_bits(_narrow_values(dst, n), src))
    lone, arena, _ = _pack(probe, [(wide.data_ptr(), n, src, dst)])
    other = _holder(len(arena))
    alone = probe.narrow_checksum_device(wide.data_ptr(), n, src, dst, other.data_ptr() + GUARD,
                                         len(arena))
    assert lone["sum"] == alone["sum"] and lone["fits"] == [alone["fits"]]
    assert np.array_equal(arena, other.cpu().numpy()[GUARD: GUARD + len(arena)])


def test_only_copies_equal_the_pack_kernel(probe, raw):
    dev, _ = raw
    spans = [(1, 17), (32, (16 << 10) + 1), (20000, 5), (20011, 0), (20016, 4096)]
    report, arena, offsets = _pack(probe, [(dev.data_ptr() + s, n, "", "") for s, n in spans])
    other = _holder(len(arena))
    plain = probe.pack_checksum_device(
        [(dev.data_ptr() + s, off, n) for (s, n), off in zip(spans, offsets)],
        other.data_ptr() + GUARD, len(arena))
    assert report["sum"] == plain["sum"] and not any(report["bad"])
    assert np.array_equal(arena, other.cpu().numpy()[GUARD: GUARD + len(arena)])


@pytest.mark.parametrize("src", ["float32", "float64", "int32", "int64"])
def test_the_probe_gives_each_segment_its_own_verdict(probe, src):
    kind = BITS[src]
    tile = (16 << 10) // np.dtype(kind).itemsize  # elements of one source tile
    n = 2 * tile + 3
    if src.startswith("float"):
        dst = probe.NARROW_TARGETS[src][0]
        segs = [_widen_bits(_narrow_values(dst, n, seed), src) for seed in (1, 2, 3)]
        poison = POISONS[src][0]
    else:
        rng = np.random.default_rng(n)
        segs = [rng.integers(0, b, n).astype(kind) for b in (200, 30000, 1 << 20)]
        poison = np.iinfo(kind).max
    clean = segs[1]
    for at in (None, 0, n - 1, tile - 1, tile):
        if at is not None:  # one poison alone, in a fresh copy of the clean segment
            segs[1] = clean.copy()
            segs[1][at] = np.array(poison).astype(clean.dtype)
        devs = [_dev(s) for s in segs]
        got = probe.pack_narrow_probe_device([(d.data_ptr(), n, src) for d in devs])["fits"]
        assert got == [probe.narrow_checksum_device(d.data_ptr(), n, src)["fits"] for d in devs]
        if at is None:
            base = got
            assert len(set(base)) == (1 if src.startswith("float") else 3)  # integers: three widths
        else:
            assert got[0] == base[0] and got[2] == base[2] and got[1] != base[1], at


@pytest.mark.parametrize("pair", [("float32", "bfloat16"), ("int64", "uint8")])
def test_a_source_that_does_not_fit_is_reported_in_its_own_word(probe, raw, pair):
    src, dst = pair
    n = _sizes(dst)[2] + 5
    good = _widen_bits(_narrow_values(dst, n), src)
    changed = good.copy()
    changed[n // 2] = np.array(POISONS[src if src.startswith("float") else dst][0]).astype(
        changed.dtype)
    devs = [_dev(good), _dev(changed)]
    report, _, _ = _pack(probe, [(devs[0].data_ptr(), n, src, dst), (raw[0].data_ptr(), 33, "", ""),
                                 (devs[1].data_ptr(), n, src, dst)])
    assert dst in report["fits"][0] and dst not in report["fits"][2] and report["bad"][1] == 0


REFUSALS = [  # (segment, field, value) or ("arena", field, value), and the message
    ((1, 0, 0), "segment 1 has 1024 elements at a null pointer"),
    ((1, 3, "int16"), "segment 1: no narrowing from kind 0 to kind 5"),
    ((1, 0, "+4"), "segment 1: src .* is not 16-byte aligned"),
    ((1, 4, 40), "segment 1: dst_off 40 is not a multiple of 16"),
    ((1, 4, 0), "segment 1: dst_off is 0, the layout rule gives 32"),
    ((2, 4, 48), "segment 2: dst_off is 48, the layout rule gives"),
    (("arena", "bytes", -16), "segment 2 ends at .*, past arena_bytes"),
    (("arena", "bytes", 8), "is not a multiple of 16"),
    (("arena", "bytes", 16 << 30), "above 16 GiB"),
    (("arena", "ptr", 0), "null arena"),
    (("arena", "ptr", "src"), "segment 1: .* overlap the arena"),
]


@pytest.mark.parametrize("change, text", REFUSALS)
def test_refusals_name_the_segment_and_leave_the_arena_alone(probe, raw, change, text):
    wide = _dev(_widen_bits(_narrow_values("bfloat16", 1024), "float32"))
    rows = [[raw[0].data_ptr() + 1, 17, "", ""], [wide.data_ptr(), 1024, "float32", "bfloat16"],
            [raw[0].data_ptr() + 32, 100, "", ""]]
    offsets, total = probe.pack_narrow_layout(rows)
    rows = [r + [off] for r, off in zip(rows, offsets)]
    outer = _holder(total)
    arena = {"ptr": outer.data_ptr() + GUARD, "bytes": total}
    probe.pack_narrow_checksum_device(rows, arena["ptr"], total)  # the unchanged call is served
    outer[GUARD: GUARD + total] = FILL
    torch.cuda.synchronize()
    where, field, value = change
    if where == "arena":
        arena[field] = {"src": wide.data_ptr() + 16}.get(value, value) if field == "ptr" else (
            total + value)
    else:
        rows[where][field] = rows[where][field] + 4 if value == "+4" else value
    with pytest.raises(probe.GpuLibError, match=text):
        probe.pack_narrow_checksum_device(rows, arena["ptr"], arena["bytes"])
    assert (outer.cpu().numpy()[GUARD: GUARD + total] == FILL).all(), "the arena was written"


@pytest.mark.parametrize("row, text", [
    ((0, 8, "int64"), "segment 1 has 8 elements at a null pointer"),
    (("+8", 8, "int64"), "segment 1: src .* is not 16-byte aligned"),
    (("+0", 8, "int16"), "segment 1: no narrowing from kind 5"),
])
def test_probe_refusals_and_the_empty_segment(probe, raw, row, text):
    ptr = raw[0].data_ptr()
    assert probe.pack_narrow_probe_device([(ptr, 0, "int64"), (0, 0, "float32")])["bad"] == [0, 0]
    row = (ptr + int(row[0]) if isinstance(row[0], str) else row[0],) + row[1:]
    with pytest.raises(probe.GpuLibError, match=text):
        probe.pack_narrow_probe_device([(ptr, 16, "int32"), row])
