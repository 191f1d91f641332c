"""MI355X tests for csp_pack_gather_checksum_dev: contiguous and strided
segments of all three kinds in one arena and one launch, against the same
views on the CPU copy followed by ``contiguous()``, laid into a numpy arena by
the layout rule.  Exact, no tolerance."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_gather_checksum import (  # noqa: E402, F401  (cases, holder and fixtures)
    CASES, DTYPES, FILL, GUARD, HOLDER, TRANSPOSED, _holder, probe, source,
)
from test_gpu_pack_checksum import reference  # noqa: E402

from covalent_ssh_plugin_amd.gpu.probe import pack_layout  # noqa: E402

pytestmark = pytest.mark.gpu

# a name of CASES, "empty", or (source byte offset, nbytes) of contiguous bytes.
# At 4 bytes: 1 + 2 + 2 + 1 + 12 + 0 + 1 + 4 + 1 + 1 = 25 units (tiles and
# patches), so under a cap of 3 every workgroup walks eight of them, of all kinds
MIXED = [(0, 17), "t65x33", (1, 16385), "cols17", "permute4d", "empty", "expand",
         "two_tiles", "every2nd", (0, 1)]


def _view(flat, es, name):
    if name == "empty":
        return flat.view(DTYPES[es])[:0].reshape(0, 3)
    if isinstance(name, tuple):
        return flat[4096 + name[0] : 4096 + name[0] + name[1]]
    return CASES[name](flat.view(DTYPES[es]), es)


def _build(source, es, names):
    """The probe's segments, the arena they must give, and each segment's
    (offset, data bytes)."""
    host, dev = source
    wants = []
    for name in names:
        flat = _view(host, es, name).contiguous()
        flat = torch.view_as_real(flat) if flat.is_complex() else flat
        wants.append(flat.reshape(-1).view(torch.uint8).numpy())
    offsets, total = pack_layout([len(w) for w in wants])
    arena = np.zeros(total, dtype=np.uint8)
    segments = []
    for name, want, off in zip(names, wants, offsets):
        arena[off : off + len(want)] = want
        view = _view(dev, es, name)
        seg = (view.data_ptr(), off, len(want))
        if not isinstance(name, tuple):
            seg += (view.element_size(), list(view.shape), list(view.stride()))
        segments.append(seg)
    return segments, arena, [(off, len(w)) for off, w in zip(offsets, wants)]


def _pack_and_check(probe, source, es, names, force=0):
    """One call and every property the kernel promises; returns the report
    and the holder."""
    segments, want, spans = _build(source, es, names)
    outer = _holder(len(want))
    try:
        assert probe.pack_gather_checksum_path(force) == force
        report = probe.pack_gather_checksum_device(segments, outer.data_ptr() + GUARD, len(want))
    finally:
        probe.pack_gather_checksum_path(0)
    got = outer.cpu().numpy()
    arena = got[GUARD : GUARD + len(want)]
    assert np.array_equal(arena, want), "data or padding differs"
    for off, n in spans:
        assert not arena[off + n : off + (n + 15) // 16 * 16].any(), "padding is not zero"
    assert (got[:GUARD] == HOLDER).all() and (got[GUARD + len(want) :] == HOLDER).all()
    assert torch.equal(source[1].cpu(), source[0]), "a source was written"
    assert report["sums"] == reference(want.tobytes())
    assert report["sums"] == probe.checksum_device(outer.data_ptr() + GUARD, len(want))
    for name, path in zip(names, report["paths"]):
        if isinstance(name, tuple) or name == "empty":
            assert path == ("none" if name == "empty" or name[1] == 0 else "copy")
        else:
            assert (path == "transpose") == (name in TRANSPOSED and not force), (name, path)
    return report, outer


@pytest.mark.parametrize("force", [0, 1])
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_all_three_kinds_in_one_arena(probe, source, es, force):
    report, _ = _pack_and_check(probe, source, es, MIXED, force)
    assert report["paths"].count("transpose") == (0 if force else 3)


@pytest.mark.parametrize("force", [0, 1])
def test_a_16_byte_transpose_between_contiguous_segments(probe, source, force):
    _pack_and_check(probe, source, 16, [(1, 100), "t130x67", (3, 16385)], force)


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_workgroups_walk_units_of_every_kind_under_small_grid_caps(probe, source, cap):
    try:
        assert probe.pack_gather_checksum_grid_cap(cap) == cap
        _pack_and_check(probe, source, 4, MIXED)
    finally:
        assert probe.pack_gather_checksum_grid_cap(0) == 1024


@pytest.mark.parametrize("name, es", [("t64x64", 1), ("permute", 2), ("channels_last", 4),
                                      ("cols33", 4), ("sub2x3", 8), ("permute3d", 8),
                                      ("offset1", 2), ("t130x67", 16)])
def test_one_strided_segment_equals_the_gather_kernel(probe, source, name, es):
    report, outer = _pack_and_check(probe, source, es, [name])
    view = _view(source[1], es, name)
    other = _holder(outer.numel() - 2 * GUARD)
    alone = probe.gather_checksum_device(
        view.data_ptr(), es, list(view.shape), list(view.stride()),
        other.data_ptr() + GUARD, other.numel() - 2 * GUARD,
    )
    assert torch.equal(other, outer) and alone["sums"] == report["sums"]


def test_contiguous_segments_only_equal_the_pack_kernel(probe, source):
    names = [(k % 16, n) for k, n in enumerate([0, 1, 15, 16, 17, 4095, 16384, 16385, 49157])]
    report, outer = _pack_and_check(probe, source, 1, names)
    segments, want, _ = _build(source, 1, names)
    other = _holder(len(want))
    packed = probe.pack_checksum_device(segments, other.data_ptr() + GUARD, len(want))
    assert torch.equal(other, outer) and packed["sum"] == report["sums"]


FIVE = ([2, 3, 2, 3, 2], [1152, 192, 48, 8, 2])  # five dimensions after collapsing


def _refusals(src, dst):
    """message -> (segments, arena, arena_bytes, what gather_supported says of
    the strided segment, or None)"""
    return {
        "segment 0: 5 dimensions are left": ([(src, 0, 72, 1) + FIVE], dst, 80, False),
        "segment 1: elem_size 3": ([(src, 0, 16), (src, 16, 48, 3, [16], [1])], dst, 64, False),
        "segment 0: nbytes is 60": ([(src, 0, 60, 4, [16], [2])], dst, 64, True),
        "segment 1: dst_off is 16": ([(src, 0, 17), (src, 16, 16)], dst, 48, None),
        "arena_bytes is 32": ([(src, 0, 16)], dst, 32, None),
        "not 16-byte aligned": ([(src, 0, 16)], dst + 8, 16, None),
        "segment 0 has 16 bytes at a null pointer": ([(0, 0, 16)], dst, 16, None),
        # (1 + 7 * 2) * 1 = 15 source bytes, the last of them the arena's first
        "segment 0: 15 source bytes .* overlap": ([(dst - 14, 0, 8, 1, [8], [2])], dst, 16, True),
    }


@pytest.mark.parametrize("message", list(_refusals(0, 0)))
def test_refusals_launch_nothing_and_name_the_segment(probe, source, message):
    outer = _holder(256)
    segments, arena, total, served = _refusals(source[1].data_ptr(), outer.data_ptr() + GUARD)[
        message]
    with pytest.raises(probe.GpuLibError, match="csp_pack_gather_checksum_dev: .*" + message):
        probe.pack_gather_checksum_device(segments, arena, total)
    got = outer.cpu().numpy()
    assert (got[GUARD:-GUARD] == FILL).all() and (got[:GUARD] == HOLDER).all()
    assert (got[-GUARD:] == HOLDER).all()
    if served is not None:
        assert probe.gather_supported(*segments[-1][3:]) is served


def test_a_strided_extent_that_only_touches_the_arena_is_accepted(probe):
    outer = _holder(16)
    dst = outer.data_ptr() + GUARD
    report = probe.pack_gather_checksum_device([(dst - 15, 0, 8, 1, [8], [2])], dst, 16)
    want = bytes([HOLDER]) * 8 + bytes(8)
    assert outer.cpu().numpy()[GUARD:-GUARD].tobytes() == want
    assert report["sums"] == reference(want) and report["paths"] == ["direct"]
