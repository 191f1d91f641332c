"""MI355X tests for the slab path of csp_gather_checksum_dev: a short inner
dimension (2 to 31 elements) directly under the unit-stride one, as in a
``channels_last`` 3 x 3 weight.  The host withholds the path (it measured
slower than the direct one), so every case runs with the slab path allowed by
the tools' force value 2 and with the direct path forced, against
``contiguous()`` on the CPU copy: exact, no tolerance."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_gather_checksum import (  # noqa: E402, F401  (holder, fixtures and helpers)
    DTYPES, GUARD, HOLDER, _gather, _holder, _shaped, probe, source,
)
from test_gpu_pack_checksum import reference  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (view of a flat typed tensor, the path that must run when the slab is allowed)
CASES = {
    # (3, 33, 9): rows start off 16-byte alignment up to 8 bytes; one partial slab per row
    "w3x3_i33": (lambda f: _shaped(f, 3, 3, 3, 33).permute(0, 3, 1, 2), "slab"),
    # (2, 300, 9): full slabs and a partial one at every element size
    "w3x3_i300": (lambda f: _shaped(f, 2, 3, 3, 300).permute(0, 3, 1, 2), "slab"),
    "w2x2_i70": (lambda f: _shaped(f, 2, 2, 2, 70).permute(0, 3, 1, 2), "slab"),  # even C: padded
    "c2_i33": (lambda f: _shaped(f, 2, 2, 33).permute(0, 2, 1), "slab"),  # the shortest C
    "c31_i33": (lambda f: _shaped(f, 2, 31, 33).permute(0, 2, 1), "slab"),  # the longest C
    # four dimensions are left: R0 and R1
    "four_d": (lambda f: _shaped(f, 2, 4, 5, 41)[:, :3, :, :40].permute(0, 1, 3, 2), "slab"),
    # the neighbours, as before
    "c32_i33": (lambda f: _shaped(f, 2, 32, 33).permute(0, 2, 1), "transpose"),
    "w3x3_i31": (lambda f: _shaped(f, 2, 3, 3, 31).permute(0, 3, 1, 2), "direct"),
}
PARAMS = [(name, es) for name in CASES for es in (1, 2, 4, 8)] + [("four_d", 16)]


def _check(probe, source, name, es):
    host, dev = source
    make, path = CASES[name]
    view = make(dev.view(DTYPES[es]))
    flat = make(host.view(DTYPES[es])).contiguous()
    want = (torch.view_as_real(flat) if es == 16 else flat).reshape(-1).view(torch.uint8).numpy()
    total = (len(want) + 15) // 16 * 16
    reports = []
    try:
        for force in (2, 1):
            probe.gather_checksum_path(force)
            outer = _holder(total)
            reports.append(_gather(probe, view, outer, total))
            got = outer.cpu().numpy()
            arena = got[GUARD : GUARD + total]
            assert np.array_equal(arena[: len(want)], want), "data differs"
            assert not arena[len(want) :].any(), "padding is not zero"
            assert (got[:GUARD] == HOLDER).all() and (got[GUARD + total :] == HOLDER).all()
            assert reports[-1]["sums"] == reference(arena.tobytes())
    finally:
        probe.gather_checksum_path(0)
    assert torch.equal(dev.cpu(), host), "the source was written"
    assert reports[0]["sums"] == reports[1]["sums"]
    assert [r["path"] for r in reports] == [path, "direct"]


@pytest.mark.parametrize("name, es", PARAMS)
def test_short_inner_dimension_against_contiguous_on_the_cpu(probe, source, name, es):
    _check(probe, source, name, es)


def test_the_host_itself_keeps_short_inner_dimensions_on_the_direct_path(probe, source):
    view = CASES["w3x3_i300"][0](source[1].view(torch.int16))
    total = view.numel() * 2
    assert _gather(probe, view, _holder(total), total)["path"] == "direct"


@pytest.mark.parametrize("cap", [1, 2, 3])
@pytest.mark.parametrize("es", [1, 4])
def test_blocks_loop_over_slabs_under_small_grid_caps(probe, source, es, cap):
    try:
        assert probe.gather_checksum_grid_cap(cap) == cap
        _check(probe, source, "w3x3_i300", es)  # 4 and 10 slabs
    finally:
        assert probe.gather_checksum_grid_cap(0) == 1024
