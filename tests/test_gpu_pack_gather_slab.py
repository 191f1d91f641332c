"""MI355X tests for slab segments in csp_pack_gather_checksum_dev: short inner
dimensions next to contiguous, direct and transposed segments in one arena and
one launch, against ``contiguous()`` on the CPU copy laid out by the layout
rule.  The host withholds the slab path, so the tools' force value 2 allows
it here.  Exact, no tolerance."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_gather_checksum import (  # noqa: E402, F401  (cases, holder and fixtures)
    CASES, DTYPES, GUARD, HOLDER, _gather, _holder, probe, source,
)
from test_gpu_gather_slab import CASES as SLAB_CASES  # noqa: E402
from test_gpu_pack_checksum import reference  # noqa: E402

from covalent_ssh_plugin_amd.gpu.probe import pack_layout  # noqa: E402

pytestmark = pytest.mark.gpu

# segment -> (view of the flat byte tensor at element size es, its path with the slab allowed
# (force 2), its path with direct forced (force 1))
MIXED = [
    (lambda b, es: b[4097 : 4097 + 16385], "copy", "copy"),  # contiguous, odd offset
    (lambda b, es: SLAB_CASES["w3x3_i33"][0](b.view(DTYPES[es])), "slab", "direct"),
    (lambda b, es: CASES["t65x33"](b.view(DTYPES[es]), es), "transpose", "direct"),
    (lambda b, es: CASES["cols17"](b.view(DTYPES[es]), es), "direct", "direct"),
    (lambda b, es: SLAB_CASES["w3x3_i300"][0](b.view(DTYPES[es])), "slab", "direct"),
    (lambda b, es: b.view(DTYPES[es])[:0].reshape(0, 3), "none", "none"),
]


def _pack(probe, source, es, cases, force):
    """One call, every property the kernel promises; the report and the holder."""
    host, dev = source
    wants = [make(host, es).contiguous().reshape(-1).view(torch.uint8).numpy()
             for make, _, _ in cases]
    offsets, total = pack_layout([len(w) for w in wants])
    want = np.zeros(total, dtype=np.uint8)  # the padding is zero
    segments = []
    for (make, _, _), w, off in zip(cases, wants, offsets):
        want[off : off + len(w)] = w
        view = make(dev, es)
        contiguous = (view.data_ptr(), off, len(w))
        strided = (view.element_size(), list(view.shape), list(view.stride()))
        segments.append(contiguous if view.dim() == 1 else contiguous + strided)
    outer = _holder(total)
    try:
        probe.pack_gather_checksum_path(force)
        report = probe.pack_gather_checksum_device(segments, outer.data_ptr() + GUARD, total)
    finally:
        probe.pack_gather_checksum_path(0)
    got = outer.cpu().numpy()
    assert np.array_equal(got[GUARD : GUARD + total], want), "data or padding differs"
    assert (got[:GUARD] == HOLDER).all() and (got[GUARD + total :] == HOLDER).all()
    assert torch.equal(dev.cpu(), host), "a source was written"
    assert report["sums"] == reference(want.tobytes())
    assert report["paths"] == [case[3 - force] for case in cases]
    return report, outer


@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("force", [2, 1])
@pytest.mark.parametrize("es", [2, 4])
def test_slabs_among_the_other_kinds_in_one_arena(probe, source, es, force, cap):
    try:
        assert probe.pack_gather_checksum_grid_cap(cap) == (cap or 1024)
        _pack(probe, source, es, MIXED, force)
    finally:
        assert probe.pack_gather_checksum_grid_cap(0) == 1024


@pytest.mark.parametrize("name, es", [("w3x3_i33", 1), ("w3x3_i300", 2), ("w2x2_i70", 4),
                                      ("c31_i33", 8), ("four_d", 8)])
def test_one_slab_segment_equals_the_gather_kernel(probe, source, name, es):
    case = (lambda b, es: SLAB_CASES[name][0](b.view(DTYPES[es])), "slab", "direct")
    report, outer = _pack(probe, source, es, [case], 2)
    total = outer.numel() - 2 * GUARD
    other = _holder(total)
    try:
        probe.gather_checksum_path(2)
        alone = _gather(probe, case[0](source[1], es), other, total)
    finally:
        probe.gather_checksum_path(0)
    assert alone["path"] == "slab" and alone["sums"] == report["sums"]
    assert torch.equal(other, outer)
