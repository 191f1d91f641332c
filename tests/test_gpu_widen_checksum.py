"""MI355X tests for csp_widen_checksum_dev against numpy integer arithmetic on the bits (the
``_widen_bits`` model of the narrow kernel's tests); no tolerance."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_narrow_checksum import (  # noqa: E402
    PAIRS, _narrow_values, _sizes, _widen_bits, probe,  # noqa: F401  (probe: a fixture)
)
from test_gpu_pack_checksum import reference  # noqa: E402  (the numpy model of the sums)

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5  # a destination before the call
HOLDER = 0x3C  # what surrounds it


def _holder(nbytes):
    """A filled destination of ``nbytes`` between guards; the pointer is 16-byte aligned."""
    outer = torch.full((GUARD + nbytes + GUARD,), HOLDER, dtype=torch.uint8, device="cuda")
    outer[GUARD: GUARD + nbytes] = FILL
    return outer


def _source(probe, narrow, wire):
    """The narrow bytes on the device, the pad bytes of the rounded buffer set to 0xFF."""
    raw = narrow.view(np.uint8)
    dev = torch.full((probe.narrow_bytes(len(narrow), wire),), 0xFF, dtype=torch.uint8,
                     device="cuda")
    dev[: len(raw)] = torch.from_numpy(raw.copy()).cuda()
    return dev


# every size class, and with grid caps of 1 to 3 more tiles than workgroups
CASES = [(p, n, 0, n % 2 == 1) for p in PAIRS for e, w, t in [_sizes(p[1])]
         for n in (1, e - 1, e, e + 1, w - 1, w + 1, t - 1, t, t + 1, 2 * t + 3)] + [
    (p, 7 * _sizes(p[1])[2] + 5, cap, cap != 2) for p in PAIRS for cap in (1, 2, 3)]


@pytest.mark.parametrize("pair, n, cap, second", CASES)
def test_narrow_patterns_widen_to_the_model(probe, pair, n, cap, second):
    wide, wire = pair
    narrow = _narrow_values(wire, n, cap)
    want = _widen_bits(narrow, wide).view(np.uint8)
    dev = _source(probe, narrow, wire)
    before = dev.cpu().numpy()
    outs = [_holder(len(want)) for _ in range(2 if second else 1)]
    torch.cuda.synchronize()
    try:
        assert probe.widen_checksum_grid_cap(cap) == (cap or 1024)
        report = probe.widen_checksum_device(
            dev.data_ptr(), n, wire, wide, *(o.data_ptr() + GUARD for o in outs))
    finally:
        probe.widen_checksum_grid_cap(0)
    assert np.array_equal(dev.cpu().numpy(), before), "src changed"
    for outer in outs:  # dst, and dst2 identical to it
        got = outer.cpu().numpy()
        assert (got[:GUARD] == HOLDER).all() and (got[GUARD + len(want):] == HOLDER).all(), "guards"
        assert np.array_equal(got[GUARD: GUARD + len(want)], want), "data differs"
    sums = probe.checksum_device(outs[0].data_ptr() + GUARD, len(want))
    assert report["sum"] == reference(want.tobytes()) == tuple(sums)
    # the round trip: the narrow kernel gives the input back
    back = torch.zeros(probe.narrow_bytes(n, wire), dtype=torch.uint8, device="cuda")
    again = probe.narrow_checksum_device(
        outs[0].data_ptr() + GUARD, n, wide, wire, back.data_ptr(), back.numel())
    assert wire in again["fits"]
    assert np.array_equal(back.cpu().numpy()[: narrow.nbytes], narrow.view(np.uint8))


@pytest.mark.parametrize("change, text", [
    (dict(src_ptr=0), "null src or dst"), (dict(dst_ptr=0), "null src or dst"),
    (dict(wide="int32"), "no widening"), (dict(narrow="float32", wide="bfloat16"), "no widening"),
    (dict(src_off=4), "16-byte aligned"), (dict(dst_off=8), "16-byte aligned"),
    (dict(dst2_off=4), "16-byte aligned"), (dict(numel=(16 << 30) // 4 + 1), "16 GiB"),
    (dict(dst_on_src=2032), "overlap"), (dict(dst2_on_src=0), "overlap"),
    (dict(dst2_off=-2048), "overlap"),
])
def test_every_refusal_launches_nothing(probe, change, text):
    src = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    dst = torch.full((3 * 4096,), FILL, dtype=torch.uint8, device="cuda")
    call = dict(src_ptr=src.data_ptr(), numel=1024, narrow="bfloat16", wide="float32",
                dst_ptr=dst.data_ptr(), dst2_ptr=dst.data_ptr() + 4096)
    assert probe.widen_checksum_device(**call)["sum"] == (0, 0)  # the zeros, widened
    assert probe.widen_checksum_device(**{**call, "numel": 0, "dst_ptr": 0})["sum"] == (0, 0)
    dst.fill_(FILL)
    torch.cuda.synchronize()
    change = dict(change)
    for name in ("src", "dst", "dst2"):
        if name + "_off" in change:
            call[name + "_ptr"] += change.pop(name + "_off")
        if name + "_on_src" in change:
            call[name + "_ptr"] = src.data_ptr() + change.pop(name + "_on_src")
    with pytest.raises(probe.GpuLibError, match=text):
        probe.widen_checksum_device(**{**call, **change})
    assert (dst.cpu().numpy() == FILL).all() and not src.cpu().numpy().any()
