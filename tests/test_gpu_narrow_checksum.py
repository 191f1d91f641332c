"""MI355X tests for csp_narrow_checksum_dev against numpy integer arithmetic on the bits: a
narrow pattern is widened to the source's bits, the kernel has to give it back; no tolerance."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_pack_checksum import reference  # noqa: E402  (the numpy model of the sums)

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5  # the destination before the call
HOLDER = 0x3C  # what surrounds it
PAIRS = [("float32", "bfloat16"), ("float64", "float32"), ("int64", "int32"), ("int64", "int16"),
         ("int64", "uint8"), ("int32", "int16"), ("int32", "uint8")]
# the integer type that carries each kind's bits
BITS = {"float32": np.uint32, "float64": np.uint64, "int32": np.int32, "int64": np.int64,
        "bfloat16": np.uint16, "int16": np.int16, "uint8": np.uint8}
# +-0, +-inf, a quiet NaN with payload, largest and smallest normal, (bf16) subnormals
EDGES = {"bfloat16": [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC1, 0x7F7F, 0x0080, 0x0001, 0x807F],
         "float32": [0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0x7F7FFFFF, 0x00800000]}
POISONS = {  # inexact source bits: bit 0, 15; bit 28, 2^-127, 2^128, a signalling NaN; limits
    "float32": [0x3F800001, 0x3F808000],
    "float64": [1023 << 52 | 1 << 28, 896 << 52, 1151 << 52, 0x7FF4 << 48],
    "int32": [1 << 31, -(1 << 31) - 1], "int16": [1 << 15, -(1 << 15) - 1], "uint8": [-1, 256],
}


def _sizes(dst):
    e = 16 // np.dtype(BITS[dst]).itemsize  # elements per output vector, wave step and tile
    return e, 64 * e, 1024 * e


def _narrow_values(dst, n, seed=7):
    """``n`` patterns of ``dst`` whose widening is exact, edges first and last."""
    rng = np.random.default_rng(seed + n)
    kind = BITS[dst]
    if dst == "float32":  # normals only between the edges
        vals = (rng.integers(0, 2, n) << 31 | rng.integers(1, 255, n) << 23
                | rng.integers(0, 1 << 23, n)).astype(kind)
    else:
        info = np.iinfo(kind)
        vals = rng.integers(info.min, info.max + 1, n).astype(kind)
    edges = np.array(EDGES.get(dst, [np.iinfo(kind).min, np.iinfo(kind).max])).astype(kind)
    k = min(n, len(edges))
    vals[:k] = edges[:k]
    vals[n - k:] = edges[len(edges) - k:]
    return vals


def _widen_bits(narrow, src):
    """The source's bits of the same values, by shifts and integer casts."""
    if src == "float32":
        return narrow.astype(np.uint32) << 16
    if src == "float64":
        x = narrow.astype(np.uint64)
        e, m = (x >> 23) & 0xFF, x & 0x7FFFFF
        e64 = np.where(e == 0, 0, np.where(e == 255, 0x7FF, e + 896)).astype(np.uint64)
        return (x >> 31) << 63 | e64 << 52 | m << 29
    return narrow.astype(BITS[src])


@pytest.fixture(scope="module")
def probe():
    from covalent_ssh_plugin_amd.gpu import probe as gpu_probe

    gpu_probe.load()  # GpuLibError if the extension was not built/shipped
    return gpu_probe


def _run(probe, pair, bits):
    """One narrowing call on ``bits`` and a probe that must agree with it."""
    src, dst = pair
    dev = torch.from_numpy(bits.view(np.uint8).copy()).cuda()
    total = probe.narrow_bytes(len(bits), dst)
    outer = torch.full((GUARD + total + GUARD,), HOLDER, dtype=torch.uint8, device="cuda")
    outer[GUARD: GUARD + total] = FILL
    torch.cuda.synchronize()
    report = probe.narrow_checksum_device(
        dev.data_ptr(), len(bits), src, dst, outer.data_ptr() + GUARD, total)
    assert probe.narrow_checksum_device(dev.data_ptr(), len(bits), src)["fits"] == report["fits"]
    assert np.array_equal(dev.cpu().numpy(), bits.view(np.uint8)), "src changed"
    got = outer.cpu().numpy()
    assert (got[:GUARD] == HOLDER).all() and (got[GUARD + total:] == HOLDER).all(), "guards"
    return report, outer, got[GUARD: GUARD + total]


# every size class, and with grid caps of 1 to 3 more tiles than workgroups
CASES = [(p, n, 0) for p in PAIRS for e, w, t in [_sizes(p[1])]
         for n in (1, e - 1, e, e + 1, w - 1, w + 1, t - 1, t, t + 1, 2 * t + 3)] + [
    (p, 7 * _sizes(p[1])[2] + 5, cap) for p in PAIRS for cap in (1, 2, 3)]


@pytest.mark.parametrize("pair, n, cap", CASES)
def test_exact_sources_narrow_to_the_model(probe, pair, n, cap):
    from covalent_ssh_plugin_amd.remote.workers import widen_result

    src, dst = pair
    narrow = _narrow_values(dst, n, cap)
    bits = _widen_bits(narrow, src)
    try:
        assert probe.narrow_checksum_grid_cap(cap) == (cap or 1024)
        report, outer, arena = _run(probe, pair, bits)
    finally:
        probe.narrow_checksum_grid_cap(0)
    want = narrow.view(np.uint8)
    assert dst in report["fits"]
    assert np.array_equal(arena[: len(want)], want), "data differs"
    assert not arena[len(want):].any(), "padding"
    sums = probe.checksum_device(outer.data_ptr() + GUARD, len(want))
    assert report["sum"] == reference(want.tobytes()) == tuple(sums)
    wide = widen_result(bytearray(arena[: len(want)]), {"wire": dst, "dtype": src, "shape": [-1]})
    assert str(wide.dtype) == "torch." + src
    assert np.array_equal(wide.view(torch.uint8).numpy(), bits.view(np.uint8)), "round trip"


@pytest.mark.parametrize(
    "pair, poison",
    [(p, x) for p in PAIRS for x in POISONS[p[0] if p[0].startswith("float") else p[1]]])
def test_one_inexact_element_clears_the_bit(probe, pair, poison):
    t = _sizes(pair[1])[2]
    n = 2 * t + 3
    for at in (0, n - 1, t - 1, t):
        bits = _widen_bits(_narrow_values(pair[1], n), pair[0])
        bits[at] = np.array(poison).astype(bits.dtype)
        report, _, _ = _run(probe, pair, bits)
        assert pair[1] not in report["fits"], at


@pytest.mark.parametrize("src", ["int64", "int32"])
@pytest.mark.parametrize("bound", [1 << 7, 1 << 8, 1 << 14, 1 << 20, 1 << 40])
@pytest.mark.parametrize("signed", [False, True])
def test_the_probe_finds_every_exact_width_and_stores_nothing(probe, src, bound, signed):
    bound = min(bound, np.iinfo(BITS[src]).max)
    n = 3 * 4096 + 1
    vals = np.random.default_rng(bound).integers(-bound if signed else 0, bound, n)
    vals[n // 2] = bound - 1
    vals[-1] = -bound if signed else 0
    vals = vals.astype(BITS[src])
    want = tuple(d for d in probe.NARROW_TARGETS[src]
                 if np.iinfo(BITS[d]).min <= vals.min() and vals.max() <= np.iinfo(BITS[d]).max)
    dev = torch.from_numpy(vals).cuda()
    report = probe.narrow_checksum_device(dev.data_ptr(), n, src)
    assert report["fits"] == want and report["sum"] == (0, 0)


def test_refusals_and_the_empty_source(probe):
    src, dst = (torch.zeros(n + 64, dtype=torch.uint8, device="cuda") for n in (4096, 2048))
    good = dict(src_ptr=src.data_ptr(), numel=1024, src="float32", dst="bfloat16",
                dst_ptr=dst.data_ptr(), dst_bytes=2048)
    assert probe.narrow_checksum_device(**good)["fits"] == ("bfloat16",)
    bad = [
        (dict(src_ptr=0), "null src"),
        (dict(dst="int16"), "no narrowing"),
        (dict(src="int16", dst_ptr=0), "no narrowing"),
        (dict(src_ptr=src.data_ptr() + 4), "16-byte aligned"),
        (dict(dst_ptr=dst.data_ptr() + 8), "16-byte aligned"),
        (dict(dst_bytes=2040), "need 2048"),
        (dict(numel=(16 << 30) // 4 + 1, dst_bytes=(8 << 30) + 16), "16 GiB"),
        (dict(dst_ptr=src.data_ptr() + 2048), "overlap"),
    ]
    for change, text in bad:
        with pytest.raises(probe.GpuLibError, match=text):
            probe.narrow_checksum_device(**{**good, **change})
    empty = probe.narrow_checksum_device(**{**good, "numel": 0, "src": "int64", "dst": "int16"})
    assert empty["fits"] == ("uint8", "int16", "int32") and empty["sum"] == (0, 0)
