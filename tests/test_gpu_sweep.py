"""MI355X tests for what the HBM sweep kernel copies.  ``csp_hbm_sweep_t`` is
the warm-up and the kernel behind ``hbm_bw_gbps``; a variant that skipped its
remainder loop or stopped a stride early would report a higher bandwidth.
``csp_hbm_sweep_dev`` launches it through the probe's own variant switch on
the caller's buffers, so every variant is checked here for an exact copy at
the sizes where its unrolled loop hands over to the single-stride loop."""

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_BYTE = 0xA5
VARIANTS = [-1, 0, 1, 2, 3, 4, 9]  # -1: the probe's default; 9: unknown, runs variant 0
BLOCKS = [1, 3]
PROBE_BLOCKS = 1024  # run_hbm_sweep's grid


def vector_counts(stride, unroll):
    """n4 around one stride, around one unrolled trip, with 1 stride left
    after it, and ragged after two and before three."""
    return sorted({
        0, 1, stride - 1, stride, stride + 1, unroll * stride - 1, unroll * stride,
        unroll * stride + 1, (unroll + 1) * stride, 2 * unroll * stride + stride + 7,
        3 * unroll * stride - 1,
    })


MAX_SMALL_BYTES = 16 * max(vector_counts(256 * max(BLOCKS), 8))
MAX_PROBE_BYTES = 16 * (PROBE_BLOCKS * 256 * 8 + PROBE_BLOCKS * 256 + 3)


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
    """Seeded random float32 bit patterns, made as random bytes so that NaN
    payloads, infinities and denormals are among them; the device buffer and
    a device copy to compare it with afterwards.  Never written to."""
    gen = torch.Generator().manual_seed(20250119)
    host = torch.randint(0, 256, (MAX_PROBE_BYTES,), dtype=torch.uint8, generator=gen)
    as_float = host[: MAX_SMALL_BYTES].view(torch.float32)
    assert bool(torch.isnan(as_float).any()), "the source holds no NaN pattern"
    dev = host.cuda()
    pristine = dev.clone()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    return dev, pristine


@pytest.fixture
def sweep_variant(probe):
    """Setter for the probe's sweep variant; the shipped default is back
    afterwards, whatever happened."""
    try:
        yield probe.set_sweep_variant
    finally:
        probe.set_sweep_variant(probe.SWEEP_VARIANT_DEFAULT)


def _unroll(probe, variant, default=None):
    if variant < 0:
        variant = probe.SWEEP_VARIANT_DEFAULT if default is None else default
    return probe.SWEEP_UNROLL.get(variant, probe.SWEEP_UNROLL[0])


class _Target:
    """A guarded destination and the image it must hold after a sweep."""

    def __init__(self, max_bytes):
        self.buf = torch.empty(GUARD + max_bytes + GUARD, dtype=torch.uint8, device="cuda")
        self.image = torch.empty_like(self.buf)
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def check(self, probe, variant, src, n4, blocks):
        """None, or what went wrong."""
        nbytes = 16 * n4
        self.buf.fill_(GUARD_BYTE)
        self.image.fill_(GUARD_BYTE)
        self.image[GUARD : GUARD + nbytes] = src[:nbytes]
        torch.cuda.synchronize()
        probe.hbm_sweep_device(variant, src.data_ptr(), self.ptr, n4, blocks)
        if torch.equal(self.buf, self.image):
            return None
        at = int((self.buf != self.image).nonzero()[0]) - GUARD
        where = "before dst" if at < 0 else "past dst" if at >= nbytes else "in dst"
        return f"first wrong byte at offset {at} ({where}), vector {at // 16} of {n4}"


def _sweep_edges(probe, target, src, variant, unroll):
    failures = []
    for blocks in BLOCKS:
        for n4 in vector_counts(256 * blocks, unroll):
            wrong = target.check(probe, variant, src, n4, blocks)
            if wrong:
                failures.append(((variant, blocks, n4), wrong))
    return failures


@pytest.mark.parametrize("variant", VARIANTS)
def test_sweep_copies_exactly_at_loop_edges(probe, source, variant):
    dev, pristine = source
    target = _Target(MAX_SMALL_BYTES)
    failures = _sweep_edges(probe, target, dev, variant, _unroll(probe, variant))
    assert not failures, f"{len(failures)} (variant, blocks, n4) differ, first: {failures[0]}"
    assert torch.equal(dev, pristine), "the source changed"


@pytest.mark.parametrize("variant", VARIANTS)
def test_sweep_copies_exactly_at_the_probe_geometry(probe, source, variant):
    """1024 blocks as in the probe: one unrolled trip for every lane, one
    single-stride trip for every lane, and three more vectors."""
    dev, pristine = source
    unroll = _unroll(probe, variant)
    n4 = PROBE_BLOCKS * 256 * unroll + PROBE_BLOCKS * 256 + 3
    target = _Target(16 * n4)
    wrong = target.check(probe, variant, dev, n4, PROBE_BLOCKS)
    assert wrong is None, (variant, n4, wrong)
    assert torch.equal(dev, pristine), "the source changed"


@pytest.mark.parametrize("chosen", [0, 1, 2, 3, 4])
def test_default_variant_follows_set_sweep_variant(probe, source, sweep_variant, chosen):
    """variant -1 runs whatever csp_set_sweep_variant chose: at the sizes
    built around that variant's unroll the copy stays exact."""
    dev, pristine = source
    sweep_variant(chosen)
    target = _Target(MAX_SMALL_BYTES)
    failures = _sweep_edges(probe, target, dev, -1, _unroll(probe, -1, default=chosen))
    assert not failures, f"{len(failures)} (variant, blocks, n4) differ, first: {failures[0]}"
    assert torch.equal(dev, pristine), "the source changed"


def test_refused_calls_launch_nothing(probe, source):
    dev, _pristine = source
    target = _Target(4096)
    target.buf.fill_(GUARD_BYTE)
    torch.cuda.synchronize()
    with pytest.raises(probe.GpuLibError, match="16-byte aligned"):
        probe.hbm_sweep_device(0, dev.data_ptr() + 4, target.ptr, 16, 1)
    with pytest.raises(probe.GpuLibError, match="16-byte aligned"):
        probe.hbm_sweep_device(0, dev.data_ptr(), target.ptr + 8, 16, 1)
    for blocks in (0, -1):
        with pytest.raises(probe.GpuLibError, match="less than 1"):
            probe.hbm_sweep_device(0, dev.data_ptr(), target.ptr, 16, blocks)
    assert bool((target.buf == GUARD_BYTE).all()), "a refused call wrote"
    # the library is fine afterwards
    assert target.check(probe, 0, dev, 16, 1) is None
