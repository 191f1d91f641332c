"""MI355X tests for csp_gather_checksum_dev.  Every case runs with the host's
path choice and with the direct path forced, against the same view operations
on the CPU copy followed by ``contiguous()``: exact, no tolerance."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_pack_checksum import reference  # noqa: E402  (the numpy model of the sums)

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5  # the destination before the call
HOLDER = 0x3C  # what surrounds it
DTYPES = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64, 16: torch.complex128}


def _shaped(f, *shape):
    return f[: int(np.prod(shape))].reshape(shape)


# name -> view of a flat typed tensor ``f``; ``es`` is its element size
CASES = {
    "t65x33": lambda f, es: _shaped(f, 65, 33).t(),
    "t64x64": lambda f, es: _shaped(f, 64, 64).t(),
    "t130x67": lambda f, es: _shaped(f, 130, 67).t(),
    "permute": lambda f, es: _shaped(f, 3, 17, 70).permute(2, 0, 1),
    "channels_last": lambda f, es: _shaped(f, 2, 5, 7, 3).permute(0, 3, 1, 2),
    # these stay 3-D and 4-D after collapsing, with U not next to C: R1, and R0 and R1
    "permute3d": lambda f, es: _shaped(f, 3, 41, 70)[:, :40].permute(2, 0, 1),
    "permute4d": lambda f, es: _shaped(f, 2, 3, 41, 70)[:, :, :40].permute(0, 3, 1, 2),
    "channels_last40": lambda f, es: _shaped(f, 3, 5, 11, 40).permute(0, 3, 1, 2),
    "cols2": lambda f, es: _shaped(f, 9, 40)[:, 1:2],
    "cols17": lambda f, es: _shaped(f, 9, 40)[:, 1:17],
    "cols33": lambda f, es: _shaped(f, 9, 40)[:, 1:33],
    "every2nd": lambda f, es: f[:301][::2],
    "sub2x3": lambda f, es: _shaped(f, 21, 31)[::2, ::3],
    "expand": lambda f, es: _shaped(f, 5, 1).expand(5, 19),
    "offset1": lambda f, es: f[1:38].reshape(1, 37, 1),
    # the output passes two 16 KiB tiles by a few elements
    "two_tiles": lambda f, es: _shaped(f, 100, 32768 // es // 100 + 1).t(),
}
TRANSPOSED = {"t65x33", "t64x64", "t130x67", "permute", "permute3d", "permute4d",
              "channels_last40", "two_tiles"}
PARAMS = [(name, es) for name in CASES for es in (1, 2, 4, 8)] + [("t130x67", 16)]


@pytest.fixture(scope="module")
def probe():
    from covalent_ssh_plugin_amd.gpu import probe as gpu_probe

    gpu_probe.load()  # GpuLibError if the extension was not built/shipped
    return gpu_probe


@pytest.fixture(scope="module")
def source():
    """Seeded random bytes on the host and their device copy, never written to."""
    gen = torch.Generator().manual_seed(20261126)
    host = torch.randint(0, 256, (1 << 18,), dtype=torch.uint8, generator=gen)
    dev = host.cuda()
    torch.cuda.synchronize()
    return host, dev


def _holder(total):
    outer = torch.full((GUARD + total + GUARD,), HOLDER, dtype=torch.uint8, device="cuda")
    outer[GUARD : GUARD + total] = FILL
    torch.cuda.synchronize()
    assert (outer.data_ptr() + GUARD) % 16 == 0
    return outer


def _gather(probe, view, outer, total):
    return probe.gather_checksum_device(
        view.data_ptr(), view.element_size(), list(view.shape), list(view.stride()),
        outer.data_ptr() + GUARD, total,
    )


def _gather_and_check(probe, source, name, es):
    """Both paths on one case, every property; the host's choice is returned."""
    host, dev = source
    want_view = CASES[name](host.view(DTYPES[es]), es)
    view = CASES[name](dev.view(DTYPES[es]), es)
    assert view.stride() == want_view.stride()
    flat = want_view.contiguous()
    want = (torch.view_as_real(flat) if es == 16 else flat).reshape(-1).view(torch.uint8).numpy()
    total = (len(want) + 15) // 16 * 16
    reports = []
    try:
        for force in (0, 1):
            assert probe.gather_checksum_path(force) == force
            outer = _holder(total)
            report = _gather(probe, view, outer, total)
            got = outer.cpu().numpy()
            arena = got[GUARD : GUARD + total]
            assert np.array_equal(arena[: len(want)], want), "data differs"
            assert not arena[len(want) :].any(), "padding is not zero"
            assert (got[:GUARD] == HOLDER).all() and (got[GUARD + total :] == HOLDER).all()
            assert report["sums"] == reference(arena.tobytes())
            assert report["sums"] == probe.checksum_device(outer.data_ptr() + GUARD, total)
            reports.append(report)
    finally:
        probe.gather_checksum_path(0)
    assert torch.equal(dev.cpu(), host), "the source was written"
    assert reports[1]["path"] == "direct" and reports[0]["sums"] == reports[1]["sums"]
    return reports[0]


@pytest.mark.parametrize("name, es", PARAMS)
def test_both_paths_against_contiguous_on_the_cpu(probe, source, name, es):
    path = _gather_and_check(probe, source, name, es)["path"]
    assert path == ("transpose" if name in TRANSPOSED else "direct")


@pytest.mark.parametrize("cap", [1, 2, 3])
@pytest.mark.parametrize("name, es", [("two_tiles", 1), ("permute4d", 4)])  # the most tiles
def test_blocks_loop_over_tiles_and_patches_under_small_grid_caps(probe, source, name, es, cap):
    try:
        assert probe.gather_checksum_grid_cap(cap) == cap
        assert _gather_and_check(probe, source, name, es)["path"] == "transpose"
    finally:
        assert probe.gather_checksum_grid_cap(0) == 1024


def test_default_cap_with_more_patches_than_blocks(probe):
    gen = torch.Generator().manual_seed(5)
    host = torch.randint(-(1 << 15), 1 << 15, (1100, 1100), dtype=torch.int16, generator=gen)
    dev = host.cuda()
    torch.cuda.synchronize()
    want = host.t().contiguous().view(torch.uint8).reshape(-1).numpy()
    outer = _holder(len(want))
    report = _gather(probe, dev.t(), outer, len(want))
    assert report["path"] == "transpose"  # 18 x 18 patches of 64 x 64
    got = outer.cpu().numpy()
    assert np.array_equal(got[GUARD : GUARD + len(want)], want)
    assert (got[:GUARD] == HOLDER).all() and (got[GUARD + len(want) :] == HOLDER).all()
    assert report["sums"] == reference(want.tobytes())


def test_path_reports_the_16_byte_sub_path(probe, source):
    # a unit-stride inner run of whole, aligned vectors: 16-byte loads
    host, dev = source
    view = _shaped(dev.view(torch.int32), 8, 64)[:, :32]
    outer = _holder(8 * 32 * 4)
    assert _gather(probe, view, outer, 8 * 32 * 4)["path"] == "direct16"
    want = _shaped(host.view(torch.int32), 8, 64)[:, :32].contiguous().view(torch.uint8)
    assert np.array_equal(outer.cpu().numpy()[GUARD:-GUARD], want.reshape(-1).numpy())


def test_no_element_and_ranges_that_touch(probe, source):
    host, dev = source
    outer = _holder(32)
    dst = outer.data_ptr() + GUARD
    report = probe.gather_checksum_device(dev.data_ptr(), 4, [3, 0], [1, 1], dst, 0)
    assert report["sums"] == (0, 0) and report["path"] == "none"
    # the source ends where the destination begins
    report = probe.gather_checksum_device(dst - 32, 1, [32], [1], dst, 32)
    got = outer.cpu().numpy()
    assert (got[GUARD : GUARD + 32] == HOLDER).all() and (got[GUARD + 32 :] == HOLDER).all()
    assert report["sums"] == reference(bytes([HOLDER]) * 32)


def _refusals(src, dst):
    five = [1152, 192, 48, 8, 2]  # every second element of (4, 6, 4, 6, 4) in each dimension
    return {
        "elem_size 3": (src, 3, [16], [1], dst, 48),
        "5 dimensions are left": (src, 1, [2, 3, 2, 3, 2], five, dst, 80),
        "9 dimensions": (src, 1, [1] * 8 + [16], [1] * 9, dst, 16),
        "null or not 16-byte aligned": (src, 1, [16], [1], 0, 16),
        "not 16-byte aligned": (src, 1, [16], [1], dst + 8, 16),
        "not aligned to 4 bytes": (src + 2, 4, [4], [1], dst, 16),
        "dst_bytes is 48": (src, 1, [16], [1], dst, 48),
        "above 16 GiB": (src, 1, [(1 << 34) + 16], [1], dst, (1 << 34) + 16),
        "overflows": (src, 8, [2], [1 << 63], dst, 16),
        "overlap": (dst + 8, 1, [8], [2], dst, 16),
    }


@pytest.mark.parametrize("message", list(_refusals(0, 0)))
def test_refusals_launch_nothing(probe, source, message):
    outer = _holder(256)
    args = _refusals(source[1].data_ptr(), outer.data_ptr() + GUARD)[message]
    with pytest.raises(probe.GpuLibError, match=r"rc=-1\): csp_gather_checksum_dev: .*" + message):
        probe.gather_checksum_device(*args)
    got = outer.cpu().numpy()
    assert (got[GUARD:-GUARD] == FILL).all() and (got[:GUARD] == HOLDER).all()
    assert (got[-GUARD:] == HOLDER).all()
