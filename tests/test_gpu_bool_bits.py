"""MI355X tests for csp_bool_pack_checksum_dev and csp_bool_unpack_checksum_dev against
``numpy.packbits`` / ``numpy.unpackbits`` with ``bitorder="little"``; no tolerance."""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_pack_checksum import reference  # noqa: E402  (the numpy model of the sums)

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5  # a destination before the call
HOLDER = 0x3C  # what surrounds it
STEP, TRIP = 8192, 32768  # bool elements of a wave step and of a workgroup trip
# an output vector, a wave step and a trip minus and plus one, two and three trips and a few;
# and with grid caps of 1 to 3 five trips, more than there are workgroups
CASES = [(n, 0) for n in (1, 7, 8, 9, 127, 128, 129, STEP - 1, STEP, STEP + 1, TRIP - 1, TRIP,
                          TRIP + 1, 2 * TRIP + 5, 3 * TRIP + 9)] + [
    (5 * TRIP - 3, cap) for cap in (1, 2, 3)]


@pytest.fixture(scope="module")
def probe():
    from covalent_ssh_plugin_amd.gpu import probe as gpu_probe

    gpu_probe.load()  # GpuLibError if the extension was not built/shipped
    return gpu_probe


def _bools(n):
    """``n`` random bool bytes with the first and the last element set."""
    x = np.random.default_rng(n).integers(0, 2, n).astype(np.uint8)
    x[0] = x[-1] = 1
    return x


def _holder(nbytes):
    """A filled destination of ``nbytes`` between guards; the pointer is 16-byte aligned."""
    outer = torch.full((GUARD + nbytes + GUARD,), HOLDER, dtype=torch.uint8, device="cuda")
    outer[GUARD: GUARD + nbytes] = FILL
    torch.cuda.synchronize()
    return outer


def _inside(outer, nbytes):
    got = outer.cpu().numpy()
    assert (got[:GUARD] == HOLDER).all() and (got[GUARD + nbytes:] == HOLDER).all(), "guards"
    return got[GUARD: GUARD + nbytes]


@pytest.mark.parametrize("n, cap", CASES)
def test_bool_bytes_pack_to_numpy_packbits(probe, n, cap):
    x = _bools(n)
    dev = torch.from_numpy(x.copy()).cuda().view(torch.bool)
    total = probe.bool_bits_bytes(n)
    want = np.zeros(total, dtype=np.uint8)
    want[: (n + 7) // 8] = np.packbits(x, bitorder="little")
    outer = _holder(total)
    try:
        assert probe.bool_pack_checksum_grid_cap(cap) == (cap or 1024)
        report = probe.bool_pack_checksum_device(dev.data_ptr(), n, outer.data_ptr() + GUARD, total)
        probed = probe.bool_pack_checksum_device(dev.data_ptr(), n)
    finally:
        probe.bool_pack_checksum_grid_cap(0)
    assert report["bad"] == 0 and probed["bad"] == 0 and probed["sum"] == (0, 0)
    assert np.array_equal(_inside(outer, total), want), "bits differ, or the padding is not zero"
    sums = probe.checksum_device(outer.data_ptr() + GUARD, total)
    assert report["sum"] == reference(want.tobytes()) == tuple(sums)
    assert np.array_equal(dev.view(torch.uint8).cpu().numpy(), x), "src changed"


@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("n, cap", CASES)
def test_bits_unpack_to_numpy_unpackbits_and_pack_back(probe, n, cap, second):
    x = _bools(n)
    bits = np.full(probe.bool_bits_bytes(n), 0xFF, dtype=np.uint8)  # pad bytes and pad bits set
    bits[: (n + 7) // 8] = np.packbits(x, bitorder="little")
    if n % 8:
        bits[n // 8] |= (0xFF << (n % 8)) & 0xFF
    want = np.unpackbits(bits, bitorder="little", count=n)
    assert np.array_equal(want, x)
    dev = torch.from_numpy(bits.copy()).cuda()
    outs = [_holder(n) for _ in range(2 if second else 1)]
    try:
        assert probe.bool_unpack_checksum_grid_cap(cap) == (cap or 1024)
        report = probe.bool_unpack_checksum_device(
            dev.data_ptr(), n, *(o.data_ptr() + GUARD for o in outs))
    finally:
        probe.bool_unpack_checksum_grid_cap(0)
    assert np.array_equal(dev.cpu().numpy(), bits), "src changed"
    for outer in outs:  # dst, and dst2 identical to it
        assert np.array_equal(_inside(outer, n), want), "data differs"
    sums = probe.checksum_device(outs[0].data_ptr() + GUARD, n)
    assert report["sum"] == reference(want.tobytes()) == tuple(sums)
    # the round trip: the pack kernel gives the bits back, the pad bits zero
    back = torch.full((len(bits),), FILL, dtype=torch.uint8, device="cuda")
    again = probe.bool_pack_checksum_device(
        outs[0].data_ptr() + GUARD, n, back.data_ptr(), len(bits))
    assert again["bad"] == 0
    assert np.array_equal(back.cpu().numpy()[: (n + 7) // 8], np.packbits(x, bitorder="little"))


@pytest.mark.parametrize("poison", [2, 0x80, 0xFF])
def test_a_byte_that_is_neither_0_nor_1_sets_bad(probe, poison):
    n = 2 * TRIP + 5
    total = probe.bool_bits_bytes(n)
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    for at in (0, n - 1, TRIP - 1, TRIP):
        x = _bools(n)
        x[at] = poison
        dev = torch.from_numpy(x).cuda().view(torch.bool)  # a uint8 tensor viewed as bool
        assert probe.bool_pack_checksum_device(dev.data_ptr(), n)["bad"] == poison & 0xFE, at
        stored = probe.bool_pack_checksum_device(dev.data_ptr(), n, out.data_ptr(), total)
        assert stored["bad"] == poison & 0xFE, at


@pytest.mark.parametrize("change, text", [
    (dict(sums=False), "null output"), (dict(bad=False), "null output"),
    (dict(src_ptr=0), "null src"), (dict(src_off=4), "16-byte aligned"),
    (dict(dst_off=8), "16-byte aligned"), (dict(dst_bytes=112), "need 128"),
    (dict(numel=(16 << 30) + 1, dst_bytes=(2 << 30) + 16), "16 GiB"),
    (dict(dst_on_src=896), "overlap"),
])
def test_every_pack_refusal_launches_nothing(probe, change, text):
    lib = probe.load()
    src = torch.ones(4096, dtype=torch.uint8, device="cuda")
    dst = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    call = dict(src_ptr=src.data_ptr(), numel=1000, dst_ptr=dst.data_ptr(), dst_bytes=128)
    assert probe.bool_pack_checksum_device(**call)["bad"] == 0
    empty = probe.bool_pack_checksum_device(**{**call, "numel": 0, "src_ptr": 0, "dst_bytes": 0})
    assert empty["sum"] == (0, 0) and empty["bad"] == 0
    dst.fill_(FILL)
    torch.cuda.synchronize()
    change = dict(change)
    sums = (ctypes.c_uint64 * 2)() if change.pop("sums", True) else None
    bad = ctypes.byref(ctypes.c_uint32()) if change.pop("bad", True) else None
    call["src_ptr"] += change.pop("src_off", 0)
    call["dst_ptr"] += change.pop("dst_off", 0)
    if "dst_on_src" in change:
        call["dst_ptr"] = src.data_ptr() + change.pop("dst_on_src")
    call.update(change)
    rc = lib.csp_bool_pack_checksum_dev(
        ctypes.c_void_p(call["src_ptr"] or None), call["numel"], ctypes.c_void_p(call["dst_ptr"]),
        call["dst_bytes"], sums, bad, None)
    assert rc == -1 and text in lib.csp_last_error().decode()
    assert (dst.cpu().numpy() == FILL).all() and (src.cpu().numpy() == 1).all()


@pytest.mark.parametrize("change, text", [
    (dict(src_ptr=0), "null src or dst"), (dict(dst_ptr=0), "null src or dst"),
    (dict(src_off=2), "16-byte aligned"), (dict(dst_off=8), "16-byte aligned"),
    (dict(dst2_off=4), "16-byte aligned"), (dict(numel=(16 << 30) + 1), "16 GiB"),
    (dict(dst_on_src=112), "overlap"), (dict(dst2_on_src=0), "overlap"),
    (dict(dst2_off=-1056), "overlap"),  # its first 8 bytes are dst's last
])
def test_every_unpack_refusal_launches_nothing(probe, change, text):
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.full((3 * 2048,), FILL, dtype=torch.uint8, device="cuda")
    call = dict(src_ptr=src.data_ptr(), numel=1000, dst_ptr=dst.data_ptr(),
                dst2_ptr=dst.data_ptr() + 2048)
    assert probe.bool_unpack_checksum_device(**call)["sum"] == (0, 0)  # the zeros, unpacked
    assert probe.bool_unpack_checksum_device(**{**call, "numel": 0, "dst_ptr": 0})["sum"] == (0, 0)
    dst.fill_(FILL)
    torch.cuda.synchronize()
    change = dict(change)
    for name in ("src", "dst", "dst2"):
        if name + "_off" in change:
            call[name + "_ptr"] += change.pop(name + "_off")
        if name + "_on_src" in change:
            call[name + "_ptr"] = src.data_ptr() + change.pop(name + "_on_src")
    with pytest.raises(probe.GpuLibError, match=text):
        probe.bool_unpack_checksum_device(**{**call, **change})
    assert (dst.cpu().numpy() == FILL).all() and not src.cpu().numpy().any()
