"""``narrow_tensor_args`` without a GPU: ``csp_io_narrow`` against numpy integer arithmetic on the
bits, the argument meta of ``extract_arg_buffers`` and the option's validation."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_narrow_checksum import (  # noqa: E402  (value helpers only: no GPU is touched)
    BITS, PAIRS, POISONS, _narrow_values, _sizes, _widen_bits,
)

from covalent_ssh_plugin_amd.remote import workers  # noqa: E402
from covalent_ssh_plugin_amd.transport import native_io  # noqa: E402

CHUNK = 4096  # a chunk boundary inside the larger cases


def _narrow_all(bits, src, dst, chunk=CHUNK):
    """``csp_io_narrow`` over ``chunk``-byte pieces: (the ORed bad word, the narrow bytes)."""
    es, nes = bits.itemsize, native_io.NARROW_ELEM_SIZE[dst]
    raw, out, bad = bytearray(bits.tobytes()), bytearray(len(bits) * nes), 0
    for off in range(0, len(raw), chunk):
        n = min(chunk, len(raw) - off) // es
        bad |= native_io.narrow(raw, n, src, dst, out, off, off // es * nes)
        assert native_io.narrow(raw, n, src, dst, None, off) == \
            native_io.narrow(bytes(raw), n, src, dst, None, off), "test pass, read-only source"
    return bad, np.frombuffer(out, dtype=BITS[dst])


@pytest.mark.parametrize("pair", PAIRS)
def test_csp_io_narrow_gives_the_narrow_patterns_and_refuses_every_poison(pair):
    src, dst = pair
    e = _sizes(dst)[0]
    poisons = POISONS[src if src.startswith("float") else dst]
    for n in (1, e, e + 1, 3 * CHUNK // BITS[src]().itemsize + 1):
        narrow = _narrow_values(dst, n)
        bits = _widen_bits(narrow, src)
        bad, got = _narrow_all(bits, src, dst)
        assert dst in native_io.narrow_fits(src, bad)
        assert np.array_equal(got, narrow)
        for poison in poisons:
            for at in {0, n - 1}:
                spoiled = bits.copy()
                spoiled[at] = np.array(poison).astype(bits.dtype)
                assert dst not in native_io.narrow_fits(src, _narrow_all(spoiled, src, dst)[0])
    for poison in poisons:  # alone
        alone = np.array([poison]).astype(BITS[src])
        assert dst not in native_io.narrow_fits(src, _narrow_all(alone, src, dst)[0])
    with pytest.raises(ValueError, match="no narrowing"):
        native_io.narrow(bytearray(16), 1, dst, src)


@pytest.mark.parametrize("src, bad, fits", [
    ("float32", 0, ("bfloat16",)), ("float32", 1, ()), ("float64", 0, ("float32",)),
    ("float64", 1 << 63, ()), ("int64", 0, ("uint8", "int16", "int32")),
    ("int64", 255, ("uint8", "int16", "int32")), ("int64", 256, ("int16", "int32")),
    ("int64", 1 << 63 | 127, ("int16", "int32")), ("int64", (1 << 15) - 1, ("int16", "int32")),
    ("int64", 1 << 15, ("int32",)), ("int64", 1 << 63 | (1 << 31) - 1, ("int32",)),
    ("int64", 1 << 31, ()), ("int32", 255, ("uint8", "int16")), ("int32", 1 << 63, ("int16",)),
    ("int32", 1 << 15, ()), ("int16", 0, ()),
])
def test_narrow_fits_agrees_with_the_kernel_table(src, bad, fits):
    assert native_io.narrow_fits(src, bad) == fits


def _meta(tensor, threshold, **options):
    _, _, meta, buffers = workers.extract_arg_buffers(
        [tensor], {}, threshold, to_device=True, **options)
    return meta[0], buffers[0]


def test_extract_marks_exact_tensors_and_leaves_the_rest_alone():
    n = 3 * workers.ARG_CACHE_CHUNK // 8 + 5  # several pieces on the thread pool
    exact = torch.arange(n, dtype=torch.int64) % 30000 - 15000
    inexact = torch.arange(n, dtype=torch.float32) / 3
    small = torch.arange(64, dtype=torch.int64)
    stats = {}
    for tensor, wire in ((exact, "int16"), (inexact, None), (small, None)):
        off, (view_off, _) = _meta(tensor, 1024)
        on, (view_on, keep) = _meta(tensor, 1024, narrow=True, narrow_stats=stats)
        assert on.pop("wire", None) == wire and on == off
        if wire is None:
            assert bytes(view_on) == bytes(view_off)
            continue
        assert bytes(view_on) == tensor.to(torch.int16).numpy().tobytes()
        assert bytes(keep[1]) == bytes(view_off), "the wide view is kept"
    assert stats["arg_narrowed"] == 1 and stats["arg_narrow_saved_bytes"] == 6 * n
    assert stats["arg_narrow_ms"] > 0
    # cacheable: decided when the bytes travel, so only marked here, same sum and key
    off, _ = _meta(exact, 1024, cache_min_bytes=4096)
    on, (view, _) = _meta(exact, 1024, cache_min_bytes=4096, narrow=True)
    assert on["cache"].pop("narrow") is True and on == off and "wire" not in on
    assert len(view) == 8 * n


def test_the_cache_send_narrows_a_store_and_never_a_ref():
    import cloudpickle

    tensor = torch.arange(4096, dtype=torch.int64) % 200
    _, _, meta, buffers = workers.extract_arg_buffers(
        [tensor], {}, 1024, to_device=True, cache_min_bytes=4096, narrow=True)
    handle = type("Handle", (), {"resident": set(), "resident_arenas": {}})()
    stats = {}
    send = workers._ArgCacheSend(handle, {}, meta, [buffers[0][0]], stats)
    request, frame = list(send.frames(full=False))
    (entry,) = cloudpickle.loads(request)["arg_buffers"]
    assert entry["wire"] == "uint8" and entry["cache"] == {"key": meta[0]["cache"]["key"],
                                                           "store": True}
    assert bytes(frame) == tensor.to(torch.uint8).numpy().tobytes() and stats["arg_narrowed"] == 1
    assert len(send.views[0]) == 8 * 4096, "the wide view stays for result deltas"
    (request,) = list(send.frames(full=False))  # resident now: a reference, nothing narrowed
    (entry,) = cloudpickle.loads(request)["arg_buffers"]
    assert "wire" not in entry and entry["cache"]["ref"] is True and stats["arg_narrowed"] == 1


def test_option_default_and_validation(local_executor):
    from covalent_ssh_plugin_amd.ssh import _EXECUTOR_PLUGIN_DEFAULTS

    assert _EXECUTOR_PLUGIN_DEFAULTS["narrow_tensor_args"] is False
    device = dict(persistent_workers=True, device_tensor_args=True)
    assert local_executor(**device).narrow_tensor_args is False
    assert local_executor(**device, narrow_tensor_args=True).narrow_tensor_args
    with pytest.raises(ValueError, match="narrow_tensor_args needs device_tensor_args=True"):
        local_executor(persistent_workers=True, narrow_tensor_args=True)
