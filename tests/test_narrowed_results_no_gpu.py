"""``narrow_tensor_results`` without a GPU: the dispatcher's widening against
integer arithmetic on the bits, the integrity check over the narrow bytes, the
option's validation and the worker template's token."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from covalent_ssh_plugin_amd.remote.workers import (  # noqa: E402
    _reconstruct, verify_result_buffers, widen_result,
)
from covalent_ssh_plugin_amd.transport import native_io  # noqa: E402


def _widen(narrow, wire, dtype):
    """The bits of ``widen_result`` on the numpy patterns ``narrow``."""
    wide = widen_result(bytearray(narrow.tobytes()), {"wire": wire, "dtype": dtype, "shape": [-1]})
    assert str(wide.dtype) == "torch." + dtype and wide.shape == (len(narrow),)
    return wide.view(torch.uint8).numpy()


def test_every_bf16_pattern_widens_to_its_bits_shifted():
    patterns = np.arange(1 << 16, dtype=np.uint16)
    want = patterns.astype(np.uint32) << 16
    assert np.array_equal(_widen(patterns, "bfloat16", "float32"), want.view(np.uint8))


def test_the_float32_edges_widen_by_the_integer_rule_and_narrow_back():
    x = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFFFFFFF, 0x7F7FFFFF,
                  0x00800000, 0x80800001, 0x3F800000, 0xC0490FDB], dtype=np.uint64)
    e, m = (x >> 23) & 0xFF, x & 0x7FFFFF
    e64 = np.where(e == 0, 0, np.where(e == 255, 0x7FF, e + 896)).astype(np.uint64)
    want = (x >> 31) << 63 | e64 << 52 | m << 29
    narrow = x.astype(np.uint32)
    got = _widen(narrow, "float32", "float64")
    assert np.array_equal(got, want.view(np.uint8))
    back = torch.from_numpy(got.copy()).view(torch.float64).to(torch.float32)
    assert np.array_equal(back.view(torch.uint8).numpy(), narrow.view(np.uint8))


@pytest.mark.parametrize("wire, dtype", [("int32", "int64"), ("int16", "int64"), ("uint8", "int64"),
                                         ("int16", "int32"), ("uint8", "int32")])
def test_integer_limits_widen_to_the_same_values(wire, dtype):
    info = np.iinfo(wire)
    narrow = np.array([info.min, info.max, 0, 1], dtype=wire)
    assert np.array_equal(_widen(narrow, wire, dtype), narrow.astype(dtype).view(np.uint8))


def test_the_narrow_bytes_are_verified_and_rebuilt_at_full_width():
    assert native_io.load() is not None, "libcsp_io.so was not built"
    ids = np.arange(-300, 300, dtype=np.int16).reshape(20, 30)
    data = bytearray(ids.tobytes())
    meta = [{"dtype": "int64", "shape": [20, 30], "wire": "int16",
             "sum": list(native_io.checksum(bytes(data)))}]
    assert verify_result_buffers(meta, [data]) == 1
    out = _reconstruct({"ids": ("__csp_tensor_buffer_v1__", 0)}, meta, [data])["ids"]
    assert out.dtype == torch.int64 and np.array_equal(out.numpy(), ids.astype(np.int64))
    data[7] ^= 0x10
    with pytest.raises(RuntimeError, match="failed its integrity check"):
        verify_result_buffers(meta, [data])


def test_option_default_validation_and_the_template_token(local_executor):
    from covalent_ssh_plugin_amd.remote.stub import render_worker
    from covalent_ssh_plugin_amd.ssh import _EXECUTOR_PLUGIN_DEFAULTS

    assert _EXECUTOR_PLUGIN_DEFAULTS["narrow_tensor_results"] is False
    assert local_executor(persistent_workers=True).narrow_tensor_results is False
    assert local_executor(narrow_tensor_results=True, isolate_tasks=True).narrow_tensor_results
    with pytest.raises(ValueError, match="narrow_tensor_results needs persistent_workers"):
        local_executor(narrow_tensor_results=True, persistent_workers=False)
    on, off = render_worker(narrow_results=True), render_worker()
    assert "NARROW_RESULTS = bool(True)" in on and "__CSP_" not in on
    compile(on, "worker.py", "exec")
    assert on.replace("NARROW_RESULTS = bool(True)", "NARROW_RESULTS = bool(False)") == off
