"""A packed result arena whose entries carry ``"wire"`` (``pack_tensor_results`` with
``narrow_tensor_results``) without a GPU: the dispatcher's rebuild against numpy on the bits, and
the integrity check over the narrow bytes."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_narrow_checksum import BITS, PAIRS, _narrow_values, _widen_bits  # noqa: E402

from covalent_ssh_plugin_amd.remote.workers import _reconstruct, verify_result_buffers  # noqa: E402
from covalent_ssh_plugin_amd.transport import native_io  # noqa: E402

SHAPE = [3, 7]


@pytest.fixture(scope="module")
def arena():
    """One wide float16 entry, then one narrowed entry per pair: (meta, bytes, wide bits)."""
    data, packed, want = bytearray(), [], []

    def add(dtype, values, bits, **wire):
        packed.append({"dtype": dtype, "shape": SHAPE, "offset": len(data),
                       "nbytes": values.nbytes, **wire})
        data.extend(values.tobytes() + b"\0" * (-values.nbytes % 16))
        want.append(bits)

    plain = np.arange(21, dtype=np.float16)
    add("float16", plain, plain.view(np.uint16))
    for src, dst in PAIRS:
        narrow = _narrow_values(dst, 21)
        add(src, narrow, _widen_bits(narrow, src), wire=dst)
    meta = [{"packed": packed, "nbytes": len(data), "sum": list(native_io.checksum(bytes(data)))}]
    return meta, data, want


def test_wire_entries_of_every_pair_widen_next_to_a_wide_one(arena):
    meta, data, want = arena
    result = [("__csp_packed_tensor_v1__", 0, j) for j in range(len(want))]
    out = _reconstruct(result, meta, [bytearray(data)])
    for t, info, bits in zip(out, meta[0]["packed"], want):
        assert str(t.dtype) == "torch." + info["dtype"] and list(t.shape) == SHAPE
        got = t.contiguous().view(torch.uint8).numpy().view(BITS.get(info["dtype"], np.uint16))
        assert np.array_equal(got.reshape(-1), bits), info


def test_the_narrow_arena_is_verified_and_a_flipped_byte_is_caught(arena):
    meta, data, _ = arena
    assert native_io.load() is not None, "libcsp_io.so was not built"
    assert verify_result_buffers(meta, [data]) == 1
    damaged = bytearray(data)
    damaged[50] ^= 0x10
    with pytest.raises(RuntimeError, match="failed its integrity check"):
        verify_result_buffers(meta, [damaged])
