"""bool tensors as ``"bits"`` without a GPU: ``csp_io_bool_pack`` against ``numpy.packbits``, the
dispatcher's ``widen_result`` and ``narrow_arg``, and what ``extract_arg_buffers`` marks."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from covalent_ssh_plugin_amd.remote import workers  # noqa: E402
from covalent_ssh_plugin_amd.transport import native_io  # noqa: E402

CHUNK = 4096  # a chunk edge inside the largest case


def _bools(n):
    x = np.random.default_rng(n).integers(0, 2, n).astype(np.uint8)
    x[0] = x[-1] = 1
    return x


def _pack_all(x, chunk=CHUNK):
    """``csp_io_bool_pack`` over ``chunk``-element pieces: (the ORed bad word, the bits)."""
    raw, out, bad = bytearray(x.tobytes()), bytearray(native_io.bool_bits_bytes(len(x))), 0
    for off in range(0, len(raw), chunk):
        n = min(chunk, len(raw) - off)
        bad |= native_io.bool_pack(raw, n, out, off, off // 8)
        assert native_io.bool_pack(bytes(raw), n, None, off) == native_io.bool_pack(raw, n, None, off)
    return bad, np.frombuffer(out, dtype=np.uint8)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 127, 128, 129, CHUNK - 1, CHUNK, 2 * CHUNK + 3])
def test_csp_io_bool_pack_gives_numpy_packbits_and_refuses_every_poison(n):
    x = _bools(n)
    bad, got = _pack_all(x)
    assert bad == 0 and np.array_equal(got, np.packbits(x, bitorder="little"))
    for poison in (2, 0x80, 0xFF):
        for at in {0, n - 1, n // 2}:
            spoiled = x.copy()
            spoiled[at] = poison
            assert _pack_all(spoiled)[0] == poison & 0xFE


@pytest.mark.parametrize("shape", [(1,), (3, 43), (2, 5, 13), (4096,)])
def test_widen_result_rebuilds_a_bool_tensor_from_bits(shape):
    x = _bools(int(np.prod(shape)))
    data = bytearray(np.packbits(x, bitorder="little").tobytes())
    out = workers.widen_result(data, {"wire": "bits", "dtype": "bool", "shape": list(shape)})
    assert out.dtype == torch.bool and tuple(out.shape) == shape
    assert np.array_equal(out.view(torch.uint8).numpy().ravel(), x)


def test_narrow_arg_packs_an_exact_bool_tensor_and_drops_an_inexact_one():
    n = 3 * CHUNK + 5  # several pieces on the thread pool
    x = _bools(n)
    stats = {}
    wire, out = workers.narrow_arg(bytearray(x.tobytes()), "bool", chunk_bytes=CHUNK, stats=stats)
    assert wire == "bits" and bytes(out) == np.packbits(x, bitorder="little").tobytes()
    assert stats["arg_narrowed"] == 1 and stats["arg_narrow_saved_bytes"] == n - (n + 7) // 8
    x[CHUNK] = 3  # a uint8 tensor viewed as bool
    assert workers.narrow_arg(bytearray(x.tobytes()), "bool", chunk_bytes=CHUNK, stats=stats) is None
    assert stats["arg_narrowed"] == 1 and stats["arg_narrow_ms"] > 0


def test_extract_marks_a_bool_argument_and_keeps_the_packed_arena_tables_free_of_bool():
    mask = torch.from_numpy(_bools(5000)).view(torch.bool)

    def meta(**options):
        _, _, entries, buffers = workers.extract_arg_buffers(
            [mask], {}, 1024, to_device=True, **options)
        return entries[0], buffers[0][0]

    off, view_off = meta()
    on, view_on = meta(narrow=True)
    assert on.pop("wire") == "bits" and on == off and len(view_off) == 5000
    assert bytes(view_on) == np.packbits(mask.numpy(), bitorder="little").tobytes()
    cached, view = meta(narrow=True, cache_min_bytes=4096)  # decided when the bytes travel
    assert cached["cache"]["narrow"] is True and "wire" not in cached and len(view) == 5000
    assert "bool" not in native_io.NARROW_TARGETS and "bits" not in native_io.NARROW_KINDS
    assert "bits" not in native_io.NARROW_ELEM_SIZE
