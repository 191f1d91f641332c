"""``pack_tensor_args`` with ``narrow_tensor_args`` without a GPU: the frame and the entry that
``extract_arg_buffers`` emits against a numpy model of the narrow layout, and the size rule."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from covalent_ssh_plugin_amd.remote import workers  # noqa: E402

N = 1001  # no multiple of any vector
# name -> (tensor, wire dtype or None, the numpy type it has on the wire)
CASES = {
    "u8": (torch.arange(N) % 256, "uint8", np.uint8),
    "i16": (torch.arange(N) * 61 - 30000, "int16", np.int16),
    "i32": (torch.arange(N) * 70001 - 9, "int32", np.int32),
    "wide": (torch.arange(N) << 33, None, np.int64),
    "bf16": ((torch.arange(N) % 251 - 125).float() / 8, "bfloat16", None),
    "thirds": (torch.arange(N).float() / 3, None, np.float32),
    "bytes": (torch.arange(77, dtype=torch.uint8), None, np.uint8),
    "f32": ((torch.arange(N).float() / 3).double(), "float32", np.float32),
}


def _extract(tensors, narrow, **more):
    stats = {}
    _, _, meta, bufs = workers.extract_arg_buffers(
        [tensors], {}, 1 << 20, to_device=True, pack_min_bytes=1, narrow=narrow,
        narrow_stats=stats, **more)
    return meta[0], bufs[0][0].tobytes(), stats


def test_the_frame_is_the_numpy_model_of_the_narrow_layout_and_the_entry_stays_wide():
    tensors = {k: v[0] for k, v in CASES.items()}
    wide, whole, _ = _extract(tensors, False)
    info, frame, stats = _extract(tensors, True)
    model = b""
    for seg, (t, wire, kind) in zip(info["packed"], CASES.values()):
        assert seg.get("wire") == wire
        if wire == "bfloat16":  # the upper halves of the float32 words
            piece = (t.numpy().view(np.uint32) >> 16).astype(np.uint16).tobytes()
        else:
            piece = t.numpy().astype(kind).tobytes()
        model += piece + bytes(-len(piece) % 16)
    assert frame == model and info["wire_nbytes"] == len(model) < len(whole) == wide["nbytes"]
    strip = [{k: v for k, v in seg.items() if k != "wire"} for seg in info["packed"]]
    assert strip == wide["packed"] and info["sum"] == wide["sum"] and info["nbytes"] == wide["nbytes"]
    assert "wire_nbytes" not in wide and stats["arg_narrowed"] == 5
    assert stats["arg_narrow_saved_bytes"] == len(whole) - len(model) and stats["arg_narrow_ms"] > 0


def test_a_cacheable_arena_is_only_marked_and_keeps_its_key_and_wide_frame():
    tensors = {k: v[0] for k, v in CASES.items()}
    off, whole, _ = _extract(tensors, False, cache_min_bytes=1 << 14)
    info, frame, stats = _extract(tensors, True, cache_min_bytes=1 << 14)
    assert frame == whole and info["cache"]["key"] == off["cache"]["key"] and not stats
    assert info["cache"]["narrow"] and "wire_nbytes" not in info and info["sum"] == off["sum"]
    wire, parts, total = workers.narrow_packed_args(info["packed"], info["cache"]["seg_views"])
    assert parts.tobytes() == _extract(tensors, True)[1] and total == parts.nbytes


@pytest.mark.parametrize("dtype, elems, narrowed", [
    # 16 wide bytes plus and minus one element: rounded sizes 16 -> 16, 32 -> 16, 16 -> 16
    (torch.int64, 2, False), (torch.int64, 3, True), (torch.int64, 1, False),
    (torch.float32, 4, False), (torch.float32, 5, True), (torch.float32, 3, False),
    (torch.int32, 4, False), (torch.int32, 5, True), (torch.int32, 3, False),
])
def test_a_segment_is_narrowed_only_where_its_rounded_size_shrinks(dtype, elems, narrowed):
    info, frame, _ = _extract([torch.ones(elems, dtype=dtype), torch.arange(64) + 300], True)
    assert ("wire" in info["packed"][0]) is narrowed and info["packed"][1]["wire"] == "int16"
    assert len(frame) == info["wire_nbytes"] == 16 + 128
