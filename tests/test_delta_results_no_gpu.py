"""``delta_tensor_results`` without a GPU: ``apply_result_delta`` and the option check."""

import numpy as np
import pytest

from covalent_ssh_plugin_amd.remote.workers import apply_result_delta
from covalent_ssh_plugin_amd.transport.channel import FrameParts

B = 4096
NBYTES = 3 * B + 5  # the last block is short
INFO = {"arg": 0, "block": B, "nbytes": NBYTES}
BASE = np.random.default_rng(7).integers(0, 256, NBYTES, dtype=np.uint8)
CUR = BASE.copy()
CUR[[3, 2 * B + 9, NBYTES - 1]] ^= 1  # blocks 0, 2 and 3, the short one


def _frame(slots):
    """The frame for blocks ``slots`` of CUR, in that order."""
    padded = np.zeros(5 * B, dtype=np.uint8)  # one block past the buffer
    padded[:NBYTES] = CUR
    blocks = b"".join(padded[k * B : (k + 1) * B].tobytes() for k in slots)
    return blocks + np.array(slots, dtype="<u4").tobytes()


@pytest.mark.parametrize("parts", [False, True], ids=["buffer", "frame-parts"])
def test_blocks_out_of_order_over_the_base(parts):
    view = BASE.tobytes()
    if parts:  # a packed arena: tensors and the padding between them
        view = FrameParts([view[:100], view[100 : 2 * B], view[2 * B :]])
    out = apply_result_delta({**INFO, "changed": 3}, _frame([3, 0, 2]), view)
    assert isinstance(out, bytearray) and bytes(out) == CUR.tobytes()
    assert bytes(apply_result_delta({**INFO, "changed": 0}, b"", view)) == BASE.tobytes()
    # a base that ends early is zero padded
    short = apply_result_delta({**INFO, "changed": 1}, _frame([0]), FrameParts([b""]))
    assert bytes(short) == CUR[:B].tobytes() + bytes(NBYTES - B)


@pytest.mark.parametrize(
    "changed, slots, cut, problem",
    [(2, [0, 2], 1, "the frame has"), (3, [0, 2], 0, "the frame has"),
     (2, [0, 4], 0, "beyond the buffer"), (2, [2, 2], 0, "appears twice")],
)
def test_refusals_are_integrity_failures(changed, slots, cut, problem):
    frame = _frame(slots)
    with pytest.raises(RuntimeError, match="delta against argument 0 failed its integrity") as e:
        apply_result_delta({**INFO, "changed": changed}, frame[: len(frame) - cut], BASE.tobytes())
    assert problem in str(e.value)


def test_the_option_needs_cache_tensor_args(tmp_path):
    from covalent_ssh_plugin_amd import SSHExecutor

    options = dict(transport="local", local_home=str(tmp_path), cache_dir=str(tmp_path / "c"))
    with pytest.raises(ValueError, match="delta_tensor_results needs cache_tensor_args"):
        SSHExecutor(delta_tensor_results=True, **options)
    assert SSHExecutor(**options).delta_tensor_results is False
