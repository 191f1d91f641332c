"""MI355X: csp_diff_checksum_dev (4 KiB block diff, compacted frame and the
result's checksum in one pass) against a numpy model."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD = 64
HOLDER = 0x3C  # the frame buffer and what surrounds it, before the call
B = 4096
SIZES = [1, 15, 16, 17, B - 1, B, B + 1, 3 * B + 5, 9 * B, 64 * B + 7]
PATTERNS = ["none", "all", "first_block", "last_block", "last_byte", "alternate"]
BASE = np.random.default_rng(20261126).integers(0, 256, max(SIZES), dtype=np.uint8)


@pytest.fixture(scope="module")
def probe():
    from covalent_ssh_plugin_amd.gpu import probe as gpu_probe

    assert torch.cuda.is_available(), "GPU tests require a visible MI355X"
    gpu_probe.load()  # GpuLibError if the extension was not built/shipped
    assert gpu_probe.diff_block_bytes() == B
    return gpu_probe


def reference(data: bytes):
    """(s0, s1) as the protocol defines them, over little-endian u32 words."""
    words = np.frombuffer(data + b"\0" * (-len(data) % 4), dtype="<u4").astype(np.uint64)
    weight = (np.arange(len(words), dtype=np.uint64) % np.uint64(1 << 32)) + np.uint64(1)
    with np.errstate(over="ignore"):
        return int(words.sum(dtype=np.uint64)), int((words * weight).sum(dtype=np.uint64))


def changed_blocks(cur, base):
    """{block number: the block of ``cur``, zero padded} where bytes differ."""
    padded = np.zeros(-(-len(cur) // B) * B, dtype=np.uint8)
    padded[: len(cur)] = cur
    differ = np.zeros(len(padded), dtype=bool)
    differ[: len(cur)] = cur != base
    return {
        int(k): padded[k * B : (k + 1) * B].tobytes()
        for k in np.flatnonzero(differ.reshape(-1, B).any(axis=1))
    }


def diff_and_check(probe, cur, base, cap):
    """One call with room for ``cap`` blocks, checked against the model."""
    n, want = len(cur), changed_blocks(cur, base)
    dev_cur = torch.from_numpy(cur).cuda()
    dev_base = torch.from_numpy(base).cuda()
    outer = torch.full((GUARD + cap * (B + 4) + GUARD,), HOLDER, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    report = probe.diff_checksum_device(
        dev_cur.data_ptr(), dev_base.data_ptr(), n, outer.data_ptr() + GUARD, cap)
    assert report["changed"] == len(want) and report["rc"] == (0 if len(want) <= cap else 1)
    assert report["sum"] == reference(cur.tobytes()) == probe.checksum_device(dev_cur.data_ptr(), n)
    assert np.array_equal(dev_cur.cpu().numpy(), cur), "cur was written to"
    assert np.array_equal(dev_base.cpu().numpy(), base), "base was written to"
    got = outer.cpu().numpy()
    assert (got[:GUARD] == HOLDER).all() and (got[-GUARD:] == HOLDER).all(), "guard bytes"
    if report["rc"] == 0:
        c = len(want)
        frame = got[GUARD : GUARD + c * (B + 4)]
        index = frame[c * B :].view("<u4")
        assert {int(k): frame[i * B : (i + 1) * B].tobytes() for i, k in enumerate(index)} == want
        assert (got[GUARD + c * (B + 4) : -GUARD] == HOLDER).all(), "bytes past the frame"


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nbytes", SIZES)
def test_diff_against_numpy(probe, nbytes, pattern):
    base = BASE[:nbytes].copy()
    cur = base.copy()
    if pattern == "all":
        cur += 1
    elif pattern != "none":
        at = {"first_block": min(5, nbytes - 1), "last_block": (nbytes - 1) // B * B,
              "last_byte": nbytes - 1,  # in the sub-16 tail where there is one
              "alternate": np.arange(0, nbytes, 2 * B) + min(6, nbytes - 1)}[pattern]
        cur[at] ^= 0x04
    changed = len(changed_blocks(cur, base))
    try:
        for grid in [0, 1, 2, 3] if nbytes >= 9 * B else [0]:  # 0: the default cap
            probe.diff_checksum_grid_cap(grid)
            for cap in sorted({changed, max(changed - 1, 0), 0, changed + 2}):
                diff_and_check(probe, cur, base, cap)
    finally:
        probe.diff_checksum_grid_cap(0)


def test_comparison_is_bitwise(probe):
    """+0.0 against -0.0 is a change, equal NaN payloads are not."""
    words = B // 4
    base = np.zeros(3 * words, dtype="<u4")
    base[:words] = 0x7FC00001  # a block of NaNs with a payload
    cur = base.copy()
    cur[words + 9] = 0x80000000  # -0.0 where +0.0 was
    cur, base = cur.view(np.uint8), base.view(np.uint8)
    assert set(changed_blocks(cur, base)) == {1}
    diff_and_check(probe, cur, base, 3)


@pytest.mark.parametrize(
    "moved",
    [("cur", 4), ("base", 8), ("delta", 4), ("delta", "cur"), ("delta", "base"),
     ("cur", None), ("base", None), ("delta", None)],
    ids=lambda m: "%s-%s" % m,
)
def test_refusals_launch_nothing(probe, moved):
    n, cap = 2 * B, 2
    cur = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    base = torch.ones(n + 16, dtype=torch.uint8, device="cuda")
    delta = torch.full((cap * (B + 4) + 16,), HOLDER, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptrs = {"cur": cur.data_ptr(), "base": base.data_ptr(), "delta": delta.data_ptr()}
    name, how = moved
    if how is None:
        ptrs[name] = 0
    elif isinstance(how, str):
        ptrs[name] = ptrs[how] + n - 16  # the frame's first bytes are the other's last
    else:
        ptrs[name] += how  # misaligned
    with pytest.raises(probe.GpuLibError, match="csp_diff_checksum_dev"):
        probe.diff_checksum_device(ptrs["cur"], ptrs["base"], n, ptrs["delta"], cap)
    assert (delta == HOLDER).all() and (cur == 0).all() and (base == 1).all()
