"""MI355X tests for ``patch_tensor_args``: csp_patch_unpack_checksum_dev on
its own (exact scatter of the new arena, guard bytes that begin at dst +
nbytes, an untouched delta, the master patched byte for byte and nowhere
else, the checksum against numpy, csp_checksum_dev and the host library,
delta padding that is not zero, tiny grid caps, more tiles than blocks,
refused calls), and patched arguments end to end through a loopback worker:
store, patch, hit, patch back, an evicted base and a wrong checksum."""

import asyncio
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD = 48  # bytes of 0xA5 after every destination; keeps the next one aligned


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests require a visible MI355X (torch.cuda unavailable)")


@pytest.fixture(scope="module")
def probe():
    from covalent_ssh_plugin_amd.gpu import probe as gpu_probe

    gpu_probe.load()  # GpuLibError if the extension was not built/shipped
    return gpu_probe


def reference(data: bytes):
    """(s0, s1) as the protocol defines them: pad to 4 bytes, view as
    little-endian u32, widen to u64, wrapping sums."""
    words = np.frombuffer(data + b"\0" * (-len(data) % 4), dtype="<u4").astype(np.uint64)
    weight = (np.arange(len(words), dtype=np.uint64) % np.uint64(1 << 32)) + np.uint64(1)
    with np.errstate(over="ignore"):
        return (
            int(words.sum(dtype=np.uint64)),
            int((words * weight).sum(dtype=np.uint64)),
        )


def make_arena(probe, sizes, seed, padding=0):
    """Host arena for ``sizes`` under the pack layout: seeded random data,
    every padding byte ``padding``.  Returns (numpy uint8, offsets)."""
    offsets, total = probe.pack_layout(sizes)
    rng = np.random.default_rng(seed)
    arena = np.full(total, padding, dtype=np.uint8)
    for off, n in zip(offsets, sizes):
        arena[off : off + n] = rng.integers(0, 256, n, dtype=np.uint8)
    return arena, offsets


def make_delta(probe, sizes, mask, seed, padding=0):
    """The delta arena for the segments of ``sizes`` that ``mask`` names, in
    the pack layout, from another seed than the master's.  Returns (numpy
    uint8, per-segment delta offset or None)."""
    patched = [n for n, m in zip(sizes, mask) if m]
    delta, offs = make_arena(probe, patched, seed, padding)
    it = iter(offs)
    return delta, [next(it) if m else None for m in mask]


def rounded(n):
    return (n + 15) // 16 * 16


def patch_and_check(probe, master_host, delta_host, sizes, offsets, delta_offs):
    """Run one patch of ``master_host`` with ``delta_host`` and check
    everything the kernel promises; returns (sum, the master afterwards)."""
    from covalent_ssh_plugin_amd.transport import native_io

    total = len(master_host)
    expect_master = master_host.copy()
    for off, n, doff in zip(offsets, sizes, delta_offs):
        if doff is not None:
            # whole vectors: the delta's padding goes into the master as it is
            expect_master[off : off + rounded(n)] = delta_host[doff : doff + rounded(n)]
    master = torch.from_numpy(master_host).cuda()
    delta = torch.from_numpy(delta_host).cuda()
    # every destination is a slice of ONE 0xA5 buffer: 16-byte aligned start,
    # guard bytes from exactly dst + nbytes
    starts = []
    cursor = 16
    for n in sizes:
        starts.append(cursor)
        cursor = (cursor + n + GUARD + 15) // 16 * 16
    backing = torch.full((cursor,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    base = backing.data_ptr()
    delta_ptr = delta.data_ptr() if len(delta_host) else 0
    assert base % 16 == 0 and master.data_ptr() % 16 == 0 and delta_ptr % 16 == 0
    segments = [
        (base + s, off, n, doff)
        for s, off, n, doff in zip(starts, offsets, sizes, delta_offs)
    ]
    out = probe.patch_unpack_checksum_device(
        master.data_ptr(), total, delta_ptr, len(delta_host), segments
    )
    after = backing.cpu().numpy()
    expect = np.full(cursor, 0xA5, dtype=np.uint8)
    for s, off, n in zip(starts, offsets, sizes):
        expect[s : s + n] = expect_master[off : off + n]
    bad = np.flatnonzero(after != expect)
    assert bad.size == 0, "first wrong destination/guard byte at %d" % bad[0]
    assert np.array_equal(delta.cpu().numpy(), delta_host), "the delta changed"
    master_after = master.cpu().numpy()
    bad = np.flatnonzero(master_after != expect_master)
    assert bad.size == 0, "first wrong master byte at %d" % bad[0]
    got = out["sum"]
    assert got == reference(expect_master.tobytes())
    assert got == probe.checksum_device(master.data_ptr(), total)
    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    assert got == tuple(native_io.checksum(expect_master.tobytes()))
    assert out["kernel_ms"] >= 0.0
    return got, master_after


def edge_sizes(probe):
    tile = probe.pack_tile_bytes()
    return [0, 1, 15, 16, 17, 4095, tile, tile + 1, 3 * tile + 5, (1 << 20) + 3]


@pytest.fixture(scope="module")
def edge_master(probe):
    """The shared master of the edge-size tests; no test writes to it."""
    sizes = edge_sizes(probe)
    arena, offsets = make_arena(probe, sizes, seed=101)
    return sizes, arena, offsets


# -- csp_patch_unpack_checksum_dev -------------------------------------------


@pytest.mark.parametrize("which", range(10))
def test_each_segment_patched_alone(probe, edge_master, which):
    sizes, master, offsets = edge_master
    mask = [k == which for k in range(len(sizes))]
    delta, delta_offs = make_delta(probe, sizes, mask, seed=200 + which)
    assert len(delta) == rounded(sizes[which])
    patch_and_check(probe, master, delta, sizes, offsets, delta_offs)


def test_all_segments_patched(probe, edge_master):
    sizes, master, offsets = edge_master
    delta, delta_offs = make_delta(probe, sizes, [True] * len(sizes), seed=211)
    assert len(delta) == len(master)
    _sum, after = patch_and_check(probe, master, delta, sizes, offsets, delta_offs)
    assert np.array_equal(after, delta)


def test_no_segment_patched_is_the_unpack(probe, edge_master):
    sizes, master, offsets = edge_master
    delta, delta_offs = make_delta(probe, sizes, [False] * len(sizes), seed=212)
    assert len(delta) == 0 and delta_offs == [None] * len(sizes)
    got, after = patch_and_check(probe, master, delta, sizes, offsets, delta_offs)
    assert np.array_equal(after, master), "the master changed"
    # the same call through the unpack kernel
    arena = torch.from_numpy(master.copy()).cuda()
    dsts = [torch.empty(max(n, 1), dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()
    segments = [(d.data_ptr(), off, n) for d, off, n in zip(dsts, offsets, sizes)]
    assert probe.unpack_checksum_device(arena.data_ptr(), len(master), segments)["sum"] == got


def test_alternating_segments_patched(probe, edge_master):
    sizes, master, offsets = edge_master
    for first in (0, 1):
        mask = [k % 2 == first for k in range(len(sizes))]
        delta, delta_offs = make_delta(probe, sizes, mask, seed=213 + first)
        patch_and_check(probe, master, delta, sizes, offsets, delta_offs)


def test_delta_padding_is_summed_and_lands_in_the_master(probe, edge_master):
    sizes, master, offsets = edge_master
    mask = [k % 2 == 0 for k in range(len(sizes))]  # 0, 15, 17, tile, 3 * tile + 5
    clean, delta_offs = make_delta(probe, sizes, mask, seed=215)
    dirty, _ = make_delta(probe, sizes, mask, seed=215, padding=0x5C)
    assert not np.array_equal(clean, dirty)
    clean_sum, _ = patch_and_check(probe, master, clean, sizes, offsets, delta_offs)
    dirty_sum, after = patch_and_check(probe, master, dirty, sizes, offsets, delta_offs)
    assert dirty_sum != clean_sum
    k = 2  # 15 bytes: one byte of padding
    assert after[offsets[k] + 15] == 0x5C and master[offsets[k] + 15] == 0
    # an unchanged neighbour keeps its old (zero) padding
    assert not after[offsets[1] + 1 : offsets[1] + 16].any()


def test_one_flipped_bit_changes_the_sum(probe, edge_master):
    sizes, master, offsets = edge_master
    mask = [k == len(sizes) - 1 for k in range(len(sizes))]
    delta, delta_offs = make_delta(probe, sizes, mask, seed=216)
    before, _ = patch_and_check(probe, master, delta, sizes, offsets, delta_offs)
    flipped = delta.copy()
    flipped[70001] ^= 0x10
    assert patch_and_check(probe, master, flipped, sizes, offsets, delta_offs)[0] != before
    # a bit in a segment that is not patched: read from the master
    other = master.copy()
    other[offsets[8] + 40001] ^= 0x02
    assert patch_and_check(probe, other, delta, sizes, offsets, delta_offs)[0] != before


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_tiny_grid_caps_loop_over_many_tiles(probe, cap):
    tile = probe.pack_tile_bytes()
    # 1 + 1 + 5 + 3 + 0 + 9 + 1 + 2 + 0 + 1 + 7 = 30 tiles (zero bytes own none)
    sizes = [tile, 5, 4 * tile + 17, 3 * tile, 0, 8 * tile + 1, 16, tile + 1, 0, 333,
             6 * tile + 4095]
    master, offsets = make_arena(probe, sizes, seed=5)
    # every second nonzero segment
    nonzero = [k for k, n in enumerate(sizes) if n]
    mask = [k in nonzero[::2] for k in range(len(sizes))]
    delta, delta_offs = make_delta(probe, sizes, mask, seed=217)
    try:
        assert probe.unpack_checksum_grid_cap(cap) == cap
        patch_and_check(probe, master, delta, sizes, offsets, delta_offs)
    finally:
        default = probe.unpack_checksum_grid_cap(0)
    assert default >= 1024


def test_more_tiles_than_blocks(probe):
    tile = probe.pack_tile_bytes()
    rng = np.random.default_rng(6)
    # a patched segment of 300 tiles and a bit, then 800 one-tile segments
    sizes = [300 * tile + 5] + [int(n) for n in rng.integers(1, 5001, 800)]
    tiles = sum((rounded(n) + tile - 1) // tile for n in sizes)
    assert tiles == 1101 > probe.unpack_checksum_grid_cap(0)
    master, offsets = make_arena(probe, sizes, seed=7)
    mask = [k % 3 == 0 for k in range(len(sizes))]
    delta, delta_offs = make_delta(probe, sizes, mask, seed=218)
    patch_and_check(probe, master, delta, sizes, offsets, delta_offs)


def _refusal_fixture(probe):
    sizes = [100, 0, 4096, 33]
    mask = [True, False, True, False]
    master_host, offsets = make_arena(probe, sizes, seed=8)
    delta_host, delta_offs = make_delta(probe, sizes, mask, seed=9)
    total, delta_bytes = len(master_host), len(delta_host)
    assert delta_bytes == 112 + 4096 and delta_offs == [0, None, 112, None]
    # room around the master and around the delta inside one allocation each
    holder = torch.zeros(total + 4096, dtype=torch.uint8, device="cuda")
    holder[16 : 16 + total] = torch.from_numpy(master_host).cuda()
    dholder = torch.zeros(delta_bytes + 4096, dtype=torch.uint8, device="cuda")
    dholder[16 : 16 + delta_bytes] = torch.from_numpy(delta_host).cuda()
    backing = torch.full((4 * 8192,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return dict(
        sizes=sizes, offsets=offsets, delta_offs=delta_offs, total=total,
        delta_bytes=delta_bytes, holder=holder, dholder=dholder, backing=backing,
        master_ptr=holder.data_ptr() + 16, delta_ptr=dholder.data_ptr() + 16,
        dsts=[backing.data_ptr() + 8192 * k for k in range(4)],
        master_host=master_host, delta_host=delta_host,
    )


REFUSALS = {
    # those of csp_unpack_checksum_dev, the master in the place of its arena
    "misaligned_master": r"master pointer \S+ is not 16-byte aligned",
    "misaligned_dst": r"dst\[2\] \S+ is not 16-byte aligned",
    "misaligned_dst_of_empty_segment": r"dst\[1\] \S+ is not 16-byte aligned",
    "null_dst": r"segment 0 has 100 bytes and a null dst",
    "null_master": r"null master",
    "first_offset": r"src_off\[0\] is 16",
    "later_offset": r"src_off\[3\] is",
    "arena_bytes_short": r"arena_bytes is",
    "arena_bytes_long": r"arena_bytes is",
    "overflow": r"segment 3 overflows",
    "dst_inside_master": r"at dst \S+ overlap the master",
    "dst_across_master_start": r"at dst \S+ overlap the master",
    "dst_across_master_end": r"at dst \S+ overlap the master",
    # and those of the delta
    "misaligned_delta": r"delta pointer \S+ is not 16-byte aligned",
    "null_delta": r"null delta for 4208 bytes",
    "first_delta_off": r"delta_off\[0\] is 16, the delta layout rule gives 0",
    "later_delta_off": r"delta_off\[2\] is 96, the delta layout rule gives 112",
    "delta_off_on_unpatched_order": r"delta_off\[3\] is 0",
    "delta_bytes_short": r"delta_bytes is 4192, the patched segments need 4208",
    "delta_bytes_long": r"delta_bytes is 4224, the patched segments need 4208",
    "delta_overflow": r"bytes at delta \S+ overflow",
    "delta_inside_master": r"at delta \S+ overlap the master",
    "delta_across_master_start": r"at delta \S+ overlap the master",
    "delta_across_master_end": r"at delta \S+ overlap the master",
    "dst_inside_delta": r"at dst \S+ overlap the delta",
    "dst_across_delta_start": r"at dst \S+ overlap the delta",
    "dst_across_delta_end": r"at dst \S+ overlap the delta",
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_calls_launch_nothing(probe, case):
    f = _refusal_fixture(probe)
    sizes, offsets, dsts = list(f["sizes"]), list(f["offsets"]), list(f["dsts"])
    delta_offs = list(f["delta_offs"])
    master_ptr, total = f["master_ptr"], f["total"]
    delta_ptr, delta_bytes = f["delta_ptr"], f["delta_bytes"]
    master_arg, total_arg, delta_arg, delta_bytes_arg = master_ptr, total, delta_ptr, delta_bytes
    if case == "misaligned_master":
        master_arg += 8
    elif case == "misaligned_dst":
        dsts[2] += 4
    elif case == "misaligned_dst_of_empty_segment":
        dsts[1] += 1
    elif case == "null_dst":
        dsts[0] = 0
    elif case == "null_master":
        master_arg = 0
    elif case == "first_offset":
        offsets[0] = 16
    elif case == "later_offset":
        offsets[3] -= 16
    elif case == "arena_bytes_short":
        total_arg -= 16
    elif case == "arena_bytes_long":
        total_arg += 16
    elif case == "overflow":
        sizes[3] = (1 << 64) - 8
    elif case == "dst_inside_master":
        dsts[2] = master_ptr + 16
    elif case == "dst_across_master_start":
        dsts[0] = master_ptr - 16  # 100 bytes from 16 before the master
    elif case == "dst_across_master_end":
        dsts[3] = master_ptr + total - 16
    elif case == "misaligned_delta":
        delta_arg += 8
    elif case == "null_delta":
        delta_arg = 0
    elif case == "first_delta_off":
        delta_offs[0] = 16
    elif case == "later_delta_off":
        delta_offs[2] = 96
    elif case == "delta_off_on_unpatched_order":
        delta_offs[3] = 0  # a third patched segment belongs at 112 + 4096
    elif case == "delta_bytes_short":
        delta_bytes_arg -= 16
    elif case == "delta_bytes_long":
        delta_bytes_arg += 16
    elif case == "delta_overflow":
        delta_arg = (1 << 64) - 16
    elif case == "delta_inside_master":
        delta_arg, total_arg = master_ptr + 16, total
        # a delta that fits inside the master: only the small segment is patched
        delta_offs, delta_bytes_arg = [0, None, None, None], 112
    elif case == "delta_across_master_start":
        delta_arg = master_ptr - 16
    elif case == "delta_across_master_end":
        delta_arg = master_ptr + total - 16
    elif case == "dst_inside_delta":
        dsts[3] = delta_ptr + 32
    elif case == "dst_across_delta_start":
        dsts[0] = delta_ptr - 16  # 100 bytes from 16 before the delta
    elif case == "dst_across_delta_end":
        dsts[3] = delta_ptr + delta_bytes - 16
    segments = list(zip(dsts, offsets, sizes, delta_offs))
    pattern = "csp_patch_unpack_checksum_dev.*" + REFUSALS[case]
    with pytest.raises(probe.GpuLibError, match=pattern):
        probe.patch_unpack_checksum_device(
            master_arg, total_arg, delta_arg, delta_bytes_arg, segments
        )
    assert backing_untouched(f["backing"])
    after = f["holder"].cpu().numpy()
    assert np.array_equal(after[16 : 16 + total], f["master_host"])
    assert not after[:16].any() and not after[16 + total :].any()
    after = f["dholder"].cpu().numpy()
    assert np.array_equal(after[16 : 16 + delta_bytes], f["delta_host"])
    assert not after[:16].any() and not after[16 + delta_bytes :].any()


def backing_untouched(backing):
    return backing.cpu().numpy().tobytes() == b"\xa5" * backing.numel()


def test_touching_ranges_and_an_empty_patch_are_fine(probe):
    f = _refusal_fixture(probe)
    sizes, offsets, delta_offs = f["sizes"], f["offsets"], f["delta_offs"]
    total, delta_bytes = f["total"], f["delta_bytes"]
    master_host, delta_host = f["master_host"], f["delta_host"]
    # one allocation: dst 0 | delta | master | dst 3, each touching the next
    at = 4096
    holder = torch.zeros(at + delta_bytes + total + 4096, dtype=torch.uint8, device="cuda")
    holder[at : at + delta_bytes] = torch.from_numpy(delta_host).cuda()
    holder[at + delta_bytes : at + delta_bytes + total] = torch.from_numpy(master_host).cuda()
    torch.cuda.synchronize()
    delta_ptr = holder.data_ptr() + at
    master_ptr = delta_ptr + delta_bytes
    segs = [(delta_ptr - 112, offsets[0], 100, delta_offs[0]), (0, offsets[1], 0, None),
            (f["dsts"][2], offsets[2], 4096, delta_offs[2]),
            (master_ptr + total, offsets[3], 33, None)]
    out = probe.patch_unpack_checksum_device(master_ptr, total, delta_ptr, delta_bytes, segs)
    expect = master_host.copy()
    expect[0:112] = delta_host[0:112]
    expect[offsets[2] : offsets[2] + 4096] = delta_host[112 : 112 + 4096]
    assert out["sum"] == reference(expect.tobytes())
    after = holder.cpu().numpy()
    assert np.array_equal(after[at - 112 : at - 12], expect[:100])
    assert not after[: at - 112].any() and not after[at - 12 : at].any()
    assert np.array_equal(after[at : at + delta_bytes], delta_host), "the delta changed"
    m0 = at + delta_bytes
    assert np.array_equal(after[m0 : m0 + total], expect)
    assert np.array_equal(after[m0 + total : m0 + total + 33],
                          expect[offsets[3] : offsets[3] + 33])
    assert not after[m0 + total + 33 :].any()
    got = f["backing"].cpu().numpy()
    assert np.array_equal(got[2 * 8192 : 2 * 8192 + 4096], expect[offsets[2] : offsets[2] + 4096])
    # nothing to patch, nothing to unpack
    assert probe.patch_unpack_checksum_device(0, 0, 0, 0, [])["sum"] == (0, 0)
    empty = [(0, 0, 0, None), (0, 0, 0, 0)]
    assert probe.patch_unpack_checksum_device(master_ptr, 0, 0, 0, empty)["sum"] == (0, 0)
    assert np.array_equal(holder.cpu().numpy(), after)


# -- end to end --------------------------------------------------------------

BIG_ELEMS = 80 * 1024  # float32: 320 KiB, above the staging threshold below
THRESHOLD = 256 * 1024
CACHE_MIN = 32 * 1024


def make_args():
    """About 40 tensors of mixed dtype, among them a 0-d tensor, a zero-size
    tensor, a non-contiguous view and one tensor under two names, and one
    tensor above the staging threshold that travels on its own."""
    gen = torch.Generator().manual_seed(77)
    state = {}
    for k in range(12):
        state["w%d" % k] = torch.randn(37 + 101 * k, generator=gen)
    for k in range(8):
        state["h%d" % k] = torch.randn(5 + k, 33, generator=gen).to(torch.bfloat16)
    for k in range(6):
        state["i%d" % k] = torch.randint(-(1 << 40), 1 << 40, (3 + 7 * k,), generator=gen)
    for k in range(5):
        state["m%d" % k] = torch.rand(13 + 50 * k, generator=gen) > 0.5
    for k in range(5):
        state["b%d" % k] = torch.randint(0, 256, (1 + 999 * k,), dtype=torch.uint8, generator=gen)
    state["scalar"] = torch.tensor(3.25)
    state["empty"] = torch.empty(0, 7)
    state["strided"] = torch.randn(64, 48, generator=gen).t()[::2]
    assert not state["strided"].is_contiguous()
    state["twice"] = state["w3"]
    state["big"] = torch.randn(BIG_ELEMS, generator=gen)
    return state




def change_three(state):
    """``state`` with three tensors replaced by other values of the same
    shape: ``b0`` (1 byte, so 1 mod 16), the 0-d ``scalar`` and ``w9``
    (3784 bytes)."""
    new = dict(state)
    new["b0"] = state["b0"] ^ 0xFF
    new["scalar"] = torch.tensor(-7.5)
    new["w9"] = state["w9"] * 2 + 1
    assert new["twice"] is new["w3"]
    return new


DELTA_BYTES = 16 + 16 + 3792  # the three changed tensors in the pack layout
BIG_BYTES = BIG_ELEMS * 4


def _make_electron():
    """A local function, so cloudpickle ships it by value."""

    def electron(state, log=None, bump=False):
        import os

        if log is not None:
            with open(log, "a") as f:
                f.write("ran\n")
        report = {"pid": os.getpid(), "tensors": {}}
        for name, t in state.items():
            report["tensors"][name] = {
                "cuda": t.is_cuda,
                "seen": t.cpu().clone(),
                "ptr": t.data_ptr(),
                "storage_bytes": t.untyped_storage().nbytes(),
                "contiguous": t.is_contiguous(),
            }
        report["twice_is_one_object"] = state["twice"] is state["w3"]
        if bump:
            for name, t in state.items():
                if name != "twice" and t.dtype in (torch.float32, torch.bfloat16):
                    t.add_(1)
        return report

    return electron


_electron = _make_electron()


def _packed_total(state):
    """Arena bytes of the packed tensors of ``state`` (distinct objects below
    the threshold), by the layout rule."""
    seen = {}
    for t in state.values():
        if t.numel() * t.element_size() < THRESHOLD:
            seen.setdefault(id(t), t)
    sizes = [t.numel() * t.element_size() for t in seen.values()]
    return len(sizes), sum((n + 15) // 16 * 16 for n in sizes), sum(sizes)


def _make_executor(tmp_path, state, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor
    from covalent_ssh_plugin_amd.transport import native_io

    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    _count, arena_bytes, _data = _packed_total(state)
    assert arena_bytes >= CACHE_MIN
    assert all(
        t.numel() * t.element_size() < CACHE_MIN for n, t in state.items() if n != "big"
    )
    home = tmp_path / "home"
    home.mkdir()
    options = dict(
        transport="local",
        local_home=str(home),
        cache_dir=str(tmp_path / "cache"),
        python_path=sys.executable,
        gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True,
        device_tensor_args=True,
        pack_tensor_args=True,
        pack_args_min_bytes=1024,
        cache_tensor_args=True,
        arg_cache_min_bytes=CACHE_MIN,
        # the budget holds exactly one arena, and never the big tensor
        arg_cache_bytes=arena_bytes + 1024,
        patch_tensor_args=True,
        pinned_staging_threshold_bytes=THRESHOLD,
        # one slot, so every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
    )
    options.update(overrides)
    return SSHExecutor(**options)


async def _send(ex, state, node, **kwargs):
    out = await ex.execute(_electron, [state], kwargs, dispatch_id="p", node_id=node)
    return out, ex.last_task_record.remote_meta


def _delivered(out, state):
    assert set(out["tensors"]) == set(state)
    ptrs = {}
    for name, want in state.items():
        got = out["tensors"][name]
        assert got["cuda"] is True, name
        assert got["seen"].dtype == want.dtype, name
        assert got["seen"].shape == want.shape, name
        assert torch.equal(got["seen"], want), name
        assert got["contiguous"], name
        nbytes = want.numel() * want.element_size()
        if nbytes and name != "twice":
            ptrs[name] = got["ptr"]
            # its own allocation, not a view into an arena (the caching
            # allocator rounds a small block up to 512 bytes)
            assert nbytes <= got["storage_bytes"] < nbytes + 512, name
    assert len(set(ptrs.values())) == len(ptrs), "two tensors share a data pointer"
    assert out["twice_is_one_object"] is True
    assert out["tensors"]["twice"]["ptr"] == out["tensors"]["w3"]["ptr"]


def test_store_patch_hit_and_patch_back(tmp_path):
    state = make_args()
    new = change_three(state)
    count, arena_bytes, _data = _packed_total(state)
    assert _packed_total(new)[:2] == (count, arena_bytes)
    ex = _make_executor(tmp_path, state)

    async def run():
        a = await _send(ex, state, 0)  # store
        b = await _send(ex, new, 1, bump=True)  # patch; overwrites its own tensors
        counters_b = dict(ex.counters)
        c = await _send(ex, new, 2)  # a reference to the new key: the master is intact
        counters_c = dict(ex.counters)
        d = await _send(ex, state, 3)  # the original state: a patch back
        await ex.close_pool()
        return a, b, counters_b, c, counters_c, d

    a, b, counters_b, c, counters_c, d = asyncio.run(run())
    _delivered(a[0], state)
    _delivered(b[0], new)
    _delivered(c[0], new)
    _delivered(d[0], state)
    saved_by_patch = arena_bytes - DELTA_BYTES
    # first dispatch: the arena is stored, the big tensor does not fit the budget
    (key_a,) = a[1]["arg_cache"]["stored"]
    assert a[1]["arg_cache"]["not_stored"] and "patched" not in a[1]["arg_cache"]
    assert a[1]["arg_staging"]["bytes"] == arena_bytes + BIG_BYTES
    # second: only the three changed tensors and the big tensor crossed the wire
    (key_b,) = b[1]["arg_cache"]["stored"]
    assert key_b != key_a
    assert b[1]["arg_cache"]["patched"] == [[key_a, key_b]]
    stage = b[1]["arg_staging"]
    assert stage["bytes"] == DELTA_BYTES + BIG_BYTES
    assert stage["patched_segments"] == 3 and stage["patched_bytes"] == DELTA_BYTES
    assert stage["patch_ms"] >= 0.0 and stage["packed_tensors"] == count
    assert stage["tensors"] == 2 and stage["verified"] == 2
    assert counters_b["arg_cache_patches"] == 1
    assert counters_b["arg_cache_bytes_saved"] == saved_by_patch
    assert counters_b["arg_cache_hits"] == 0 and counters_b["arg_cache_misses"] == 0
    # third: a hit on the new key, served from the patched master
    assert c[1]["arg_cache"]["hits"] == [key_b]
    assert c[1]["arg_staging"]["bytes"] == BIG_BYTES
    assert counters_c["arg_cache_hits"] == 1 and counters_c["arg_cache_patches"] == 1
    assert counters_c["arg_cache_bytes_saved"] == saved_by_patch + arena_bytes
    # fourth: patched back to the first key
    assert d[1]["arg_cache"]["patched"] == [[key_b, key_a]]
    assert d[1]["arg_cache"]["stored"] == [key_a]
    assert d[1]["arg_staging"]["bytes"] == DELTA_BYTES + BIG_BYTES
    assert ex.counters["arg_cache_patches"] == 2
    assert ex.counters["arg_cache_bytes_saved"] == 2 * saved_by_patch + arena_bytes
    assert ex.counters["arg_cache_misses"] == 0
    # one worker, no resend, one arena held throughout
    assert {m["pid"] for _o, m in (a, b, c, d)} == {a[1]["pid"]}
    assert d[1]["served"] == a[1]["served"] + 3
    assert d[1]["arg_cache"]["resident_bytes"] == arena_bytes


def test_evicted_base_costs_exactly_one_resend(tmp_path):
    state = make_args()
    new = change_three(state)
    _count, arena_bytes, _data = _packed_total(state)
    # another layout (w0 one element longer), so never a patch of the first
    other = dict(state, w0=torch.randn(38))
    assert _packed_total(other)[1] == arena_bytes
    ex = _make_executor(tmp_path, state)
    log = tmp_path / "ran.log"

    async def run():
        a = await _send(ex, state, 0)  # store
        c = await _send(ex, other, 1)  # a store that evicts the first arena
        d = await _send(ex, new, 2, log=str(log))  # a patch of what is gone
        await ex.close_pool()
        return a, c, d

    a, c, d = asyncio.run(run())
    _delivered(c[0], other)
    _delivered(d[0], new)
    assert c[1]["arg_cache"]["evicted"] == a[1]["arg_cache"]["stored"]
    assert "patched" not in c[1]["arg_cache"]
    assert ex.counters["arg_cache_misses"] == 1
    assert ex.counters["arg_cache_patches"] == 0
    assert d[1]["arg_cache"]["resent"] is True
    assert len(d[1]["arg_cache"]["stored"]) == 1 and "patched" not in d[1]["arg_cache"]
    assert d[1]["arg_staging"]["bytes"] == arena_bytes + BIG_BYTES, "not a full store"
    assert d[1]["served"] == c[1]["served"] + 2, "not exactly one resend"
    assert log.read_text() == "ran\n"


def test_wrong_sum_on_a_patch_fails_the_task_and_keeps_the_worker(tmp_path, monkeypatch):
    from covalent_ssh_plugin_amd.remote import workers as worker_pool

    state = make_args()
    new = change_three(state)
    _count, arena_bytes, _data = _packed_total(state)
    ex = _make_executor(tmp_path, state)
    log = tmp_path / "ran.log"
    real = worker_pool.compose_packed_checksum

    def off_by_one(sums, offsets):
        s0, s1 = real(sums, offsets)
        return s0, (s1 + 1) % (1 << 64)

    async def run():
        a = await _send(ex, state, 0)  # store
        with monkeypatch.context() as patch:
            patch.setattr(worker_pool, "compose_packed_checksum", off_by_one)
            with pytest.raises(RuntimeError, match="failed its integrity check"):
                await _send(ex, new, 1, log=str(log))
        bad_meta = ex.last_task_record.remote_meta
        counters_bad = dict(ex.counters)
        out, good_meta = await _send(ex, new, 2, log=str(log))
        await ex.close_pool()
        return a, bad_meta, counters_bad, out, good_meta

    a, bad_meta, counters_bad, out, good_meta = asyncio.run(run())
    # the patch missed (wrong checksum), the one resend failed its check too
    assert counters_bad["arg_cache_misses"] == 1 and counters_bad["arg_cache_patches"] == 0
    assert bad_meta["arg_cache"]["resent"] is True
    assert bad_meta["served"] == a[1]["served"] + 2, "not exactly one resend"
    assert "user_fn" not in bad_meta["phases_ms"], "user code ran on unverified data"
    assert not bad_meta["arg_cache"]["stored"]
    # the next good dispatch stores the arena whole
    _delivered(out, new)
    assert good_meta["pid"] == bad_meta["pid"] == a[1]["pid"], "the worker was replaced"
    assert good_meta["served"] == bad_meta["served"] + 1
    assert len(good_meta["arg_cache"]["stored"]) == 1
    assert "patched" not in good_meta["arg_cache"]
    assert good_meta["arg_staging"]["bytes"] == arena_bytes + BIG_BYTES
    assert ex.counters["arg_cache_patches"] == 0
    assert log.read_text() == "ran\n"
