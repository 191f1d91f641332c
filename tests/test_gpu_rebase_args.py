"""MI355X tests for ``rebase_tensor_args``: csp_rebase_unpack_checksum_dev on
its own (exact scatter of the new arena, guard bytes that begin at dst +
nbytes, the new master byte for byte against a numpy model, base and delta
untouched, the checksum against numpy, csp_checksum_dev and the host library,
reordered, inserted, removed, resized and shared segments, the transient
rebase without a new master, padding that is not zero, tiny grid caps, more
tiles than blocks, refused calls), and rebased arguments end to end through a
loopback worker: store, rebase, hit, an evicted base, a wrong checksum and a
budget too small for base and new together."""

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


def rounded(n):
    return (n + 15) // 16 * 16


def plan(probe, new_sizes, base_offs, seed, padding=0):
    """A rebase plan: segment k of ``new_sizes`` comes from the base at
    ``base_offs[k]``, or from the delta where that is None.  Returns (delta
    host arena, out offsets, arena bytes, delta offsets or None)."""
    out_offs, total = probe.pack_layout(new_sizes)
    from_delta = [n for n, b in zip(new_sizes, base_offs) if b is None]
    delta, offs = make_arena(probe, from_delta, seed, padding)
    it = iter(offs)
    return delta, out_offs, total, [next(it) if b is None else None for b in base_offs]


def rebase_and_check(probe, base_host, delta_host, sizes, out_offs, total, base_offs,
                     delta_offs, keep=True):
    """Run one rebase and check everything the kernel promises; returns (sum,
    the new arena as the model has it, the new master as the GPU wrote it or
    None for a transient rebase)."""
    from covalent_ssh_plugin_amd.transport import native_io

    model = np.zeros(total, dtype=np.uint8)
    for off, n, boff, doff in zip(out_offs, sizes, base_offs, delta_offs):
        # whole vectors: the source's padding goes into the new arena as it is
        src, at = (base_host, boff) if doff is None else (delta_host, doff)
        model[off : off + rounded(n)] = src[at : at + rounded(n)]
    base = torch.from_numpy(base_host).cuda()
    delta = torch.from_numpy(delta_host).cuda()
    # the new master inside a 0x3C holder: nothing around it may change
    holder = torch.full((total + 64,), 0x3C, dtype=torch.uint8, device="cuda")
    # every destination is a slice of ONE 0xA5 buffer: 16-byte aligned start,
    # guard bytes from exactly dst + nbytes
    starts = []
    cursor = 16
    for n in sizes:
        starts.append(cursor)
        cursor = (cursor + n + GUARD + 15) // 16 * 16
    backing = torch.full((cursor,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    first = backing.data_ptr()
    base_ptr = base.data_ptr() if len(base_host) else 0
    delta_ptr = delta.data_ptr() if len(delta_host) else 0
    out_ptr = holder.data_ptr() + 32 if keep else 0
    assert first % 16 == 0 and base_ptr % 16 == 0 and delta_ptr % 16 == 0 and out_ptr % 16 == 0
    segments = [
        (first + s, off, n, boff, doff)
        for s, off, n, boff, doff in zip(starts, out_offs, sizes, base_offs, delta_offs)
    ]
    out = probe.rebase_unpack_checksum_device(
        base_ptr, len(base_host), delta_ptr, len(delta_host), out_ptr, total, segments
    )
    after = backing.cpu().numpy()
    expect = np.full(cursor, 0xA5, dtype=np.uint8)
    for s, off, n in zip(starts, out_offs, sizes):
        expect[s : s + n] = model[off : off + n]
    bad = np.flatnonzero(after != expect)
    assert bad.size == 0, "first wrong destination/guard byte at %d" % bad[0]
    assert np.array_equal(base.cpu().numpy(), base_host), "the base changed"
    assert np.array_equal(delta.cpu().numpy(), delta_host), "the delta changed"
    held = holder.cpu().numpy()
    assert (held[:32] == 0x3C).all() and (held[32 + total :] == 0x3C).all()
    got = out["sum"]
    assert got == reference(model.tobytes())
    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    assert got == tuple(native_io.checksum(model.tobytes()))
    if keep:
        bad = np.flatnonzero(held[32 : 32 + total] != model)
        assert bad.size == 0, "first wrong byte of the new master at %d" % bad[0]
        if total:
            assert got == probe.checksum_device(out_ptr, total)
    else:
        assert (held == 0x3C).all(), "a transient rebase wrote a master"
    assert out["kernel_ms"] >= 0.0
    return got, model, (held[32 : 32 + total].copy() if keep else None)


def edge_sizes(probe):
    tile = probe.pack_tile_bytes()
    return [0, 1, 15, 16, 17, 4095, tile, tile + 1, 3 * tile + 5, (1 << 20) + 3]


@pytest.fixture(scope="module")
def edge_base(probe):
    """The shared base of the edge-size tests; no test writes to it."""
    sizes = edge_sizes(probe)
    arena, offsets = make_arena(probe, sizes, seed=301)
    return sizes, arena, offsets


# -- csp_rebase_unpack_checksum_dev ------------------------------------------


def test_reversed_order_with_an_empty_delta(probe, edge_base):
    sizes, base, offsets = edge_base
    new_sizes, base_offs = sizes[::-1], offsets[::-1]
    delta, out_offs, total, delta_offs = plan(probe, new_sizes, base_offs, seed=400)
    assert len(delta) == 0 and total == len(base)
    _sum, model, _m = rebase_and_check(probe, base, delta, new_sizes, out_offs, total,
                                       base_offs, delta_offs)
    assert not np.array_equal(model, base)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("extra", [1000, 70001])
def test_one_segment_inserted_from_the_delta(probe, edge_base, where, extra):
    sizes, base, offsets = edge_base
    at = {"first": 0, "middle": 5, "last": len(sizes)}[where]
    new_sizes = sizes[:at] + [extra] + sizes[at:]
    base_offs = offsets[:at] + [None] + offsets[at:]
    delta, out_offs, total, delta_offs = plan(probe, new_sizes, base_offs, seed=401 + at)
    assert len(delta) == rounded(extra) and total == len(base) + rounded(extra)
    rebase_and_check(probe, base, delta, new_sizes, out_offs, total, base_offs, delta_offs)


@pytest.mark.parametrize("which", range(10))
def test_each_segment_removed_alone(probe, edge_base, which):
    sizes, base, offsets = edge_base
    new_sizes = sizes[:which] + sizes[which + 1 :]
    base_offs = offsets[:which] + offsets[which + 1 :]
    delta, out_offs, total, delta_offs = plan(probe, new_sizes, base_offs, seed=420)
    assert len(delta) == 0 and total == len(base) - rounded(sizes[which])
    rebase_and_check(probe, base, delta, new_sizes, out_offs, total, base_offs, delta_offs)


@pytest.mark.parametrize("step", [-1, 1])
@pytest.mark.parametrize("which", range(1, 10))
def test_each_nonzero_segment_resized_by_one_byte(probe, edge_base, which, step):
    sizes, base, offsets = edge_base
    new_sizes = list(sizes)
    new_sizes[which] += step
    base_offs = list(offsets)
    base_offs[which] = None
    delta, out_offs, total, delta_offs = plan(probe, new_sizes, base_offs, seed=430 + which)
    assert len(delta) == rounded(new_sizes[which])
    rebase_and_check(probe, base, delta, new_sizes, out_offs, total, base_offs, delta_offs)


def test_one_base_segment_read_by_two_new_segments(probe, edge_base):
    sizes, base, offsets = edge_base
    # the 3 * tile + 5 segment twice, and the 17-byte one twice, among the rest
    new_sizes = [sizes[8], sizes[4]] + sizes + [sizes[8]]
    base_offs = [offsets[8], offsets[4]] + offsets + [offsets[8]]
    delta, out_offs, total, delta_offs = plan(probe, new_sizes, base_offs, seed=440)
    assert len(delta) == 0
    rebase_and_check(probe, base, delta, new_sizes, out_offs, total, base_offs, delta_offs)


def test_same_layout_equals_the_patch_kernel(probe, edge_base):
    """Every second segment from the delta, the layout kept: the sum and the
    new master must be what csp_patch_unpack_checksum_dev (unchanged code)
    makes of a copy of the base."""
    sizes, base, offsets = edge_base
    for first in (0, 1):
        base_offs = [None if k % 2 == first else off for k, off in enumerate(offsets)]
        delta, out_offs, total, delta_offs = plan(probe, sizes, base_offs, seed=450 + first)
        assert out_offs == offsets and total == len(base)
        got, _model, master = rebase_and_check(probe, base, delta, sizes, out_offs, total,
                                               base_offs, delta_offs)
        copy = torch.from_numpy(base.copy()).cuda()
        dev_delta = torch.from_numpy(delta).cuda()
        dsts = [torch.empty(max(n, 1), dtype=torch.uint8, device="cuda") for n in sizes]
        torch.cuda.synchronize()
        segments = [(d.data_ptr(), off, n, doff)
                    for d, off, n, doff in zip(dsts, offsets, sizes, delta_offs)]
        ref = probe.patch_unpack_checksum_device(
            copy.data_ptr(), total, dev_delta.data_ptr(), len(delta), segments
        )
        assert got == ref["sum"]
        assert np.array_equal(master, copy.cpu().numpy())


def test_transient_rebase_writes_no_master(probe, edge_base):
    sizes, base, offsets = edge_base
    new_sizes = sizes[::-1] + [333]
    base_offs = offsets[::-1] + [None]
    delta, out_offs, total, delta_offs = plan(probe, new_sizes, base_offs, seed=460)
    kept, _m, _a = rebase_and_check(probe, base, delta, new_sizes, out_offs, total,
                                    base_offs, delta_offs)
    transient, _m, master = rebase_and_check(probe, base, delta, new_sizes, out_offs, total,
                                             base_offs, delta_offs, keep=False)
    assert transient == kept and master is None


def test_padding_of_base_and_delta_is_carried_and_summed(probe, edge_base):
    sizes, clean_base, offsets = edge_base
    dirty_base, _ = make_arena(probe, sizes, seed=301, padding=0x6D)
    base_offs = [None if k % 2 == 0 else off for k, off in enumerate(offsets)]
    clean, out_offs, total, delta_offs = plan(probe, sizes, base_offs, seed=470)
    dirty, _o, _t, _d = plan(probe, sizes, base_offs, seed=470, padding=0x5C)
    args = (sizes, out_offs, total, base_offs, delta_offs)
    s_clean, _m, _a = rebase_and_check(probe, clean_base, clean, *args)
    s_delta, _m, after = rebase_and_check(probe, clean_base, dirty, *args)
    # segment 2 (15 bytes, from the delta) and segment 1 (1 byte, from the base)
    assert after[out_offs[2] + 15] == 0x5C and not after[out_offs[1] + 1 : out_offs[1] + 16].any()
    s_base, _m, after = rebase_and_check(probe, dirty_base, clean, *args)
    assert (after[out_offs[1] + 1 : out_offs[1] + 16] == 0x6D).all()
    assert after[out_offs[2] + 15] == 0
    assert len({s_clean, s_delta, s_base}) == 3


def test_one_flipped_bit_changes_the_sum(probe, edge_base):
    sizes, base, offsets = edge_base
    base_offs = list(offsets)
    base_offs[9] = None
    delta, out_offs, total, delta_offs = plan(probe, sizes, base_offs, seed=480)
    args = (sizes, out_offs, total, base_offs, delta_offs)
    before, _m, _a = rebase_and_check(probe, base, delta, *args)
    flipped = delta.copy()
    flipped[70001] ^= 0x10
    assert rebase_and_check(probe, base, flipped, *args)[0] != before
    other = base.copy()
    other[offsets[8] + 40001] ^= 0x02
    assert rebase_and_check(probe, other, delta, *args)[0] != before


def _many_tiles(probe):
    tile = probe.pack_tile_bytes()
    # 1 + 1 + 5 + 3 + 0 + 9 + 1 + 2 + 0 + 1 + 7 = 30 tiles (zero bytes own none)
    sizes = [tile, 5, 4 * tile + 17, 3 * tile, 0, 8 * tile + 1, 16, tile + 1, 0, 333,
             6 * tile + 4095]
    base, offsets = make_arena(probe, sizes, seed=15)
    # reversed, every second nonzero segment from the delta
    new_sizes, base_offs = sizes[::-1], offsets[::-1]
    nonzero = [k for k, n in enumerate(new_sizes) if n]
    base_offs = [None if k in nonzero[::2] else b for k, b in enumerate(base_offs)]
    return base, new_sizes, base_offs


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_tiny_grid_caps_loop_over_many_tiles(probe, cap, keep):
    base, new_sizes, base_offs = _many_tiles(probe)
    delta, out_offs, total, delta_offs = plan(probe, new_sizes, base_offs, seed=490)
    try:
        assert probe.unpack_checksum_grid_cap(cap) == cap
        rebase_and_check(probe, base, delta, new_sizes, out_offs, total, base_offs,
                         delta_offs, keep=keep)
    finally:
        default = probe.unpack_checksum_grid_cap(0)
    assert default >= 1024


def test_more_tiles_than_blocks(probe):
    tile = probe.pack_tile_bytes()
    rng = np.random.default_rng(16)
    sizes = [300 * tile + 5] + [int(n) for n in rng.integers(1, 5001, 800)]
    tiles = sum((rounded(n) + tile - 1) // tile for n in sizes)
    assert tiles == 1101 > probe.unpack_checksum_grid_cap(0)
    base, offsets = make_arena(probe, sizes, seed=17)
    # the big segment moves to the end; every third small one from the delta
    order = list(range(1, len(sizes))) + [0]
    new_sizes = [sizes[k] for k in order]
    base_offs = [None if k % 3 == 1 else offsets[k] for k in order]
    delta, out_offs, total, delta_offs = plan(probe, new_sizes, base_offs, seed=491)
    rebase_and_check(probe, base, delta, new_sizes, out_offs, total, base_offs, delta_offs)


def _refusal_fixture(probe):
    base_sizes = [33, 4096, 100]
    base_host, base_layout = make_arena(probe, base_sizes, seed=18)
    assert base_layout == [0, 48, 4144] and len(base_host) == 4256
    # new: the 100-byte base segment, an empty one, 4096 new bytes, the
    # 33-byte base segment, 50 new bytes
    sizes = [100, 0, 4096, 33, 50]
    base_offs = [4144, None, None, 0, None]
    delta_host, out_offs, total, delta_offs = plan(probe, sizes, base_offs, seed=19)
    delta_bytes, base_bytes = len(delta_host), len(base_host)
    assert delta_offs == [None, 0, 0, None, 4096] and delta_bytes == 4096 + 64
    assert out_offs == [0, 112, 112, 4208, 4256] and total == 4320
    # room around base, delta and new master inside one allocation each
    bholder = torch.zeros(base_bytes + 8192, dtype=torch.uint8, device="cuda")
    bholder[16 : 16 + base_bytes] = torch.from_numpy(base_host).cuda()
    dholder = torch.zeros(delta_bytes + 8192, dtype=torch.uint8, device="cuda")
    dholder[16 : 16 + delta_bytes] = torch.from_numpy(delta_host).cuda()
    oholder = torch.full((total + 8192,), 0x3C, dtype=torch.uint8, device="cuda")
    backing = torch.full((5 * 8192,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return dict(
        sizes=sizes, out_offs=out_offs, base_offs=base_offs, delta_offs=delta_offs,
        total=total, delta_bytes=delta_bytes, base_bytes=base_bytes,
        bholder=bholder, dholder=dholder, oholder=oholder, backing=backing,
        base_ptr=bholder.data_ptr() + 16, delta_ptr=dholder.data_ptr() + 16,
        out_ptr=oholder.data_ptr() + 16,
        dsts=[backing.data_ptr() + 8192 * k for k in range(5)],
        base_host=base_host, delta_host=delta_host,
    )


REFUSALS = {
    # those of csp_unpack_checksum_dev on the new layout
    "misaligned_dst": r"dst\[2\] \S+ is not 16-byte aligned",
    "misaligned_dst_of_empty_segment": r"dst\[1\] \S+ is not 16-byte aligned",
    "null_dst": r"segment 0 has 100 bytes and a null dst",
    "dst_overflow": r"dst\[4\] \S+ with 50 bytes overflows",
    "first_offset": r"out_off\[0\] is 16, the layout rule gives 0",
    "later_offset": r"out_off\[3\] is 4192, the layout rule gives 4208",
    "arena_bytes_short": r"arena_bytes is 4304, the segments need 4320",
    "arena_bytes_long": r"arena_bytes is 4336, the segments need 4320",
    "overflow": r"segment 4 overflows",
    "too_many_segments": r"segments are too many",
    # the three arenas
    "misaligned_base": r"base pointer \S+ is not 16-byte aligned",
    "misaligned_delta": r"delta pointer \S+ is not 16-byte aligned",
    "misaligned_out_arena": r"out_arena pointer \S+ is not 16-byte aligned",
    "null_base": r"null base",
    "null_delta": r"null delta for 4160 bytes",
    # sources
    "base_off_not_16": r"base_off\[3\] is 8, not a multiple of 16",
    "base_off_past_end": r"base_off\[0\] 4160 with 112 rounded bytes exceeds the base's 4256",
    "base_off_far_past_end": r"base_off\[3\] \d+ with 48 rounded bytes exceeds",
    "base_bytes_short": r"base_off\[0\] 4144 with 112 rounded bytes exceeds the base's 4240",
    "both_sources": r"segment 3 has both a base_off and a delta_off",
    "both_sources_empty_segment": r"segment 1 has both",
    "no_source": r"segment 2 has neither a base_off nor a delta_off",
    "first_delta_off": r"delta_off\[1\] is 16, the delta layout rule gives 0",
    "later_delta_off": r"delta_off\[4\] is 4080, the delta layout rule gives 4096",
    "delta_bytes_short": r"delta_bytes is 4144, the delta-sourced segments need 4160",
    "delta_bytes_long": r"delta_bytes is 4176, the delta-sourced segments need 4160",
    # overlaps
    "out_inside_base": r"at out_arena \S+ overlap the base",
    "out_across_base_start": r"at out_arena \S+ overlap the base",
    "out_across_base_end": r"at out_arena \S+ overlap the base",
    "out_across_delta_start": r"at out_arena \S+ overlap the delta",
    "out_across_delta_end": r"at out_arena \S+ overlap the delta",
    "dst_inside_out": r"at dst \S+ overlap the out_arena",
    "dst_across_out_start": r"at dst \S+ overlap the out_arena",
    "dst_across_out_end": r"at dst \S+ overlap the out_arena",
    "dst_inside_base": r"at dst \S+ overlap the base",
    "dst_across_base_start": r"at dst \S+ overlap the base",
    "dst_across_base_end": r"at dst \S+ overlap the base",
    "dst_inside_delta": r"at dst \S+ overlap the delta",
    "dst_across_delta_start": r"at dst \S+ overlap the delta",
    "dst_across_delta_end": r"at dst \S+ overlap the delta",
    "transient_dst_inside_base": r"at dst \S+ overlap the base",
}


def _raw_call(probe, nseg):
    """The C entry with a claimed ``nseg`` and no tables: refused before any
    table is read."""
    import ctypes

    lib = probe.load()
    out = (ctypes.c_uint64 * 2)()
    rc = lib.csp_rebase_unpack_checksum_dev(None, 0, None, 0, None, 0, None, None, None, None,
                                            None, nseg, out, None)
    if rc != 0:
        raise probe.GpuLibError(
            "csp_rebase_unpack_checksum_dev: " + lib.csp_last_error().decode()
        )


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_calls_launch_nothing(probe, case):
    f = _refusal_fixture(probe)
    sizes, out_offs, dsts = list(f["sizes"]), list(f["out_offs"]), list(f["dsts"])
    base_offs, delta_offs = list(f["base_offs"]), list(f["delta_offs"])
    base_ptr, base_bytes = f["base_ptr"], f["base_bytes"]
    delta_ptr, delta_bytes = f["delta_ptr"], f["delta_bytes"]
    out_ptr, total = f["out_ptr"], f["total"]
    a = dict(base=base_ptr, base_bytes=base_bytes, delta=delta_ptr, delta_bytes=delta_bytes,
             out=out_ptr, total=total)
    if case == "misaligned_dst":
        dsts[2] += 4
    elif case == "misaligned_dst_of_empty_segment":
        dsts[1] += 1
    elif case == "null_dst":
        dsts[0] = 0
    elif case == "dst_overflow":
        dsts[4] = (1 << 64) - 32
    elif case == "first_offset":
        out_offs[0] = 16
    elif case == "later_offset":
        out_offs[3] -= 16
    elif case == "arena_bytes_short":
        a["total"] -= 16
    elif case == "arena_bytes_long":
        a["total"] += 16
    elif case == "overflow":
        sizes[4] = (1 << 64) - 8
    elif case == "misaligned_base":
        a["base"] += 8
    elif case == "misaligned_delta":
        a["delta"] += 8
    elif case == "misaligned_out_arena":
        a["out"] += 8
    elif case == "null_base":
        a["base"] = 0
    elif case == "null_delta":
        a["delta"] = 0
    elif case == "base_off_not_16":
        base_offs[3] = 8
    elif case == "base_off_past_end":
        base_offs[0] = 4160  # 112 rounded bytes end 16 past the base
    elif case == "base_off_far_past_end":
        base_offs[3] = (1 << 64) - 32  # base_off + rounded wraps
    elif case == "base_bytes_short":
        a["base_bytes"] -= 16
    elif case == "both_sources":
        delta_offs[3] = 4096
    elif case == "both_sources_empty_segment":
        base_offs[1] = 0
    elif case == "no_source":
        delta_offs[2] = None
    elif case == "first_delta_off":
        delta_offs[1] = 16
    elif case == "later_delta_off":
        delta_offs[4] = 4080
    elif case == "delta_bytes_short":
        a["delta_bytes"] -= 16
    elif case == "delta_bytes_long":
        a["delta_bytes"] += 16
    elif case == "out_inside_base":
        # a base large enough to hold the new arena: claim more of the holder
        a["base_bytes"], a["out"] = base_bytes + 4096, base_ptr + 16
    elif case == "out_across_base_start":
        a["out"] = base_ptr - 16
    elif case == "out_across_base_end":
        a["out"] = base_ptr + base_bytes - 16
    elif case == "out_across_delta_start":
        a["out"] = delta_ptr - 16
    elif case == "out_across_delta_end":
        a["out"] = delta_ptr + delta_bytes - 16
    elif case == "dst_inside_out":
        dsts[2] = out_ptr + 16
    elif case == "dst_across_out_start":
        dsts[0] = out_ptr - 16  # 100 bytes from 16 before the new master
    elif case == "dst_across_out_end":
        dsts[3] = out_ptr + total - 16
    elif case == "dst_inside_base":
        dsts[3] = base_ptr + 32
    elif case == "dst_across_base_start":
        dsts[0] = base_ptr - 16
    elif case == "dst_across_base_end":
        dsts[3] = base_ptr + base_bytes - 16
    elif case == "dst_inside_delta":
        dsts[3] = delta_ptr + 32
    elif case == "dst_across_delta_start":
        dsts[0] = delta_ptr - 16
    elif case == "dst_across_delta_end":
        dsts[3] = delta_ptr + delta_bytes - 16
    elif case == "transient_dst_inside_base":
        a["out"] = 0
        dsts[3] = base_ptr + 32
    segments = list(zip(dsts, out_offs, sizes, base_offs, delta_offs))
    pattern = "csp_rebase_unpack_checksum_dev.*" + REFUSALS[case]
    with pytest.raises(probe.GpuLibError, match=pattern):
        if case == "too_many_segments":
            _raw_call(probe, 1 << 31)
        else:
            probe.rebase_unpack_checksum_device(
                a["base"], a["base_bytes"], a["delta"], a["delta_bytes"], a["out"],
                a["total"], segments
            )
    assert f["backing"].cpu().numpy().tobytes() == b"\xa5" * f["backing"].numel()
    after = f["bholder"].cpu().numpy()
    assert np.array_equal(after[16 : 16 + base_bytes], f["base_host"])
    assert not after[:16].any() and not after[16 + base_bytes :].any()
    after = f["dholder"].cpu().numpy()
    assert np.array_equal(after[16 : 16 + delta_bytes], f["delta_host"])
    assert not after[:16].any() and not after[16 + delta_bytes :].any()
    assert (f["oholder"].cpu().numpy() == 0x3C).all()


def test_touching_ranges_and_overlapping_sources_are_fine(probe):
    f = _refusal_fixture(probe)
    sizes, out_offs = f["sizes"], f["out_offs"]
    base_offs, delta_offs = f["base_offs"], f["delta_offs"]
    total, delta_bytes, base_bytes = f["total"], f["delta_bytes"], f["base_bytes"]
    base_host, delta_host = f["base_host"], f["delta_host"]
    # one allocation: dst 0 | delta | base | out | dst 3, each touching the next
    at = 4096
    holder = torch.zeros(at + delta_bytes + base_bytes + total + 4096, dtype=torch.uint8,
                         device="cuda")
    holder[at : at + delta_bytes] = torch.from_numpy(delta_host).cuda()
    b0 = at + delta_bytes
    holder[b0 : b0 + base_bytes] = torch.from_numpy(base_host).cuda()
    torch.cuda.synchronize()
    delta_ptr = holder.data_ptr() + at
    base_ptr = delta_ptr + delta_bytes
    out_ptr = base_ptr + base_bytes
    dsts = [delta_ptr - 112, 0, f["dsts"][2], out_ptr + total, f["dsts"][4]]
    segs = list(zip(dsts, out_offs, sizes, base_offs, delta_offs))
    out = probe.rebase_unpack_checksum_device(
        base_ptr, base_bytes, delta_ptr, delta_bytes, out_ptr, total, segs
    )
    model = np.zeros(total, dtype=np.uint8)
    model[0:112] = base_host[4144:4256]
    model[112:4208] = delta_host[0:4096]
    model[4208:4256] = base_host[0:48]
    model[4256:4320] = delta_host[4096:4160]
    assert out["sum"] == reference(model.tobytes())
    after = holder.cpu().numpy()
    assert np.array_equal(after[at - 112 : at - 12], model[:100])
    assert not after[: at - 112].any() and not after[at - 12 : at].any()
    assert np.array_equal(after[at : at + delta_bytes], delta_host), "the delta changed"
    assert np.array_equal(after[b0 : b0 + base_bytes], base_host), "the base changed"
    o0 = b0 + base_bytes
    assert np.array_equal(after[o0 : o0 + total], model)
    assert np.array_equal(after[o0 + total : o0 + total + 33], model[4208 : 4208 + 33])
    assert not after[o0 + total + 33 :].any()
    got = f["backing"].cpu().numpy()
    assert np.array_equal(got[2 * 8192 : 2 * 8192 + 4096], model[112:4208])
    assert np.array_equal(got[4 * 8192 : 4 * 8192 + 50], model[4256 : 4256 + 50])
    # base and delta ranges that overlap each other: both are only read.  The
    # "base" is the allocation from the delta's start to the base's end.
    wide = [None if b is None else b + delta_bytes for b in base_offs]
    segs = list(zip(f["dsts"], out_offs, sizes, wide, delta_offs))
    again = probe.rebase_unpack_checksum_device(
        delta_ptr, delta_bytes + base_bytes, delta_ptr, delta_bytes, f["out_ptr"], total, segs
    )
    assert again["sum"] == out["sum"]
    assert np.array_equal(f["oholder"].cpu().numpy()[16 : 16 + total], model)
    # nothing to rebase, nothing to unpack
    assert probe.rebase_unpack_checksum_device(0, 0, 0, 0, 0, 0, [])["sum"] == (0, 0)
    empty = [(0, 0, 0, 0, None), (0, 0, 0, None, 0)]
    assert probe.rebase_unpack_checksum_device(base_ptr, 16, 0, 0, 0, 0, empty)["sum"] == (0, 0)
    assert np.array_equal(holder.cpu().numpy(), after)


# -- end to end --------------------------------------------------------------

BIG_ELEMS = 80 * 1024  # float32: 320 KiB, above the staging threshold below
THRESHOLD = 256 * 1024
CACHE_MIN = 32 * 1024
BIG_BYTES = BIG_ELEMS * 4


def make_args(seed=77):
    """About 40 tensors of mixed dtype, among them a 0-d tensor, a zero-size
    tensor, a non-contiguous view and one tensor under two names, and one
    tensor above the staging threshold that travels on its own."""
    gen = torch.Generator().manual_seed(seed)
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


def resized_and_added(state):
    """``state`` with ``w9`` one element longer (3788 bytes: another layout
    from there on) and a new 200-byte tensor in front of ``scalar``."""
    new = {}
    for name, t in state.items():
        if name == "scalar":
            new["extra"] = torch.arange(50, dtype=torch.float32)
        new[name] = torch.cat([t, torch.ones(1)]) if name == "w9" else t
    assert new["twice"] is new["w3"] and list(new).index("extra") < list(new).index("scalar")
    return new


OTHER_LAYOUT_DELTA = 3792 + 208  # w9 and extra in the pack layout


def change_three(state):
    """``state`` with three tensors replaced by other values of the same
    shape: ``b0`` (1 byte), the 0-d ``scalar`` and ``w9`` (3784 bytes)."""
    new = dict(state)
    new["b0"] = state["b0"] ^ 0xFF
    new["scalar"] = torch.tensor(-7.5)
    new["w9"] = state["w9"] * 2 + 1
    return new


SAME_LAYOUT_DELTA = 16 + 16 + 3792


def _make_electron():
    """A local function, so cloudpickle ships it by value."""

    def electron(state, log=None):
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
        # overwrite the private tensors: a master must not see it
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
    return len(sizes), sum((n + 15) // 16 * 16 for n in sizes)


def _make_executor(tmp_path, budget, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor
    from covalent_ssh_plugin_amd.transport import native_io

    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    assert budget < BIG_BYTES  # never the big tensor
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
        arg_cache_bytes=budget,
        patch_tensor_args=True,
        rebase_tensor_args=True,
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


def test_store_rebase_to_another_layout_and_hit_the_base(tmp_path):
    state = make_args()
    new = resized_and_added(state)
    count_a, arena_a = _packed_total(state)
    count_b, arena_b = _packed_total(new)
    assert count_b == count_a + 1 and arena_b == arena_a + 208 >= CACHE_MIN
    ex = _make_executor(tmp_path, arena_a + arena_b + 1024)

    async def run():
        a = await _send(ex, state, 0)  # store
        b = await _send(ex, new, 1)  # rebase
        counters_b = dict(ex.counters)
        c = await _send(ex, state, 2)  # the base is still there: a hit
        counters_c = dict(ex.counters)
        d = await _send(ex, new, 3)  # and so is the new master, intact
        await ex.close_pool()
        return a, b, counters_b, c, counters_c, d

    a, b, counters_b, c, counters_c, d = asyncio.run(run())
    for (out, _meta), want in ((a, state), (b, new), (c, state), (d, new)):
        _delivered(out, want)
    (key_a,) = a[1]["arg_cache"]["stored"]
    assert a[1]["arg_staging"]["bytes"] == arena_a + BIG_BYTES
    # second: only the resized and the added tensor and the big one crossed the wire
    (key_b,) = b[1]["arg_cache"]["stored"]
    assert key_b != key_a
    assert b[1]["arg_cache"]["rebased"] == [[key_a, key_b]]
    assert "patched" not in b[1]["arg_cache"] and not b[1]["arg_cache"]["evicted"]
    stage = b[1]["arg_staging"]
    assert stage["bytes"] == OTHER_LAYOUT_DELTA + BIG_BYTES
    assert stage["rebased_segments"] == 2 and stage["rebased_bytes"] == OTHER_LAYOUT_DELTA
    assert stage["rebase_ms"] >= 0.0 and stage["packed_tensors"] == count_b
    assert stage["tensors"] == 2 and stage["verified"] == 2
    assert b[1]["arg_cache"]["resident_bytes"] == arena_a + arena_b
    assert counters_b["arg_cache_rebases"] == 1 and counters_b["arg_cache_patches"] == 0
    assert counters_b["arg_cache_bytes_saved"] == arena_b - OTHER_LAYOUT_DELTA
    assert counters_b["arg_cache_hits"] == 0 and counters_b["arg_cache_misses"] == 0
    # third: the first state is a hit with no argument frame but the big tensor's
    assert c[1]["arg_cache"]["hits"] == [key_a]
    assert c[1]["arg_staging"]["bytes"] == BIG_BYTES
    assert counters_c["arg_cache_hits"] == 1 and counters_c["arg_cache_rebases"] == 1
    # fourth: a hit on the new master, which the electrons' writes did not reach
    assert d[1]["arg_cache"]["hits"] == [key_b]
    assert d[1]["arg_staging"]["bytes"] == BIG_BYTES
    assert ex.counters["arg_cache_hits"] == 2 and ex.counters["arg_cache_misses"] == 0
    assert ex.counters["arg_cache_bytes_saved"] == (
        arena_b - OTHER_LAYOUT_DELTA + arena_a + arena_b
    )
    assert {m["pid"] for _o, m in (a, b, c, d)} == {a[1]["pid"]}
    assert d[1]["served"] == a[1]["served"] + 3


def test_same_layout_alternation_is_store_rebase_hit_hit(tmp_path):
    state = make_args()
    new = change_three(state)
    _count, arena = _packed_total(state)
    assert _packed_total(new)[1] == arena
    ex = _make_executor(tmp_path, 2 * arena + 1024)

    async def run():
        sent = [await _send(ex, s, k) for k, s in enumerate((state, new, state, new))]
        await ex.close_pool()
        return sent

    a, b, c, d = asyncio.run(run())
    for (out, _meta), want in ((a, state), (b, new), (c, state), (d, new)):
        _delivered(out, want)
    (key_a,) = a[1]["arg_cache"]["stored"]
    (key_b,) = b[1]["arg_cache"]["stored"]
    assert b[1]["arg_cache"]["rebased"] == [[key_a, key_b]]
    assert b[1]["arg_staging"]["bytes"] == SAME_LAYOUT_DELTA + BIG_BYTES
    assert b[1]["arg_staging"]["rebased_segments"] == 3
    assert c[1]["arg_cache"]["hits"] == [key_a] and d[1]["arg_cache"]["hits"] == [key_b]
    assert c[1]["arg_staging"]["bytes"] == d[1]["arg_staging"]["bytes"] == BIG_BYTES
    assert ex.counters["arg_cache_rebases"] == 1 and ex.counters["arg_cache_hits"] == 2
    assert ex.counters["arg_cache_patches"] == 0 and ex.counters["arg_cache_misses"] == 0
    assert d[1]["arg_cache"]["resident_bytes"] == 2 * arena


def test_evicted_base_costs_exactly_one_resend(tmp_path):
    state = make_args()
    new = resized_and_added(state)
    _count, arena = _packed_total(state)
    # nearly nothing in common with the first: stored whole, never a rebase
    other = make_args(seed=78)
    assert _packed_total(other)[1] == arena
    ex = _make_executor(tmp_path, arena + 1024)  # one arena
    log = tmp_path / "ran.log"

    async def run():
        a = await _send(ex, state, 0)  # store
        c = await _send(ex, other, 1)  # a store that evicts the first arena
        d = await _send(ex, new, 2, log=str(log))  # a rebase on what is gone
        await ex.close_pool()
        return a, c, d

    a, c, d = asyncio.run(run())
    _delivered(c[0], other)
    _delivered(d[0], new)
    assert c[1]["arg_cache"]["evicted"] == a[1]["arg_cache"]["stored"]
    assert "rebased" not in c[1]["arg_cache"]
    assert ex.counters["arg_cache_misses"] == 1
    assert ex.counters["arg_cache_rebases"] == 0
    assert d[1]["arg_cache"]["resent"] is True
    assert len(d[1]["arg_cache"]["stored"]) == 1 and "rebased" not in d[1]["arg_cache"]
    assert d[1]["arg_staging"]["bytes"] == _packed_total(new)[1] + BIG_BYTES, "not a full store"
    assert d[1]["served"] == c[1]["served"] + 2, "not exactly one resend"
    assert log.read_text() == "ran\n"


def test_wrong_sum_on_a_rebase_is_a_miss_and_the_resend_succeeds(tmp_path, monkeypatch):
    import cloudpickle

    from covalent_ssh_plugin_amd.remote import workers as worker_pool

    state = make_args()
    new = resized_and_added(state)
    _count, arena_a = _packed_total(state)
    arena_b = _packed_total(new)[1]
    ex = _make_executor(tmp_path, arena_a + arena_b + 1024)
    log = tmp_path / "ran.log"
    real = worker_pool._ArgCacheSend.frames
    spoiled = []

    def frames(self, full):
        """The request of a rebase goes out with another checksum."""
        inner = real(self, full)
        first = next(inner)
        request = cloudpickle.loads(first)
        for info in request["arg_buffers"]:
            if "rebase" in (info.get("cache") or {}):
                info["sum"] = [info["sum"][0], info["sum"][1] ^ 1]
                spoiled.append(info["cache"]["rebase"]["base"])
                first = cloudpickle.dumps(request)
        yield first
        yield from inner

    async def run():
        a = await _send(ex, state, 0)  # store
        with monkeypatch.context() as patch:
            patch.setattr(worker_pool._ArgCacheSend, "frames", frames)
            b = await _send(ex, new, 1, log=str(log))
        counters_b = dict(ex.counters)
        c = await _send(ex, state, 2)
        await ex.close_pool()
        return a, b, counters_b, c

    a, b, counters_b, c = asyncio.run(run())
    (key_a,) = a[1]["arg_cache"]["stored"]
    assert spoiled == [key_a], "the first attempt was not a rebase"
    # the rebase missed, user code did not run on it, the one full resend stored
    _delivered(b[0], new)
    assert counters_b["arg_cache_misses"] == 1 and counters_b["arg_cache_rebases"] == 0
    assert b[1]["arg_cache"]["resent"] is True and "rebased" not in b[1]["arg_cache"]
    (key_b,) = b[1]["arg_cache"]["stored"]
    assert b[1]["arg_staging"]["bytes"] == arena_b + BIG_BYTES
    assert b[1]["served"] == a[1]["served"] + 2, "not exactly one resend"
    assert log.read_text() == "ran\n"
    # both keys were gone: the worker holds the resent arena alone
    assert b[1]["arg_cache"]["entries"] == 1
    assert b[1]["arg_cache"]["resident_bytes"] == arena_b
    # and the dispatcher no longer believes in the first: no reference, no miss
    _delivered(c[0], state)
    assert not c[1]["arg_cache"]["hits"] and "resent" not in c[1]["arg_cache"]
    assert c[1]["arg_cache"]["rebased"] == [[key_b, key_a]]
    assert ex.counters["arg_cache_misses"] == 1
    assert c[1]["pid"] == a[1]["pid"], "the worker was replaced"


def test_a_budget_below_two_arenas_serves_the_rebase_transient(tmp_path):
    state = make_args()
    new = resized_and_added(state)
    _count, arena_a = _packed_total(state)
    arena_b = _packed_total(new)[1]
    ex = _make_executor(tmp_path, arena_a + arena_b // 2)

    async def run():
        a = await _send(ex, state, 0)  # store
        b = await _send(ex, new, 1)  # rebase, no room for a second master
        c = await _send(ex, state, 2)  # the base was not evicted for it: a hit
        await ex.close_pool()
        return a, b, c

    a, b, c = asyncio.run(run())
    _delivered(a[0], state)
    _delivered(b[0], new)
    _delivered(c[0], state)
    (key_a,) = a[1]["arg_cache"]["stored"]
    report = b[1]["arg_cache"]
    assert len(report["not_stored"]) == 2  # the new arena and, as always, the big tensor
    assert not report["stored"] and not report["evicted"] and not report["miss"]
    ((base, key_b),) = report["rebased"]
    assert base == key_a and key_b in report["not_stored"]
    assert report["resident_bytes"] == arena_a and report["entries"] == 1
    assert b[1]["arg_staging"]["bytes"] == OTHER_LAYOUT_DELTA + BIG_BYTES
    assert b[1]["arg_staging"]["rebased_bytes"] == OTHER_LAYOUT_DELTA
    assert c[1]["arg_cache"]["hits"] == [key_a]
    assert c[1]["arg_staging"]["bytes"] == BIG_BYTES
    assert ex.counters["arg_cache_rebases"] == 1 and ex.counters["arg_cache_hits"] == 1
    assert ex.counters["arg_cache_misses"] == 0
    assert c[1]["served"] == a[1]["served"] + 2
