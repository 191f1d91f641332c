"""MI355X tests for ``pack_tensor_args``: csp_unpack_checksum_dev on its own
(exact scatter, guard bytes that begin at dst + nbytes, an untouched arena,
the checksum against numpy, csp_checksum_dev and the host library, padding
that is not zero, tiny grid caps, more tiles than blocks, refused calls), and
packed arguments end to end through a loopback worker: persistent and
isolated delivery, a wrong checksum, and the arena as a cached master."""

import asyncio
import ctypes
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


def unpack_and_check(probe, arena_host, sizes, offsets):
    """Run one unpack of ``arena_host`` and check everything the kernel
    promises; returns the sum."""
    from covalent_ssh_plugin_amd.transport import native_io

    total = len(arena_host)
    arena = torch.from_numpy(arena_host).cuda()
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
    assert base % 16 == 0 and arena.data_ptr() % 16 == 0
    segments = [(base + s, off, n) for s, off, n in zip(starts, offsets, sizes)]
    out = probe.unpack_checksum_device(arena.data_ptr(), total, segments)
    after = backing.cpu().numpy()
    expect = np.full(cursor, 0xA5, dtype=np.uint8)
    for s, off, n in zip(starts, offsets, sizes):
        expect[s : s + n] = arena_host[off : off + n]
    bad = np.flatnonzero(after != expect)
    assert bad.size == 0, "first wrong destination/guard byte at %d" % bad[0]
    assert np.array_equal(arena.cpu().numpy(), arena_host), "the arena changed"
    got = out["sum"]
    assert got == reference(arena_host.tobytes())
    assert got == probe.checksum_device(arena.data_ptr(), total)
    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    assert got == tuple(native_io.checksum(arena_host.tobytes()))
    assert out["kernel_ms"] >= 0.0
    return got


def edge_sizes(probe):
    tile = probe.pack_tile_bytes()
    return [0, 1, 15, 16, 17, 4095, tile, tile + 1, 3 * tile + 5, (1 << 20) + 3]


# -- csp_unpack_checksum_dev -------------------------------------------------


def test_all_edge_sizes_in_one_call(probe):
    sizes = edge_sizes(probe)
    arena, offsets = make_arena(probe, sizes, seed=1)
    unpack_and_check(probe, arena, sizes, offsets)


@pytest.mark.parametrize("which", range(10))
def test_each_edge_size_alone(probe, which):
    sizes = [edge_sizes(probe)[which]]
    arena, offsets = make_arena(probe, sizes, seed=2 + which)
    got = unpack_and_check(probe, arena, sizes, offsets)
    if sizes[0] == 0:
        assert got == (0, 0)


def test_nonzero_padding_is_summed_and_not_stored(probe):
    sizes = edge_sizes(probe)
    zero_padded, offsets = make_arena(probe, sizes, seed=3)
    dirty, _ = make_arena(probe, sizes, seed=3, padding=0x5C)
    assert not np.array_equal(zero_padded, dirty)
    clean_sum = unpack_and_check(probe, zero_padded, sizes, offsets)
    dirty_sum = unpack_and_check(probe, dirty, sizes, offsets)
    assert dirty_sum != clean_sum


def test_one_flipped_bit_changes_the_sum(probe):
    sizes = edge_sizes(probe)
    arena, offsets = make_arena(probe, sizes, seed=4)
    before = unpack_and_check(probe, arena, sizes, offsets)
    arena[offsets[-1] + 70001] ^= 0x10
    assert unpack_and_check(probe, arena, sizes, offsets) != before


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_tiny_grid_caps_loop_over_many_tiles(probe, cap):
    tile = probe.pack_tile_bytes()
    # 1 + 1 + 5 + 3 + 0 + 9 + 1 + 2 + 0 + 1 + 7 = 30 tiles (zero bytes own none)
    sizes = [tile, 5, 4 * tile + 17, 3 * tile, 0, 8 * tile + 1, 16, tile + 1, 0, 333,
             6 * tile + 4095]
    arena, offsets = make_arena(probe, sizes, seed=5)
    try:
        assert probe.unpack_checksum_grid_cap(cap) == cap
        unpack_and_check(probe, arena, sizes, offsets)
    finally:
        default = probe.unpack_checksum_grid_cap(0)
    assert default >= 1024


def test_more_tiles_than_blocks(probe):
    rng = np.random.default_rng(6)
    sizes = [int(n) for n in rng.integers(0, 5001, 3000)]
    sizes[17] = 0
    assert sum(1 for n in sizes if n) > probe.unpack_checksum_grid_cap(0)
    arena, offsets = make_arena(probe, sizes, seed=7)
    unpack_and_check(probe, arena, sizes, offsets)


def _refusal_fixture(probe):
    sizes = [100, 0, 4096, 33]
    arena_host, offsets = make_arena(probe, sizes, seed=8)
    total = len(arena_host)
    # room before and after the arena inside one allocation
    holder = torch.zeros(total + 4096, dtype=torch.uint8, device="cuda")
    holder[16 : 16 + total] = torch.from_numpy(arena_host).cuda()
    backing = torch.full((4 * 8192,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    arena_ptr = holder.data_ptr() + 16
    dsts = [backing.data_ptr() + 8192 * k for k in range(4)]
    return sizes, offsets, total, holder, arena_ptr, backing, dsts, arena_host


REFUSALS = [
    "misaligned_arena", "misaligned_dst", "misaligned_dst_of_empty_segment",
    "null_dst", "null_arena", "first_offset", "later_offset", "arena_bytes_short",
    "arena_bytes_long", "overflow", "dst_inside_arena", "dst_across_arena_start",
    "dst_across_arena_end",
]


@pytest.mark.parametrize("case", REFUSALS)
def test_refused_calls_launch_nothing(probe, case):
    sizes, offsets, total, holder, arena_ptr, backing, dsts, arena_host = _refusal_fixture(probe)
    sizes, offsets, dsts = list(sizes), list(offsets), list(dsts)
    arena_arg, total_arg = arena_ptr, total
    if case == "misaligned_arena":
        arena_arg += 8
    elif case == "misaligned_dst":
        dsts[2] += 4
    elif case == "misaligned_dst_of_empty_segment":
        dsts[1] += 1
    elif case == "null_dst":
        dsts[0] = 0
    elif case == "null_arena":
        arena_arg = 0
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
    elif case == "dst_inside_arena":
        dsts[2] = arena_ptr + 16
    elif case == "dst_across_arena_start":
        dsts[0] = arena_ptr - 16  # 100 bytes from 16 before the arena
    elif case == "dst_across_arena_end":
        dsts[3] = arena_ptr + total - 16
    segments = list(zip(dsts, offsets, sizes))
    with pytest.raises(probe.GpuLibError, match="csp_unpack_checksum_dev"):
        probe.unpack_checksum_device(arena_arg, total_arg, segments)
    assert backing.cpu().numpy().tobytes() == b"\xa5" * backing.numel()
    after = holder.cpu().numpy()
    assert np.array_equal(after[16 : 16 + total], arena_host)
    assert not after[:16].any() and not after[16 + total :].any()


def test_too_many_segments_are_refused(probe):
    """nseg is checked before any table is read, so one-entry tables do."""
    lib = probe.load()
    arena = torch.zeros(16, dtype=torch.uint8, device="cuda")
    dst_t = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dst = (ctypes.c_void_p * 1)(dst_t.data_ptr())
    off = (ctypes.c_uint64 * 1)(0)
    size = (ctypes.c_uint64 * 1)(16)
    out = (ctypes.c_uint64 * 2)()
    rc = lib.csp_unpack_checksum_dev(
        ctypes.c_void_p(arena.data_ptr()), 16, dst, off, size, 1 << 31, out, None
    )
    assert rc == -1
    assert b"too many" in lib.csp_last_error()
    assert dst_t.cpu().numpy().tobytes() == b"\xa5" * 16


def test_touching_ranges_and_empty_arena_are_fine(probe):
    sizes, offsets, total, holder, arena_ptr, backing, dsts, arena_host = _refusal_fixture(probe)
    # a destination that ends where the arena begins, one that begins where it ends
    holder2 = torch.zeros(total + 8192, dtype=torch.uint8, device="cuda")
    holder2[4096 : 4096 + total] = torch.from_numpy(arena_host).cuda()
    torch.cuda.synchronize()
    arena2 = holder2.data_ptr() + 4096
    segs = [(arena2 - 112, offsets[0], 100), (0, offsets[1], 0),
            (dsts[2], offsets[2], 4096), (arena2 + total, offsets[3], 33)]
    out = probe.unpack_checksum_device(arena2, total, segs)
    assert out["sum"] == reference(arena_host.tobytes())
    after = holder2.cpu().numpy()
    assert np.array_equal(after[4096 - 112 : 4096 - 12], arena_host[:100])
    assert not after[4096 - 12 : 4096].any(), "wrote past a destination into the arena's front"
    assert np.array_equal(after[4096 + total : 4096 + total + 33],
                          arena_host[offsets[3] : offsets[3] + 33])
    assert not after[4096 + total + 33 :].any()
    assert np.array_equal(after[4096 : 4096 + total], arena_host)
    assert probe.unpack_checksum_device(0, 0, [])["sum"] == (0, 0)
    assert probe.unpack_checksum_device(arena2, 0, [(0, 0, 0), (0, 0, 0)])["sum"] == (0, 0)


# -- end to end --------------------------------------------------------------

BIG_ELEMS = 80 * 1024  # float32: 320 KiB, above the staging threshold below
THRESHOLD = 256 * 1024


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


def _make_executor(tmp_path, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor
    from covalent_ssh_plugin_amd.transport import native_io

    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
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


def _packed_total(state):
    """Arena bytes of the packed tensors of ``state`` (distinct objects below
    the threshold), by the layout rule."""
    seen = {}
    for t in state.values():
        if t.numel() * t.element_size() < THRESHOLD:
            seen.setdefault(id(t), t)
    sizes = [t.numel() * t.element_size() for t in seen.values()]
    return len(sizes), sum((n + 15) // 16 * 16 for n in sizes), sum(sizes)


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


@pytest.mark.parametrize("mode", ["persistent", "isolated"])
def test_packed_arguments_are_delivered(tmp_path, mode):
    state = make_args()
    overrides = {} if mode == "persistent" else dict(isolate_tasks=True, isolate_preload="torch")
    ex = _make_executor(tmp_path, **overrides)

    async def run():
        first = await _send(ex, state, 0)
        await ex.close_pool()
        return first

    out, meta = asyncio.run(run())
    _delivered(out, state)
    count, arena_bytes, data_bytes = _packed_total(state)
    assert count == len(state) - 2  # all but "big" and the second name of w3
    stage = meta["arg_staging"]
    assert stage["packed_tensors"] == count
    assert stage["packed_bytes"] == data_bytes
    # one verified arena and the big tensor on its own
    assert stage["tensors"] == 2 and stage["verified"] == 2
    assert stage["bytes"] == arena_bytes + BIG_ELEMS * 4
    assert stage["unpack_ms"] >= 0.0
    assert stage["mode"] == ("pinned-h2d" if mode == "persistent" else "isolated-copy")
    assert "arg_cache" not in meta


def test_wrong_sum_fails_the_task_and_keeps_the_worker(tmp_path, monkeypatch):
    from covalent_ssh_plugin_amd.remote import workers as worker_pool

    ex = _make_executor(tmp_path)
    state = make_args()
    log = tmp_path / "ran.log"
    real = worker_pool.compose_packed_checksum

    def off_by_one(sums, offsets):
        s0, s1 = real(sums, offsets)
        return s0, (s1 + 1) % (1 << 64)

    async def run():
        with monkeypatch.context() as patch:
            patch.setattr(worker_pool, "compose_packed_checksum", off_by_one)
            with pytest.raises(RuntimeError, match="failed its integrity check"):
                await _send(ex, state, 0, log=str(log))
        bad_meta = ex.last_task_record.remote_meta
        out, good_meta = await _send(ex, state, 1, log=str(log))
        await ex.close_pool()
        return bad_meta, out, good_meta

    bad_meta, out, good_meta = asyncio.run(run())
    assert "user_fn" not in bad_meta["phases_ms"], "user code ran on unverified data"
    _delivered(out, state)
    assert good_meta["pid"] == bad_meta["pid"], "the worker was replaced"
    assert good_meta["served"] == bad_meta["served"] + 1
    assert log.read_text() == "ran\n"


def test_arena_is_cached_under_one_key(tmp_path):
    state = make_args()
    count, arena_bytes, _data = _packed_total(state)
    ex = _make_executor(
        tmp_path, cache_tensor_args=True, arg_cache_min_bytes=32 * 1024,
        arg_cache_bytes=arena_bytes + 1024,
    )
    assert arena_bytes >= 32 * 1024
    assert all(
        t.numel() * t.element_size() < 32 * 1024 for n, t in state.items() if n != "big"
    )
    other = {k: (v + 1 if v.dtype == torch.float32 else v) for k, v in make_args().items()}
    other["twice"] = other["w3"]

    async def run():
        a = await _send(ex, state, 0, bump=True)  # store; overwrites its tensors
        saved0 = ex.counters["arg_cache_bytes_saved"]
        b = await _send(ex, state, 1, bump=True)  # hit: sees the original values
        counters_b = dict(ex.counters)
        c = await _send(ex, other, 2)  # another arena: evicts the first
        d = await _send(ex, state, 3)  # a reference to what is gone: one resend
        await ex.close_pool()
        return a, saved0, b, counters_b, c, d

    a, saved0, b, counters_b, c, d = asyncio.run(run())
    for out, _meta in (a, b, d):
        _delivered(out, state)
    _delivered(c[0], other)
    big_bytes = BIG_ELEMS * 4
    # first dispatch: the arena and the big tensor are both stored
    assert len(a[1]["arg_cache"]["stored"]) == 1 and a[1]["arg_cache"]["not_stored"]
    assert saved0 == 0
    # second dispatch: the arena is a hit and no arena frame was sent
    assert counters_b["arg_cache_hits"] == 1
    assert counters_b["arg_cache_bytes_saved"] == arena_bytes
    assert counters_b["arg_cache_misses"] == 0
    assert b[1]["arg_cache"]["hits"] == a[1]["arg_cache"]["stored"]
    assert b[1]["arg_staging"]["bytes"] == big_bytes, "the arena travelled again"
    assert b[1]["arg_staging"]["packed_tensors"] == count
    # third: the budget holds one arena
    assert c[1]["arg_cache"]["evicted"] == a[1]["arg_cache"]["stored"]
    # fourth: exactly one miss and one resend
    assert ex.counters["arg_cache_misses"] == 1
    assert ex.counters["arg_cache_hits"] == 1
    assert d[1]["arg_cache"]["resent"] is True
    assert d[1]["arg_cache"]["stored"] == a[1]["arg_cache"]["stored"]
    assert d[1]["arg_staging"]["bytes"] == arena_bytes + big_bytes
    assert d[1]["served"] == c[1]["served"] + 2, "not exactly one resend"
