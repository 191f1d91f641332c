"""MI355X tests for ``retain_tensor_results`` end to end through a loopback
worker: electron A returns CUDA tensors, the worker keeps them in HBM as
argument masters, electron B takes them and only their name travels.  One
large tensor (aligned and as a view one byte past a boundary), a deep copy,
an in-place change, a dict of small tensors as one arena (hit, empty-delta
rebase, one-segment rebase), the budget, the integrity failure, a wrong sum on
a reference and a respawned worker.

The thresholds are low so that a 2 MiB tensor counts as large: a CUDA result
of at least 1,100,000 bytes is its own buffer, smaller ones share the arena,
and an arena of at least that many bytes is kept."""

import asyncio
import copy
import hashlib
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

STAGING = 3 << 19  # 1.5 MiB
CACHE_MIN = 1_100_000
BIG = (2 << 20) + 3
BIG_ROUNDED = (BIG + 15) // 16 * 16
TILE = 16384
EDGE_SIZES = [0, 1, 15, 16, 17, 4095, TILE, TILE + 1, 3 * TILE + 5, (1 << 20) + 3]
ARENA = sum((n + 15) // 16 * 16 for n in EDGE_SIZES)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests require a visible MI355X (torch.cuda unavailable)")


def _make_electrons():
    """Local functions, so cloudpickle ships them by value."""

    def host_bytes(nbytes, seed):
        import torch

        gen = torch.Generator().manual_seed(seed)
        return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=gen)

    def produce(nbytes, seed, offset=0):
        """A: one CUDA tensor whose first byte lies ``offset`` bytes past a
        16-byte boundary."""
        import torch

        base = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
        out = base[offset : offset + nbytes]
        out.copy_(host_bytes(nbytes, seed))
        assert out.data_ptr() % 16 == offset
        torch.cuda.synchronize()
        return out

    def produce_dict(sizes, seed):
        """A: a dict of small CUDA tensors, one per size."""
        import torch

        out = {"t%d" % i: host_bytes(n, seed + i).cuda() for i, n in enumerate(sizes)}
        torch.cuda.synchronize()
        return out

    def consume(value):
        """B: where the tensors are and a digest of each one's bytes."""
        import hashlib
        import os

        tensors = value if isinstance(value, dict) else {"x": value}
        return {
            "pid": os.getpid(),
            "cuda": all(t.is_cuda for t in tensors.values()),
            "digests": {
                name: hashlib.blake2b(t.cpu().numpy().tobytes(), digest_size=16).hexdigest()
                for name, t in tensors.items()
            },
        }

    return host_bytes, produce, produce_dict, consume


_host_bytes, _produce, _produce_dict, _consume = _make_electrons()


def _digest(t):
    return hashlib.blake2b(t.numpy().tobytes(), digest_size=16).hexdigest()


def _make_executor(tmp_path, monkeypatch, name="home", **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor
    from covalent_ssh_plugin_amd.transport import native_io
    from covalent_ssh_plugin_amd.transport.channel import Channel

    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    monkeypatch.setattr(Channel, "large_frame_threshold", 1 << 20)
    home = tmp_path / name
    home.mkdir()
    options = dict(
        transport="local",
        local_home=str(home),
        cache_dir=str(tmp_path / ("cache-" + name)),
        python_path=sys.executable,
        gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True,
        device_tensor_args=True,
        cache_tensor_args=True,
        arg_cache_min_bytes=CACHE_MIN,
        arg_cache_bytes=64 << 20,
        pack_tensor_results=True,
        pack_results_min_bytes=0,
        pack_tensor_args=True,
        pack_args_min_bytes=0,
        patch_tensor_args=True,
        rebase_tensor_args=True,
        retain_tensor_results=True,
        pinned_staging_threshold_bytes=STAGING,
        # one slot, so every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
    )
    options.update(overrides)
    return SSHExecutor(**options)


_node = [0]


async def _run(ex, fn, *args):
    _node[0] += 1
    out = await ex.execute(fn, list(args), {}, dispatch_id="r", node_id=_node[0])
    return out, ex.last_task_record.remote_meta


def _handle():
    from covalent_ssh_plugin_amd.remote import workers as worker_pool

    (handle,) = [h for h in worker_pool._workers.values() if h.alive]
    return handle


def _assert_retained_large(meta, nbytes):
    (info,) = meta["buffers"]
    assert info["shape"] == [nbytes] and info["dtype"] == "uint8"
    assert len(info["sum"]) == 2
    name = info["retained"]
    assert name.startswith("r:") and name.endswith(":0")
    assert meta["retained"] == {"stored": [name], "not_stored": [], "evicted": []}
    assert meta["result_integrity"]["verified"] == 1
    staging = meta["staging"]
    assert "retain_fallback" not in staging, staging
    assert staging["retained_buffers"] == 1 and staging["retained_bytes"] == nbytes
    assert staging["retain_ms"] >= 0.0 and staging["pinned_tensors"] == 1
    return name


# -- one large tensor ----------------------------------------------------------


@pytest.mark.parametrize("offset", [0, 1])
def test_large_result_is_one_hit_as_an_argument(tmp_path, monkeypatch, offset):
    on = _make_executor(tmp_path, monkeypatch)
    off = _make_executor(tmp_path, monkeypatch, name="off", retain_tensor_results=False)
    want = _host_bytes(BIG, 3)

    async def run():
        rows = []
        for ex in (on, off):
            value, meta_a = await _run(ex, _produce, BIG, 3, offset)
            before = dict(ex.counters)
            out, meta_b = await _run(ex, _consume, value)
            rows.append((value, meta_a, out, meta_b, before, dict(ex.counters)))
        await on.close_pool()
        return rows

    (value, meta_a, out, meta_b, before, after), off_row = asyncio.run(run())
    assert torch.equal(value, want) and not value.is_cuda
    name = _assert_retained_large(meta_a, BIG)
    assert before["results_retained"] == 1 and before["results_retained_bytes"] == BIG
    # B: one hit, no argument byte on the wire, a private exact copy
    assert out["cuda"] is True and out["digests"] == {"x": _digest(want)}
    assert after["arg_cache_hits"] == before["arg_cache_hits"] + 1 == 1
    assert after["arg_cache_bytes_saved"] == BIG and after["arg_cache_misses"] == 0
    assert meta_b["arg_cache"]["hits"] == [name]
    assert meta_b["arg_staging"]["mode"] == "cached" and meta_b["arg_staging"]["bytes"] == 0
    assert out["pid"] == meta_a["pid"]
    # the same chain with the option off: today's reply, and B is a store
    value, meta_a, out, meta_b, before, after = off_row
    assert torch.equal(value, want)
    assert meta_a["buffers"] == [{"dtype": "uint8", "shape": [BIG]}]
    assert "retained" not in meta_a and "result_integrity" not in meta_a
    assert "retained_buffers" not in meta_a["staging"]
    assert out["digests"] == {"x": _digest(want)}
    assert after["arg_cache_hits"] == 0 and after["arg_cache_bytes_saved"] == 0
    assert after["results_retained"] == 0
    assert meta_b["arg_staging"]["bytes"] == BIG
    assert len(meta_b["arg_cache"]["stored"]) == 1 and not meta_b["arg_cache"]["hits"]


def test_a_deep_copy_hits_and_an_in_place_change_is_a_plain_store(tmp_path, monkeypatch):
    ex = _make_executor(tmp_path, monkeypatch)
    want = _host_bytes(BIG, 4)

    async def run():
        value, meta_a = await _run(ex, _produce, BIG, 4)
        other = copy.deepcopy(value)  # another object, the same bytes
        assert other is not value and other.data_ptr() != value.data_ptr()
        out_copy, meta_copy = await _run(ex, _consume, other)
        hit = dict(ex.counters)
        value[5] ^= 0x40  # changed in place before it goes on
        out_changed, meta_changed = await _run(ex, _consume, value)
        await ex.close_pool()
        return value, meta_a, out_copy, meta_copy, hit, out_changed, meta_changed

    value, meta_a, out_copy, meta_copy, hit, out_changed, meta_changed = asyncio.run(run())
    name = _assert_retained_large(meta_a, BIG)
    assert out_copy["digests"] == {"x": _digest(want)}
    assert hit["arg_cache_hits"] == 1 and hit["arg_cache_bytes_saved"] == BIG
    assert meta_copy["arg_cache"]["hits"] == [name]
    assert meta_copy["arg_staging"]["mode"] == "cached"
    changed = want.clone()
    changed[5] ^= 0x40
    assert torch.equal(value, changed)
    assert out_changed["digests"] == {"x": _digest(changed)}
    assert ex.counters["arg_cache_hits"] == 1 and ex.counters["arg_cache_misses"] == 0
    assert "resent" not in meta_changed["arg_cache"]
    assert len(meta_changed["arg_cache"]["stored"]) == 1
    assert meta_changed["arg_staging"]["bytes"] == BIG


# -- a dict of small tensors: one arena ------------------------------------------


def test_small_results_are_one_arena_hit_rebased_and_rebased_again(tmp_path, monkeypatch):
    ex = _make_executor(tmp_path, monkeypatch)
    assert CACHE_MIN <= ARENA - 48 and max(EDGE_SIZES) < CACHE_MIN < STAGING
    want = {"t%d" % i: _host_bytes(n, 20 + i) for i, n in enumerate(EDGE_SIZES)}

    async def run():
        value, meta_a = await _run(ex, _produce_dict, EDGE_SIZES, 20)
        same, meta_same = await _run(ex, _consume, value)
        c_same = dict(ex.counters)
        # a reversed subset: without the 1-byte and the 17-byte tensor
        subset = {k: value[k] for k in reversed(list(value)) if k not in ("t1", "t4")}
        sub, meta_sub = await _run(ex, _consume, subset)
        c_sub = dict(ex.counters)
        changed = dict(value)
        changed["t5"] = value["t5"] ^ 0xFF  # the 4095-byte tensor
        chg, meta_chg = await _run(ex, _consume, changed)
        await ex.close_pool()
        return value, meta_a, same, meta_same, c_same, sub, meta_sub, c_sub, chg, meta_chg

    (value, meta_a, same, meta_same, c_same, sub, meta_sub, c_sub, chg,
     meta_chg) = asyncio.run(run())
    assert list(value) == list(want)
    for k in want:
        assert torch.equal(value[k], want[k]), k
    # A: one packed arena, retained under the worker's name
    (info,) = meta_a["buffers"]
    assert info["nbytes"] == ARENA and len(info["packed"]) == len(EDGE_SIZES)
    name = info["retained"]
    assert meta_a["retained"] == {"stored": [name], "not_stored": [], "evicted": []}
    assert meta_a["staging"]["retained_bytes"] == ARENA
    assert "pack_fallback" not in meta_a["staging"] and "retain_fallback" not in meta_a["staging"]
    assert meta_a["result_integrity"]["verified"] == 1
    digests = {k: _digest(t) for k, t in want.items()}
    # B with the same dict: a hit on the arena
    assert same["cuda"] and same["digests"] == digests
    assert c_same["arg_cache_hits"] == 1 and c_same["arg_cache_bytes_saved"] == ARENA
    assert meta_same["arg_cache"]["hits"] == [name]
    assert meta_same["arg_staging"]["mode"] == "cached"
    # B with a reversed subset: one rebase with an empty delta
    assert sub["digests"] == {k: digests[k] for k in reversed(list(want)) if k not in ("t1", "t4")}
    assert c_sub["arg_cache_rebases"] == 1 and c_sub["arg_cache_misses"] == 0
    assert c_sub["arg_cache_bytes_saved"] == ARENA + (ARENA - 48)
    stage = meta_sub["arg_staging"]
    assert stage["rebased_bytes"] == 0 and stage["rebased_segments"] == 0
    assert stage["bytes"] == 0
    assert [pair[0] for pair in meta_sub["arg_cache"]["rebased"]] == [name]
    # B with one tensor changed: a rebase whose delta is that segment
    assert chg["digests"] == dict(digests, t5=_digest(want["t5"] ^ 0xFF))
    assert ex.counters["arg_cache_rebases"] == 2 and ex.counters["arg_cache_misses"] == 0
    stage = meta_chg["arg_staging"]
    assert stage["rebased_bytes"] == 4096 and stage["rebased_segments"] == 1
    assert stage["bytes"] == 4096
    assert [pair[0] for pair in meta_chg["arg_cache"]["rebased"]] == [name]
    assert {same["pid"], sub["pid"], chg["pid"]} == {meta_a["pid"]}


# -- the budget ----------------------------------------------------------------------


def test_a_budget_for_one_result_evicts_the_first_which_is_then_a_store(tmp_path, monkeypatch):
    ex = _make_executor(tmp_path, monkeypatch, arg_cache_bytes=BIG_ROUNDED + 1024)

    async def run():
        first, meta_1 = await _run(ex, _produce, BIG, 5)
        second, meta_2 = await _run(ex, _produce, BIG, 6)
        handle = _handle()
        believed = set(handle.retained)
        out, meta_b = await _run(ex, _consume, first)
        await ex.close_pool()
        return first, meta_1, second, meta_2, believed, out, meta_b

    first, meta_1, second, meta_2, believed, out, meta_b = asyncio.run(run())
    name_1 = _assert_retained_large(meta_1, BIG)
    name_2 = meta_2["buffers"][0]["retained"]
    assert meta_2["retained"] == {"stored": [name_2], "not_stored": [], "evicted": [name_1]}
    assert believed == {name_2}
    assert torch.equal(second, _host_bytes(BIG, 6))
    # the evicted result costs a plain store: no reference, no miss, no resend
    assert out["digests"] == {"x": _digest(_host_bytes(BIG, 5))}
    assert ex.counters["arg_cache_misses"] == 0 and ex.counters["arg_cache_hits"] == 0
    assert "resent" not in meta_b["arg_cache"]
    assert meta_b["arg_staging"]["bytes"] == BIG
    assert meta_b["served"] == meta_2["served"] + 1


def test_a_result_larger_than_the_budget_is_not_retained(tmp_path, monkeypatch):
    ex = _make_executor(tmp_path, monkeypatch, arg_cache_bytes=STAGING)

    async def run():
        value, meta = await _run(ex, _produce, BIG, 7, 1)
        handle = _handle()
        state = (set(handle.retained), dict(handle.names))
        await ex.close_pool()
        return value, meta, state

    value, meta, state = asyncio.run(run())
    assert torch.equal(value, _host_bytes(BIG, 7))
    assert meta["buffers"] == [{"dtype": "uint8", "shape": [BIG]}]  # today's path
    assert meta["retained"]["stored"] == [] and meta["retained"]["evicted"] == []
    assert len(meta["retained"]["not_stored"]) == 1
    assert "budget" in meta["staging"]["retain_fallback"]
    assert meta["staging"]["retained_buffers"] == 0 and meta["staging"]["retained_bytes"] == 0
    assert state == (set(), {})
    assert ex.counters["results_retained"] == 0


# -- failures ------------------------------------------------------------------------


def test_a_corrupted_frame_fails_and_registers_nothing(tmp_path, monkeypatch):
    from covalent_ssh_plugin_amd.transport import native_io

    ex = _make_executor(tmp_path, monkeypatch)
    real = native_io.checksum

    def off_by_one(*args, **kwargs):
        s0, s1 = real(*args, **kwargs)
        return s0, (s1 + 1) % (1 << 64)

    async def run():
        _, meta_0 = await _run(ex, _consume, torch.zeros(4))  # starts the worker
        with monkeypatch.context() as patch:
            patch.setattr(native_io, "checksum", off_by_one)
            with pytest.raises(RuntimeError, match="integrity") as failure:
                await _run(ex, _produce, BIG, 8)
        handle = _handle()
        state = (set(handle.retained), dict(handle.names), set(handle.resident))
        value, meta = await _run(ex, _produce, BIG, 9)
        await ex.close_pool()
        return meta_0, str(failure.value), state, value, meta

    meta_0, message, state, value, meta = asyncio.run(run())
    assert "result buffer 0" in message
    assert state == (set(), {}, set())
    assert ex.counters["results_retained"] == 1  # the later, verified one alone
    assert torch.equal(value, _host_bytes(BIG, 9))
    assert meta["pid"] == meta_0["pid"], "the worker was replaced"


def test_a_wrong_sum_on_a_reference_to_a_retained_master_is_one_resend(tmp_path, monkeypatch):
    import cloudpickle

    from covalent_ssh_plugin_amd.remote import workers as worker_pool

    ex = _make_executor(tmp_path, monkeypatch)
    real = worker_pool._ArgCacheSend.frames
    spoiled = []

    def frames(self, full):
        """A reference goes out with another checksum."""
        inner = real(self, full)
        first = next(inner)
        request = cloudpickle.loads(first)
        for info in request["arg_buffers"]:
            if (info.get("cache") or {}).get("ref"):
                info["sum"] = [info["sum"][0], info["sum"][1] ^ 1]
                spoiled.append(info["cache"]["key"])
                first = cloudpickle.dumps(request)
        yield first
        yield from inner

    async def run():
        value, meta_a = await _run(ex, _produce, BIG, 10)
        with monkeypatch.context() as patch:
            patch.setattr(worker_pool._ArgCacheSend, "frames", frames)
            out, meta_b = await _run(ex, _consume, value)
        handle = _handle()
        state = (set(handle.retained), dict(handle.names))
        await ex.close_pool()
        return meta_a, out, meta_b, state

    meta_a, out, meta_b, state = asyncio.run(run())
    name = _assert_retained_large(meta_a, BIG)
    assert spoiled == [name], "the first attempt was not a reference by name"
    assert out["digests"] == {"x": _digest(_host_bytes(BIG, 10))}
    assert ex.counters["arg_cache_misses"] == 1 and ex.counters["arg_cache_hits"] == 0
    assert meta_b["arg_cache"]["resent"] is True
    assert meta_b["served"] == meta_a["served"] + 2, "not exactly one resend"
    assert meta_b["arg_staging"]["bytes"] == BIG
    assert state == (set(), {}), "the name is still believed held"


def test_a_respawned_worker_is_assumed_to_hold_nothing(tmp_path, monkeypatch):
    from covalent_ssh_plugin_amd.remote import workers as worker_pool

    ex = _make_executor(tmp_path, monkeypatch)

    async def run():
        value, meta_a = await _run(ex, _produce, BIG, 11)
        assert _handle().retained
        for key in list(worker_pool._workers):
            await worker_pool.kill(key)
        out, meta_b = await _run(ex, _consume, value)
        handle = _handle()
        state = (set(handle.retained), dict(handle.names))
        await ex.close_pool()
        return meta_a, out, meta_b, state

    meta_a, out, meta_b, state = asyncio.run(run())
    _assert_retained_large(meta_a, BIG)
    assert out["pid"] != meta_a["pid"]
    assert out["digests"] == {"x": _digest(_host_bytes(BIG, 11))}
    assert ex.counters["arg_cache_hits"] == 0 and ex.counters["arg_cache_misses"] == 0
    assert "resent" not in meta_b["arg_cache"]
    assert len(meta_b["arg_cache"]["stored"]) == 1
    assert meta_b["arg_staging"]["bytes"] == BIG
    assert state == (set(), {})
