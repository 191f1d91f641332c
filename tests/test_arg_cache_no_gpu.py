"""``cache_tensor_args`` without a GPU: the content key, the threaded
checksum, the per-tensor key memo, the constructor's refusals, and a worker
that cannot take device arguments (no resend loop, the resident set comes
back empty)."""

import asyncio

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from covalent_ssh_plugin_amd.remote import workers as worker_pool  # noqa: E402
from covalent_ssh_plugin_amd.transport import native_io  # noqa: E402

SMALL_CHUNK = 4096


def _bytes(n, seed=7):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


# -- content key -------------------------------------------------------------


@pytest.mark.parametrize("chunk", [worker_pool.ARG_CACHE_CHUNK, SMALL_CHUNK])
def test_equal_bytes_give_equal_keys(chunk):
    raw = _bytes(10 * SMALL_CHUNK + 8)
    as_float = torch.frombuffer(bytearray(raw.tobytes()), dtype=torch.float32)
    as_int = torch.frombuffer(bytearray(raw.tobytes()), dtype=torch.int16)
    keys = {
        worker_pool.content_key(raw, chunk),
        worker_pool.content_key(raw.copy(), chunk),
        worker_pool.content_key(as_float.numpy(), chunk),
        worker_pool.content_key(as_int.numpy(), chunk),
        worker_pool.content_key(raw.tobytes(), chunk, threads=1),
    }
    assert len(keys) == 1
    (key,) = keys
    assert len(bytes.fromhex(key)) == 16


@pytest.mark.parametrize("chunk", [worker_pool.ARG_CACHE_CHUNK, SMALL_CHUNK])
@pytest.mark.parametrize("where", [0, SMALL_CHUNK - 1, SMALL_CHUNK, 10 * SMALL_CHUNK + 7])
def test_one_flipped_byte_changes_the_key(chunk, where):
    raw = _bytes(10 * SMALL_CHUNK + 8)
    other = raw.copy()
    other[where] ^= 0x01
    assert worker_pool.content_key(raw, chunk) != worker_pool.content_key(other, chunk)


def test_the_byte_count_is_part_of_the_key():
    zeros = np.zeros(2 * SMALL_CHUNK, dtype=np.uint8)
    assert worker_pool.content_key(zeros[:SMALL_CHUNK], SMALL_CHUNK) != worker_pool.content_key(
        zeros[: SMALL_CHUNK + 1], SMALL_CHUNK
    )
    assert worker_pool.content_key(b"", SMALL_CHUNK) != worker_pool.content_key(
        b"\0", SMALL_CHUNK
    )


@pytest.mark.parametrize("chunk", [worker_pool.ARG_CACHE_CHUNK, SMALL_CHUNK])
def test_perturbation_that_keeps_the_checksum_changes_the_key(chunk):
    """+1, -2, +1 on three neighbouring words leaves s0 (the sum) and s1
    (the sum weighted by position) as they were: the checksum cannot be
    the identity of a cache entry."""
    words = np.random.default_rng(3).integers(10, 1 << 31, 5000, dtype=np.uint32)
    other = words.copy()
    other[2000] += 1
    other[2001] -= 2
    other[2002] += 1
    assert native_io.load() is not None, "libcsp_io.so was not built"
    assert native_io.checksum(words) == native_io.checksum(other)
    assert worker_pool.content_key(words, chunk) != worker_pool.content_key(other, chunk)


# -- threaded checksum -------------------------------------------------------


@pytest.mark.parametrize(
    "nbytes",
    [0, 1, 3, SMALL_CHUNK - 1, SMALL_CHUNK, SMALL_CHUNK + 1, 2 * SMALL_CHUNK,
     2 * SMALL_CHUNK + 2, 7 * SMALL_CHUNK + 3, 16 * SMALL_CHUNK + 4093],
)
@pytest.mark.parametrize("threads", [None, 1, 3])
def test_threaded_sum_equals_one_call(nbytes, threads):
    assert native_io.load() is not None, "libcsp_io.so was not built"
    raw = _bytes(16 * SMALL_CHUNK + 4093, seed=11)[:nbytes]
    # heavy words, so the position weights overflow 64 bits and wrap
    raw[3::4] |= 0xF0
    assert worker_pool.threaded_checksum(raw, SMALL_CHUNK, threads) == native_io.checksum(raw)


def test_threaded_sum_matches_the_definition():
    """Both the single call and the composition against the sums written
    out from their definition in exact integers."""
    assert native_io.load() is not None, "libcsp_io.so was not built"
    raw = _bytes(4 * SMALL_CHUNK, seed=5)
    one_call = native_io.checksum(raw)
    assert worker_pool.threaded_checksum(raw, SMALL_CHUNK) == one_call
    # by hand, from the definition
    words = raw.view("<u4").astype(object)
    s0 = sum(words) % (1 << 64)
    s1 = sum(int(w) * (i + 1) for i, w in enumerate(words)) % (1 << 64)
    assert one_call == (s0, s1)


def test_threaded_sum_refuses_a_chunk_that_is_no_power_of_two():
    with pytest.raises(ValueError):
        worker_pool.threaded_checksum(b"abcdefgh", 6)


def test_no_sum_without_the_library(monkeypatch):
    monkeypatch.setattr(native_io, "force_absent", True)
    assert worker_pool.threaded_checksum(_bytes(100), SMALL_CHUNK) is None
    t = torch.arange(4096, dtype=torch.float32)
    _a, _k, meta, _bufs = worker_pool.extract_arg_buffers(
        [t], {}, 1 << 30, to_device=True, cache_min_bytes=1
    )
    assert "sum" not in meta[0] and "cache" not in meta[0]


def test_pool_is_small():
    assert 1 <= worker_pool.hash_threads() <= 8


# -- extraction and the memo -------------------------------------------------


def test_entries_carry_the_key_from_the_threshold_up():
    assert native_io.load() is not None, "libcsp_io.so was not built"
    big = torch.arange(4096, dtype=torch.float32)  # 16 KiB
    small = torch.arange(16, dtype=torch.float32)
    _a, _k, meta, _bufs = worker_pool.extract_arg_buffers(
        [big, small], {}, 1 << 30, to_device=True, cache_min_bytes=4096
    )
    assert meta[0]["cache"] == {"key": worker_pool.content_key(big.numpy())}
    assert meta[0]["sum"] == list(native_io.checksum(big.numpy()))
    assert "cache" not in meta[1] and "sum" in meta[1]
    # the option off: exactly the entries of before
    _a, _k, meta_off, _bufs = worker_pool.extract_arg_buffers(
        [big, small], {}, 1 << 30, to_device=True
    )
    assert all("cache" not in info for info in meta_off)
    assert meta_off[0]["sum"] == meta[0]["sum"]


def test_memo_follows_in_place_changes(monkeypatch):
    assert native_io.load() is not None, "libcsp_io.so was not built"
    calls = []
    real = worker_pool.content_key

    def counting(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(worker_pool, "content_key", counting)
    t = torch.arange(4096, dtype=torch.float32)

    def key_of(tensor):
        _a, _k, meta, _bufs = worker_pool.extract_arg_buffers(
            [tensor], {}, 1 << 30, to_device=True, cache_min_bytes=1
        )
        return meta[0]["cache"]["key"]

    first = key_of(t)
    assert key_of(t) == first
    assert len(calls) == 1, "the second dispatch hashed again"
    t.add_(1)  # bumps _version
    changed = key_of(t)
    assert changed != first and len(calls) == 2
    assert changed == real(t.numpy())
    # an equal tensor that is another object has the same key
    assert key_of(t.clone()) == changed


def test_memo_lets_go_of_dead_tensors():
    import gc

    assert native_io.load() is not None, "libcsp_io.so was not built"

    def dispatch_one():
        t = torch.arange(4096, dtype=torch.float32)
        worker_pool.extract_arg_buffers(
            [t], {}, 1 << 30, to_device=True, cache_min_bytes=1
        )
        assert id(t) in worker_pool._key_memo
        return id(t)

    ident = dispatch_one()
    gc.collect()
    assert ident not in worker_pool._key_memo, "the memo kept a dead tensor"


# -- constructor -------------------------------------------------------------


def test_defaults():
    from covalent_ssh_plugin_amd.ssh import _EXECUTOR_PLUGIN_DEFAULTS

    assert _EXECUTOR_PLUGIN_DEFAULTS["cache_tensor_args"] is False
    assert _EXECUTOR_PLUGIN_DEFAULTS["arg_cache_bytes"] == 8 << 30
    assert _EXECUTOR_PLUGIN_DEFAULTS["arg_cache_min_bytes"] > 0


@pytest.mark.parametrize(
    "options, message",
    [
        (dict(cache_tensor_args=True), "device_tensor_args"),
        (dict(cache_tensor_args=True, persistent_workers=True), "device_tensor_args"),
        (dict(cache_tensor_args=True, device_tensor_args=True, isolate_tasks=True),
         "isolate_tasks.*zygote"),
        (dict(cache_tensor_args=True, device_tensor_args=True, persistent_workers=True,
              isolate_tasks=True), "isolate_tasks.*zygote"),
        (dict(cache_tensor_args=True, device_tensor_args=True, persistent_workers=True,
              arg_cache_bytes=0), "arg_cache_bytes"),
        (dict(cache_tensor_args=True, device_tensor_args=True, persistent_workers=True,
              arg_cache_min_bytes=-1), "arg_cache_min_bytes"),
    ],
)
def test_refused_option_combinations(local_executor, options, message):
    with pytest.raises(ValueError, match=message):
        local_executor(**options)


def test_accepted_options_reach_the_executor_and_its_stats(local_executor):
    ex = local_executor(
        persistent_workers=True, device_tensor_args=True, cache_tensor_args=True,
        arg_cache_bytes=1 << 20, arg_cache_min_bytes=4096,
    )
    assert (ex.cache_tensor_args, ex.arg_cache_bytes, ex.arg_cache_min_bytes) == (
        True, 1 << 20, 4096,
    )
    counters = ex.stats()["counters"]
    assert counters["arg_cache_hits"] == 0
    assert counters["arg_cache_misses"] == 0
    assert counters["arg_cache_bytes_saved"] == 0


def test_worker_script_carries_the_budget():
    from covalent_ssh_plugin_amd.remote.stub import render_worker

    text = render_worker(arg_cache_bytes=12345)
    assert "__CSP_" not in text
    assert "ARG_CACHE_BYTES = int(12345)" in text
    assert "ARG_CACHE_BYTES = int(0)" in render_worker()


# -- a worker that cannot take device arguments --------------------------------


def test_worker_without_gpu_library_no_resend_loop(local_executor, monkeypatch):
    from covalent_ssh_plugin_amd.gpu import probe
    from covalent_ssh_plugin_amd.transport.channel import Channel

    assert native_io.load() is not None, "libcsp_io.so was not built"
    monkeypatch.setattr(probe, "local_gpu_lib_path", lambda: "")
    ex = local_executor(
        persistent_workers=True, device_tensor_args=True, cache_tensor_args=True,
        arg_cache_min_bytes=4096, cpu_workers=1,
        # on a host with several GPUs too, every electron meets one worker
        hip_visible_devices_policy="fixed", fixed_gpu=0,
    )
    exchanges = []
    real_exchange = Channel.exchange

    async def counting(self, *args, **kwargs):
        exchanges.append(1)
        return await real_exchange(self, *args, **kwargs)

    monkeypatch.setattr(Channel, "exchange", counting)

    def takes_tensor(t):
        return float(t.sum())  # must never run

    def plain(x):
        import os

        return x + 1, os.getpid()

    big = torch.arange(64 * 1024 // 4, dtype=torch.float32)

    async def main():
        _, pid0 = await ex.execute(plain, [0], {}, dispatch_id="d", node_id=0)
        metas = []
        for node in (1, 2):  # the store, then what would have been a reference
            with pytest.raises(RuntimeError, match="need a GPU worker with the CDNA4 library"):
                await ex.execute(takes_tensor, [big.clone()], {}, dispatch_id="d", node_id=node)
            metas.append(ex.last_task_record.remote_meta)
            handles = list(worker_pool._workers.values())
            assert len(handles) == 1
            assert handles[0].resident == set(), "resident set was not reconciled"
        value, pid1 = await ex.execute(plain, [41], {}, dispatch_id="d", node_id=3)
        await ex.close_pool()
        return pid0, metas, value, pid1

    pid0, metas, value, pid1 = asyncio.run(main())
    assert value == 42 and pid1 == pid0, "the worker was replaced"
    assert len(exchanges) == 4, "a task was sent more than once"
    for meta in metas:
        assert meta["pid"] == pid0
        assert "user_fn" not in meta["phases_ms"]
        report = meta["arg_cache"]
        assert report["miss"] == [] and report["stored"] == [] and report["hits"] == []
        assert "resent" not in report
        assert meta["arg_staging"]["bytes"] == 0
    assert ex.counters["arg_cache_hits"] == 0
    assert ex.counters["arg_cache_misses"] == 0
