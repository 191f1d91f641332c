"""``retain_tensor_results`` without a GPU: option validation, the worker
template's token, and the dispatcher's side against a scripted channel: a
verified reply's retained buffers noted and keyed in the background, the keying
joined before the next request is planned, the worker's name on the wire for a
reference, a patch base and a rebase base, the worker's report mapped back,
evicted names forgotten (before and after their keying), the empty-delta
rebase under the option alone, and a reply without retained buffers handled
as before."""

import asyncio

import cloudpickle
import pytest

torch = pytest.importorskip("torch")

from covalent_ssh_plugin_amd.gpu.probe import pack_layout  # noqa: E402
from covalent_ssh_plugin_amd.ops import build as ops_build  # noqa: E402
from covalent_ssh_plugin_amd.remote import workers as worker_pool  # noqa: E402
from covalent_ssh_plugin_amd.transport import native_io  # noqa: E402
from covalent_ssh_plugin_amd.transport.channel import FrameParts  # noqa: E402

THRESHOLD = 256 * 1024
CACHE_MIN = 8192
NAME = "r:op-a:0"


@pytest.fixture
def io_lib():
    ops_build.build_io(verbose=False)
    assert native_io.load() is not None, "libcsp_io.so did not load"


def raw(t) -> bytes:
    if t.numel() == 0:
        return b""
    return t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()


def make_state(seed=5):
    gen = torch.Generator().manual_seed(seed)
    return {
        "a": torch.randn(1000, generator=gen),  # 4000 bytes
        "b": torch.randn(33, 7, generator=gen).to(torch.bfloat16),  # 462 bytes: padded
        "c": torch.empty(0, 3),
        "d": torch.randn(40, 30, generator=gen),  # 4800 bytes
        "e": torch.tensor(7, dtype=torch.int64),  # 0-d
        "f": torch.randint(0, 256, (4097,), dtype=torch.uint8, generator=gen),  # 1 mod 16
    }


class ScriptedChannel:
    """What run_task touches of a Channel: consumes the request's frames in
    order, then plays the next scripted reply."""

    def __init__(self):
        self.sent = []  # per request: [first frame bytes, payload bytes, ...]
        self.replies = []  # (meta, result, buffers)
        self.log = []

    async def exchange(self, frames, reply_frames, timeout=None):
        self.log.append("planned")
        self.sent.append(
            [f.tobytes() if isinstance(f, FrameParts) else bytes(f) for f in frames]
        )
        op_id = cloudpickle.loads(self.sent[-1][0])["op_id"]
        assert reply_frames(cloudpickle.dumps(("A1", op_id))) is None
        meta, result, buffers = self.replies.pop(0)
        main = cloudpickle.dumps(("R1", cloudpickle.dumps((result, None)), meta, len(buffers)))
        assert reply_frames(main) == len(buffers)
        return main, buffers


def make_handle():
    channel = ScriptedChannel()
    return worker_pool.WorkerHandle(channel=channel, startup_meta={}, key=("t",)), channel


def large_reply(t, name=NAME, evicted=()):
    """The reply of an electron that returned CUDA tensor ``t``, retained."""
    data = bytearray(raw(t))
    info = {"dtype": str(t.dtype).replace("torch.", ""), "shape": list(t.shape),
            "sum": list(native_io.checksum(bytes(data))), "retained": name}
    meta = {"buffers": [info],
            "retained": {"stored": [name], "not_stored": [], "evicted": list(evicted)}}
    return meta, ("__csp_tensor_buffer_v1__", 0), [data]


def arena_reply(state, name=NAME):
    """The reply of an electron that returned ``state`` as CUDA tensors, packed
    into one retained arena."""
    blobs = [raw(t) for t in state.values()]
    offsets, total = pack_layout([len(b) for b in blobs])
    arena = bytearray(total)
    for off, b in zip(offsets, blobs):
        arena[off : off + len(b)] = b
    info = {
        "packed": [
            {"dtype": str(t.dtype).replace("torch.", ""), "shape": list(t.shape),
             "offset": off, "nbytes": len(b)}
            for t, off, b in zip(state.values(), offsets, blobs)
        ],
        "nbytes": total, "sum": list(native_io.checksum(bytes(arena))), "retained": name,
    }
    meta = {"buffers": [info],
            "retained": {"stored": [name], "not_stored": [], "evicted": []}}
    result = {k: ("__csp_packed_tensor_v1__", 0, j) for j, k in enumerate(state)}
    return meta, result, [arena]


async def run(handle, args, op_id="op-b", stats=None, retain_segments=True, **extract):
    """extract_arg_buffers + run_task as the executor calls them."""
    options = dict(to_device=True, cache_min_bytes=CACHE_MIN, pack_min_bytes=0,
                   patch_max_fraction=0.5, rebase=True, retain=True)
    options.update(extract)
    _a, _k, meta, buffers = worker_pool.extract_arg_buffers(args, {}, THRESHOLD, **options)
    return await worker_pool.run_task(
        handle, op_id, ".", b"fn", arg_buffer_meta=meta, arg_buffers=buffers,
        cache_stats=stats, retain_segments=retain_segments,
    )


def wire_of(channel, request=-1):
    return cloudpickle.loads(channel.sent[request][0])["arg_buffers"]


# -- options and template -------------------------------------------------------


def test_option_validation(local_executor):
    from covalent_ssh_plugin_amd.ssh import _EXECUTOR_PLUGIN_DEFAULTS

    assert _EXECUTOR_PLUGIN_DEFAULTS["retain_tensor_results"] is False
    with pytest.raises(ValueError, match="retain_tensor_results needs cache_tensor_args=True"):
        local_executor(retain_tensor_results=True, persistent_workers=True,
                       device_tensor_args=True)
    with pytest.raises(ValueError, match="held as a master in the worker's argument cache"):
        local_executor(retain_tensor_results=True)
    base = dict(persistent_workers=True, device_tensor_args=True, cache_tensor_args=True)
    ex = local_executor(retain_tensor_results=True, **base)
    assert ex.retain_tensor_results is True
    assert ex.counters["results_retained"] == 0 and ex.counters["results_retained_bytes"] == 0
    assert local_executor(**base).retain_tensor_results is False


def test_template_renders_the_token_in_both_values():
    from covalent_ssh_plugin_amd.remote.stub import render_worker

    on = render_worker(arg_cache_bytes=1 << 20, retain_min_bytes=12345)
    assert "RETAIN_MIN_BYTES = int(12345)" in on and "__CSP_" not in on
    compile(on, "worker.py", "exec")
    off = render_worker(arg_cache_bytes=1 << 20)
    assert "RETAIN_MIN_BYTES = int(-1)" in off and "__CSP_" not in off
    compile(off, "worker.py", "exec")
    assert on.replace("int(12345)", "int(-1)") == off
    assert "RETAIN_MIN_BYTES = int(0)" in render_worker(retain_min_bytes=0)


# -- a large retained result ----------------------------------------------------


def test_retained_result_is_keyed_in_the_background_and_referenced_by_name(io_lib, monkeypatch):
    t = torch.arange(5000, dtype=torch.float32)  # 20000 bytes >= CACHE_MIN
    handle, channel = make_handle()
    real = worker_pool._key_retained

    def logged(items):
        channel.log.append("keyed")
        return real(items)

    monkeypatch.setattr(worker_pool, "_key_retained", logged)

    async def main():
        stats = {}
        channel.replies.append(large_reply(t))
        value, exc, meta = await worker_pool.run_task(
            handle, "op-a", ".", b"fn", cache_stats=stats
        )
        # in the caller's hands before anything was hashed
        assert exc is None and torch.equal(value, t)
        assert meta["result_integrity"] == {"verified": 1}
        assert handle.retained == {NAME} and handle.names == {} and handle.resident == set()
        assert len(handle.keying) == 1 and not handle.keying[0].done()
        assert channel.log == ["planned"]
        assert stats == {"results_retained": 1, "results_retained_bytes": 20000}
        # B takes it: the keying is joined before the request is planned
        channel.replies.append(
            ({"buffers": [], "arg_cache": {"hits": [NAME], "stored": [], "miss": []}}, 1, [])
        )
        out, _exc, _meta = await run(handle, [value], stats=stats)
        return value, out, stats

    value, out, stats = asyncio.run(main())
    assert out == 1
    assert channel.log == ["planned", "keyed", "planned"]
    key = worker_pool.content_key(raw(t))
    assert handle.names == {key: NAME} and handle.resident == {key}
    assert handle.retained == {NAME} and handle.keying == []
    # the wire names what the worker holds, and carries no frame for it
    (entry,) = wire_of(channel)
    assert entry["cache"] == {"key": NAME, "ref": True}
    assert len(channel.sent[-1]) == 1
    # the report, in the worker's names, counts under the content key
    assert stats["arg_cache_hits"] == 1 and stats["arg_cache_bytes_saved"] == 20000
    assert stats["arg_cache_misses"] == 0
    # the memo was seeded: the same object is not hashed again
    memo = worker_pool._key_memo[id(value)]
    assert memo[0]() is value and memo[2] == key


def test_another_object_with_the_same_bytes_is_referenced_too(io_lib):
    t = torch.arange(5000, dtype=torch.float32)
    handle, channel = make_handle()

    async def main():
        channel.replies.append(large_reply(t))
        await worker_pool.run_task(handle, "op-a", ".", b"fn")
        channel.replies.append(
            ({"buffers": [], "arg_cache": {"hits": [NAME], "stored": [], "miss": []}}, 1, [])
        )
        await run(handle, [t.clone()])

    asyncio.run(main())
    assert wire_of(channel)[0]["cache"] == {"key": NAME, "ref": True}


def test_a_missed_reference_forgets_the_name_and_the_resend_stores_the_key(io_lib):
    t = torch.arange(5000, dtype=torch.float32)
    handle, channel = make_handle()
    key = worker_pool.content_key(raw(t))

    async def main():
        channel.replies.append(large_reply(t))
        value, _e, _m = await worker_pool.run_task(handle, "op-a", ".", b"fn")
        channel.replies.append(
            ({"buffers": [], "arg_cache": {"hits": [], "stored": [], "miss": [0]}}, None, [])
        )
        channel.replies.append(
            ({"buffers": [], "arg_cache": {"hits": [], "stored": [key], "miss": []}}, 2, [])
        )
        stats = {}
        out, _e, meta = await run(handle, [value], stats=stats)
        return out, meta, stats

    out, meta, stats = asyncio.run(main())
    assert out == 2 and meta["arg_cache"]["resent"] is True
    assert stats["arg_cache_misses"] == 1
    assert wire_of(channel, -2)[0]["cache"] == {"key": NAME, "ref": True}
    assert wire_of(channel, -1)[0]["cache"] == {"key": key, "store": True}
    assert channel.sent[-1][1] == raw(t)
    assert handle.names == {} and handle.retained == set() and handle.resident == {key}


# -- evicted ----------------------------------------------------------------------


def test_evicted_names_and_keys_are_forgotten_at_once(io_lib):
    t = torch.arange(5000, dtype=torch.float32)
    u = torch.arange(6000, dtype=torch.float32)
    handle, channel = make_handle()
    old_key = "0" * 32  # an argument master stored under its content key
    handle.resident.add(old_key)
    handle.resident_arenas[old_key] = (("1" * 32, 16),)

    async def main():
        channel.replies.append(large_reply(t))
        await worker_pool.run_task(handle, "op-a", ".", b"fn")
        await worker_pool.join_retained_keying(handle)
        assert set(handle.names.values()) == {NAME} and old_key in handle.resident
        # the next retained result pushed both out of the worker's budget
        channel.replies.append(large_reply(u, name="r:op-c:0", evicted=[NAME, old_key]))
        await worker_pool.run_task(handle, "op-c", ".", b"fn")
        await worker_pool.join_retained_keying(handle)

    asyncio.run(main())
    key_u = worker_pool.content_key(raw(u))
    assert handle.retained == {"r:op-c:0"} and handle.names == {key_u: "r:op-c:0"}
    assert handle.resident == {key_u} and handle.resident_arenas == {}


def test_a_name_evicted_before_its_keying_finishes_is_never_registered(io_lib):
    t = torch.arange(5000, dtype=torch.float32)
    handle, channel = make_handle()

    async def main():
        channel.replies.append(large_reply(t))
        await worker_pool.run_task(handle, "op-a", ".", b"fn")
        assert handle.retained == {NAME} and not handle.keying[0].done()
        gone = {"buffers": [], "retained": {"stored": [], "not_stored": [], "evicted": [NAME]}}
        worker_pool.retain_results(handle, gone, {}, True)
        assert handle.retained == set()
        await worker_pool.join_retained_keying(handle)

    asyncio.run(main())
    assert handle.names == {} and handle.resident == set() and handle.retained == set()
    assert handle.keying == []


def test_a_tensor_changed_in_place_while_it_is_hashed_is_not_registered(io_lib, monkeypatch):
    t = torch.arange(5000, dtype=torch.float32)
    state = make_state()
    real = worker_pool.tensor_content_key

    def hashed_while_the_caller_writes(tensor, view, threads=None):
        key = real(tensor, view, threads=threads)
        if tensor is t or tensor is state["d"]:
            tensor.add_(1)  # the caller, on another thread, mid-hash
        return key

    quiet = worker_pool._key_retained([("r:x:0", t.clone()), ("r:x:1", list(state.values()))])
    assert [name for name, _k, _s in quiet] == ["r:x:0", "r:x:1"]
    monkeypatch.setattr(worker_pool, "tensor_content_key", hashed_while_the_caller_writes)
    keyed = worker_pool._key_retained(
        [("r:x:0", t), ("r:x:1", list(state.values())), ("r:x:2", t.clone())]
    )
    assert [name for name, _k, _s in keyed] == ["r:x:2"]


# -- a retained arena ------------------------------------------------------------------


def _retained_arena(retain_segments=True):
    state = make_state()
    handle, channel = make_handle()

    async def main():
        channel.replies.append(arena_reply(state))
        value, _e, _m = await worker_pool.run_task(
            handle, "op-a", ".", b"fn", retain_segments=retain_segments
        )
        await worker_pool.join_retained_keying(handle)
        return value

    value = asyncio.run(main())
    assert list(value) == list(state)
    for k in state:
        assert torch.equal(value[k], state[k]), k
    return state, value, handle, channel


def test_retained_arena_is_keyed_as_the_argument_side_keys_it(io_lib):
    state, value, handle, channel = _retained_arena()
    _a, _k, meta, _b = worker_pool.extract_arg_buffers(
        [value], {}, THRESHOLD, to_device=True, cache_min_bytes=CACHE_MIN, pack_min_bytes=0,
        patch_max_fraction=0.5, rebase=True, retain=True,
    )
    key = meta[0]["cache"]["key"]
    assert handle.names == {key: NAME} and handle.resident == {key}
    assert list(handle.resident_arenas) == [key]
    assert handle.resident_arenas[key] == meta[0]["cache"]["segments"]
    # without patch_tensor_args the arena is no base
    _s, _v, plain, _c = _retained_arena(retain_segments=False)
    assert plain.names == {key: NAME} and plain.resident_arenas == {}


def test_reference_rebase_base_and_patch_base_travel_as_the_name(io_lib):
    state, value, handle, channel = _retained_arena()
    (key,) = handle.names
    total = pack_layout([len(raw(t)) for t in state.values()])[1]

    async def main():
        stats = {}
        channel.replies.append(
            ({"buffers": [], "arg_cache": {"hits": [NAME], "stored": [], "miss": []}}, 1, [])
        )
        await run(handle, [value], stats=stats)
        assert wire_of(channel)[0]["cache"] == {"key": NAME, "ref": True}
        assert stats["arg_cache_hits"] == 1 and stats["arg_cache_bytes_saved"] == total
        # one tensor changed: a rebase on the retained arena, named as the worker names it
        changed = dict(value, e=torch.tensor(8, dtype=torch.int64))
        _a, _k, meta, _b = worker_pool.extract_arg_buffers(
            [changed], {}, THRESHOLD, to_device=True, cache_min_bytes=CACHE_MIN,
            pack_min_bytes=0, patch_max_fraction=0.5, rebase=True, retain=True,
        )
        new_key = meta[0]["cache"]["key"]
        report = {"hits": [], "stored": [new_key], "rebased": [[NAME, new_key]], "miss": []}
        channel.replies.append(({"buffers": [], "arg_cache": report}, 2, []))
        await run(handle, [changed], stats=stats)
        entry = wire_of(channel)[0]
        assert entry["cache"]["key"] == new_key
        assert entry["cache"]["rebase"]["base"] == NAME
        assert entry["rebase_nbytes"] == 16 and channel.sent[-1][1] == raw(changed["e"]) + bytes(8)
        assert stats["arg_cache_rebases"] == 1
        assert stats["arg_cache_bytes_saved"] == total + total - 16
        assert handle.resident == {key, new_key} and handle.names == {key: NAME}
        return stats

    asyncio.run(main())
    # in-place patch (no rebase_tensor_args): the base is named, and consumed
    state, value, handle, channel = _retained_arena()
    (key,) = handle.names

    async def patch():
        changed = dict(value, e=torch.tensor(9, dtype=torch.int64))
        _a, _k, meta, _b = worker_pool.extract_arg_buffers(
            [changed], {}, THRESHOLD, to_device=True, cache_min_bytes=CACHE_MIN,
            pack_min_bytes=0, patch_max_fraction=0.5,
        )
        new_key = meta[0]["cache"]["key"]
        report = {"hits": [], "stored": [new_key], "patched": [[NAME, new_key]], "miss": []}
        channel.replies.append(({"buffers": [], "arg_cache": report}, 3, []))
        stats = {}
        await run(handle, [changed], stats=stats, rebase=False, retain=False)
        return new_key, stats

    new_key, stats = asyncio.run(patch())
    entry = wire_of(channel)[0]
    assert entry["cache"] == {"key": new_key, "patch": {"base": NAME, "segments": [4]}}
    assert stats["arg_cache_patches"] == 1
    assert handle.names == {} and handle.retained == set() and handle.resident == {new_key}


def test_the_empty_delta_rebase_only_with_the_option(io_lib):
    for retain in (True, False):
        state, value, handle, channel = _retained_arena()
        (key,) = handle.names
        subset = {k: value[k] for k in ("f", "d", "a")}  # reordered, three left out

        async def main():
            _a, _k, meta, _b = worker_pool.extract_arg_buffers(
                [subset], {}, THRESHOLD, to_device=True, cache_min_bytes=CACHE_MIN,
                pack_min_bytes=0, patch_max_fraction=0.5, rebase=True, retain=retain,
            )
            new_key = meta[0]["cache"]["key"]
            report = {"hits": [], "stored": [new_key], "miss": []}
            if retain:
                report["rebased"] = [[NAME, new_key]]
            channel.replies.append(({"buffers": [], "arg_cache": report}, 1, []))
            stats = {}
            await run(handle, [subset], stats=stats, retain=retain)
            return new_key, stats

        new_key, stats = asyncio.run(main())
        entry = wire_of(channel)[0]
        total = entry["nbytes"]
        if retain:
            assert entry["cache"] == {
                "key": new_key,
                "rebase": {"base": NAME, "base_nbytes": 13392, "sources": [9280, 4464, 0]},
            }
            assert entry["rebase_nbytes"] == 0
            assert channel.sent[-1][1:] == [b""]  # one frame, zero bytes
            assert stats["arg_cache_rebases"] == 1 and stats["arg_cache_bytes_saved"] == total
        else:
            assert entry["cache"] == {"key": new_key, "store": True}
            assert "rebase_nbytes" not in entry and len(channel.sent[-1][1]) == total
            assert "arg_cache_rebases" not in stats
        assert "retain" not in entry["cache"] and "segments" not in entry["cache"]


# -- nothing retained ----------------------------------------------------------------------


def test_a_reply_without_retained_buffers_is_handled_as_before(io_lib):
    t = torch.arange(5000, dtype=torch.float32)
    handle, channel = make_handle()
    meta, result, buffers = large_reply(t)
    del meta["retained"], meta["buffers"][0]["retained"], meta["buffers"][0]["sum"]

    async def main():
        channel.replies.append((meta, result, buffers))
        return await worker_pool.run_task(handle, "op-a", ".", b"fn", cache_stats={})

    value, exc, got = asyncio.run(main())
    assert exc is None and torch.equal(value, t)
    assert got == {"buffers": [{"dtype": "float32", "shape": [5000]}]}
    assert handle.retained == set() and handle.names == {} and handle.keying == []
    # _reconstruct with its three arguments, as other callers use it
    again = worker_pool._reconstruct(result, meta["buffers"], [bytearray(raw(t))])
    assert torch.equal(again, t)
    state = make_state()
    meta, result, buffers = arena_reply(state)
    plain = worker_pool._reconstruct(result, meta["buffers"], buffers)
    collected = {}
    same = worker_pool._reconstruct(result, meta["buffers"], buffers, collected)
    assert list(plain) == list(same) == list(state)
    assert all(torch.equal(plain[k], same[k]) for k in state)
    assert set(collected) == {(0, j) for j in range(len(state))}
