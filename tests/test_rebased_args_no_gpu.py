"""``rebase_tensor_args`` without a GPU: option validation, what the option
leaves alone when it is off, the dispatcher's rebase plan against a fake
worker handle (which base wins, ties, the fraction bound, the candidate bound,
duplicates and zero-byte segments, the delta frame, the wire meta, the
resident sets after the send and after the worker's report, the counters, the
full resend), the worker's check of ``sources``, and a rebase entry against a
worker that cannot take device arguments."""

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


@pytest.fixture
def io_lib():
    ops_build.build_io(verbose=False)
    assert native_io.load() is not None, "libcsp_io.so did not load"


def raw(t) -> bytes:
    """The contiguous bytes of a CPU tensor."""
    if t.numel() == 0:
        return b""
    return t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()


def materialise(blobs) -> bytes:
    """The arena that the layout rule describes, as bytes."""
    offsets, total = pack_layout([len(b) for b in blobs])
    arena = bytearray(total)
    for off, b in zip(offsets, blobs):
        arena[off : off + len(b)] = b
    return bytes(arena)


def make_state(seed=5):
    gen = torch.Generator().manual_seed(seed)
    return {
        "a": torch.randn(1000, generator=gen),  # 4000 bytes
        "b": torch.randn(33, 7, generator=gen).to(torch.bfloat16),  # 462 bytes: padded
        "c": torch.empty(0, 3),
        "d": torch.randn(40, 30, generator=gen).t(),  # not contiguous, 4800 bytes
        "e": torch.tensor(7, dtype=torch.int64),  # 0-d
        "f": torch.randint(0, 256, (4097,), dtype=torch.uint8, generator=gen),  # 1 mod 16
    }


# layout of make_state(): a 0, b 4000, c 4464, d 4464, e 9264, f 9280; 13392 bytes
BASE_OFFSETS = {"a": 0, "b": 4000, "c": 4464, "d": 4464, "e": 9264, "f": 9280}
BASE_BYTES = 13392


def other_layout(state):
    """``state`` with one tensor resized (b: one row fewer), one added in
    front and the rest reordered."""
    new = {"g": torch.arange(100, dtype=torch.float32)}  # 400 bytes, new
    for name in ("f", "e", "d", "c", "a"):
        new[name] = state[name]
    new["b"] = state["b"][:32].clone()  # 448 bytes, resized
    return new


def extract(state, fraction=0.5, rebase=True, **options):
    options.setdefault("pack_min_bytes", 0)
    options.setdefault("cache_min_bytes", 8192)
    return worker_pool.extract_arg_buffers(
        [state], {}, THRESHOLD, to_device=True, patch_max_fraction=fraction,
        rebase=rebase, **options
    )


class FakeHandle:
    """What _ArgCacheSend touches of a WorkerHandle."""

    def __init__(self):
        self.resident = set()
        self.resident_arenas = {}


def send(handle, state, full=False, fraction=0.5, stats=None, rebase=True):
    """Run one request's frames as the channel would; returns the sender, the
    decoded wire entries, the payload frames as bytes and the meta."""
    _a, _k, meta, buffers = extract(state, fraction, rebase=rebase)
    sender = worker_pool._ArgCacheSend(
        handle, {"op_id": "x"}, meta, [view for view, _keep in buffers], stats
    )
    frames = list(sender.frames(full=full))
    wire = cloudpickle.loads(frames[0])["arg_buffers"]
    payload = [f.tobytes() if isinstance(f, FrameParts) else bytes(f) for f in frames[1:]]
    return sender, wire, payload, meta


# -- options --------------------------------------------------------------------


def test_option_validation(local_executor):
    base = dict(persistent_workers=True, device_tensor_args=True, cache_tensor_args=True,
                pack_tensor_args=True)
    with pytest.raises(ValueError, match="rebase_tensor_args needs patch_tensor_args=True"):
        local_executor(rebase_tensor_args=True, **base)
    ex = local_executor(rebase_tensor_args=True, patch_tensor_args=True, **base)
    assert ex.rebase_tensor_args is True and ex.patch_args_max_fraction == 0.5
    assert ex.counters["arg_cache_rebases"] == 0
    ex = local_executor(patch_tensor_args=True, **base)
    assert ex.rebase_tensor_args is False
    assert ex.counters["arg_cache_rebases"] == 0


def test_defaults_are_registered():
    from covalent_ssh_plugin_amd.ssh import _EXECUTOR_PLUGIN_DEFAULTS

    assert _EXECUTOR_PLUGIN_DEFAULTS["rebase_tensor_args"] is False
    assert worker_pool.REBASE_CANDIDATES == 8


# -- option off -------------------------------------------------------------------


def test_option_off_changes_nothing(io_lib):
    state = make_state()
    same_layout = dict(state, e=torch.tensor(8, dtype=torch.int64))
    options = dict(to_device=True, pack_min_bytes=0, cache_min_bytes=8192,
                   patch_max_fraction=0.5)
    today = worker_pool.extract_arg_buffers([state], {}, THRESHOLD, **options)
    off = worker_pool.extract_arg_buffers([state], {}, THRESHOLD, rebase=False, **options)
    assert off[0] == today[0] and off[1] == today[1]
    assert cloudpickle.dumps(off[2]) == cloudpickle.dumps(today[2])
    assert "rebase" not in off[2][0]["cache"]
    assert [v.tobytes() for v, _k in off[3]] == [v.tobytes() for v, _k in today[3]]
    # the wire: store, in-place patch, and for another layout a store again,
    # frame for frame what comes out without the keyword
    handles = (FakeHandle(), FakeHandle())
    kinds = []
    for current in (state, same_layout, other_layout(state)):
        sent = []
        for handle, keyword in zip(handles, ({}, {"rebase": False})):
            _a, _k, meta, buffers = worker_pool.extract_arg_buffers(
                [current], {}, THRESHOLD, **options, **keyword
            )
            sender = worker_pool._ArgCacheSend(
                handle, {"op_id": "x"}, meta, [view for view, _keep in buffers], None
            )
            frames = list(sender.frames(full=False))
            sent.append([frames[0]] + [f.tobytes() for f in frames[1:]])
        assert sent[0] == sent[1]
        wire = cloudpickle.loads(sent[0][0])["arg_buffers"]
        assert "rebase" not in wire[0]["cache"] and "rebase_nbytes" not in wire[0]
        kinds.append(sorted(set(wire[0]["cache"]) - {"key"}))
    assert kinds == [["store"], ["patch"], ["store"]]
    assert handles[0].resident == handles[1].resident
    assert list(handles[0].resident_arenas) == list(handles[1].resident_arenas)
    # the in-place patch consumed its base, the other layout was stored beside it
    assert len(handles[0].resident) == 2


# -- the rebase plan ----------------------------------------------------------------


def test_rebase_wire_meta_delta_frame_and_sum(io_lib):
    state = make_state()
    new = other_layout(state)
    handle = FakeHandle()
    _s, wire, _p, base_meta = send(handle, state)
    base_key = base_meta[0]["cache"]["key"]
    assert wire[0]["cache"] == {"key": base_key, "store": True}
    assert base_meta[0]["nbytes"] == BASE_BYTES
    assert [seg["offset"] for seg in base_meta[0]["packed"]] == list(BASE_OFFSETS.values())
    stats = {}
    sender, wire, payload, meta = send(handle, new, stats=stats)
    new_key = meta[0]["cache"]["key"]
    assert new_key != base_key
    # g and the resized b come from the delta, the rest from the base, moved
    sources = [-1] + [BASE_OFFSETS[name] for name in ("f", "e", "d", "c", "a")] + [-1]
    assert wire[0]["cache"] == {
        "key": new_key,
        "rebase": {"base": base_key, "base_nbytes": BASE_BYTES, "sources": sources},
    }
    delta = materialise([raw(new["g"]), raw(new["b"])])
    assert wire[0]["rebase_nbytes"] == len(delta) == 400 + 448
    assert "patch_nbytes" not in wire[0] and "segments" not in wire[0]["cache"]
    assert wire[0]["packed"] == meta[0]["packed"]
    assert payload == [delta]
    blobs = [raw(t) for t in new.values()]
    assert wire[0]["nbytes"] == len(materialise(blobs))
    assert wire[0]["sum"] == list(native_io.checksum(materialise(blobs)))
    # after the send: both resident, the base used, the new one most recent
    assert handle.resident == {base_key, new_key}
    assert list(handle.resident_arenas) == [base_key, new_key]
    total = wire[0]["nbytes"]
    missed = sender.reconcile(
        {"arg_cache": {"stored": [new_key], "rebased": [[base_key, new_key]], "miss": []}}
    )
    assert missed is False
    assert handle.resident == {base_key, new_key}
    assert stats["arg_cache_rebases"] == 1
    assert stats["arg_cache_bytes_saved"] == total - len(delta)
    assert stats["arg_cache_misses"] == 0 and "arg_cache_patches" not in stats
    # both states again are references; a use makes an arena the most recent
    _s, wire, payload, _m = send(handle, state)
    assert wire[0]["cache"] == {"key": base_key, "ref": True} and payload == []
    assert list(handle.resident_arenas) == [new_key, base_key]
    _s, wire, payload, _m = send(handle, new)
    assert wire[0]["cache"] == {"key": new_key, "ref": True} and payload == []
    assert list(handle.resident_arenas) == [base_key, new_key]


def test_same_layout_is_a_rebase_that_keeps_the_base(io_lib):
    state = make_state()
    new = dict(state, e=torch.tensor(8, dtype=torch.int64))
    handle = FakeHandle()
    _s, _w, _p, base_meta = send(handle, state)
    base_key = base_meta[0]["cache"]["key"]
    _s, wire, payload, _m = send(handle, new)
    sources = list(BASE_OFFSETS.values())
    sources[4] = -1
    assert wire[0]["cache"]["rebase"] == {
        "base": base_key, "base_nbytes": BASE_BYTES, "sources": sources,
    }
    assert "patch" not in wire[0]["cache"]
    assert payload == [raw(new["e"]) + bytes(8)]
    assert base_key in handle.resident and len(handle.resident) == 2
    # alternating between the two states from here on sends no frame
    for current in (state, new, state):
        _s, wire, payload, _m = send(handle, current)
        assert wire[0]["cache"].get("ref") is True and payload == []


def test_the_base_with_the_fewest_delta_bytes_wins(io_lib):
    state = make_state()
    far = dict(state, a=state["a"] + 1, f=state["f"] ^ 1)
    handle = FakeHandle()
    _s, _w, _p, near_meta = send(handle, state)
    _s, wire, _p, far_meta = send(handle, far, fraction=1e-9)  # too far: a store
    assert wire[0]["cache"].get("store") is True
    near_key, far_key = near_meta[0]["cache"]["key"], far_meta[0]["cache"]["key"]
    assert list(handle.resident_arenas) == [near_key, far_key]
    new = dict(state, e=torch.tensor(9, dtype=torch.int64))
    _s, wire, payload, _m = send(handle, new)
    # the older arena needs 16 delta bytes, the most recent 4000 + 16 + 4112
    assert wire[0]["cache"]["rebase"]["base"] == near_key
    assert payload == [raw(new["e"]) + bytes(8)]
    assert list(handle.resident_arenas)[-2:] == [near_key, wire[0]["cache"]["key"]]
    assert far_key in handle.resident


def test_a_tie_goes_to_the_most_recent(io_lib):
    state = make_state()
    one = dict(state, e=torch.tensor(1, dtype=torch.int64))
    two = dict(state, e=torch.tensor(2, dtype=torch.int64))
    handle = FakeHandle()
    _s, _w, _p, one_meta = send(handle, one)
    _s, _w, _p, two_meta = send(handle, two, fraction=1e-9)
    one_key, two_key = one_meta[0]["cache"]["key"], two_meta[0]["cache"]["key"]
    three = dict(state, e=torch.tensor(3, dtype=torch.int64))
    _s, wire, _p, _m = send(handle, three)
    assert wire[0]["cache"]["rebase"]["base"] == two_key
    # a use of the older one turns the tie round
    send(handle, one)
    assert list(handle.resident_arenas)[-1] == one_key
    four = dict(state, e=torch.tensor(4, dtype=torch.int64))
    _s, wire, _p, _m = send(handle, four, fraction=1e-9)  # stored: not a candidate winner
    five = dict(state, e=torch.tensor(5, dtype=torch.int64))
    handle.resident.discard(wire[0]["cache"]["key"])  # and no longer believed resident
    _s, wire, _p, _m = send(handle, five)
    assert wire[0]["cache"]["rebase"]["base"] == one_key


def test_the_fraction_bound_and_the_fallbacks_to_a_store(io_lib):
    state = make_state()
    new = other_layout(state)
    blobs = [raw(t) for t in new.values()]
    total = len(materialise(blobs))
    delta_bytes = 400 + 448

    def resident_base():
        handle = FakeHandle()
        _s, _w, _p, meta = send(handle, state)
        return handle, meta[0]["cache"]["key"]

    def is_store(wire, payload, handle, base_key):
        assert wire[0]["cache"] == {"key": wire[0]["cache"]["key"], "store": True}
        assert "rebase_nbytes" not in wire[0] and "patch_nbytes" not in wire[0]
        assert payload == [materialise(blobs)]
        assert handle.resident == {base_key, wire[0]["cache"]["key"]}

    # just more than the fraction: a store; just less: a rebase
    handle, base_key = resident_base()
    _s, wire, payload, _m = send(handle, new, fraction=(delta_bytes - 0.5) / total)
    is_store(wire, payload, handle, base_key)
    handle, base_key = resident_base()
    _s, wire, payload, _m = send(handle, new, fraction=(delta_bytes + 0.5) / total)
    assert wire[0]["cache"]["rebase"]["base"] == base_key
    # the resend never rebases
    handle, base_key = resident_base()
    _s, wire, payload, _m = send(handle, new, full=True)
    is_store(wire, payload, handle, base_key)
    # a base that is no longer believed resident
    handle, base_key = resident_base()
    handle.resident.discard(base_key)
    _s, wire, payload, _m = send(handle, new)
    assert wire[0]["cache"].get("store") is True
    # nothing in common: every byte would be delta
    handle, base_key = resident_base()
    fresh = {k: (t + 1 if t.numel() else torch.empty(0, 5)) for k, t in make_state(6).items()}
    _s, wire, payload, _m = send(handle, fresh, fraction=0.99)
    assert wire[0]["cache"].get("store") is True
    # no delta bytes at all (the same tensors reordered) is still a new arena:
    # nothing to send as a delta, so it is stored whole
    handle, base_key = resident_base()
    reordered = {name: state[name] for name in ("f", "a", "b", "c", "d", "e")}
    _s, wire, payload, _m = send(handle, reordered)
    assert wire[0]["cache"].get("store") is True


def test_only_the_eight_most_recent_arenas_are_candidates(io_lib):
    state = make_state()
    handle = FakeHandle()
    _s, _w, _p, first_meta = send(handle, state)
    first_key = first_meta[0]["cache"]["key"]
    # eight arenas that share only the small tensors with the first
    for k in range(8):
        filler = dict(state, a=state["a"] + k + 1, d=state["d"] + k + 1, f=state["f"] ^ (k + 1))
        _s, wire, _p, _m = send(handle, filler, fraction=1e-9)
        assert wire[0]["cache"].get("store") is True
    assert len(handle.resident_arenas) == 9 and list(handle.resident_arenas)[0] == first_key
    new = dict(state, e=torch.tensor(9, dtype=torch.int64))
    _s, wire, _p, _m = send(handle, new, fraction=0.01)
    # the first arena would need 16 bytes, but it is the ninth most recent
    assert wire[0]["cache"].get("store") is True
    # once used it is a candidate again
    send(handle, state)
    newer = dict(state, e=torch.tensor(10, dtype=torch.int64))
    _s, wire, _p, _m = send(handle, newer, fraction=0.01)
    assert wire[0]["cache"]["rebase"]["base"] == first_key


def test_duplicates_and_zero_byte_segments(io_lib):
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(1400, generator=gen)  # 5600 bytes
    y = torch.randn(1500, generator=gen)  # 6000 bytes
    base = {"x": x, "y": y, "empty": torch.empty(0)}
    handle = FakeHandle()
    _s, _w, _p, base_meta = send(handle, base)
    base_key = base_meta[0]["cache"]["key"]
    # x twice as two distinct objects of equal content, a new zero-byte tensor
    # of another dtype (the same content key: no bytes), y gone, z new
    z = torch.randn(10, generator=gen)  # 40 bytes
    new = {"x1": x.clone(), "z": z, "x2": x.clone(), "none": torch.empty(0, dtype=torch.int8)}
    _s, wire, payload, meta = send(handle, new)
    rebase = wire[0]["cache"]["rebase"]
    assert rebase["base"] == base_key and rebase["base_nbytes"] == 5600 + 6000
    assert rebase["sources"][0] == 0 and rebase["sources"][2] == 0  # one source twice
    assert rebase["sources"][1] == -1
    # a zero-byte segment costs nothing wherever it comes from
    assert rebase["sources"][3] in (-1, 5600 + 6000)
    assert wire[0]["rebase_nbytes"] == 48
    assert payload == [raw(z) + bytes(8)]


def test_resident_sets_after_the_report(io_lib):
    state = make_state()
    new = other_layout(state)
    # a miss forgets both keys, and the resend stores the new one whole
    handle = FakeHandle()
    _s, _w, _p, base_meta = send(handle, state)
    base_key = base_meta[0]["cache"]["key"]
    stats = {}
    sender, wire, _p, meta = send(handle, new, stats=stats)
    new_key = meta[0]["cache"]["key"]
    assert "rebase" in wire[0]["cache"]
    assert sender.reconcile({"arg_cache": {"stored": [], "hits": [], "miss": [0]}}) is True
    assert handle.resident == set() and handle.resident_arenas == {}
    assert stats["arg_cache_misses"] == 1 and "arg_cache_rebases" not in stats
    frames = list(sender.frames(full=True))
    wire = cloudpickle.loads(frames[0])["arg_buffers"]
    assert wire[0]["cache"] == {"key": new_key, "store": True}
    assert "rebase_nbytes" not in wire[0]
    assert frames[1].nbytes == wire[0]["nbytes"]
    assert sender.reconcile({"arg_cache": {"stored": [new_key], "miss": []}}) is False
    assert handle.resident == {new_key} and set(handle.resident_arenas) == {new_key}
    assert "arg_cache_rebases" not in stats
    # served transient: the new key in not_stored is forgotten alone, and counted
    handle = FakeHandle()
    send(handle, state)
    stats = {}
    sender, wire, payload, _m = send(handle, new, stats=stats)
    report = {"stored": [], "not_stored": [new_key], "rebased": [[base_key, new_key]],
              "miss": []}
    assert sender.reconcile({"arg_cache": report}) is False
    assert handle.resident == {base_key} and set(handle.resident_arenas) == {base_key}
    assert stats["arg_cache_rebases"] == 1
    assert stats["arg_cache_bytes_saved"] == wire[0]["nbytes"] - len(payload[0])
    # a report that names another pair counts nothing
    stats = {}
    sender, _w, _p, _m = send(handle, new, stats=stats)
    assert sender.reconcile(
        {"arg_cache": {"stored": [new_key], "rebased": [["x", new_key]], "miss": []}}
    ) is False
    assert "arg_cache_rebases" not in stats
    assert handle.resident == {base_key, new_key}
    # the worker's evicted list is not consumed: the base is believed until a miss
    sender, _w, _p, _m = send(handle, dict(new, e=torch.tensor(1, dtype=torch.int64)))
    sender.reconcile({"arg_cache": {"stored": sender.keys, "evicted": [base_key], "miss": []}})
    assert base_key in handle.resident


# -- the worker's check of the sources ------------------------------------------------


def _worker_namespace():
    """The worker template's module-level functions, without running it."""
    import re
    from pathlib import Path

    import covalent_ssh_plugin_amd.remote as remote

    text = (Path(remote.__file__).parent / "worker_template.py").read_text()
    start = text.index("def _rebase_sources(")
    end = text.index("\ndef ", start + 1)
    namespace = {}
    exec(compile(text[start:end], "worker_template.py", "exec"), namespace)  # noqa: S102
    assert re.search(r"_rebase_sources\(info, cache, entry\[1\]\)", text)
    return namespace


def test_worker_checks_the_sources_before_the_call():
    check = _worker_namespace()["_rebase_sources"]
    info = {"packed": [{"nbytes": 100}, {"nbytes": 0}, {"nbytes": 33}, {"nbytes": 17}],
            "rebase_nbytes": 48 + 32}
    none = (1 << 64) - 1

    def cache(sources):
        return {"rebase": {"base": "k", "base_nbytes": 256, "sources": sources}}

    base_offs, delta_offs, from_delta = check(info, cache([144, 0, -1, -1]), 256)
    assert base_offs == [144, 0, none, none] and delta_offs == [none, none, 0, 48]
    assert from_delta == 2
    for bad in (
        [144, 0, -1],  # one short
        None,
        [152, 0, -1, -1],  # not a multiple of 16
        [160, 0, -1, -1],  # 112 rounded bytes end past 256
        [-2, 0, -1, -1],
        [144.0, 0, -1, -1],
        [True, 0, -1, -1],
        [144, 0, -1, 16],  # the delta is then 48 bytes, not 80
        [-1, 0, -1, -1],  # the delta is then 192 bytes
        [144, 272, -1, -1],  # an empty segment past the base's end
    ):
        with pytest.raises(ValueError):
            check(info, cache(bad), 256)
    # an empty segment may sit at the very end of the base
    check(info, cache([144, 256, -1, -1]), 256)


# -- a worker that cannot take device arguments -----------------------------------


def test_rebase_entry_is_drained_on_a_worker_without_the_library(local_executor, monkeypatch,
                                                                  io_lib):
    from covalent_ssh_plugin_amd.gpu import probe

    monkeypatch.setattr(probe, "local_gpu_lib_path", lambda: "")
    ex = local_executor(
        persistent_workers=True, device_tensor_args=True, pack_tensor_args=True,
        pack_args_min_bytes=0, cache_tensor_args=True, arg_cache_min_bytes=8192,
        patch_tensor_args=True, rebase_tensor_args=True, cpu_workers=1,
        pinned_staging_threshold_bytes=THRESHOLD,
        # one CPU-tagged worker also on a host that has GPUs
        hip_visible_devices_policy="none",
    )

    def takes_state(state):
        return float(sum(t.sum() for t in state.values()))  # must never run

    def plain(x):
        import os

        return x + 1, os.getpid()

    state = make_state()
    new = other_layout(state)
    _a, _k, base_meta, _b = extract(state)
    base = base_meta[0]["cache"]
    sent = []
    real_frames = worker_pool._ArgCacheSend.frames

    def recording_frames(self, full):
        for frame in real_frames(self, full):
            sent.append(frame)
            yield frame

    monkeypatch.setattr(worker_pool._ArgCacheSend, "frames", recording_frames)

    async def main():
        # a first plain electron starts the worker and tells us its pid
        _, pid0 = await ex.execute(plain, [0], {}, dispatch_id="d", node_id=0)
        (handle,) = [h for h in worker_pool._workers.values() if h.alive]
        # the handle is told that the worker holds the base arena
        handle.resident.add(base["key"])
        handle.resident_arenas[base["key"]] = base["segments"]
        with pytest.raises(RuntimeError, match="need a GPU worker with the CDNA4 library"):
            await ex.execute(takes_state, [new], {}, dispatch_id="d", node_id=1)
        failed_meta = ex.last_task_record.remote_meta
        resident = set(handle.resident)
        value, pid1 = await ex.execute(plain, [41], {}, dispatch_id="d", node_id=2)
        served = ex.last_task_record.remote_meta["served"]
        await ex.close_pool()
        return pid0, failed_meta, resident, value, pid1, served

    pid0, failed_meta, resident, value, pid1, served = asyncio.run(main())
    # it went out as a rebase: one request, one delta frame
    assert len(sent) == 2
    wire = cloudpickle.loads(sent[0])["arg_buffers"]
    assert wire[0]["cache"]["rebase"]["base"] == base["key"]
    assert sent[1].nbytes == wire[0]["rebase_nbytes"] == 848 < wire[0]["nbytes"]
    # the frame was drained: the stream is aligned, the same worker goes on
    assert value == 42
    assert pid1 == pid0 == failed_meta["pid"], "the worker was replaced"
    assert served == 3
    assert failed_meta["arg_staging"]["verified"] == 0
    assert "user_fn" not in failed_meta["phases_ms"]
    assert wire[0]["cache"]["key"] not in resident, "the new arena is still believed resident"
    assert ex.counters["arg_cache_rebases"] == 0
