"""``patch_tensor_args`` without a GPU: option validation, what the option
leaves alone when it is off, the dispatcher's patch decision against a fake
worker handle (wire meta, delta frame, checksum, fallbacks, the resident sets
after the send and after the worker's report), and a patch entry against a
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
        "d": torch.randn(40, 30, generator=gen).t(),  # not contiguous
        "e": torch.tensor(7, dtype=torch.int64),  # 0-d
        "f": torch.randint(0, 256, (4097,), dtype=torch.uint8, generator=gen),  # 1 mod 16
    }


def changed_state(state):
    """Three tensors changed: one of 1 byte mod 16, one 0-d, one padded."""
    new = dict(state)
    new["f"] = state["f"] ^ 0xFF
    new["e"] = torch.tensor(8, dtype=torch.int64)
    new["b"] = state["b"] + 1
    return new, [1, 4, 5]


def extract(state, fraction=0.5, **options):
    options.setdefault("pack_min_bytes", 0)
    options.setdefault("cache_min_bytes", 8192)
    return worker_pool.extract_arg_buffers(
        [state], {}, THRESHOLD, to_device=True, patch_max_fraction=fraction, **options
    )


class FakeHandle:
    """What _ArgCacheSend touches of a WorkerHandle."""

    def __init__(self):
        self.resident = set()
        self.resident_arenas = {}


def send(handle, state, full=False, fraction=0.5, stats=None):
    """Run one request's frames as the channel would; returns the sender, the
    decoded wire entries and the payload frames as bytes."""
    _a, _k, meta, buffers = extract(state, fraction)
    sender = worker_pool._ArgCacheSend(
        handle, {"op_id": "x"}, meta, [view for view, _keep in buffers], stats
    )
    frames = list(sender.frames(full=full))
    wire = cloudpickle.loads(frames[0])["arg_buffers"]
    payload = [f.tobytes() if isinstance(f, FrameParts) else bytes(f) for f in frames[1:]]
    return sender, wire, payload, meta


# -- options --------------------------------------------------------------------


def test_option_validation(local_executor):
    base = dict(persistent_workers=True, device_tensor_args=True)
    with pytest.raises(ValueError, match="patch_tensor_args needs cache_tensor_args"):
        local_executor(patch_tensor_args=True, pack_tensor_args=True, **base)
    with pytest.raises(ValueError, match="patch_tensor_args needs cache_tensor_args"):
        local_executor(patch_tensor_args=True, cache_tensor_args=True, **base)
    on = dict(base, patch_tensor_args=True, cache_tensor_args=True, pack_tensor_args=True)
    for bad in (0, -0.1, 1.5):
        with pytest.raises(ValueError, match=r"patch_args_max_fraction must be in \(0, 1\]"):
            local_executor(patch_args_max_fraction=bad, **on)
    ex = local_executor(**on)
    assert ex.patch_tensor_args is True and ex.patch_args_max_fraction == 0.5
    assert local_executor(patch_args_max_fraction=1, **on).patch_args_max_fraction == 1.0
    ex = local_executor(cache_tensor_args=True, pack_tensor_args=True, **base)
    assert ex.patch_tensor_args is False
    assert ex.counters["arg_cache_patches"] == 0


def test_defaults_are_registered():
    from covalent_ssh_plugin_amd.ssh import _EXECUTOR_PLUGIN_DEFAULTS

    assert _EXECUTOR_PLUGIN_DEFAULTS["patch_tensor_args"] is False
    assert _EXECUTOR_PLUGIN_DEFAULTS["patch_args_max_fraction"] == 0.5


# -- option off -------------------------------------------------------------------


def test_option_off_changes_nothing(io_lib):
    state = make_state()
    new, _ = changed_state(state)
    options = dict(to_device=True, pack_min_bytes=0, cache_min_bytes=8192)
    today = worker_pool.extract_arg_buffers([state], {}, THRESHOLD, **options)
    off = worker_pool.extract_arg_buffers(
        [state], {}, THRESHOLD, patch_max_fraction=None, **options
    )
    assert off[0] == today[0] and off[1] == today[1] and off[2] == today[2]
    assert set(off[2][0]["cache"]) == {"key"}
    assert [v.tobytes() for v, _k in off[3]] == [v.tobytes() for v, _k in today[3]]
    # the wire: a store, then for a changed state a store again, never a patch
    handle = FakeHandle()
    for current in (state, new):
        _a, _k, meta, buffers = worker_pool.extract_arg_buffers(
            [current], {}, THRESHOLD, **options
        )
        sender = worker_pool._ArgCacheSend(
            handle, {"op_id": "x"}, meta, [view for view, _keep in buffers], None
        )
        frames = list(sender.frames(full=False))
        wire = cloudpickle.loads(frames[0])["arg_buffers"]
        assert wire[0]["cache"] == {"key": meta[0]["cache"]["key"], "store": True}
        assert "patch_nbytes" not in wire[0]
        assert frames[1].tobytes() == materialise([raw(t) for t in current.values()])
    assert len(handle.resident) == 2 and handle.resident_arenas == {}


def test_option_on_keeps_segments_off_the_wire(io_lib):
    state = make_state()
    handle = FakeHandle()
    _s, wire, payload, meta = send(handle, state)
    cache = meta[0]["cache"]
    assert [n for _key, n in cache["segments"]] == [4000, 462, 0, 4800, 8, 4097]
    assert [worker_pool.content_key(raw(t)) for t in state.values()] == [
        key for key, _n in cache["segments"]
    ]
    assert wire[0]["cache"] == {"key": cache["key"], "store": True}
    assert payload == [materialise([raw(t) for t in state.values()])]
    assert handle.resident == {cache["key"]}
    assert handle.resident_arenas == {cache["key"]: cache["segments"]}


# -- the patch decision -------------------------------------------------------------


def test_patch_wire_meta_delta_frame_and_sum(io_lib):
    state = make_state()
    new, changed = changed_state(state)
    handle = FakeHandle()
    _s, _w, _p, base_meta = send(handle, state)
    base_key = base_meta[0]["cache"]["key"]
    stats = {}
    sender, wire, payload, meta = send(handle, new, stats=stats)
    new_key = meta[0]["cache"]["key"]
    assert new_key != base_key
    blobs = [raw(t) for t in new.values()]
    delta = materialise([blobs[j] for j in changed])
    assert wire[0]["cache"] == {
        "key": new_key, "patch": {"base": base_key, "segments": changed},
    }
    assert wire[0]["patch_nbytes"] == len(delta) == 464 + 16 + 4112
    assert wire[0]["nbytes"] == base_meta[0]["nbytes"]
    assert wire[0]["packed"] == meta[0]["packed"]
    # the delta: the changed tensors at the pack layout, zero padded
    assert payload == [delta]
    # the checksum is that of the whole new arena
    assert wire[0]["sum"] == list(native_io.checksum(materialise(blobs)))
    # after the send: the base is consumed, the new key is resident
    assert handle.resident == {new_key}
    assert handle.resident_arenas == {new_key: meta[0]["cache"]["segments"]}
    # the worker's report of a patch: counted, the sets stay
    total = wire[0]["nbytes"]
    missed = sender.reconcile(
        {"arg_cache": {"stored": [new_key], "patched": [[base_key, new_key]], "miss": []}}
    )
    assert missed is False
    assert handle.resident == {new_key} and set(handle.resident_arenas) == {new_key}
    assert stats["arg_cache_patches"] == 1
    assert stats["arg_cache_bytes_saved"] == total - len(delta)
    assert stats["arg_cache_misses"] == 0
    # the same state again is a reference
    _s, wire, payload, _m = send(handle, new)
    assert wire[0]["cache"] == {"key": new_key, "ref": True} and payload == []
    # and the original state a patch back
    _s, wire, payload, _m = send(handle, state)
    assert wire[0]["cache"]["patch"] == {"base": new_key, "segments": changed}
    old = [raw(t) for t in state.values()]
    assert payload == [materialise([old[j] for j in changed])]
    assert handle.resident == {base_key}


def test_the_closest_resident_arena_is_the_base(io_lib):
    state = make_state()
    far = dict(state, a=state["a"] + 1, f=state["f"] ^ 1)
    handle = FakeHandle()
    _s, _w, _p, near_meta = send(handle, state)
    _s, wire, _p, far_meta = send(handle, far, fraction=1e-9)  # too far: a store
    assert wire[0]["cache"].get("store") is True
    assert len(handle.resident_arenas) == 2
    new = dict(state, e=torch.tensor(9, dtype=torch.int64))
    _s, wire, payload, _m = send(handle, new)
    assert wire[0]["cache"]["patch"] == {
        "base": near_meta[0]["cache"]["key"], "segments": [4],
    }
    assert payload == [raw(new["e"]) + bytes(8)]
    assert far_meta[0]["cache"]["key"] in handle.resident


def test_fallbacks_to_a_store(io_lib):
    state = make_state()
    new, changed = changed_state(state)
    blobs = [raw(t) for t in new.values()]
    _, total = pack_layout([len(b) for b in blobs])
    delta_bytes = 464 + 16 + 4112

    def resident_base():
        handle = FakeHandle()
        _s, _w, _p, meta = send(handle, state)
        return handle, meta[0]["cache"]["key"]

    def is_store(wire, payload, handle, base_key):
        assert wire[0]["cache"] == {"key": wire[0]["cache"]["key"], "store": True}
        assert "patch_nbytes" not in wire[0]
        assert payload == [materialise(blobs)]
        assert base_key in handle.resident and base_key in handle.resident_arenas
        assert len(handle.resident) == 2

    # another layout: one tensor one element longer
    handle, base_key = resident_base()
    longer = dict(state, a=torch.cat([state["a"], torch.zeros(1)]))
    _s, wire, payload, _m = send(handle, longer)
    assert wire[0]["cache"].get("store") is True and base_key in handle.resident
    # just more than the fraction changed; just less is a patch
    handle, base_key = resident_base()
    _s, wire, payload, _m = send(handle, new, fraction=(delta_bytes - 0.5) / total)
    is_store(wire, payload, handle, base_key)
    handle, base_key = resident_base()
    _s, wire, payload, _m = send(handle, new, fraction=(delta_bytes + 0.5) / total)
    assert wire[0]["cache"]["patch"]["base"] == base_key
    # the resend never patches
    handle, base_key = resident_base()
    _s, wire, payload, _m = send(handle, new, full=True)
    is_store(wire, payload, handle, base_key)
    # a base that is no longer believed resident
    handle, base_key = resident_base()
    handle.resident.discard(base_key)
    _s, wire, payload, _m = send(handle, new)
    assert wire[0]["cache"].get("store") is True


def test_resident_sets_after_the_report(io_lib):
    state = make_state()
    new, _changed = changed_state(state)
    # a miss forgets both keys, and the resend stores the new one
    handle = FakeHandle()
    _s, _w, _p, base_meta = send(handle, state)
    base_key = base_meta[0]["cache"]["key"]
    stats = {}
    sender, wire, _p, meta = send(handle, new, stats=stats)
    new_key = meta[0]["cache"]["key"]
    assert "patch" in wire[0]["cache"]
    assert sender.reconcile({"arg_cache": {"stored": [], "hits": [], "miss": [0]}}) is True
    assert handle.resident == set() and handle.resident_arenas == {}
    assert stats["arg_cache_misses"] == 1 and "arg_cache_patches" not in stats
    frames = list(sender.frames(full=True))
    wire = cloudpickle.loads(frames[0])["arg_buffers"]
    assert wire[0]["cache"] == {"key": new_key, "store": True}
    assert frames[1].nbytes == wire[0]["nbytes"]
    assert sender.reconcile({"arg_cache": {"stored": [new_key], "miss": []}}) is False
    assert handle.resident == {new_key} and set(handle.resident_arenas) == {new_key}
    assert "arg_cache_patches" not in stats
    # the new key already resident: a reference, and the base stays
    handle = FakeHandle()
    send(handle, state)
    _s, wire, _p, _m = send(handle, new, fraction=1e-9)  # stored beside the base
    assert handle.resident == {base_key, new_key}
    sender, wire, payload, _m = send(handle, new)
    assert wire[0]["cache"] == {"key": new_key, "ref": True} and payload == []
    assert sender.reconcile({"arg_cache": {"hits": [new_key], "miss": []}}) is False
    assert handle.resident == {base_key, new_key}
    assert set(handle.resident_arenas) == {base_key, new_key}
    # a key the worker reports neither stored nor hit is forgotten with its arena
    sender, _w, _p, _m = send(handle, state)
    assert sender.reconcile({"arg_cache": {"not_stored": [base_key], "miss": []}}) is False
    assert handle.resident == {new_key} and set(handle.resident_arenas) == {new_key}


# -- a worker that cannot take device arguments -----------------------------------


def test_patch_entry_is_drained_on_a_worker_without_the_library(local_executor, monkeypatch, io_lib):
    from covalent_ssh_plugin_amd.gpu import probe

    monkeypatch.setattr(probe, "local_gpu_lib_path", lambda: "")
    ex = local_executor(
        persistent_workers=True, device_tensor_args=True, pack_tensor_args=True,
        pack_args_min_bytes=0, cache_tensor_args=True, arg_cache_min_bytes=8192,
        patch_tensor_args=True, cpu_workers=1,
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
    new, changed = changed_state(state)
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
        sets = (set(handle.resident), dict(handle.resident_arenas))
        value, pid1 = await ex.execute(plain, [41], {}, dispatch_id="d", node_id=2)
        served = ex.last_task_record.remote_meta["served"]
        await ex.close_pool()
        return pid0, failed_meta, sets, value, pid1, served

    pid0, failed_meta, sets, value, pid1, served = asyncio.run(main())
    # it went out as a patch: one request, one delta frame
    assert len(sent) == 2
    wire = cloudpickle.loads(sent[0])["arg_buffers"]
    assert wire[0]["cache"]["patch"] == {"base": base["key"], "segments": changed}
    assert sent[1].nbytes == wire[0]["patch_nbytes"] < wire[0]["nbytes"]
    # the frame was drained: the stream is aligned, the same worker goes on
    assert value == 42
    assert pid1 == pid0 == failed_meta["pid"], "the worker was replaced"
    assert served == 3
    assert failed_meta["arg_staging"]["verified"] == 0
    assert "user_fn" not in failed_meta["phases_ms"]
    assert sets == (set(), {}), "the dispatcher still believes an arena resident"
    assert ex.counters["arg_cache_patches"] == 0
