"""The argument checksum on the host (libcsp_io.so: csp_io_checksum behind
native_io.checksum) against a numpy reference, what the two sums do and do
not notice, and the dispatcher side of ``device_tensor_args``:
extract_arg_buffers(to_device=True) and the executor option."""

import numpy as np
import pytest

from covalent_ssh_plugin_amd.transport import native_io

SIZES = [0, 1, 3, 4, 5, 15, 16, 17, 4099, (1 << 20) + 1]


def reference(data: bytes):
    """(s0, s1) as the protocol defines them: pad to 4 bytes, view as
    little-endian u32, widen to u64, wrapping sums."""
    data = bytes(data)
    words = np.frombuffer(data + b"\0" * (-len(data) % 4), dtype="<u4").astype(np.uint64)
    weight = (np.arange(len(words), dtype=np.uint64) % np.uint64(1 << 32)) + np.uint64(1)
    with np.errstate(over="ignore"):
        s0 = int(words.sum(dtype=np.uint64))
        s1 = int((words * weight).sum(dtype=np.uint64))
    return s0, s1


@pytest.fixture(scope="module")
def payload():
    rng = np.random.default_rng(20241020)
    return rng.integers(0, 256, max(SIZES) + 1, dtype=np.uint8).tobytes()


@pytest.fixture(autouse=True)
def _need_io_lib():
    assert native_io.load() is not None, "libcsp_io.so was not built"


@pytest.mark.parametrize("n", SIZES)
def test_checksum_matches_reference(payload, n):
    buf = bytearray(payload)
    assert native_io.checksum(buf, n) == reference(payload[:n])
    # read-only input takes the bytes-by-pointer path
    assert native_io.checksum(payload[:n]) == reference(payload[:n])


@pytest.mark.parametrize("n", SIZES)
def test_checksum_unaligned_pointer(payload, n):
    """bytearray storage is at least 8-byte aligned, so offset 1 is an odd
    address."""
    buf = bytearray(payload)
    assert native_io.checksum(buf, n, 1) == reference(payload[1 : 1 + n])


def test_checksum_default_length_and_range(payload):
    buf = bytearray(payload[:100])
    assert native_io.checksum(buf, offset=3) == reference(payload[3:100])
    with pytest.raises(ValueError):
        native_io.checksum(buf, 101)


def test_reference_weights_are_positions():
    """Pin the reference itself on a hand-computed case: words 1, 2, 3 and
    a padded last word 0x0504."""
    data = np.array([1, 2, 3], dtype="<u4").tobytes() + bytes([4, 5])
    assert reference(data) == (1 + 2 + 3 + 0x0504, 1 * 1 + 2 * 2 + 3 * 3 + 0x0504 * 4)
    assert native_io.checksum(data) == reference(data)


def test_exchanging_two_words_changes_s1_only(payload):
    words = np.frombuffer(payload[:4096], dtype="<u4").copy()
    i, j = 7, 900
    assert words[i] != words[j]
    before = native_io.checksum(words.tobytes())
    words[[i, j]] = words[[j, i]]
    after = native_io.checksum(words.tobytes())
    assert after[0] == before[0]
    assert after[1] != before[1]


@pytest.mark.parametrize("n", [4096, 4099])
def test_dropping_the_last_word_changes_both(payload, n):
    data = bytearray(payload[:n])
    data[-1] = data[-1] or 1  # the last (possibly partial) word is non-zero
    last_word_start = (n - 1) // 4 * 4
    whole = native_io.checksum(bytes(data))
    short = native_io.checksum(bytes(data[:last_word_start]))
    assert whole[0] != short[0]
    assert whole[1] != short[1]


def test_checksum_none_without_library(monkeypatch):
    monkeypatch.setattr(native_io, "force_absent", True)
    assert native_io.checksum(b"abcd") is None


# -- dispatcher side ---------------------------------------------------------


def _arg_tensors():
    torch = pytest.importorskip("torch")
    gen = torch.Generator().manual_seed(7)
    return torch, {
        "ten": torch.randn(10, generator=gen),
        "transposed": torch.randn(12, 5, generator=gen).t(),
        "bf16_odd": torch.randn(33, generator=gen).to(torch.bfloat16),
        "empty": torch.empty(0, 3),
    }


def _raw(torch, t):
    return t.contiguous().view(torch.uint8).numpy().tobytes() if t.numel() else b""


def test_extract_to_device_takes_every_tensor():
    from covalent_ssh_plugin_amd.remote.workers import extract_arg_buffers

    torch, t = _arg_tensors()
    assert not t["transposed"].is_contiguous()
    args = [{"a": t["ten"], "b": [t["transposed"], 5]}]
    kwargs = {"k": (t["bf16_odd"], t["empty"]), "name": "x"}
    new_args, new_kwargs, meta, bufs = extract_arg_buffers(
        args, kwargs, 64 << 20, to_device=True
    )
    assert len(meta) == len(bufs) == 4
    marker = "__csp_tensor_buffer_v1__"
    assert new_args[0]["a"] == (marker, 0)
    assert new_args[0]["b"] == [(marker, 1), 5]
    assert new_kwargs["k"] == ((marker, 2), (marker, 3))
    assert new_kwargs["name"] == "x"
    order = ["ten", "transposed", "bf16_odd", "empty"]
    for info, (view, _keep), name in zip(meta, bufs, order):
        raw = _raw(torch, t[name])
        assert info["device"] is True
        assert info["shape"] == list(t[name].shape)
        assert bytes(view) == raw, name
        assert tuple(info["sum"]) == reference(raw), name
    assert meta[2]["dtype"] == "bfloat16" and len(bytes(bufs[2][0])) == 66
    assert tuple(meta[3]["sum"]) == (0, 0)


def test_extract_default_leaves_small_tensors_inline():
    from covalent_ssh_plugin_amd.remote.workers import extract_arg_buffers

    torch, t = _arg_tensors()
    args = [t["ten"], t["transposed"]]
    kwargs = {"k": t["bf16_odd"], "e": t["empty"]}
    new_args, new_kwargs, meta, bufs = extract_arg_buffers(args, kwargs, 64 << 20)
    assert meta == [] and bufs == []
    assert new_args[0] is t["ten"] and new_kwargs["k"] is t["bf16_odd"]
    # above the threshold, positionally as before: extracted, unmarked
    _a, _k, meta, bufs = extract_arg_buffers(args, kwargs, 40)
    assert len(meta) == 3  # ten (40 B), transposed (240 B), bf16_odd (66 B)
    assert all("device" not in info and "sum" not in info for info in meta)


def test_extract_to_device_without_library_sends_no_sum(monkeypatch):
    from covalent_ssh_plugin_amd.remote.workers import extract_arg_buffers

    torch, t = _arg_tensors()
    monkeypatch.setattr(native_io, "force_absent", True)
    _a, _k, meta, _b = extract_arg_buffers([t["ten"]], {}, 64 << 20, to_device=True)
    assert meta == [{"dtype": "float32", "shape": [10], "device": True}]


def test_option_needs_the_worker_channel(tmp_path):
    from covalent_ssh_plugin_amd import SSHExecutor
    from covalent_ssh_plugin_amd.ssh import _EXECUTOR_PLUGIN_DEFAULTS

    assert _EXECUTOR_PLUGIN_DEFAULTS["device_tensor_args"] is False
    common = dict(transport="local", cache_dir=str(tmp_path / "c"), local_home=str(tmp_path))
    with pytest.raises(ValueError, match="device_tensor_args"):
        SSHExecutor(device_tensor_args=True, **common)
    assert SSHExecutor(**common).device_tensor_args is False
    assert SSHExecutor(device_tensor_args=True, persistent_workers=True, **common).device_tensor_args
    assert SSHExecutor(device_tensor_args=True, isolate_tasks=True, **common).device_tensor_args
