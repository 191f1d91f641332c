"""MI355X tests for ``gather_tensor_results`` inside the packed result arena,
end to end through a loopback worker: a dict of small CUDA tensors, most of
them non-contiguous, filled into the arena by csp_pack_gather_checksum_dev."""

import asyncio
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SERVED = ("conv1", "conv2", "conv3", "fc1_t", "fc2_t", "cols")  # strided segments


def _make_electrons():
    """Local functions, so cloudpickle ships them by value."""

    def build(device):
        import torch

        gen = torch.Generator().manual_seed(23)
        rand = lambda *shape: torch.randn(*shape, generator=gen).to(device)  # noqa: E731
        cl = torch.channels_last
        return {
            "conv1": rand(16, 3, 3, 3).to(memory_format=cl),
            "bias1": rand(16),
            "conv2": rand(32, 16, 3, 3).bfloat16().to(memory_format=cl),
            "bias2": rand(32).bfloat16(),
            "conv3": rand(40, 32, 1, 5).to(memory_format=cl),
            "fc1_t": rand(48, 40).t(),
            "fc2_t": rand(33, 65).double().t(),
            "cols": rand(9, 40)[:, 1:17],
            "five": rand(4, 4, 4, 4, 4)[::2, ::2, ::2, ::2, ::2],  # contiguous() for it alone
            "bias3": rand(40),
            "scale": rand(1),
            "steps": torch.arange(7, device=device),
        }

    def produce():
        return build("cuda")

    def digests(value):
        import hashlib

        import torch

        return {
            k: hashlib.blake2b(
                v.contiguous().view(torch.uint8).cpu().numpy().tobytes(), digest_size=16
            ).hexdigest()
            for k, v in value.items()
        }

    def consume(value):
        return all(v.is_cuda for v in value.values()), digests(value)

    return build, produce, digests, consume


_build, _produce, _digests, _consume = _make_electrons()


def _run(tmp_path, take=False, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor

    home = tmp_path / "home"
    home.mkdir()
    options = dict(
        transport="local", local_home=str(home), cache_dir=str(tmp_path / "cache"),
        python_path=sys.executable, gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True, pack_tensor_results=True, pack_results_min_bytes=4096,
        gather_tensor_results=True, hip_visible_devices_policy="fixed", fixed_gpu=0,
    )
    options.update(overrides)
    ex = SSHExecutor(**options)

    async def run():
        value = await ex.execute(_produce, [], {}, dispatch_id="p", node_id=1)
        meta, out = ex.last_task_record.remote_meta, None
        if take:
            out = await ex.execute(_consume, [value], {}, dispatch_id="p", node_id=2)
            out = (out, ex.last_task_record.remote_meta)
        await ex.close_pool()
        return value, meta, out

    return asyncio.run(run())


def _check_values(value):
    want = _build("cpu")
    assert list(value) == list(want)
    assert sum(v.numel() * v.element_size() for v in want.values()) > 4096  # the threshold
    for key, w in want.items():
        got = value[key]
        assert not got.is_cuda and got.dtype == w.dtype and got.shape == w.shape, key
        assert torch.equal(got, w), key


@pytest.mark.parametrize("gather", [True, False])
def test_a_dict_of_strided_tensors_through_the_packed_arena(tmp_path, gather):
    value, meta, _ = _run(tmp_path, gather_tensor_results=gather)
    _check_values(value)
    staging = meta["staging"]
    assert staging["packed_tensors"] == 12
    assert "gather_fallback" not in staging and "pack_fallback" not in staging
    if gather:
        want = _build("cpu")
        assert staging["gathered_tensors"] == len(SERVED)
        assert staging["gathered_bytes"] == sum(
            want[k].numel() * want[k].element_size() for k in SERVED)
    else:
        assert "gathered_tensors" not in staging


def test_the_retained_arena_is_verified_and_a_hit_as_arguments(tmp_path):
    value, meta, (out, meta_b) = _run(
        tmp_path, take=True, device_tensor_args=True, pack_tensor_args=True,
        pack_args_min_bytes=0, cache_tensor_args=True, arg_cache_bytes=64 << 20,
        # above every tensor, so that all of them share the arena, and below their total
        arg_cache_min_bytes=32768, retain_tensor_results=True,
    )
    _check_values(value)
    staging = meta["staging"]
    assert staging["gathered_tensors"] == len(SERVED) and staging["packed_tensors"] == 12
    assert "gather_fallback" not in staging and "retain_fallback" not in staging
    (info,) = meta["buffers"]
    # the dispatcher verified the frame against the sum the kernel produced
    assert info["retained"] == meta["retained"]["stored"][0] and len(info["sum"]) == 2
    assert meta["result_integrity"]["verified"] >= 1
    assert meta_b["arg_cache"]["hits"] == [info["retained"]]
    assert out == (True, _digests(_build("cpu")))
