"""``gather_tensor_results`` without a GPU: the option's default and plumbing,
the worker template's token, and a CPU-only electron with the option on."""

import asyncio

import pytest

torch = pytest.importorskip("torch")


def test_option_default_and_plumbing(local_executor):
    from covalent_ssh_plugin_amd.ssh import _EXECUTOR_PLUGIN_DEFAULTS

    assert _EXECUTOR_PLUGIN_DEFAULTS["gather_tensor_results"] is False
    assert local_executor().gather_tensor_results is False
    assert local_executor(gather_tensor_results=True).gather_tensor_results is True


def test_template_renders_the_token_in_both_values():
    from covalent_ssh_plugin_amd.remote.stub import render_worker

    on = render_worker(gather_results=True)
    off = render_worker()
    assert "GATHER_RESULTS = bool(True)" in on and "__CSP_" not in on
    assert "GATHER_RESULTS = bool(False)" in off and "__CSP_" not in off
    compile(on, "worker.py", "exec")
    assert on.replace("GATHER_RESULTS = bool(True)", "GATHER_RESULTS = bool(False)") == off


def test_a_cpu_electron_is_untouched_without_a_library(local_executor):
    def electron(n):
        import torch

        return torch.arange(n * n, dtype=torch.float32).reshape(n, n).t()

    ex = local_executor(gather_tensor_results=True, persistent_workers=True,
                        pinned_staging_threshold_bytes=1024)

    async def run():
        out = await ex.execute(electron, [40], {}, dispatch_id="g", node_id=0)
        meta = ex.last_task_record.remote_meta
        await ex.close_pool()
        return out, meta

    out, meta = asyncio.run(run())
    assert torch.equal(out, torch.arange(1600, dtype=torch.float32).reshape(40, 40).t())
    assert "gathered_tensors" not in meta["staging"] and "gather_fallback" not in meta["staging"]
