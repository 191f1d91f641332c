"""bool tensors as bits: an electron takes a padding mask and returns the mask
of the activations it kept; with ``narrow_tensor_args`` and
``narrow_tensor_results`` both cross the pipe at one bit per element and arrive
bit for bit as they were.

    python examples/bool_bits.py

Needs one MI355X and the built libraries (``python -m
covalent_ssh_plugin_amd.ops.build``).  The tables of ``profiles/bool_bits.md``
come from ``tools/bool_bits_bench.py``.
"""

import asyncio
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from covalent_ssh_plugin_amd import SSHExecutor  # noqa: E402


def keep_mask(padding):
    """The electron: which unpadded activations a ReLU lets through."""
    import torch

    x = torch.randn(padding.shape, device="cuda")
    return (x > 0) & padding


async def main():
    padding = torch.arange(4096).expand(2048, 4096) < torch.randint(1, 4096, (2048, 1))
    padding = padding.contiguous()
    with tempfile.TemporaryDirectory() as home:
        ex = SSHExecutor(
            transport="local", local_home=home, cache_dir=home + "/cache",
            python_path=sys.executable, persistent_workers=True, device_tensor_args=True,
            narrow_tensor_args=True, narrow_tensor_results=True,
            pinned_staging_threshold_bytes=1 << 20,
            hip_visible_devices_policy="fixed", fixed_gpu=0,
        )
        kept = await ex.execute(keep_mask, [padding], {}, dispatch_id="bits", node_id=0)
        meta = ex.last_task_record.remote_meta
        await ex.close_pool()
    print("argument: %d bool elements, %d bytes on the wire" % (
        padding.numel(), meta["arg_staging"].get("wire_bytes", padding.numel())))
    print("result:   %s %s on the wire as %s, %d bytes saved" % (
        kept.dtype, tuple(kept.shape), meta["buffers"][0].get("wire", "itself"),
        meta["staging"].get("narrow_saved_bytes", 0)))
    assert kept.dtype == torch.bool and not (kept & ~padding).any()


if __name__ == "__main__":
    asyncio.run(main())
