"""``narrow_tensor_results``: an electron returns the float32 logits of a bf16
model and the token ids it picked; the logits cross the pipe as bfloat16 and
the int64 ids as int16 or int32, and both arrive bit for bit as they were.

    python examples/narrowed_results.py

Needs one MI355X and the built libraries (``python -m
covalent_ssh_plugin_amd.ops.build``).  The tables of
``profiles/narrowed_results.md`` come from ``tools/narrow_results_bench.py``.
"""

import asyncio
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from covalent_ssh_plugin_amd import SSHExecutor  # noqa: E402


def decode_step(batch, vocab):
    """The electron: logits of a bf16 projection, upcast at the end, their
    argmax, and float32 noise that no narrower type holds."""
    import torch

    hidden = torch.randn(batch, 1024, device="cuda", dtype=torch.bfloat16)
    head = torch.randn(1024, vocab, device="cuda", dtype=torch.bfloat16)
    logits = (hidden @ head).float()
    return {"logits": logits, "ids": logits.argsort(dim=-1), "noise": torch.randn_like(logits)}


async def main():
    with tempfile.TemporaryDirectory() as home:
        ex = SSHExecutor(
            transport="local", local_home=home, cache_dir=home + "/cache",
            python_path=sys.executable, persistent_workers=True,
            narrow_tensor_results=True, pinned_staging_threshold_bytes=1 << 20,
            hip_visible_devices_policy="fixed", fixed_gpu=0,
        )
        out = await ex.execute(decode_step, [64, 32000], {}, dispatch_id="narrow", node_id=0)
        meta = ex.last_task_record.remote_meta
        await ex.close_pool()
    for name, info in zip(out, meta["buffers"]):
        tensor = out[name]
        print("%-6s %s %s on the wire as %s" % (
            name, tensor.dtype, tuple(tensor.shape), info.get("wire", "itself")))
    staging = meta["staging"]
    print("narrowed %d of %d tensors, %d of %d bytes saved, %s ms on the worker" % (
        staging.get("narrowed", 0), staging["tensors"], staging.get("narrow_saved_bytes", 0),
        staging["bytes"], staging.get("narrow_ms")))
    print("the one that travels whole:", staging.get("narrow_fallback"))
    assert out["logits"].dtype.is_floating_point and int(out["ids"].max()) == 31999


if __name__ == "__main__":
    asyncio.run(main())
