"""``narrow_tensor_args``: an electron takes the int64 ``edge_index`` of a
graph, float32 features that came out of a bf16 pipeline and float32 noise;
the indices cross the pipe as int32, the features as bfloat16, the noise whole,
and all three arrive in HBM bit for bit as they were.  Sent again, the cached
ones travel as a key alone and nothing is narrowed.

    python examples/narrowed_args.py

Needs one MI355X and the built libraries (``python -m
covalent_ssh_plugin_amd.ops.build``).  The tables of
``profiles/narrowed_args.md`` come from ``tools/narrow_args_bench.py``.
"""

import asyncio
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from covalent_ssh_plugin_amd import SSHExecutor  # noqa: E402


def aggregate(edge_index, features, noise):
    """The electron: one round of neighbour sums on the GPU."""
    import torch

    assert edge_index.is_cuda and features.is_cuda and noise.is_cuda
    out = torch.zeros_like(features)
    out.index_add_(0, edge_index[1], features[edge_index[0]])
    return float(out.sum() + noise.sum())


async def main():
    nodes, edges = 100_000, 2_000_000
    edge_index = torch.randint(0, nodes, (2, edges))
    features = torch.randn(nodes, 64, dtype=torch.bfloat16).float()
    noise = torch.randn(nodes, 64)
    with tempfile.TemporaryDirectory() as home:
        ex = SSHExecutor(
            transport="local", local_home=home, cache_dir=home + "/cache",
            python_path=sys.executable, persistent_workers=True, device_tensor_args=True,
            narrow_tensor_args=True, cache_tensor_args=True,
            pinned_staging_threshold_bytes=1 << 20,
            hip_visible_devices_policy="fixed", fixed_gpu=0,
        )
        for node in range(2):
            value = await ex.execute(aggregate, [edge_index, features, noise], {},
                                     dispatch_id="narrow", node_id=node)
            stage = ex.last_task_record.remote_meta["arg_staging"]
            print("run %d: %.1f; widened %d tensors from %d bytes in %.3f ms, mode %s" % (
                node, value, stage.get("widened", 0), stage.get("wire_bytes", 0),
                stage.get("widen_ms", 0.0), stage["mode"]))
        print({k: v for k, v in ex.counters.items() if k.startswith(("arg_narrow", "arg_cache"))})
        assert ex.counters["arg_narrowed"] == 2 and ex.counters["arg_cache_hits"] == 3
        await ex.close_pool()


if __name__ == "__main__":
    asyncio.run(main())
