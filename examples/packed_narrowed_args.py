"""Small tensor arguments narrowed inside the packed arena.

``pack_tensor_args=True`` sends the small CPU tensors of an electron's
arguments as one frame; with ``narrow_tensor_args=True`` as well, each of them
crosses the pipe at the narrowest width that gives every element back bit for
bit: a ``state_dict`` of float32 tensors upcast from bf16 at half its bytes,
int64 index tensors at a quarter or an eighth.  One
``csp_unpack_widen_checksum_dev`` launch on the worker reads the narrow arena,
writes every tensor at full width and verifies the whole.  Needs one MI355X.

    python examples/packed_narrowed_args.py
"""

import asyncio
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from covalent_ssh_plugin_amd import SSHExecutor  # noqa: E402


def state():
    gen = torch.Generator().manual_seed(7)
    out = {}
    for layer in range(40):
        out["w%d" % layer] = torch.randn(256, 256, generator=gen).bfloat16().float()
        out["idx%d" % layer] = torch.randint(0, 30000, (4096,), generator=gen)
    return out


def digest(tensors):
    """What arrived: all on the GPU, and a sum per dtype."""
    return (all(t.is_cuda for t in tensors.values()),
            float(sum(t.double().sum() for t in tensors.values())))


async def main():
    tensors = state()
    want = float(sum(t.double().sum() for t in tensors.values()))
    with tempfile.TemporaryDirectory() as home:
        for narrow in (False, True):
            ex = SSHExecutor(
                transport="local", local_home=home, cache_dir=home + "/cache",
                python_path=sys.executable, persistent_workers=True, device_tensor_args=True,
                pack_tensor_args=True, narrow_tensor_args=narrow,
            )
            try:
                cuda, got = await ex.execute(digest, [tensors], {}, dispatch_id="demo",
                                             node_id=int(narrow))
                stage = ex.last_task_record.remote_meta["arg_staging"]
            finally:
                await ex.close_pool()
            assert cuda and got == want
            print(
                "narrow_tensor_args=%s: %d tensors, %d arena bytes, frame %d bytes, "
                "%d segments widened, saved %d"
                % (narrow, stage["packed_tensors"], stage["bytes"],
                   stage.get("wire_bytes", stage["bytes"]), stage.get("widened", 0),
                   ex.counters["arg_narrow_saved_bytes"])
            )


if __name__ == "__main__":
    asyncio.run(main())
