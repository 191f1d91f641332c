"""Small CUDA results narrowed inside the packed arena.

``pack_tensor_results=True`` sends the small CUDA tensors of a result as one
arena; with ``narrow_tensor_results=True`` as well, each of them crosses the
pipe at the narrowest width that gives every element back bit for bit: a
``state_dict`` of float32 tensors upcast from bf16 at half its bytes, int64
index tensors at a quarter or an eighth.  One probe launch and one
fill-and-sum launch serve the whole arena.  Needs one MI355X.

    python examples/packed_narrowed_results.py
"""

import asyncio
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from covalent_ssh_plugin_amd import SSHExecutor  # noqa: E402


def state():
    import torch

    gen = torch.Generator().manual_seed(7)
    out = {}
    for layer in range(40):
        w = torch.randn(256, 256, generator=gen).bfloat16()
        out["w%d" % layer] = w.cuda().float()  # bf16 values held as float32
        out["idx%d" % layer] = torch.randint(0, 30000, (4096,), generator=gen).cuda()
    return out


async def main():
    with tempfile.TemporaryDirectory() as home:
        for narrow in (False, True):
            ex = SSHExecutor(
                transport="local", local_home=home, cache_dir=home + "/cache",
                python_path=sys.executable, persistent_workers=True,
                pack_tensor_results=True, narrow_tensor_results=narrow,
            )
            try:
                value = await ex.execute(state, [], {}, dispatch_id="demo", node_id=int(narrow))
                meta = ex.last_task_record.remote_meta
            finally:
                await ex.close_pool()
            info = meta["buffers"][0]
            wires = sorted({e.get("wire", "-") for e in info["packed"]})
            print(
                "narrow_tensor_results=%s: %d tensors, frame %d bytes, wire dtypes %s, saved %d"
                % (narrow, len(value), info["nbytes"], wires,
                   meta["staging"].get("narrow_saved_bytes", 0))
            )


if __name__ == "__main__":
    asyncio.run(main())
