"""Build driver for the in-tree native libraries.

``ops/libcsp_gpu.so`` is built from ``ops/hip/csp_gpu.hip`` with hipcc
for **gfx950 only** (MI355X; no multi-arch fatbin, no CUDA path).  hipcc
cross-compiles without a GPU, so this runs in CPU-only CI; the built .so
travels to the GPU box in the repo snapshot and to the remote execution
host via the executor's content-addressed lib provisioning (ssh.py
_provision_gpu_lib).

``ops/libcsp_io.so`` is built from ``ops/csrc/csp_io.cpp`` with the host
C++ compiler (hipcc only as a fallback): host-only exact-length fd I/O
for the dispatcher side of the worker channel, no HIP or ROCm in it.
"""

from __future__ import annotations

import os
import shutil
import subprocess
import sys
from pathlib import Path
from typing import List

OPS_DIR = Path(__file__).resolve().parent
SRC = OPS_DIR / "hip" / "csp_gpu.hip"
OUT = OPS_DIR / "libcsp_gpu.so"
IO_SRC = OPS_DIR / "csrc" / "csp_io.cpp"
IO_HDR = OPS_DIR / "csrc" / "csp_io.h"
IO_OUT = OPS_DIR / "libcsp_io.so"

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def _stale(out: Path, sources: List[Path]) -> bool:
    if not out.exists():
        return True
    built = out.stat().st_mtime
    return any(built < src.stat().st_mtime for src in sources)


def gpu_needs_build() -> bool:
    return _stale(OUT, [SRC, IO_HDR])


def io_needs_build() -> bool:
    return _stale(IO_OUT, [IO_SRC, IO_HDR])


def needs_build() -> bool:
    return gpu_needs_build() or io_needs_build()


def _run(cmd: List[str], verbose: bool) -> None:
    if verbose:
        print("+", " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)


def host_cxx() -> str:
    """The host C++ compiler for libcsp_io.so: $CXX, c++, g++, clang++,
    and hipcc (which compiles plain C++ too) only when none of them is
    there."""
    for name in (os.environ.get("CXX", ""), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    return HIPCC


def build_io(force: bool = False, verbose: bool = True) -> Path:
    if not force and not io_needs_build():
        return IO_OUT
    _run(
        [
            host_cxx(),
            "-O3",  # the checksum loop wants the vectoriser (gcc < 12: not at -O2)
            "-std=c++17",
            "-fPIC",
            "-shared",
            "-pthread",
            str(IO_SRC),
            "-o",
            str(IO_OUT),
        ],
        verbose,
    )
    return IO_OUT


def build_gpu(force: bool = False, verbose: bool = True) -> Path:
    if not force and not gpu_needs_build():
        return OUT
    _run(
        [
            HIPCC,
            f"--offload-arch={ARCH}",
            "-O3",
            "-std=c++17",
            "-fPIC",
            "-shared",
            str(SRC),
            "-o",
            str(OUT),
        ],
        verbose,
    )
    return OUT


def build(force: bool = False, verbose: bool = True) -> Path:
    """Build both libraries (each only when stale); returns the GPU
    library's path, as before."""
    build_io(force=force, verbose=verbose)
    return build_gpu(force=force, verbose=verbose)


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(OUT)
    print(IO_OUT)
