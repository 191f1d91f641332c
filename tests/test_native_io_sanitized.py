"""AddressSanitizer + UBSan over the host-only I/O library: a stand-alone
C++ program (tests/native/csp_io_selftest.cpp, its own main) is compiled
together with csp_io.cpp and run as its own process.  The sanitizer
runtime is linked into that binary only and never enters Python."""

import subprocess
from pathlib import Path

from covalent_ssh_plugin_amd.ops import build as ops_build

SELFTEST = Path(__file__).parent / "native" / "csp_io_selftest.cpp"


def test_csp_io_selftest_under_asan_ubsan(tmp_path):
    binary = tmp_path / "csp_io_selftest"
    compile_cmd = [
        ops_build.host_cxx(),
        "-std=c++17",
        "-O1",
        "-g",
        "-fno-omit-frame-pointer",
        "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all",
        "-pthread",
        str(ops_build.IO_SRC),
        str(SELFTEST),
        "-o",
        str(binary),
    ]
    built = subprocess.run(compile_cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(binary)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "csp_io selftest ok" in ran.stdout
