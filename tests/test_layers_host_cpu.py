"""feedback_gnn_amd/csrc/fgnn_layers.h on its own: tests/layers_check.cpp, built with the host compiler (the header includes no HIP
header), run plain and under the address and undefined-behaviour sanitizers.  The program states what it checks."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_layerings_and_their_tables_on_an_irregular_graph(flags):
    src = os.path.join(ROOT, "tests", "layers_check.cpp")
    inc = os.path.join(ROOT, "feedback_gnn_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "layers_check")
        cc = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I" + inc, src, "-o", exe],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert cc.returncode == 0 and not cc.stdout, cc.stdout
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout == "ok\n", (run.returncode, run.stdout[-2000:])
