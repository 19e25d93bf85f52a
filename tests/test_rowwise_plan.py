"""The host dispatch of the row-wise kernels (csrc/rowwise_plan.h: RMSNorm MAXC / waves / workgroups / chained-dw
columns, CE register chunks, SwiGLU kernel family and grid, RoPE grid and FastDiv) is plain C++ with no HIP
dependency; tests/rowwise_plan_check.cpp sweeps fdiv(n, make_fastdiv(d)) == n / d over every d in 1..4096, the powers
of two +-1 up to 2^30 and random d, at the edges of every quotient and random n < 2^31. CPU only."""
import os
import subprocess

from picotron_amd import build

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rowwise_plan_check.cpp")


def compile_check(tmp_path):
    exe = str(tmp_path / "rowwise_plan_check")
    # host only: the plan header must compile without the HIP headers
    subprocess.run([build.HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-nogpuinc", "-nogpulib",
                    "-o", exe, SRC], check=True)
    return exe


def test_fastdiv_sweep(tmp_path):
    r = subprocess.run([compile_check(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout
