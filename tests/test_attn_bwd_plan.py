"""The host plan of the split attention backward (csrc/attn_bwd_plan.h: kernel choice, block groups, hsplit, grids,
workspace layout) is plain C++ with no HIP dependency; tests/attn_bwd_plan_check.cpp sweeps it over head dims,
causal, sequence lengths, batch x heads, GQA groups, the three pico_select knobs and CU counts, and checks that
every key block is in exactly one group, hsplit is a power of two (1 with groups), the workspace regions are
disjoint, ordered, aligned and end at the reported total, and the block size matches the kernel chosen. CPU only."""
import os
import subprocess

from picotron_amd import build


def test_plan_sweep(tmp_path):
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_bwd_plan_check.cpp")
    exe = str(tmp_path / "attn_bwd_plan_check")
    # host only: the plan header must compile without the HIP headers
    subprocess.run([build.HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-nogpuinc", "-nogpulib",
                    "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout
