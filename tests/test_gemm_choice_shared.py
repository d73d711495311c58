"""Host check of the split-bf16 GEMM's two tile rules (csrc/gemm_choice.hpp): by makespan on an empty chip, and by chip time for a
launch that shares the GPU with another stream (option ``g3_shared``)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_gemm_choice_shared_rule_on_the_host(tmp_path):
    """`choose_g3(..., shared)` compiled for the host: at the four ViT-B/32 block shapes (M = 12 800, 256 CUs) the chip-time rule
    picks the 8-phase kernel, uncut, and the default rule what it picked before; plus the patch embedding, a so400m shape, 64 and
    304 CUs and the small grids where both rules agree (tests/native/gemm_choice_shared_check.cpp holds the table)."""
    exe = tmp_path / "gemm_choice_shared_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe),
                    str(ROOT / "tests" / "native" / "gemm_choice_shared_check.cpp")], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout
