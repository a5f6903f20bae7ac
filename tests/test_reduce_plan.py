"""The fold launch plan (csrc/reduce_plan.hpp) without a GPU: the stand-alone
program tests/cpp/test_reduce_plan.cpp under the address and undefined-
behaviour sanitizers.  It reproduces the recorded plans of
tests/golden/reduce_plan_cases.txt line for line, checks the production shapes
that the GPU tests and DESIGN.md state, and that the grid reaches exactly the
combinations expected_combinations() of test_gpu_wide_small.py lists, plus the
small shape.
"""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "ipls-java-api_amd"
CASES = ROOT / "tests" / "golden" / "reduce_plan_cases.txt"


def test_reduce_plan_under_the_sanitizers():
    subprocess.run(["make", "-C", str(PKG), "reduce_plan_test"], check=True, capture_output=True)
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "test_reduce_plan"), str(CASES)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"reduce_plan ok: (\d+) plans", r.stdout)
    assert m, r.stdout
    # 19 lengths x 18 partition counts x (10 rows of doubles + 8 of the trainer formats)
    lines = len(CASES.read_text().splitlines())
    assert lines == 19 * 18 * 18
    assert int(m.group(1)) == lines, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
