"""The source-operand resolver (csrc/operand.hpp) without a GPU: the stand-alone
program tests/cpp/test_operand.cpp under the address and undefined-behaviour
sanitizers.  It runs every entry-point row x every operand kind over short,
exact and long counts, misaligned sources, null sources and whole, cut and
empty containers, and checks each outcome -- the refusal's code and text, or
the payload pointer, count, format and memory -- against a second statement of
the entry points' contract written out in the program.
"""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "ipls-java-api_amd"


def test_operand_resolver_under_the_sanitizers():
    subprocess.run(["make", "-C", str(PKG), "operand_test"], check=True, capture_output=True)
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "test_operand")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"operand ok: (\d+) cases over 12 rows", r.stdout)
    assert m, r.stdout
    # 12 rows x 18 kinds x 3 lengths x 4 counts x (5 offsets + a null source) is 15552; the containers come on top
    assert int(m.group(1)) > 15552, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
