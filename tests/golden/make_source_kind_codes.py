"""Records tests/golden/source_kind_codes.txt: the return code and error text
of every case of tests/source_kind_cases.py, one `id<TAB>code<TAB>text` line
each, from the library that IPLS_AGG_LIB names (default: the tree's own).

The committed file was recorded on an MI355X from a build of the commit before
the source-operand resolver (csrc/operand.hpp), so that
tests/test_gpu_source_kinds.py holds every entry point to the codes and texts
it had then:
    IPLS_AGG_LIB=<that build>/libipls_agg.so python tests/golden/make_source_kind_codes.py OUT
"""
import sys
from pathlib import Path

import torch   # before the library loads (tests/conftest.py)

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (ROOT, ROOT / "ipls-java-api_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import ipls   # noqa: E402
import source_kind_cases as C   # noqa: E402


def record(rig, cases, lines):
    rig.prepare()
    for case in cases:
        r = rig.run(case)
        assert "\t" not in r.text and "\n" not in r.text, r.text
        lines.append(f"{case.id}\t{r.rc}\t{r.text}")
        rig.finish(case)
        rig.prepare()
    rig.close()


def main(out):
    lines = []
    record(C.Rig(ipls, torch), [c for call in C.CALLS for c in C.cases(call)], lines)
    for L in C.SEAM_LENS:
        record(C.Rig(ipls, torch, 0, 1, bucket_len=L), [c for c in C.seam_cases() if c.id.startswith(f"seam{L}.")], lines)
    Path(out).write_text("\n".join(lines) + "\n")
    print(f"{len(lines)} cases -> {out}")


if __name__ == "__main__":
    main(sys.argv[1])
