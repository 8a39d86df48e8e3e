"""Every `file:line` citation of the reference (headers, docs, docstrings) must point into an existing file of the
reference tree and inside its length.  The reference's file lengths are stored in tests/golden/reference_line_counts.json
(regenerate with `python tests/test_citations.py <reference checkout>`), so the check needs nothing outside the
repository."""
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE_COUNTS = os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")
FILE_PAT = r"(?:src|include/DPGO|examples|tests|cmake)/[A-Za-z0-9_/]+\.(?:cpp|h|cmake)|CMakeLists\.txt"
PAT = re.compile(r"(" + FILE_PAT + r"):(\d+)(?:-(\d+))?")


def test_reference_citations_exist():
    lengths = json.load(open(LINE_COUNTS))
    files = [os.path.join(ROOT, f) for f in ("DESIGN.md", "INTEGRATION.md", "README.md", "bench.py", "__graft_entry__.py")]
    for pat in ("include/*.h", "include/*.hpp", "dpgo_amd/*.py", "dpgo_amd/csrc/*.hip", "dpgo_amd/csrc/*.cpp",
                "dpgo_amd/csrc/*.h", "dpgo_amd/csrc/kernels/*.h", "oracle/*.py", "oracle/*.c", "tests/*.py", "tests/cxx/*.cpp",
                "examples/*.py"):
        files += glob.glob(os.path.join(ROOT, pat))
    bad, n = [], 0
    for f in files:
        if os.path.basename(f) == "test_citations.py":
            continue
        text = open(f, errors="replace").read()
        for m in PAT.finditer(text):
            rel, lo, hi = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
            # the repo's own tests/ and include/ paths are not reference citations
            if rel.startswith("tests/") and os.path.exists(os.path.join(ROOT, rel)):
                continue
            n += 1
            if rel not in lengths:
                bad.append("%s: %s does not exist in the reference" % (os.path.relpath(f, ROOT), m.group(0)))
                continue
            if lo < 1 or hi < lo or hi > lengths[rel]:
                bad.append("%s: %s is outside the file (%d lines)" % (os.path.relpath(f, ROOT), m.group(0), lengths[rel]))
    assert n > 200, "citation pattern no longer matches anything"
    assert not bad, "\n".join(bad[:40])


if __name__ == "__main__":  # python tests/test_citations.py <reference checkout>: rewrite the stored file lengths
    ref = sys.argv[1]
    counts = {}
    for dirpath, _, names in os.walk(ref):
        for name in names:
            path = os.path.join(dirpath, name)
            rel = os.path.relpath(path, ref).replace(os.sep, "/")
            if re.fullmatch(FILE_PAT, rel):
                counts[rel] = sum(1 for _ in open(path, errors="replace"))
    with open(LINE_COUNTS, "w") as out:
        json.dump(dict(sorted(counts.items())), out, indent=1)
        out.write("\n")
