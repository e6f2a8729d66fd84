"""Writes tests/golden/mirror_records.json: the bytes every make_* builder of the Python mirror produces for the cases of
tests/mirror_cases.py.  The file pins the builders as they were BEFORE they were folded into records.fill / records.build; it was
recorded once from that commit's package and is not to be regenerated from later code (a change of a C record changes the header, the
record and this file together, in a commit that says so).

    python tests/golden/make_golden_mirror.py [output]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry      # noqa: E402
import mirror_cases                   # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "mirror_records.json")
    got = mirror_cases.run_cases(entry.load_package())
    with open(out, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} cases, {sum(len(v) for v in got.values()) // 2} bytes of records -> {out}")
