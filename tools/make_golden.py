"""Generate tests/golden/oracle_ccs.json, tests/golden/record_cases.json and
tests/golden/shred_cases.json (regression vectors of the oracle)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import Poa  # noqa: E402
from tests.zmw_cases import (RECORD_FAMILIES, record_golden_entry, shred_cases, shred_golden_entry,  # noqa: E402
                             synth)

cases = []
for hole, L, passes, mode in [(1, 2000, 8, 0), (2, 3000, 6, 0), (3, 2500, 5, 1), (4, 1200, 20, 0), (5, 4500, 7, 0)]:
    p = synth(hole, L, passes)
    out = Poa().zmw(p.seqs, p.offs, p.lens, mode)
    cases.append({"hole": hole, "L": L, "passes": passes, "mode": mode, "len": len(out),
                  "sha256": hashlib.sha256(out).hexdigest(), "prefix": out[:60].decode()})
with open(os.path.join(ROOT, "tests", "golden", "oracle_ccs.json"), "w") as f:
    json.dump({"generator": "tools/make_golden.py", "seed": 20201104, "cases": cases}, f, indent=1)
print("wrote", len(cases), "cases")

# the constructed case families (tests/test_record_cases.py): per case the CCS
# of both modes and a SHA-256 of the consensus codes and the MSA bytes
poa = Poa()
fams = {f: {name: record_golden_entry(poa, reads) for name, reads in gen().items()} for f, gen in RECORD_FAMILIES.items()}
with open(os.path.join(ROOT, "tests", "golden", "record_cases.json"), "w") as f:
    json.dump({"generator": "tools/make_golden.py", "families": fams}, f, indent=0, sort_keys=True)
print("wrote", sum(len(v) for v in fams.values()), "record cases")

# the shredding-loop family (tests/test_shred_cases.py): per case the SHA-256
# of the shredded CCS and the whole breakpoint log
shred = {name: shred_golden_entry(poa, reads) for name, reads in shred_cases().items()}
with open(os.path.join(ROOT, "tests", "golden", "shred_cases.json"), "w") as f:
    json.dump({"generator": "tools/make_golden.py", "cases": shred}, f, indent=0, sort_keys=True)
print("wrote", len(shred), "shred cases")
