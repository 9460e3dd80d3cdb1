"""Record tests/golden/phys_launches.json (GPU box): the launch counts and
counters of every case of tests/test_gpu_phys_launches.py, from the library
LDPC_HIP_LIB names -- one built at the commit BEFORE a change to the host loops
of ldpc_api.cpp, so that the test compares the change with its parent.  Every
case runs twice; a case whose two runs differ is not deterministic and stops
the recording (nothing is written).
usage: LDPC_HIP_LIB=/path/to/parent/libldpc_hip.so python tools/record_phys_launches.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ldpc-simulator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_gpu_phys_launches import CASES, GOLDEN_FILE, run_case  # noqa: E402
from ldpc_amd import _lib  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN_FILE
print(f"library: {_lib.LIB_PATH}")
recorded, unstable = {}, []
for case_id in sorted(CASES):
    first, second = run_case(case_id), run_case(case_id)
    print(case_id, json.dumps(first))
    if first != second:
        unstable.append(case_id)
        print(f"  second run differs: {json.dumps(second)}")
    recorded[case_id] = first
if unstable:
    sys.exit(f"not deterministic, nothing written: {unstable}")
with open(out_path, "w") as f:
    json.dump(recorded, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"wrote {len(recorded)} cases to {out_path}")
