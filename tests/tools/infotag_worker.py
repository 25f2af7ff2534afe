"""TEST TOOL: one Info tag check (tests/infotag_cases.py) in a process of its own, for the checks that depend on what the library reads from the
environment once (LAMEJS_HIP_NO_SMALL_CALLS, LAMEJS_HIP_NO_FRAME_KERNEL).  Last line of output: the JSON result.
usage: python tests/tools/infotag_worker.py <batch|resv_batch|goldens> [case name ...]      (library: LAMEJS_HIP_LIB, or the HIP library)"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import infotag_cases as ic  # noqa: E402
import lamejs_amd  # noqa: E402

lib = lamejs_amd.load_library()
what = sys.argv[1]
if what == "batch":
    res = {"paths": sorted(ic.mixed_batch_check(lib))}
elif what == "resv_batch":
    res = {"paths": sorted(ic.resv_batch_check(lib))}
elif what == "goldens":
    seen, n = set(), 0
    for c in ic.goldens():
        if c["name"] in sys.argv[2:]:
            ic.run_golden_case(lib, c)
            seen |= set(lamejs_amd.last_batch_paths(lib))
            n += 1
    res = {"cases": n, "paths": sorted(seen)}
else:
    raise SystemExit("unknown check " + what)
print(json.dumps(res))
