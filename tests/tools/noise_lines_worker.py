"""TEST TOOL: the cases of tests/noise_lines_cases.py on the device in one environment, in a process of its own because the library reads
LAMEJS_HIP_PAIR_MAX_FRAMES once per process.

usage: noise_lines_worker.py <environment name>

Encodes every case call by call (calls completing 1, 2, 9, 17 and 20 frames, then the flush), compares each call's bytes with the oracle's and
prints one JSON line per call: the case, the call, the frames it completed, the path set the library reports for it and the first differing
byte (null = equal).  The last line is {"done": true, ...}.  Exit status 0 unless the program itself failed: mismatches are for the parent to
judge."""
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import libs
import noise_lines_cases as nl
from path_matrix_cases import ENVS, SWITCHES


def main():
    env_name = sys.argv[1]
    t0 = time.time()
    lib = libs.gpu_library()
    assert {k: os.environ[k] for k in SWITCHES if k in os.environ} == ENVS[env_name], env_name
    frames = 0
    for c in nl.CASES:
        for r in nl.encode_case(lib, c, nl.SEQ_GPU):
            frames += r["frames"]
            print(json.dumps(r), flush=True)
    print(json.dumps({"done": True, "cases": len(nl.CASES), "frames": frames, "seconds": round(time.time() - t0, 2)}), flush=True)


if __name__ == "__main__":
    main()
