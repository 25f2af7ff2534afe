"""TEST/BENCH helper: one process of bench.py's cpu_baseline aggregate leg -- the plain-C oracle (oracle/, test infrastructure) encoding
a bench stream on one host core for a FIXED TIME: the stream is fed in chunks of 250 frames until `seconds` have passed (or its K
frames are done).  Prints `frames seconds` (the encode only; PCM generation and start-up are outside the clock).
usage: cpu_port_worker.py <corpus> <channels> <kbps> <max frames> <seed> <seconds> [start_after_epoch_seconds]"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import pcm  # noqa: E402
import oracle_py  # noqa: E402
from lamejs_amd import tables_blob  # noqa: E402

corpus, ch, kbps, k, seed, secs = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6])
L, R = pcm.CORPORA[corpus](1152 * k, ch, seed=seed)
L = np.ascontiguousarray(L, dtype=np.int16)
R = None if ch == 1 else np.ascontiguousarray(R, dtype=np.int16)
o = oracle_py.OracleStream(tables_blob(ch, 44100, kbps, False, False))
CH = 250
if len(sys.argv) > 7:                                                                  # all workers start their clock together
    while time.time() < float(sys.argv[7]):
        time.sleep(0.005)
t0 = time.perf_counter()
done = 0
while done < k:
    m = min(CH, k - done)
    o.encode(L[1152 * done:1152 * (done + m)], None if R is None else R[1152 * done:1152 * (done + m)])
    done += m
    if time.perf_counter() - t0 >= secs:
        break
dt = time.perf_counter() - t0
o.close()
print(done, dt, flush=True)
