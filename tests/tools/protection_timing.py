"""DEV TOOL (GPU box): what frame protection costs, and the host-call latency of the library in use (LAMEJS_HIP_LIB selects it: the A/B of the
untouched path runs this tool with the parent commit's library and with this tree's).
  calls     480 host calls of 1152 samples (the one-frame program), one and two channels, 44.1 kHz 128 kbps, no options: us per call
  protect   unprotected against { protect } streams on the same samples and shapes, alternated: the step (one device-resident stream of
            `frames` frames; one and two channels), the formatter kernel's time from one extra timed run, the 1152-sample call, and the
            reservoir walk (64 streams x 100 frames).  The material differs slightly by construction: a protected frame has 16 bits less
            for its main data, so the searches behind it are not the same searches.
usage: python tests/tools/protection_timing.py calls | protect [frames] [repetitions]"""
import ctypes
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402
assert torch.cuda.is_available()
torch.zeros(1, device="cuda")
import lamejs_amd  # noqa: E402
import pcm  # noqa: E402

lib = lamejs_amd.load_library()


def calls(ch, ncalls=480, **kw):
    L, R = pcm.sine(1152 * (ncalls + 2), ch)
    enc = lamejs_amd.Mp3Encoder(ch, 44100, 128, **kw)
    enc.encodeBuffer(L[:2304], None if R is None else R[:2304])
    t0 = time.perf_counter()
    for p in range(2304, len(L), 1152):
        enc.encodeBuffer(L[p:p + 1152], None if R is None else R[p:p + 1152])
    dt = time.perf_counter() - t0
    enc.close()
    return 1e6 * dt / ncalls


if sys.argv[1] == "calls":
    print(" ".join(f"ch={ch} 480 calls of 1152 samples: {calls(ch):.1f} us/call" for ch in (1, 2)))
    sys.exit(0)

F = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731


def step(ch, dev, nstreams, n, timing=False, **kw):
    encs = [lamejs_amd.Mp3Encoder(ch, 44100, 128, **kw) for _ in range(nstreams)]
    cap = int(lib.lhip_max_output_bytes(encs[0]._h, n))
    out = torch.zeros(cap * nstreams, dtype=torch.uint8, device="cuda")
    H = (ctypes.c_void_p * nstreams)(*[e._h for e in encs])
    lp = (ctypes.c_void_p * nstreams)(*[dev[0].data_ptr()] * nstreams)
    rp = (ctypes.c_void_p * nstreams)(*[(dev[1] if dev[1] is not None else dev[0]).data_ptr()] * nstreams)
    ns, cp, wr = (ctypes.c_size_t * nstreams)(*[n] * nstreams), (ctypes.c_size_t * nstreams)(*[cap] * nstreams), (ctypes.c_int64 * nstreams)()
    op = (ctypes.c_void_p * nstreams)(*[out.data_ptr() + i * cap for i in range(nstreams)])
    nk = lib.lhip_kernel_timing(1) if timing else 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = lib.lhip_encode_batch_device_pcm(H, nstreams, 0, lp, rp, ns, op, cp, wr, 1)
    dt = time.perf_counter() - t0
    assert rc == 0, lib.lhip_last_error()
    kt = {}
    for i in range(nk):
        nm, ms, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64()
        lib.lhip_kernel_times(i, ctypes.byref(nm), ctypes.byref(ms), ctypes.byref(cnt))
        kt[nm.value.decode()] = round(ms.value, 4)
    if timing:
        lib.lhip_kernel_timing(0)
    for e in encs:
        e.close()
    return dt * 1e3, kt


SHAPES = [("mono_1e5", 1, 1, F, {}), ("stereo_1e5", 2, 1, F, {}), ("reservoir_64x100", 2, 64, 100, {"reservoir": True})]
print(f"{REPS} alternated repetitions per shape; 44.1 kHz, 128 kbps, sine corpus, device-resident, sync = 1")
for name, ch, nstreams, frames, kw in SHAPES:
    L, R = pcm.sine(1152 * frames, ch)
    dev = (t(L), None if R is None else t(R))
    res = {False: [], True: []}
    for p in (False, True):
        step(ch, dev, nstreams, 1152 * frames, protect=p, **kw)          # warm-up
    for rep in range(REPS):
        for p in (False, True):
            res[p].append(round(step(ch, dev, nstreams, 1152 * frames, protect=p, **kw)[0], 3))
    for p in (False, True):
        _, kt = step(ch, dev, nstreams, 1152 * frames, timing=True, protect=p, **kw)
        print(f"{name:18s} {'protect' if p else 'plain  '} step_ms {res[p]} median {sorted(res[p])[len(res[p]) // 2]}   kernels_ms (timed run) " + " ".join(f"{k} {v}" for k, v in kt.items() if k in ("bits", "quant", "resv_stream")))
for rep in range(REPS):
    print(f"calls480 rep{rep + 1} " + " ".join(f"ch={ch} plain {calls(ch):.1f} protect {calls(ch, protect=True):.1f} us/call" for ch in (1, 2)))
