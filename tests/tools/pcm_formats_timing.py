"""DEV TOOL (GPU box): what the sample formats cost.  Config 3's shape -- one two-channel 44.1 kHz 128 kbps stream, 1e5 frames, device-resident --
through lhip_encode_batch_device_pcm in all four formats, alternated, md5 of every format checked against Int16 planar's; per format the
step time and the per-kernel times (lhip_kernel_timing) of the kernels that read samples.  Then the host scan: one 1e5-frame lhip_encode_pcm
Float32 host call against the same samples as Int16 through lhip_encode, and the scan alone (a call refused at its last sample).
usage: python tests/tools/pcm_formats_timing.py [frames] [repetitions]"""
import ctypes
import hashlib
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
assert torch.cuda.is_available()
torch.zeros(1, device="cuda")
import lamejs_amd  # noqa: E402
import pcm  # noqa: E402

F = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
lib = lamejs_amd.load_library()
n = 1152 * F
L, R = pcm.sine(n, 2)
IL = np.empty(2 * n, np.int16)
IL[0::2], IL[1::2] = L, R
dev = {0: (torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()), 2: (torch.from_numpy(IL).cuda(), None),
       1: (torch.from_numpy(L.astype(np.float32)).cuda(), torch.from_numpy(R.astype(np.float32)).cuda()), 3: (torch.from_numpy(IL.astype(np.float32)).cuda(), None)}
NAMES = {0: "s16_planar", 2: "s16_interleaved", 1: "f32_planar", 3: "f32_interleaved"}
_e = lamejs_amd.Mp3Encoder(2, 44100, 128)
cap = int(lib.lhip_max_output_bytes(_e._h, n))
_e.close()
out = torch.zeros(cap, dtype=torch.uint8, device="cuda")


def step(fmt, timing=False):
    enc = lamejs_amd.Mp3Encoder(2, 44100, 128)
    a, b = dev[fmt]
    H, lp, rp = (ctypes.c_void_p * 1)(enc._h), (ctypes.c_void_p * 1)(a.data_ptr()), (ctypes.c_void_p * 1)((b if b is not None else a).data_ptr())
    ns, op, cp, wr = (ctypes.c_size_t * 1)(n), (ctypes.c_void_p * 1)(out.data_ptr()), (ctypes.c_size_t * 1)(cap), (ctypes.c_int64 * 1)()
    nk = lib.lhip_kernel_timing(1) if timing else 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = lib.lhip_encode_batch_device_pcm(H, 1, fmt, lp, rp, ns, op, cp, wr, 1)
    dt = time.perf_counter() - t0
    assert rc == 0, lib.lhip_last_error()
    kt = {}
    for i in range(nk):
        nm, ms, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64()
        lib.lhip_kernel_times(i, ctypes.byref(nm), ctypes.byref(ms), ctypes.byref(cnt))
        kt[nm.value.decode()] = round(ms.value, 4)
    if timing:
        lib.lhip_kernel_timing(0)
    digest = hashlib.md5(out[: wr[0]].cpu().numpy().tobytes()).hexdigest()
    enc.close()
    return dt * 1e3, digest, kt


for fmt in NAMES:
    step(fmt)                                   # warm-up
ref = None
times = {f: [] for f in NAMES}
for rep in range(REPS):
    for fmt in NAMES:
        ms, dg, _ = step(fmt)
        ref = ref or dg
        assert dg == ref, (NAMES[fmt], dg, ref)
        times[fmt].append(round(ms, 3))
print(f"shape: 1 stream x {F} two-channel frames, 44.1 kHz, 128 kbps, device-resident, sync = 1; {REPS} alternated repetitions; md5 of every format == s16_planar's: {ref}")
for fmt in NAMES:
    _, _, kt = step(fmt, timing=True)
    print(f"{NAMES[fmt]:16s} step_ms {times[fmt]} median {sorted(times[fmt])[len(times[fmt]) // 2]}   kernels_ms (timed run) " + " ".join(f"{k} {v}" for k, v in kt.items()))

# ---- host calls: the scan of a Float32 host call ----
Lf, Rf = L.astype(np.float32), R.astype(np.float32)
res = {"s16_host": [], "f32_host": [], "scan_only": []}
obuf = np.empty(cap, np.uint8)
for rep in range(REPS + 1):
    for name in ("s16_host", "f32_host"):
        enc = lamejs_amd.Mp3Encoder(2, 44100, 128)
        t0 = time.perf_counter()
        if name == "s16_host":
            w = lib.lhip_encode(enc._h, L.ctypes.data, R.ctypes.data, n, obuf.ctypes.data, cap)
        else:
            w = lib.lhip_encode_pcm(enc._h, 1, Lf.ctypes.data, Rf.ctypes.data, n, obuf.ctypes.data, cap)
        dt = (time.perf_counter() - t0) * 1e3
        assert w > 0 and hashlib.md5(obuf[:w].tobytes()).hexdigest() == ref
        enc.close()
        if rep:
            res[name].append(round(dt, 2))
    # the library's own scan, alone: the same call with the LAST sample of the right plane out of contract is scanned whole, then refused (-4)
    bad = Rf.copy()
    bad[-1] = np.inf
    enc = lamejs_amd.Mp3Encoder(2, 44100, 128)
    t0 = time.perf_counter()
    w = lib.lhip_encode_pcm(enc._h, 1, Lf.ctypes.data, bad.ctypes.data, n, obuf.ctypes.data, cap)
    dt = (time.perf_counter() - t0) * 1e3
    assert w == -4
    enc.close()
    if rep:
        res["scan_only"].append(round(dt, 2))
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
print("host call of", F, "frames (ms):", res)
print(f"medians: s16_host {med['s16_host']}  f32_host {med['f32_host']}  scan_only {med['scan_only']}  -> the scan is {100 * med['scan_only'] / med['f32_host']:.1f} % of the Float32 host call (serial, in front of the first copy)")
