"""DEV TOOL (GPU box): what the downmix costs.  Config 2's shape -- one 44.1 kHz 128 kbps mono stream, 1e5 frames, device-resident -- fed one
channel, against the same output produced by { downmix } from planar and from interleaved stereo, Int16 and Float32, alternated.  Every
encoder is built with scale = 1 and the stereo pair has l + r even, so the one-channel feed m = (l + r) / 2 is exact and all variants must
give one md5.  Per variant the step time (median of the repetitions) and, from one extra timed run, the per-kernel times (lhip_kernel_timing)
of the kernels that read samples.
usage: python tests/tools/inputmix_timing.py [frames] [repetitions]"""
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
L, R = L.astype(np.int32), R.astype(np.int32)
R = R - ((L + R) & 1)
R[R < -32768] += 2
M = ((L + R) // 2).astype(np.int16)
L, R = L.astype(np.int16), R.astype(np.int16)
IL = np.empty(2 * n, np.int16)
IL[0::2], IL[1::2] = L, R
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
# name -> (channels in, downmix, format, left, right)
VAR = {
    "mono_s16": (1, False, 0, t(M), None), "mono_f32": (1, False, 1, t(M.astype(np.float32)), None),
    "downmix_s16_planar": (2, True, 0, t(L), t(R)), "downmix_s16_interleaved": (2, True, 2, t(IL), None),
    "downmix_f32_planar": (2, True, 1, t(L.astype(np.float32)), t(R.astype(np.float32))), "downmix_f32_interleaved": (2, True, 3, t(IL.astype(np.float32)), None),
}
mk = lambda v: lamejs_amd.Mp3Encoder(v[0], 44100, 128, downmix=v[1], scale=1.0)      # noqa: E731
_e = mk(VAR["mono_s16"])
cap = int(lib.lhip_max_output_bytes(_e._h, n))
_e.close()
out = torch.zeros(cap, dtype=torch.uint8, device="cuda")


def step(name, timing=False):
    v = VAR[name]
    enc = mk(v)
    a, b = v[3], v[4]
    H, lp, rp = (ctypes.c_void_p * 1)(enc._h), (ctypes.c_void_p * 1)(a.data_ptr()), (ctypes.c_void_p * 1)((b if b is not None else a).data_ptr())
    ns, op, cp, wr = (ctypes.c_size_t * 1)(n), (ctypes.c_void_p * 1)(out.data_ptr()), (ctypes.c_size_t * 1)(cap), (ctypes.c_int64 * 1)()
    nk = lib.lhip_kernel_timing(1) if timing else 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = lib.lhip_encode_batch_device_pcm(H, 1, v[2], lp, rp, ns, op, cp, wr, 1)
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


for name in VAR:
    step(name)                                  # warm-up
ref = None
times = {k: [] for k in VAR}
for rep in range(REPS):
    for name in VAR:
        ms, dg, _ = step(name)
        ref = ref or dg
        assert dg == ref, (name, dg, ref)
        times[name].append(round(ms, 3))
print(f"shape: 1 stream x {F} mono frames out, 44.1 kHz, 128 kbps, scale 1, device-resident, sync = 1; {REPS} alternated repetitions; md5 of every variant: {ref}")
for name in VAR:
    _, _, kt = step(name, timing=True)
    print(f"{name:24s} step_ms {times[name]} median {sorted(times[name])[len(times[name]) // 2]}   kernels_ms (timed run) " + " ".join(f"{k} {v}" for k, v in kt.items() if k in ("psyA", "polyphase", "save", "count_rejected", "prep")))
