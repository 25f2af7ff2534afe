"""DEV TOOL (GPU box): what the WAV sample types cost (DESIGN_EXTENSIONS.md 4.10).  Config 3's shape -- one two-channel 44.1 kHz 128 kbps stream,
1e5 frames.
  device   device-resident: S24 interleaved (g_ingest in front), Float32 interleaved (read in place) and Int16 planar, alternated; one md5 per
           variant; the step time, g_ingest's own time (lhip_kernel_timing) and its bytes moved over that time against the HBM roofline
  host     one host call of the same samples as packed 24-bit: lhip_encode_pcm(LHIP_PCM_S24) where the library has it, and what a caller does
           without it -- numpy widening to Float32 (timed on its own), then the Float32 host call.  LAMEJS_HIP_LIB selects the library, so the
           second form also runs on a build from before the sample types.
usage: python tests/tools/wavpcm_timing.py device|host [frames] [repetitions]"""
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

MODE = sys.argv[1] if len(sys.argv) > 1 else "device"
F = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
HBM_TBS = 8.0          # MI355X: 8 TB/s peak HBM3E bandwidth
S16, F32, INTER, S24 = 0, 1, 2, 8
lib = ctypes.CDLL(str(Path(__import__("os").environ.get("LAMEJS_HIP_LIB", ROOT / "lamejs_amd" / "lib" / "liblamejs_hip.so"))))
for name, (restype, argtypes) in lamejs_amd.ABI.items():          # (a build from before this change lacks the newest entries)
    if hasattr(lib, name):
        getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
n = 1152 * F
L, R = pcm.sine(n, 2)
IL = np.empty(2 * n, np.int16)
IL[0::2], IL[1::2] = L, R
raw24 = np.zeros((2 * n, 3), np.uint8)          # v * 256 as packed 24-bit: the low byte is zero, then the Int16's two bytes
raw24[:, 1:] = IL.view(np.uint8).reshape(-1, 2)
raw24 = raw24.reshape(-1)
enc0 = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib)
cap = int(lib.lhip_max_output_bytes(enc0._h, n))
enc0.close()
median = lambda v: sorted(v)[len(v) // 2]


def kernel_times(nk):
    kt = {}
    for i in range(nk):
        nm, ms, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64()
        lib.lhip_kernel_times(i, ctypes.byref(nm), ctypes.byref(ms), ctypes.byref(cnt))
        kt[nm.value.decode()] = round(ms.value, 4)
    return kt


if MODE == "device":
    dev = {"s24_interleaved": (S24 | INTER, torch.from_numpy(raw24).cuda(), None), "f32_interleaved": (F32 | INTER, torch.from_numpy(IL.astype(np.float32)).cuda(), None),
           "s16_planar": (S16, torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())}
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")

    def step(name, timing=False):
        fmt, a, b = dev[name]
        enc = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib)
        H, lp, rp = (ctypes.c_void_p * 1)(enc._h), (ctypes.c_void_p * 1)(a.data_ptr()), (ctypes.c_void_p * 1)((b if b is not None else a).data_ptr())
        ns, op, cp, wr = (ctypes.c_size_t * 1)(n), (ctypes.c_void_p * 1)(out.data_ptr()), (ctypes.c_size_t * 1)(cap), (ctypes.c_int64 * 1)()
        nk = lib.lhip_kernel_timing(1) if timing else 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.lhip_encode_batch_device_pcm(H, 1, fmt, lp, rp, ns, op, cp, wr, 1)
        dt = time.perf_counter() - t0
        assert rc == 0, lib.lhip_last_error()
        kt = kernel_times(nk)
        if timing:
            lib.lhip_kernel_timing(0)
        digest = hashlib.md5(out[: wr[0]].cpu().numpy().tobytes()).hexdigest()
        enc.close()
        return dt * 1e3, digest, kt

    for name in dev:
        step(name)          # warm-up
    times, md5 = {k: [] for k in dev}, {}
    for rep in range(REPS):
        for name in dev:
            ms, dg, _ = step(name)
            assert md5.setdefault(name, dg) == dg
            times[name].append(round(ms, 3))
    assert len(set(md5.values())) == 1, md5
    print(f"shape: 1 stream x {F} two-channel frames, 44.1 kHz, 128 kbps, device-resident, sync = 1; {REPS} alternated repetitions; md5 of every variant: {md5['s16_planar']}")
    for name in dev:
        _, _, kt = step(name, timing=True)
        print(f"{name:16s} step_ms {times[name]} median {median(times[name])}   kernels_ms (timed run) " + " ".join(f"{k} {v}" for k, v in kt.items() if v))
        if name == "s24_interleaved" and kt.get("ingest"):
            moved = 2 * n * (3 + 4)
            print(f"  g_ingest: {kt['ingest']} ms for {moved / 1e9:.3f} GB ({2 * n * 3 / 1e9:.3f} in, {2 * n * 4 / 1e9:.3f} out) = {moved / kt['ingest'] / 1e9:.2f} TB/s = "
                  f"{100 * moved / kt['ingest'] / 1e9 / HBM_TBS:.1f} % of the {HBM_TBS} TB/s HBM roofline; {100 * kt['ingest'] / median(times[name]):.2f} % of the step")
elif MODE == "host":
    obuf = np.empty(cap, np.uint8)
    have = hasattr(lib, "lhip_debug_ingest")
    res = {"s24_call": [], "widen": [], "f32_call": []}
    ref = None
    for rep in range(REPS + 1):
        if have:
            enc = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib)
            t0 = time.perf_counter()
            w = lib.lhip_encode_pcm(enc._h, S24 | INTER, raw24.ctypes.data, None, n, obuf.ctypes.data, cap)
            dt = (time.perf_counter() - t0) * 1e3
            assert w > 0, lib.lhip_last_error()
            dg = hashlib.md5(obuf[:w].tobytes()).hexdigest()
            ref = ref or dg
            assert dg == ref
            enc.close()
            if rep:
                res["s24_call"].append(round(dt, 2))
        # what a caller does without the type: widen on the host, then the Float32 call
        t0 = time.perf_counter()
        b = raw24.reshape(-1, 3)
        v = b[:, 0].astype(np.int32) | (b[:, 1].astype(np.int32) << 8) | (b[:, 2].view(np.int8).astype(np.int32) << 16)
        wide = v.astype(np.float32) * np.float32(1 / 256)
        t1 = time.perf_counter()
        enc = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib)
        t2 = time.perf_counter()
        w = lib.lhip_encode_pcm(enc._h, F32 | INTER, wide.ctypes.data, None, n, obuf.ctypes.data, cap)
        t3 = time.perf_counter()
        assert w > 0, lib.lhip_last_error()
        dg = hashlib.md5(obuf[:w].tobytes()).hexdigest()
        ref = ref or dg
        assert dg == ref
        enc.close()
        if rep:
            res["widen"].append(round((t1 - t0) * 1e3, 2))
            res["f32_call"].append(round((t3 - t2) * 1e3, 2))
    print(f"host call of {F} two-channel frames as packed 24-bit ({lib.lhip_version().decode()}; S24 entry: {'yes' if have else 'no'}); md5 {ref}; ms per repetition:", res)
    med = {k: median(v) for k, v in res.items() if v}
    print("medians:", med, f"-> widen + Float32 call {med['widen'] + med['f32_call']:.2f} ms" + (f"; S24 call {med['s24_call']} ms" if have else ""))
else:
    sys.exit(2)
