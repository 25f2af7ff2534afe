"""DEV TOOL (GPU box): what the fast encoding mode (quality 7) costs and what its own quantization kernel gives.
Three variants on the same device-resident samples, alternated REPS times, each run in a process of its own (LAMEJS_HIP_NO_FAST_QUANT is read once
per process):
  q3          quality 3 (the general kernels, noise shaping and all)
  q7_general  quality 7 through the general kernels (LAMEJS_HIP_NO_FAST_QUANT=1: they read the switches)
  q7_fast     quality 7 through g_quant_fast
Shapes: bench.py's configs 3 and 2 -- one stream of `frames` frames, two channels / one channel, 44.1 kHz 128 kbps, the `sine` corpus, seed 12345,
sync = 1.  Per run: three timed steps behind a warm-up (ms, frames/s from the median), then one extra step with per-kernel timing (HIP events around
every launch: the kernels' own times and their share of that step), the launch paths and the md5 of the bytes.  The md5 of the two quality-7 variants
must be equal.  Then `calls`: 480 host calls of 1152 samples per variant (the one-frame program).
Achieved occupancy needs a counter run of its own (rocprofv3 --pmc) and is not collected here; the resident waves by registers and LDS are in
profiles/quality7_code_object_diff_parent_vs_result.txt.
usage: python tests/tools/quality_timing.py [frames] [repetitions]            (the parent: spawns the runs, prints the table)
       python tests/tools/quality_timing.py one <variant> <channels> <frames>  (one run -> one JSON line)
       python tests/tools/quality_timing.py calls <variant>                    (480 calls -> one JSON line)"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
VARIANTS = {"q3": (3, False), "q7_general": (7, True), "q7_fast": (7, False)}


def child(args, variant, timeout=300):
    e = dict(os.environ)
    e.pop("LAMEJS_HIP_NO_FAST_QUANT", None)
    if VARIANTS[variant][1]:
        e["LAMEJS_HIP_NO_FAST_QUANT"] = "1"
    r = subprocess.run([sys.executable, __file__] + args, capture_output=True, text=True, env=e, timeout=timeout)
    if r.returncode != 0:      # a run that faulted, hung or failed ends the series: nothing more is started on the device
        print(f"run {args} failed with exit code {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def gpu_imports():
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import numpy as np
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")
    import lamejs_amd
    import pcm
    return np, torch, lamejs_amd, pcm


def one(variant, ch, frames):
    np, torch, lamejs_amd, pcm = gpu_imports()
    lib = lamejs_amd.load_library()
    quality = VARIANTS[variant][0]
    L, R = pcm.sine(1152 * frames, ch, seed=12345)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ((L, R) if ch == 2 else (L, L))]
    n = 1152 * frames

    def step(timing=False):
        enc = lamejs_amd.Mp3Encoder(ch, 44100, 128, quality=quality)
        cap = int(lib.lhip_max_output_bytes(enc._h, n))
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        H, lp, rp = (ctypes.c_void_p * 1)(enc._h), (ctypes.c_void_p * 1)(dev[0].data_ptr()), (ctypes.c_void_p * 1)(dev[1].data_ptr())
        ns, cp, wr, op = (ctypes.c_size_t * 1)(n), (ctypes.c_size_t * 1)(cap), (ctypes.c_int64 * 1)(), (ctypes.c_void_p * 1)(out.data_ptr())
        nk = lib.lhip_kernel_timing(1) if timing else 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.lhip_encode_batch_device_pcm(H, 1, 0, lp, rp, ns, op, cp, wr, 1)
        dt = time.perf_counter() - t0
        assert rc == 0, lib.lhip_last_error()
        kt = {}
        for i in range(nk):
            nm, ms, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64()
            lib.lhip_kernel_times(i, ctypes.byref(nm), ctypes.byref(ms), ctypes.byref(cnt))
            if ms.value > 0:
                kt[nm.value.decode()] = round(ms.value, 4)
        if timing:
            lib.lhip_kernel_timing(0)
        paths = sorted(lamejs_amd.last_batch_paths(lib))
        stats = enc.last_batch_stats()
        md5 = hashlib.md5(out[:wr[0]].cpu().numpy().tobytes()).hexdigest()
        enc.close()
        return dt * 1e3, kt, paths, md5, stats

    step()                                      # warm-up
    ms = [round(step()[0], 3) for _ in range(3)]
    tms, kt, paths, md5, stats = step(timing=True)
    med = sorted(ms)[1]
    print(json.dumps({"variant": variant, "ch": ch, "frames": frames, "step_ms": ms, "median_ms": med, "frames_per_s": round(frames / med * 1e3), "timed_step_ms": round(tms, 3),
                      "kernels_ms": kt, "share_pct": {k: round(100 * v / sum(kt.values()), 1) for k, v in kt.items()}, "paths": paths, "md5": md5, "repaired_frames": stats["repaired_frames"]}))


def calls(variant, ncalls=480):
    np, torch, lamejs_amd, pcm = gpu_imports()
    quality = VARIANTS[variant][0]
    res = {"variant": variant}
    for ch in (1, 2):
        L, R = pcm.sine(1152 * (ncalls + 2), ch)
        enc = lamejs_amd.Mp3Encoder(ch, 44100, 128, quality=quality)
        enc.encodeBuffer(L[:2304], None if R is None else R[:2304])
        t0 = time.perf_counter()
        for p in range(2304, len(L), 1152):
            enc.encodeBuffer(L[p:p + 1152], None if R is None else R[p:p + 1152])
        res[f"ch{ch}_us_per_call"] = round(1e6 * (time.perf_counter() - t0) / ncalls, 1)
        enc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "one":
        one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    elif len(sys.argv) > 1 and sys.argv[1] == "calls":
        calls(sys.argv[2])
    else:
        F = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
        REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
        print(f"{REPS} alternated repetitions per shape and variant, each a process of its own; 44.1 kHz, 128 kbps, sine corpus (seed 12345), {F} frames, device-resident, sync = 1", flush=True)
        for name, ch in (("config3_stereo", 2), ("config2_mono", 1)):
            runs = {v: [] for v in VARIANTS}
            for rep in range(REPS):
                for v in VARIANTS:
                    runs[v].append(child(["one", v, str(ch), str(F)], v))
            for v in VARIANTS:
                meds = [r["median_ms"] for r in runs[v]]
                last = runs[v][-1]
                print(f"{name:15s} {v:11s} median_ms per repetition {meds}  spread {round(max(meds) - min(meds), 3)}  frames/s {[r['frames_per_s'] for r in runs[v]]}  repaired {last['repaired_frames']}")
                print(f"{'':15s} {'':11s} steps_ms {[r['step_ms'] for r in runs[v]]}")
                print(f"{'':15s} {'':11s} kernels_ms (timed run of the last repetition, step {last['timed_step_ms']} ms) " + " ".join(f"{k} {x} ({last['share_pct'][k]} %)" for k, x in last["kernels_ms"].items()))
                print(f"{'':15s} {'':11s} quant / validate over the repetitions {[(r['kernels_ms'].get('quant'), r['kernels_ms'].get('validate')) for r in runs[v]]}  paths {' '.join(last['paths'])}  md5 {last['md5']}")
            same = {r["md5"] for r in runs["q7_general"]} == {r["md5"] for r in runs["q7_fast"]} and len({r["md5"] for r in runs["q7_fast"]}) == 1
            print(f"{name:15s} md5 of q7_general and q7_fast equal: {same}; differs from q3: {runs['q3'][0]['md5'] != runs['q7_fast'][0]['md5']}", flush=True)
            if not same:
                sys.exit(1)
        for rep in range(REPS):
            print(f"calls480 rep{rep + 1} " + "  ".join(f"{v} ch=1 {r['ch1_us_per_call']} ch=2 {r['ch2_us_per_call']} us/call" for v in VARIANTS for r in [child(["calls", v], v)]), flush=True)
