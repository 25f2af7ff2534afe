"""DEV TOOL (GPU box): what the ReplayGain analysis costs (the library in use: LAMEJS_HIP_LIB).
  step      one device-resident stream of `frames` frames, 44.1 kHz 128 kbps two channels (the flagship shape), with the option against without, alternated
            `repetitions` times: ms per step, the margin being the spread of the runs without the option; then one extra timed run with the option for
            g_gain_stage's and g_gain's own times (lhip_kernel_times), the bytes they move and the rate as a fraction of the HBM roofline (8 TB/s)
  call      480 host calls of 1152 samples, with the option against without, alternated: us per call (one more launch pair per call)
usage: python tests/tools/replaygain_timing.py step [frames] [repetitions] | call"""
import ctypes
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402
assert torch.cuda.is_available()
torch.zeros(1, device="cuda")
import lamejs_amd  # noqa: E402
import pcm  # noqa: E402

lib = lamejs_amd.load_library()
HBM_BYTES_PER_S = 8e12
WINDOW, WF = 2205, 1984          # 44.1 kHz (lamejs_amd/csrc/k_gain.h)


def calls(on, ch=2, ncalls=480):
    L, R = pcm.sine(1152 * (ncalls + 2), ch)
    enc = lamejs_amd.Mp3Encoder(ch, 44100, 128, replay_gain=on)
    enc.encodeBuffer(L[:2304], None if R is None else R[:2304])
    t0 = time.perf_counter()
    for p in range(2304, len(L), 1152):
        enc.encodeBuffer(L[p:p + 1152], None if R is None else R[p:p + 1152])
    dt = time.perf_counter() - t0
    res = enc.replay_gain() if on else None
    enc.close()
    return 1e6 * dt / ncalls, res


def step(dev, n, on, timing=False):
    enc = lamejs_amd.Mp3Encoder(2, 44100, 128, replay_gain=on)
    cap = int(lib.lhip_max_output_bytes(enc._h, n))
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    H, lp, rp = (ctypes.c_void_p * 1)(enc._h), (ctypes.c_void_p * 1)(dev[0].data_ptr()), (ctypes.c_void_p * 1)(dev[1].data_ptr())
    ns, cp, wr, op = (ctypes.c_size_t * 1)(n), (ctypes.c_size_t * 1)(cap), (ctypes.c_int64 * 1)(), (ctypes.c_void_p * 1)(out.data_ptr())
    nk = lib.lhip_kernel_timing(1) if timing else 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    assert lib.lhip_encode_batch_device(H, 1, lp, rp, ns, op, cp, wr, 1) == 0, lib.lhip_last_error()
    dt = time.perf_counter() - t0
    kt = {}
    for i in range(nk):
        name, ms, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64()
        lib.lhip_kernel_times(i, ctypes.byref(name), ctypes.byref(ms), ctypes.byref(cnt))
        kt[name.value.decode()] = (ms.value, cnt.value)
    if timing:
        lib.lhip_kernel_timing(0)
    res = enc.replay_gain() if on else None
    enc.close()
    return 1e3 * dt, int(wr[0]), kt, res


what = sys.argv[1]
if what == "call":
    for rep in range(3):
        a, b = calls(False), calls(True)
        print(f"rep {rep}: without {a[0]:.1f} us/call   with replay_gain {b[0]:.1f} us/call   {b[1]}")
elif what == "step":
    F = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    n = 1152 * F
    L, R = pcm.sine(n, 2)
    dev = (torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    step(dev, n, False); step(dev, n, True)          # warm-up: workspaces, tables
    off, on = [], []
    for rep in range(REPS):
        a, b = step(dev, n, False), step(dev, n, True)
        off.append(a[0]); on.append(b[0])
        print(f"rep {rep}: without {a[0]:.2f} ms ({a[1]} bytes)   with replay_gain {b[0]:.2f} ms ({b[1]} bytes)   {b[3]}")
    print(f"without: {min(off):.2f} .. {max(off):.2f} ms (spread {max(off) - min(off):.2f});  with: {min(on):.2f} .. {max(on):.2f} ms;  difference of the medians {sorted(on)[len(on) // 2] - sorted(off)[len(off) // 2]:+.2f} ms")
    ms, nbytes, kt, res = step(dev, n, True, timing=True)
    st_ms, g_ms = kt.get("gain_stage", (0.0, 0))[0], kt.get("gain", (0.0, 0))[0]
    st_bytes = 2 * n * (2 + 4 + 4)                                   # Int16 read, row written, (the tail) history written
    g_bytes = 2 * (n // WINDOW) * (WF + WINDOW) * 4                  # every window's lane reads wf + window floats per channel
    print(f"timed run: step {ms:.2f} ms; g_gain_stage {st_ms:.3f} ms over {st_bytes} bytes = {100 * st_bytes / max(st_ms * 1e-3, 1e-12) / HBM_BYTES_PER_S:.2f} % of the HBM roofline; "
          f"g_gain {g_ms:.3f} ms over {g_bytes} bytes = {100 * g_bytes / max(g_ms * 1e-3, 1e-12) / HBM_BYTES_PER_S:.2f} % of the HBM roofline ({n // WINDOW} windows, {(n // WINDOW + 63) // 64} waves)")
