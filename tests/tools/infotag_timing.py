"""DEV TOOL (GPU box): what the Info tag costs, and what its CRC would cost on the host (the library in use: LAMEJS_HIP_LIB).
  step      one device-resident stream of `frames` frames, 44.1 kHz 128 kbps two channels (the flagship shape), tagged against untagged, alternated
            `repetitions` times: ms per step; then one extra timed run of the tagged step for g_out_crc's own time (lhip_kernel_times), the bytes it
            read and the rate as a fraction of the HBM roofline (8 TB/s)
  call      480 host calls of 1152 samples, tagged against untagged, alternated: us per call (the small-call path: host CRC, no launch gained)
  size      lhip_debug_crc16 (device path: upload + kernel + fetch) for buffers of 1 KiB .. 64 MiB: us per call, for the boundary discussion
  hostcrc   the host's byte-at-a-time table CRC over `mib` MiB (the walk of lhip_infotag.h, compiled here as a small C program): ms and GB/s
usage: python tests/tools/infotag_timing.py step [frames] [repetitions] | call | size | hostcrc [mib]"""
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
HBM_BYTES_PER_S = 8e12


def calls(tagged, ch=2, ncalls=480):
    L, R = pcm.sine(1152 * (ncalls + 2), ch)
    enc = lamejs_amd.Mp3Encoder(ch, 44100, 128, info_tag=tagged)
    enc.encodeBuffer(L[:2304], None if R is None else R[:2304])
    t0 = time.perf_counter()
    for p in range(2304, len(L), 1152):
        enc.encodeBuffer(L[p:p + 1152], None if R is None else R[p:p + 1152])
    dt = time.perf_counter() - t0
    enc.close()
    return 1e6 * dt / ncalls


def step(dev, n, tagged, timing=False):
    enc = lamejs_amd.Mp3Encoder(2, 44100, 128, info_tag=tagged)
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
    enc.close()
    return 1e3 * dt, int(wr[0]), kt


what = sys.argv[1]
if what == "call":
    for rep in range(3):
        print(f"rep {rep}: untagged {calls(False):.1f} us/call   tagged {calls(True):.1f} us/call")
elif what == "step":
    F = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    L, R = pcm.sine(1152 * F, 2)
    dev = (torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    step(dev, 1152 * F, False); step(dev, 1152 * F, True)          # warm-up: workspaces, tables
    for rep in range(REPS):
        a, b = step(dev, 1152 * F, False), step(dev, 1152 * F, True)
        print(f"rep {rep}: untagged {a[0]:.2f} ms ({a[1]} bytes)   tagged {b[0]:.2f} ms ({b[1]} bytes)")
    ms, nbytes, kt = step(dev, 1152 * F, True, timing=True)
    crc_ms, launches = kt.get("out_crc", (0.0, 0))
    print(f"timed run: step {ms:.2f} ms; g_out_crc + fold {crc_ms * 1e3:.1f} us in {launches} launches over {nbytes} bytes = "
          f"{nbytes / max(crc_ms, 1e-9) / 1e9 * 1e3:.1f} GB/s = {100 * nbytes / max(crc_ms * 1e-3, 1e-12) / HBM_BYTES_PER_S:.2f} % of the HBM roofline")
elif what == "hostcrc":
    import subprocess
    import tempfile
    mib = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    src = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
int main(int argc, char** argv) {
    size_t n = (size_t)atoi(argv[1]) << 20; uint8_t* p = malloc(n); uint16_t t[256]; uint32_t x = 12345;
    for (size_t i = 0; i < n; i++) { x = x * 1103515245u + 12345u; p[i] = (uint8_t)(x >> 16); }
    for (int i = 0; i < 256; i++) { uint32_t c = i; for (int b = 0; b < 8; b++) c = (c & 1) ? (c >> 1) ^ 0xA001u : c >> 1; t[i] = (uint16_t)c; }
    for (int rep = 0; rep < 3; rep++) {
        struct timespec a, b; clock_gettime(CLOCK_MONOTONIC, &a);
        uint32_t crc = 0; for (size_t i = 0; i < n; i++) crc = (crc >> 8) ^ t[(crc ^ p[i]) & 0xff];
        clock_gettime(CLOCK_MONOTONIC, &b);
        double ms = (b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) / 1e6;
        printf("rep %d: %zu bytes, crc %04x, %.2f ms = %.2f GB/s\n", rep, n, crc, ms, n / ms / 1e6);
    }
    return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "c.c").write_text(src)
        subprocess.run(["gcc", "-O2", "-o", str(Path(d) / "c"), str(Path(d) / "c.c")], check=True)
        print(subprocess.run([str(Path(d) / "c"), str(mib)], capture_output=True, text=True, check=True).stdout, end="")
elif what == "size":
    rng = np.random.RandomState(5)
    for kib in (1, 16, 256, 1024, 8192, 41 * 1024, 65536):
        buf = rng.randint(0, 256, kib * 1024).astype(np.uint8)
        r = ctypes.c_uint32()
        lib.lhip_debug_crc16(buf.ctypes.data, len(buf), 0, ctypes.byref(r))
        t0 = time.perf_counter()
        for _ in range(3):
            lib.lhip_debug_crc16(buf.ctypes.data, len(buf), 0, ctypes.byref(r))
        print(f"{kib} KiB: {1e6 * (time.perf_counter() - t0) / 3:.0f} us per call (allocation + upload + kernels + fetch)")
