"""TEST INFRASTRUCTURE shared by tests/test_pcmformats_cpu.py and tests/test_pcmformats_gpu.py: sample formats of the C ABI (Int16 / Float32,
planar / interleaved).  Float PCM is derived from the Int16 corpora by exact dyadic arithmetic, bit-identical to
tests/tools/gen_golden_floatpcm.js; the goldens are the unmodified reference's bytes for Float32Array input."""
import ctypes
import json

import numpy as np

import pcm
from conftest import ROOT
from golden_cases import check_stream, feed_calls, load, pinned

S16, F32, INTER = 0, 1, 2
FORMATS = {"s16_planar": S16, "s16_interleaved": S16 | INTER, "f32_planar": F32, "f32_interleaved": F32 | INTER}
HOT = {"sine": 12, "bursts": 6}
KINDS = ("frac", "unit", "hot", "ints")


def golden_floatpcm():
    return load("golden_floatpcm")["cases"]


def float_pcm(kind, corpus, a, right=False):
    """v = (a * K + k) / 2^m on integers (at most 22 significant bits: exact in Float32), as tests/tools/gen_golden_floatpcm.js."""
    a = np.asarray(a).astype(np.int64)
    i = np.arange(len(a), dtype=np.int64)
    k = ((i * 5 + 1) & 15) if right else ((i * 7 + 3) & 15)
    if kind == "frac":
        v = (a * 16 + k) / 16.0
    elif kind == "unit":
        v = (a * 16 + k) / 524288.0
    elif kind == "hot":
        v = (a * 16 * HOT[corpus] + k) / 16.0
    else:
        v = a.astype(np.float64)
    f = v.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), v)      # nothing was rounded
    return f


def case_pcm(case):
    A, B = pcm.CORPORA[case["corpus"]](case["nsamples"], case["channels"])
    L = float_pcm(case["kind"], case["corpus"], A)
    R = float_pcm(case["kind"], case["corpus"], B, True) if case["channels"] == 2 else None
    pinned((L, R), case["pcm_md5"])
    return L, R, A, B


def make_encoder(lib, case_or_cfg, **kw):
    import lamejs_amd
    c = case_or_cfg
    if isinstance(c, dict):
        return lamejs_amd.Mp3Encoder(c["channels"], c["samplerate"], c["kbps"], lib=lib, joint=bool(c.get("joint")), reservoir=bool(c.get("reservoir")),
                                     fractional_resample=bool(c.get("frac")), **kw)
    return lamejs_amd.Mp3Encoder(*c, lib=lib, **kw)


def interleave(l, r):
    if r is None:
        return np.ascontiguousarray(l)
    out = np.empty(2 * len(l), dtype=l.dtype)
    out[0::2] = l
    out[1::2] = r
    return out


def encode_fmt(lib, enc, fmt, l, r, strict=True):
    """One call of lhip_encode_pcm: l / r are planar arrays of the format's sample type; interleaved formats get them interleaved here."""
    dt = np.float32 if fmt & F32 else np.int16
    l = np.ascontiguousarray(l, dtype=dt)
    r = None if (r is None or enc.channels == 1) else np.ascontiguousarray(r, dtype=dt)
    n = len(l)
    if n == 0:
        return b""
    if fmt & INTER:
        a = interleave(l, r)
        pl, pr = a.ctypes.data, None
    else:
        a = None
        pl, pr = l.ctypes.data, (r if r is not None else l).ctypes.data
    exact = lib.lhip_output_bytes_is_exact(enc._h) == 1
    cap = lib.lhip_encode_output_bytes(enc._h, n)
    assert cap >= 0, lib.lhip_last_error()
    out = np.empty(cap + 8, dtype=np.uint8)
    w = lib.lhip_encode_pcm(enc._h, fmt, pl, pr, n, out.ctypes.data, cap)
    if w < 0:
        if strict:
            raise AssertionError((w, lib.lhip_last_error()))
        return w
    assert (w == cap) if exact else (w <= cap)
    return out[:w].tobytes()


def run_golden_case(lib, case, fmt=F32):
    """Every call and the flush of a golden case through lhip_encode_pcm in `fmt` (a Float32 format)."""
    L, R, _, _ = case_pcm(case)
    enc = make_encoder(lib, case)
    try:
        parts = feed_calls(case["call_lens"], L, R, lambda i, l, r: encode_fmt(lib, enc, fmt, l, r))
        # with the bit reservoir a call's byte count depends on when the library hands over finished frames: the stream is judged whole.  A
        # non-integer-ratio stream: the flush frames the reference makes of its own NaN samples are silent stand-ins of equal length by design
        # (include/lamejs_hip.h; tests/test_fracresample_*.py): calls exact, flush by length
        resv = bool(case["reservoir"])
        check_stream(case, parts, enc.flush(), call_bytes=not resv, enc_md5=not resv, flush_md5=not resv and not case["frac"], all_md5=resv)
    finally:
        enc.close()


def run_all_goldens(lib, cases, fmt=F32):
    ran = {k: 0 for k in KINDS}
    for case in cases:
        run_golden_case(lib, case, fmt)
        ran[case["kind"]] += 1
    return ran


# ---- the seeded random family: integer-valued input, so the unchanged oracle (Int16 only) is the reference for every format ----
FAMILY_CONFIGS = [
    # channels, samplerate, kbps, joint, reservoir
    (1, 44100, 128, 0, 0), (2, 44100, 128, 0, 0), (2, 44100, 320, 0, 0), (1, 44100, 64, 0, 0), (2, 48000, 192, 0, 0), (1, 16000, 32, 0, 0),
    (2, 22050, 64, 0, 0), (1, 44100, 32, 0, 0), (2, 44100, 48, 0, 0), (2, 44100, 128, 1, 0), (2, 44100, 192, 1, 0), (2, 44100, 128, 0, 1),
    (1, 44100, 128, 0, 1), (2, 44100, 128, 1, 1),
]


def family(seed, count, max_frames=6):
    """`count` cases: configuration, corpus, amplitude, length, call pattern."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        cfg = FAMILY_CONFIGS[i % len(FAMILY_CONFIGS)]
        n = int(rng.randint(1, max_frames * 1152))
        pattern = ["one", "calls1152", "odd"][int(rng.randint(0, 3))]
        lens, p = [], 0
        while p < n:
            m = n if pattern == "one" else 1152 if pattern == "calls1152" else int(rng.choice([1, 7, 333, 777, 1151, 1153, 2305]))
            m = min(m, n - p)
            lens.append(m)
            p += m
        out.append({"cfg": cfg, "corpus": ["sine", "bursts"][int(rng.randint(0, 2))], "seed": int(rng.randint(1, 1 << 30)), "n": n, "lens": lens})
    return out


def family_pcm(fc):
    ch = fc["cfg"][0]
    return pcm.CORPORA[fc["corpus"]](fc["n"], ch, fc["seed"])


def family_oracle(fc):
    from oracle_py import oracle_encode
    ch, sr, kb, joint, resv = fc["cfg"]
    L, R = family_pcm(fc)
    return oracle_encode(ch, sr, kb, L, R, joint=bool(joint), reservoir=bool(resv))


def family_encode(lib, fc, fmt_of_call):
    """The case through lhip_encode_pcm, call c in format fmt_of_call(c); returns calls + flush."""
    ch, sr, kb, joint, resv = fc["cfg"]
    L, R = family_pcm(fc)
    enc = make_encoder(lib, {"channels": ch, "samplerate": sr, "kbps": kb, "joint": joint, "reservoir": resv})
    try:
        p, got = 0, []
        for c, n in enumerate(fc["lens"]):
            got.append(encode_fmt(lib, enc, fmt_of_call(c), L[p:p + n], None if R is None else R[p:p + n]))
            p += n
        got.append(enc.flush())
        return b"".join(got)
    finally:
        enc.close()


def batch_pcm(lib, encs, fmt, Ls, Rs, device=False, sync=1, keep=None):
    """lhip_encode_batch_pcm (host arrays) or lhip_encode_batch_device_pcm (torch tensors on the GPU) over planar per-stream arrays; returns
    the bytes per stream.  `keep`: a list that receives the device tensors (they must outlive an unsynchronised call)."""
    n = len(encs)
    dt = np.float32 if fmt & F32 else np.int16
    ch = encs[0].channels
    host = []
    for l, r in zip(Ls, Rs):
        l = np.ascontiguousarray(l, dtype=dt)
        r = None if (r is None or ch == 1) else np.ascontiguousarray(r, dtype=dt)
        host.append((interleave(l, r), None) if fmt & INTER else (l, r if r is not None else l))
    counts = [len(l) for l in Ls]
    caps = [int(lib.lhip_max_output_bytes(e._h, c)) for e, c in zip(encs, counts)]
    H = (ctypes.c_void_p * n)(*[e._h for e in encs])
    ns = (ctypes.c_size_t * n)(*counts)
    cp = (ctypes.c_size_t * n)(*caps)
    wr = (ctypes.c_int64 * n)()
    if device:
        import torch
        dev = [(torch.from_numpy(a).cuda(), None if b is None else torch.from_numpy(b).cuda()) for a, b in host]
        outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
        torch.cuda.synchronize()
        lp = (ctypes.c_void_p * n)(*[a.data_ptr() for a, _ in dev])
        rp = (ctypes.c_void_p * n)(*[(b if b is not None else a).data_ptr() for a, b in dev])
        op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
        if keep is not None:
            keep.extend([dev, outs])
        rc = lib.lhip_encode_batch_device_pcm(H, n, fmt, lp, rp, ns, op, cp, wr, sync)
        assert rc == 0, (rc, lib.lhip_last_error())
        rejected = int(lib.lhip_last_batch_rejected_samples())      # waits for the batch
        torch.cuda.synchronize()
        return [outs[i][: wr[i]].cpu().numpy().tobytes() for i in range(n)], rejected
    outs = [np.empty(c, dtype=np.uint8) for c in caps]
    lp = (ctypes.c_void_p * n)(*[a.ctypes.data for a, _ in host])
    rp = (ctypes.c_void_p * n)(*[(b if b is not None else a).ctypes.data for a, b in host])
    op = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    rc = lib.lhip_encode_batch_pcm(H, n, fmt, lp, rp, ns, op, cp, wr)
    if rc != 0:
        return rc, list(wr)
    return [outs[i][: wr[i]].tobytes() for i in range(n)], 0


BAD = [float("nan"), float("inf"), 131072.5, -1e9]


def sim_device_call(lib, enc, fmt, l, r, right_is_left=False):
    """lhip_encode_batch_device_pcm of a SIMULATION (its device pointers are host pointers), sync = 0 -> (bytes, rejected count)."""
    dt = np.float32 if fmt & F32 else np.int16
    l = np.ascontiguousarray(l, dtype=dt)
    r = None if (r is None or enc.channels == 1) else np.ascontiguousarray(r, dtype=dt)
    a, b = (interleave(l, r), None) if fmt & INTER else (l, r if r is not None else l)
    cap = int(lib.lhip_max_output_bytes(enc._h, len(l)))
    out = np.empty(cap, dtype=np.uint8)
    H, lp = (ctypes.c_void_p * 1)(enc._h), (ctypes.c_void_p * 1)(a.ctypes.data)
    rp = (ctypes.c_void_p * 1)(None if right_is_left else (b if b is not None else a).ctypes.data)
    ns, op, cp, wr = (ctypes.c_size_t * 1)(len(l)), (ctypes.c_void_p * 1)(out.ctypes.data), (ctypes.c_size_t * 1)(cap), (ctypes.c_int64 * 1)()
    rc = lib.lhip_encode_batch_device_pcm(H, 1, fmt, lp, rp, ns, op, cp, wr, 0)
    assert rc == 0, (rc, lib.lhip_last_error())
    return out[: wr[0]].tobytes(), int(lib.lhip_last_batch_rejected_samples())


def gpu_device_call(lib, enc, fmt, l, r):
    """The same call on the real library, over torch tensors."""
    keep = []
    (got,), rejected = batch_pcm(lib, [enc], fmt, [l], [r], device=True, sync=0, keep=keep)
    return got, rejected


def device_sanitise_check(lib, call=gpu_device_call, long_call=9 * 1152):
    """The device-pointer entry cannot see the values: out-of-contract Float32 samples are read as 0.0f at every read site -- the bytes equal the
    encode of the input with zeros there -- and counted.  One-frame launches and many-frame batches, direct configurations, both resamplers
    and the reservoir, planar and interleaved.  ONE body for the simulations (call = sim_device_call) and the GPU."""
    G = golden_floatpcm()
    rng = np.random.RandomState(7)
    calls = 0
    for name in ("m1_128_stereo", "m1_128_mono", "resample_int_mono", "resample_frac_stereo", "reservoir_stereo"):
        case = next(c for c in G if c["kind"] == "frac" and c["name"] == name)
        L, R, _, _ = case_pcm(case)
        for fmt in (F32, F32 | INTER):
            dirty, clean = make_encoder(lib, case), make_encoder(lib, case)
            lens = [576] * 10 if case["frac"] else [1152, 1152, long_call, 777, 1152]
            p = 0
            for n in lens:
                l, r = L[p:p + n].copy(), (None if R is None else R[p:p + n].copy())
                zl, zr = l.copy(), (None if r is None else r.copy())
                nbad = 0
                for arr, zarr in ((l, zl), (r, zr)):
                    if arr is None:
                        continue
                    for i in rng.choice(n, size=9, replace=False):
                        arr[i] = BAD[int(rng.randint(0, 4))]
                        zarr[i] = 0.0
                        nbad += 1
                p += n
                got, rejected = call(lib, dirty, fmt, l, r)
                want, zero = call(lib, clean, fmt, zl, zr)
                assert got == want and rejected == nbad and zero == 0, (name, fmt, n, rejected, nbad)
                calls += 1
            assert dirty.flush() == clean.flush()
            dirty.close()
            clean.close()
    return calls


def device_batch_check(lib, fmt):
    """lhip_encode_batch_device_pcm with sync = 0 over torch tensors (float32 / int16, planar / interleaved): many streams of many frames
    (two channels: about 100 frame slots, which is the pair kernel g_quant_pair; one channel: g_quant), one frame per stream (g_frame), reservoir
    streams (g_resv_stream) == the oracle."""
    from oracle_py import oracle_encode
    batches = 0
    for cfg, resv, lens in (((2, 44100, 128), False, [1152 * 40 + 7, 1152 * 25, 777, 1152 * 33 + 1]), ((2, 44100, 128), False, [1152] * 6), ((1, 44100, 128), False, [1152 * 30, 1152 * 11 + 5]),
                            ((2, 44100, 128), True, [1152 * 6, 1152 * 4 + 3, 1152 * 5])):
        rounds = 3
        pcms = [pcm.bursts(n * rounds, cfg[0], seed=300 + i) if i % 2 else pcm.sine(n * rounds, cfg[0], seed=300 + i) for i, n in enumerate(lens)]
        want = [oracle_encode(*cfg, l, r, reservoir=resv) for l, r in pcms]
        encs = [make_encoder(lib, {"channels": cfg[0], "samplerate": cfg[1], "kbps": cfg[2], "reservoir": resv}) for _ in lens]
        got = [b""] * len(lens)
        keep = []
        for k in range(rounds):
            part, rejected = batch_pcm(lib, encs, FORMATS[fmt], [p[0][n * k:n * (k + 1)] for p, n in zip(pcms, lens)],
                                       [None if p[1] is None else p[1][n * k:n * (k + 1)] for p, n in zip(pcms, lens)], device=True, sync=0, keep=keep)
            assert rejected == 0
            got = [g + p for g, p in zip(got, part)]
            batches += 1
        assert [g + e.flush() for g, e in zip(got, encs)] == want, (fmt, cfg, resv, lens)
        for e in encs:
            e.close()
    return batches


if __name__ == "__main__":
    # the checks that hold torch tensors run in a process of their own: torch initialises the GPU first, then the library is loaded
    import sys
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")
    sys.path.insert(0, str(ROOT))
    import lamejs_amd
    if sys.argv[1:] == ["--device-sanitise"]:
        print(json.dumps({"device_sanitise_calls": device_sanitise_check(lamejs_amd.load_library())}))
    elif sys.argv[1:2] == ["--device-batch"]:
        print(json.dumps({"device_batches": device_batch_check(lamejs_amd.load_library(), sys.argv[2])}))
    else:
        sys.exit(2)
