"""TEST INFRASTRUCTURE shared by tests/test_wavpcm_cpu.py and tests/test_wavpcm_gpu.py: the sample types a WAV file stores (LHIP_PCM_U8 ..
LHIP_PCM_F64 of include/lamejs_hip.h).  The yardsticks are the ones the Float32 formats have: the goldens of the unmodified reference for
Float32Array input (tests/golden/golden_floatpcm.json) -- their `frac` PCM is (a * 16 + k) / 16, which packed 24-bit integers, 32-bit integers
and normalised floats reach exactly -- and the unchanged oracle on Int16 values for 8-bit input."""
import ctypes
import json
import sys

import numpy as np

import pcm
import pcmformats_cases as pc
from conftest import ROOT
from golden_cases import check_stream, feed_calls

U8, S24, S32, F32N, F64N, F64, INTER = 4, 8, 12, 16, 20, 24, 2
BYTES = {U8: 1, S24: 3, S32: 4, F32N: 4, F64N: 8, F64: 8}
NAMES = {U8: "u8", S24: "s24", S32: "s32", F32N: "f32n", F64N: "f64n", F64: "f64"}
LIMIT = 131072.0


# ---- elements <-> bytes -------------------------------------------------------------------------------------------------------------
def pack(typ, v):
    """The elements `v` (integers for the integer types, floats for the float types) as the bytes a WAV file holds."""
    v = np.asarray(v)
    if typ == U8:
        assert v.min(initial=0) >= 0 and v.max(initial=0) <= 255
        return v.astype(np.uint8).tobytes()
    if typ == S24:
        v = v.astype(np.int64)
        assert v.min(initial=0) >= -(1 << 23) and v.max(initial=0) < (1 << 23)
        return np.ascontiguousarray((v & 0xffffff).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
    if typ == S32:
        v = v.astype(np.int64)
        assert v.min(initial=0) >= -(1 << 31) and v.max(initial=0) < (1 << 31)
        return v.astype("<i4").tobytes()
    return np.asarray(v, dtype="<f4" if typ == F32N else "<f8").tobytes()


def expected_f32(typ, v):
    """numpy's form of the header's table: the Float32 the encoder sees, and which elements are refused (read as zero)."""
    v = np.asarray(v)
    if typ == U8:
        return ((v.astype(np.int64) - 128) * 256).astype(np.float32), np.zeros(len(v), bool)
    if typ == S24:
        return (v.astype(np.float64) / 256.0).astype(np.float32), np.zeros(len(v), bool)
    if typ == S32:
        return (v.astype(np.float64) / 65536.0).astype(np.float32), np.zeros(len(v), bool)
    with np.errstate(over="ignore", invalid="ignore"):
        if typ == F32N:
            d = (v.astype(np.float32) * np.float32(32768.0)).astype(np.float64)
        else:
            d = v.astype(np.float64) * 32768.0 if typ == F64N else v.astype(np.float64)
        bad = ~(np.abs(d) <= LIMIT)
        out = np.where(bad, 0.0, d).astype(np.float32)
    return out, bad


def debug_ingest(lib, typ, v, channels=1, layout="mono", misalign=0):
    """lhip_debug_ingest over the elements `v` (channels * n of them: interleaved, or plane after plane) -> (left, right or None, rejected)."""
    raw = np.frombuffer(pack(typ, v), dtype=np.uint8)
    n = len(raw) // (BYTES[typ] * channels)
    left, right = np.full(n, 7.0, np.float32), np.full(n, 7.0, np.float32)
    rej = ctypes.c_int64(-1)
    fmt = typ | (INTER if layout == "interleaved" else 0)
    rc = lib.lhip_debug_ingest(fmt, channels, raw.ctypes.data, n, misalign, left.ctypes.data, right.ctypes.data if channels == 2 else None, ctypes.byref(rej))
    assert rc == 0, (rc, lib.lhip_last_error())
    return left, (right if channels == 2 else None), rej.value


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- exact conversion ------------------------------------------------------------------------------------------------------------------
_exact_runs = 0


def _exact(lib, typ, v):
    global _exact_runs
    _exact_runs += 1
    got, _, rej = debug_ingest(lib, typ, v)
    want, bad = expected_f32(typ, v)
    assert same_bits(got, want), (NAMES[typ], [(x, a, b) for x, a, b in zip(np.asarray(v).tolist(), got.tolist(), want.tolist()) if np.float32(a).tobytes() != np.float32(b).tobytes()][:5])
    assert rej == int(bad.sum())
    return got, rej


def exact_conversion_check(lib):
    """lhip_debug_ingest against numpy, bit pattern for bit pattern; returns the number of arrays checked."""
    global _exact_runs
    _exact_runs = 0
    rng = np.random.RandomState(32)
    # S32: the ends of the range, exact ties at 25 and more significant bits (to even: down and up), random values
    ties = [0x40000040, 0x400000C0, -0x40000040, -0x400000C0, 0x01000001, 0x01000003, 0x7fffff40, 0x7fffffc0, 0x20000020, 0x20000060]
    s32 = np.array([(1 << 31) - 1, -((1 << 31) - 1), -(1 << 31), 0, 1, -1] + ties + rng.randint(-(1 << 31), 1 << 31, 4096, dtype=np.int64).tolist(), dtype=np.int64)
    got, _ = _exact(lib, S32, s32)
    assert got[6] == np.float32(0x40000000 / 65536.0) and got[7] == np.float32(0x40000100 / 65536.0)          # ties to even
    _exact(lib, S24, np.array([-(1 << 23), (1 << 23) - 1, 0, 1, -1] + rng.randint(-(1 << 23), 1 << 23, 4096).tolist()))
    _exact(lib, U8, np.arange(256))
    # F64N / F64: ties of the one rounding, results that are Float32 denormals, +-0, a value that rounds onto the limit
    tie_f64 = [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24), 1.0 + 2.0 ** -24 + 2.0 ** -50, 0.1, 1 / 3.0]
    den = [2.0 ** -140, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, -(2.0 ** -127), 1e-42, 2.0 ** -126 - 2.0 ** -160]
    for typ, scale in ((F64N, 32768.0), (F64, 1.0)):
        v = np.array(tie_f64 + [d / scale for d in den] + [0.0, -0.0, np.nextafter(131072.0, 0) / scale, -np.nextafter(131072.0, 0) / scale, 131072.0 / scale, -131072.0 / scale] +
                     (rng.uniform(-4, 4, 512) * (1 if typ == F64N else 32768)).tolist())
        got, rej = _exact(lib, typ, v)
        assert rej == 0
        k = len(tie_f64) + len(den)
        assert got[k].tobytes() == np.float32(0.0).tobytes() and got[k + 1].tobytes() == np.float32(-0.0).tobytes()
        assert got[k + 2] == np.float32(131072.0) and got[k + 3] == np.float32(-131072.0)          # rounds onto the limit: accepted
        assert 0 < abs(float(got[len(tie_f64)])) < 2.0 ** -126                                   # a Float32 denormal came out
    # F32N: 4.0 gives 131072 and is accepted
    got, rej = _exact(lib, F32N, np.array([4.0, -4.0, 1.0, -1.0, 0.5, 2.0 ** -140, 0.0, -0.0], dtype=np.float32))
    assert got[0] == np.float32(131072.0) and rej == 0
    # bad values: counted and read as zero
    for typ in (F64N, F64):
        s = 1.0 if typ == F64N else 32768.0
        v = np.array([0.25 * s, float("nan"), float("inf"), -float("inf"), 1e300, 4.0000001 * s, -4.0000001 * s, 0.5 * s])
        got, rej = _exact(lib, typ, v)
        assert rej == 6 and not got[1:7].any() and got[0] != 0 and got[7] != 0
    got, rej = _exact(lib, F32N, np.array([np.nan, np.inf, -np.inf, 4.0000005, 3e38, 1.0], dtype=np.float32))
    assert rej == 5 and not got[:5].any()
    return _exact_runs


# ---- the golden cases in the WAV types ------------------------------------------------------------------------------------------------
def q_of(a, right=False):
    a = np.asarray(a).astype(np.int64)
    i = np.arange(len(a), dtype=np.int64)
    return a * 16 + (((i * 5 + 1) & 15) if right else ((i * 7 + 3) & 15))


def case_elements(case, typ):
    """The elements of a golden case in sample type `typ` (planes L, R or None) and the case they must give the bytes of.  `frac` cases:
    S24 q * 16, S32 q * 4096, F32N / F64N q / 524288, F64 q / 16; `hot` cases: F32N / F64N hot / 32768, F64 hot.  Asserts that nothing is rounded:
    the header's conversion of the elements IS the golden's Float32 PCM."""
    L, R, A, B = pc.case_pcm(case)
    planes = []
    for f32, a, right in ((L, A, False), (R, B, True)):
        if f32 is None:
            planes.append(None)
            continue
        if case["kind"] == "frac" and typ in (S24, S32):
            v = q_of(a, right) * (16 if typ == S24 else 4096)
        elif typ == F32N:
            v = (f32.astype(np.float64) / 32768.0).astype(np.float32)
        elif typ == F64N:
            v = f32.astype(np.float64) / 32768.0
        elif typ == F64:
            v = f32.astype(np.float64)
        else:
            raise AssertionError((case["kind"], typ))
        want, bad = expected_f32(typ, v)
        assert same_bits(want, f32) and not bad.any(), (case["name"], typ)          # nothing was rounded, nothing refused
        planes.append(v)
    return planes[0], planes[1]


def interleave(l, r):
    return l if r is None else pc.interleave(np.asarray(l), np.asarray(r))


def encode_raw(lib, enc, typ, l, r, inter, strict=True, odd=True, entry="host"):
    """One call over the elements l / r (planes); U8 and S24 start at an odd address.  entry "host": lhip_encode_pcm; "device":
    lhip_encode_batch_device_pcm with one stream -- over torch.uint8 tensors on the GPU, over the host arrays in a simulation (its device pointers
    are host pointers) -- which always launches g_ingest (a host call this small is converted by the host)."""
    n = len(l)
    if n == 0:
        return b""
    r = None if enc.channels == 1 else r
    shift = 1 if (odd and typ in (U8, S24)) else 0
    sim = b"HOST SIMULATION" in lib.lhip_version()

    def place(b):
        buf = np.empty(len(b) + shift, np.uint8)
        buf[shift:] = np.frombuffer(b, np.uint8)
        if entry == "device" and not sim:
            import torch
            t = torch.from_numpy(buf).cuda()
            return t, t.data_ptr() + shift
        return buf, buf.ctypes.data + shift
    if inter or r is None:
        a, pl = place(pack(typ, interleave(l, r)))
        pr, keep = None, (a,)
    else:
        (a, pl), (b, pr) = place(pack(typ, l)), place(pack(typ, r))
        keep = (a, b)
    fmt = typ | (INTER if inter else 0)
    if entry == "device":
        cap = int(lib.lhip_max_output_bytes(enc._h, n))
        if sim:
            out = np.empty(cap, np.uint8)
            optr = out.ctypes.data
        else:
            import torch
            out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            optr = out.data_ptr()
        H, lp, rp, op = (ctypes.c_void_p * 1)(enc._h), (ctypes.c_void_p * 1)(pl), (ctypes.c_void_p * 1)(pr), (ctypes.c_void_p * 1)(optr)
        ns, cp, wr = (ctypes.c_size_t * 1)(n), (ctypes.c_size_t * 1)(cap), (ctypes.c_int64 * 1)()
        rc = lib.lhip_encode_batch_device_pcm(H, 1, fmt, lp, rp, ns, op, cp, wr, 1)
        assert rc == 0 and wr[0] >= 0, (rc, lib.lhip_last_error())
        assert "INGEST" in enc.last_batch_paths() and int(lib.lhip_last_batch_rejected_samples()) == 0
        del keep
        return out[: wr[0]].tobytes() if sim else out[: wr[0]].cpu().numpy().tobytes()
    cap = lib.lhip_encode_output_bytes(enc._h, n)
    assert cap >= 0, lib.lhip_last_error()
    out = np.empty(cap + 8, np.uint8)
    w = lib.lhip_encode_pcm(enc._h, fmt, pl, pr, n, out.ctypes.data, cap)
    del keep
    if w < 0:
        if strict:
            raise AssertionError((w, lib.lhip_last_error()))
        return w
    assert (w == cap) if lib.lhip_output_bytes_is_exact(enc._h) == 1 else (w <= cap)
    return out[:w].tobytes()


def run_golden_case(lib, case, typ, inter=True, entry="host"):
    """Every call and the flush of a golden case in sample type `typ`, with the exemptions pcmformats_cases.run_golden_case makes."""
    L, R = case_elements(case, typ)
    enc = pc.make_encoder(lib, case)
    try:
        parts = feed_calls(case["call_lens"], L, R, lambda i, l, r: encode_raw(lib, enc, typ, l, r, inter, entry=entry))
        resv = bool(case["reservoir"])
        check_stream(case, parts, enc.flush(), call_bytes=not resv, enc_md5=not resv, flush_md5=not resv and not case["frac"], all_md5=resv)
    finally:
        enc.close()


FRAC_TYPES, HOT_TYPES = (S24, S32, F32N, F64N, F64), (F32N, F64N, F64)


def run_goldens(lib, G, kind, typ, entries=("host", "device"), planar_first=5):
    """All cases of `kind` interleaved, the first `planar_first` of them planar as well, through each of `entries`; returns (cases, runs)."""
    cases = [c for c in G if c["kind"] == kind]
    runs = 0
    for entry in entries:
        for i, case in enumerate(cases):
            run_golden_case(lib, case, typ, True, entry)
            runs += 1
            if i < planar_first:
                run_golden_case(lib, case, typ, False, entry)
                runs += 1
    return len(cases), runs


def u8_family_check(lib, seed, configs=None, max_frames=4, entries=("host", "device")):
    """Random bytes in every configuration of pcmformats_cases.FAMILY_CONFIGS == oracle_encode of (b - 128) * 256 as Int16."""
    from oracle_py import oracle_encode
    rng = np.random.RandomState(seed)
    ran = 0
    for ci, cfg in enumerate(configs or pc.FAMILY_CONFIGS):
        ch, sr, kb, joint, resv = cfg
        n = int(rng.randint(1152, max_frames * 1152))
        b = [rng.randint(0, 256, n).astype(np.int64) for _ in range(ch)]
        pcm16 = [((x - 128) * 256).astype(np.int16) for x in b]
        want = oracle_encode(ch, sr, kb, pcm16[0], pcm16[1] if ch == 2 else None, joint=bool(joint), reservoir=bool(resv))
        lens, p = [], 0
        while p < n:
            m = min(n - p, [n, 1152, int(rng.choice([1, 333, 1151, 1153]))][ci % 3])
            lens.append(m)
            p += m
        enc = pc.make_encoder(lib, {"channels": ch, "samplerate": sr, "kbps": kb, "joint": joint, "reservoir": resv})
        parts = feed_calls(lens, b[0], b[1] if ch == 2 else None, lambda i, l, r: encode_raw(lib, enc, U8, l, r, inter=bool((ci + i) & 1), entry=entries[(ci // 2 + i) % len(entries)]))
        got = b"".join(parts) + enc.flush()
        enc.close()
        assert got == want, (cfg, n, lens[:4])
        ran += 1
    return ran


# ---- shapes where the kernel can go wrong -------------------------------------------------------------------------------------------------
SHAPE_N = (1, 2, 5, 15, 16, 17, 21, 1151, 1153)


def shapes_check(lib):
    """S24 at every misalignment 0 .. 15 and the lengths of SHAPE_N, mono, interleaved stereo and planar stereo; U8 at odd addresses -- the
    planes bit for bit numpy's, no float outside them touched (the hook's planes are exactly n floats)."""
    rng = np.random.RandomState(24)
    ran = 0
    for n in SHAPE_N:
        for mis in range(16):
            for ch, layout in ((1, "mono"), (2, "interleaved"), (2, "planar")):
                v = rng.randint(-(1 << 23), 1 << 23, n * ch)
                l, r, rej = debug_ingest(lib, S24, v, ch, layout, mis)
                want, _ = expected_f32(S24, v)
                wl, wr = (want, None) if ch == 1 else (want[0::2], want[1::2]) if layout == "interleaved" else (want[:n], want[n:])
                assert same_bits(l, np.ascontiguousarray(wl)) and (ch == 1 or same_bits(r, np.ascontiguousarray(wr))) and rej == 0, (n, mis, layout)
                ran += 1
    for n in (1, 17, 1009, 2 * 8064 + 5):
        for mis in (1, 3, 15):
            for ch, layout in ((1, "mono"), (2, "interleaved"), (2, "planar")):
                v = rng.randint(0, 256, n * ch)
                l, r, rej = debug_ingest(lib, U8, v, ch, layout, mis)
                want, _ = expected_f32(U8, v)
                wl, wr = (want, None) if ch == 1 else (want[0::2], want[1::2]) if layout == "interleaved" else (want[:n], want[n:])
                assert same_bits(l, np.ascontiguousarray(wl)) and (ch == 1 or same_bits(r, np.ascontiguousarray(wr))) and rej == 0, (n, mis, layout)
                ran += 1
    return ran


SIX = (0, 1, 1152, 1153, 2305, 777)


def six_streams_batch(lib, device=False, downmix=False):
    """One batch over six streams of SIX samples, S24, each stream's bytes starting where the one before it ended (one buffer) == the
    oracle on the Int16 values.  `device`: torch uint8 tensor and the device-pointer entry (GPU), else the host batch entry (a simulation's
    device entry takes host pointers: both are run there).  `downmix`: two channels in, a mono stream out."""
    from oracle_py import oracle_encode
    rng = np.random.RandomState(6)
    ch = 2
    cfg = (2, 44100, 128)
    kw = {"downmix": True} if downmix else {}
    el = [[rng.randint(-32768, 32768, n).astype(np.int64) for _ in range(ch)] for n in SIX]
    if downmix:
        want = None
    else:
        want = [oracle_encode(*cfg, e[0].astype(np.int16), e[1].astype(np.int16)) for e in el]
    blobs = [pack(S24, interleave(e[0] * 256, e[1] * 256)) for e in el]
    offs = np.cumsum([0] + [len(b) for b in blobs])
    buf = np.frombuffer(b"".join(blobs), np.uint8).copy()
    results = []
    entries = ("device",) if device else ("host", "simdevice")
    for entry in entries:
        encs = [pc.make_encoder(lib, cfg, **kw) for _ in SIX]
        n = len(SIX)
        caps = [int(lib.lhip_max_output_bytes(e._h, c)) for e, c in zip(encs, SIX)]
        H = (ctypes.c_void_p * n)(*[e._h for e in encs])
        ns, cp, wr = (ctypes.c_size_t * n)(*SIX), (ctypes.c_size_t * n)(*caps), (ctypes.c_int64 * n)()
        if entry == "device":
            import torch
            t = torch.from_numpy(buf).cuda()
            outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
            torch.cuda.synchronize()
            lp = (ctypes.c_void_p * n)(*[t.data_ptr() + int(o) for o in offs[:-1]])
            op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
            rc = lib.lhip_encode_batch_device_pcm(H, n, S24 | INTER, lp, lp, ns, op, cp, wr, 1)
            assert rc == 0, (rc, lib.lhip_last_error())
            assert "INGEST" in encs[0].last_batch_paths()
            got = [outs[i][: wr[i]].cpu().numpy().tobytes() for i in range(n)]
        else:
            outs = [np.empty(c, np.uint8) for c in caps]
            lp = (ctypes.c_void_p * n)(*[buf.ctypes.data + int(o) for o in offs[:-1]])
            op = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
            if entry == "host":
                rc = lib.lhip_encode_batch_pcm(H, n, S24 | INTER, lp, lp, ns, op, cp, wr)
            else:
                rc = lib.lhip_encode_batch_device_pcm(H, n, S24 | INTER, lp, lp, ns, op, cp, wr, 1)
                assert "INGEST" in encs[0].last_batch_paths()
            assert rc == 0, (rc, lib.lhip_last_error())
            got = [outs[i][: wr[i]].tobytes() for i in range(n)]
        got = [g + e.flush() for g, e in zip(got, encs)]
        for e in encs:
            e.close()
        results.append(got)
    if downmix:          # the yardstick: the same stream fed as Int16 planes (the downmix itself is tests/test_inputmix_*.py's subject)
        want = []
        for e in el:
            enc = pc.make_encoder(lib, cfg, **kw)
            want.append((enc.encodeBuffer(e[0].astype(np.int16), e[1].astype(np.int16)) if len(e[0]) else b"") + enc.flush())
            enc.close()
    for got in results:
        assert got == want, [len(g) for g in got]
    return len(results)


# ---- the launch paths (GPU, in a process of its own: torch initialises the GPU first) ------------------------------------------------------
def device_paths_check(lib):
    """The device-pointer entry over torch.uint8 tensors: many frames per stream, one frame per stream (g_frame), reservoir streams; S24
    interleaved and S32 planar; `INGEST` in every batch's paths; == the oracle."""
    import torch
    from oracle_py import oracle_encode
    batches = 0
    for cfg, resv, lens in (((2, 44100, 128), False, [1152 * 20 + 7, 777, 1152 * 9 + 1]), ((2, 44100, 128), False, [1152] * 4), ((2, 44100, 128), True, [1152 * 3, 1152 * 2 + 3])):
        for typ, inter in ((S24, True), (S32, False)):
            rounds = 2
            pcms = [pcm.bursts(n * rounds, 2, seed=500 + i) if i % 2 else pcm.sine(n * rounds, 2, seed=500 + i) for i, n in enumerate(lens)]
            want = [oracle_encode(*cfg, l, r, reservoir=resv) for l, r in pcms]
            encs = [pc.make_encoder(lib, {"channels": 2, "samplerate": cfg[1], "kbps": cfg[2], "reservoir": resv}) for _ in lens]
            got = [b""] * len(lens)
            mul = 256 if typ == S24 else 65536
            n = len(lens)
            for k in range(rounds):
                tens = []
                for (l, r), m in zip(pcms, lens):
                    l, r = l[m * k:m * (k + 1)].astype(np.int64) * mul, r[m * k:m * (k + 1)].astype(np.int64) * mul
                    if inter:
                        tens.append((torch.from_numpy(np.frombuffer(pack(typ, interleave(l, r)), np.uint8).copy()).cuda(), None))
                    else:
                        tens.append((torch.from_numpy(np.frombuffer(pack(typ, l), np.uint8).copy()).cuda(), torch.from_numpy(np.frombuffer(pack(typ, r), np.uint8).copy()).cuda()))
                caps = [int(lib.lhip_max_output_bytes(e._h, c)) for e, c in zip(encs, lens)]
                outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
                torch.cuda.synchronize()
                H = (ctypes.c_void_p * n)(*[e._h for e in encs])
                lp = (ctypes.c_void_p * n)(*[a.data_ptr() for a, _ in tens])
                rp = (ctypes.c_void_p * n)(*[(b if b is not None else a).data_ptr() for a, b in tens])
                op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
                ns, cp, wr = (ctypes.c_size_t * n)(*lens), (ctypes.c_size_t * n)(*caps), (ctypes.c_int64 * n)()
                rc = lib.lhip_encode_batch_device_pcm(H, n, typ | (INTER if inter else 0), lp, rp, ns, op, cp, wr, 0)
                assert rc == 0, (rc, lib.lhip_last_error())
                assert int(lib.lhip_last_batch_rejected_samples()) == 0          # waits for the batch
                paths = encs[0].last_batch_paths()
                assert "INGEST" in paths and (("FRAME" in paths or "FRAME_RESV" in paths) == (max(lens) == 1152)), paths
                torch.cuda.synchronize()
                got = [g + outs[i][: wr[i]].cpu().numpy().tobytes() for i, g in enumerate(got)]
                batches += 1
            assert [g + e.flush() for g, e in zip(got, encs)] == want, (cfg, resv, typ)
            for e in encs:
                e.close()
    # refused float samples by device pointer: read as zero and counted (F64N interleaved)
    enc, clean = pc.make_encoder(lib, (2, 44100, 128)), pc.make_encoder(lib, (2, 44100, 128))
    rng = np.random.RandomState(3)
    v = rng.uniform(-1, 1, 2 * 1152 * 3)
    z = v.copy()
    for i, b in zip((5, 1000, 4001), (float("nan"), float("inf"), 1e300)):
        v[i], z[i] = b, 0.0
    res = []
    for e, x in ((enc, v), (clean, z)):
        t = torch.from_numpy(np.frombuffer(pack(F64N, x), np.uint8).copy()).cuda()
        cap = int(lib.lhip_max_output_bytes(e._h, 1152 * 3))
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        H, lp, op = (ctypes.c_void_p * 1)(e._h), (ctypes.c_void_p * 1)(t.data_ptr()), (ctypes.c_void_p * 1)(out.data_ptr())
        ns, cp, wr = (ctypes.c_size_t * 1)(1152 * 3), (ctypes.c_size_t * 1)(cap), (ctypes.c_int64 * 1)()
        assert lib.lhip_encode_batch_device_pcm(H, 1, F64N | INTER, lp, lp, ns, op, cp, wr, 0) == 0, lib.lhip_last_error()
        rej = int(lib.lhip_last_batch_rejected_samples())
        torch.cuda.synchronize()
        res.append((out[: wr[0]].cpu().numpy().tobytes() + e.flush(), rej))
        # a misaligned device pointer of a 4- or 8-byte type: refused, nothing consumed (S24 at the same address is taken: tests of the shapes)
        ns2 = (ctypes.c_size_t * 1)(100)
        for typ2, off, word in ((F64N | INTER, 4, b"multiple of 8"), (F64, 4, b"multiple of 8"), (S32, 2, b"multiple of 4"), (S32 | INTER, 1, b"multiple of 4"), (F32N, 2, b"multiple of 4")):
            lp2, ok2 = (ctypes.c_void_p * 1)(t.data_ptr() + off), (ctypes.c_void_p * 1)(t.data_ptr())
            for a2, b2 in ((lp2, lp2), (ok2, lp2)) if not typ2 & INTER else ((lp2, lp2),):
                assert lib.lhip_encode_batch_device_pcm(H, 1, typ2, a2, b2, ns2, op, cp, wr, 1) == -4 and wr[0] == -4 and word in lib.lhip_last_error(), (typ2, off)
        e.close()
    assert res[0][0] == res[1][0] and res[0][1] == 3 and res[1][1] == 0, (res[0][1], res[1][1])
    return batches


class _Stderr:
    """What the C library writes to stderr inside the block (file descriptor 2), as text."""
    def __enter__(self):
        import os
        import tempfile
        self.tmp = tempfile.TemporaryFile()
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        import os
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def host_paths_check(lib, expect_ingest, expect_units=0):
    """Host calls of a 20-frame stream in S24 / F32N / U8 and as Int16, the type changing from call to call; whether `INGEST` shows is the
    caller's to say (the environment decides: small calls, or the general / chunked path)."""
    from oracle_py import oracle_encode
    L, R = pcm.bursts(1152 * 60 + 11, 2, seed=77)
    L, R = (L.astype(np.int64) // 256) * 256, (R.astype(np.int64) // 256) * 256          # multiples of 256: every type below holds them exactly
    want = oracle_encode(2, 44100, 128, L.astype(np.int16), R.astype(np.int16))
    enc = pc.make_encoder(lib, (2, 44100, 128))
    cuts = [0, 1152 * 20, 1152 * 21, 1152 * 40 + 3, 1152 * 41, len(L)]
    kinds = [S24, U8, F32N, "s16", S32]
    got, seen = b"", []
    for (a, b), typ in zip(zip(cuts, cuts[1:]), kinds):
        l, r = L[a:b], R[a:b]
        if typ == "s16":
            got += enc.encodeBuffer(l.astype(np.int16), r.astype(np.int16))
        else:
            el = {S24: (l * 256, r * 256), S32: (l * 65536, r * 65536), U8: (l // 256 + 128, r // 256 + 128), F32N: (l / 32768.0, r / 32768.0)}[typ]
            with _Stderr() as err:
                got += encode_raw(lib, enc, typ, el[0], el[1], inter=typ != S32)
            if typ == S24 and expect_units:          # the 20-frame call really went through encode_host_pipelined, cut into units (LAMEJS_HIP_TRACE_CHUNKS=1 names each)
                assert err.text.count("[lhip unit ") == expect_units, err.text
        seen.append("INGEST" in enc.last_batch_paths())
    got += enc.flush()
    enc.close()
    assert got == want
    assert seen == [e for e in expect_ingest], seen
    return len(seen)


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    import lamejs_amd
    if sys.argv[1:] == ["--host-paths"]:
        import os
        exp = json.loads(os.environ["WAVPCM_EXPECT_INGEST"])
        print(json.dumps({"calls": host_paths_check(lamejs_amd.load_library(), exp, int(os.environ.get("WAVPCM_EXPECT_UNITS", "0")))}))
        sys.exit(0)
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")
    lib = lamejs_amd.load_library()
    if sys.argv[1:] == ["--device-paths"]:
        print(json.dumps({"batches": device_paths_check(lib)}))
    elif sys.argv[1:2] == ["--goldens-device"]:          # the goldens of one kind in one type through the device entry (torch.uint8 tensors)
        kind, typ = sys.argv[2], {v: k for k, v in NAMES.items()}[sys.argv[3]]
        print(json.dumps({"runs": run_goldens(lib, pc.golden_floatpcm(), kind, typ, entries=("device",))[1]}))
    elif sys.argv[1:] == ["--u8-device"]:
        print(json.dumps({"configs": u8_family_check(lib, 803, entries=("device",))}))
    elif sys.argv[1:] == ["--six-streams"]:
        print(json.dumps({"runs": six_streams_batch(lib, device=True) + six_streams_batch(lib, device=True, downmix=True)}))
    else:
        sys.exit(2)
