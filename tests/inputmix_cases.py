"""TEST INFRASTRUCTURE shared by tests/test_inputmix_cpu.py and tests/test_inputmix_gpu.py: the input gains (scale, scale_left, scale_right)
and the stereo-to-mono downmix.  The goldens (tests/golden/golden_inputmix.json, tests/tools/gen_golden_inputmix.js) are the unmodified
reference's bytes; the random family is checked against the unchanged oracle on a blob built with ``scale: 1`` and fed the premix computed
here in numpy with the reference's roundings (``premix``).  The oracle takes Int16 only, so the family draws its samples such that every
value behind gains and mix is a whole number inside the Int16 range (``family_pcm``): the roundings themselves -- the preset's 0.95 on the
left samples only, fractional Float32 input -- are pinned by the goldens."""
import hashlib
import json

import numpy as np

import pcm
from conftest import ROOT
from golden_cases import check_stream, feed_calls, load, pinned
from pcmformats_cases import F32, INTER, S16, encode_fmt, float_pcm

FORMATS = (S16, S16 | INTER, F32, F32 | INTER)


def goldens():
    return load("golden_inputmix")["cases"]


def case_opts(c):
    return {"downmix": bool(c.get("downmix")), "scale": c.get("scale"), "scale_left": c.get("scaleLeft"), "scale_right": c.get("scaleRight")}


def case_pcm(c):
    A, B = pcm.CORPORA[c["corpus"]](c["nsamples"], c["channels"])
    if c["kind"] == "f32":
        L, R = float_pcm("frac", c["corpus"], A), (float_pcm("frac", c["corpus"], B, True) if c["channels"] == 2 else None)
    elif c["kind"] == "q20":      # shaped so that the premix is whole numbers (tests/tools/gen_golden_inputmix.js: shape)
        a, b = np.asarray(A).astype(np.int64), np.asarray(B).astype(np.int64)
        k = a // 20
        r = b - ((k + b) & 1)
        r[r < -32768] += 2
        L, R = (20 * k).astype(np.int16), r.astype(np.int16)
    elif c["kind"] == "even4":
        a, b = np.asarray(A).astype(np.int64), np.asarray(B).astype(np.int64)
        L, R = ((a >> 2) & ~1).astype(np.int16), ((b >> 2) & ~3).astype(np.int16)
    else:
        L, R = np.asarray(A, dtype=np.int16), (np.asarray(B, dtype=np.int16) if c["channels"] == 2 else None)
    return pinned((L, R), c["pcm_md5"])


def make_encoder(lib, c, **kw):
    import lamejs_amd
    return lamejs_amd.Mp3Encoder(c["channels"], c["samplerate"], c["kbps"], lib=lib, fractional_resample=bool(c.get("frac")), **case_opts(c), **kw)


def run_golden_case(lib, c, fmt_of_call=None):
    """Every call and the flush of a golden case through lhip_encode_pcm; fmt_of_call(i): the call's layout bit (the sample type is the case's)."""
    L, R = case_pcm(c)
    enc = make_encoder(lib, c)
    try:
        kind = F32 if c["kind"] == "f32" else S16
        parts = feed_calls(c["call_lens"], L, R, lambda i, l, r: encode_fmt(lib, enc, kind | (fmt_of_call(i) if fmt_of_call else 0), l, r))
        # (a non-integer-ratio stream's flush frames are silent stand-ins of equal length by design: include/lamejs_hip.h)
        check_stream(c, parts, enc.flush(), flush_md5=not c["name"].endswith("_frac"))
    finally:
        enc.close()


# ---- the reference's arithmetic in numpy (Lame.js:1551-1584): every `*=` is an f64 product stored to Float32 ----
def neq(a, b):
    """BitStream.NEQ (BitStream.js:22-30)."""
    a, b = float(a), float(b)
    eq = abs(a - b) <= abs(a) * 1e-6 if abs(a) > abs(b) else abs(a - b) <= abs(b) * 1e-6
    return not eq


def in_force(g):
    return neq(g, 0) and neq(g, 1)


def mul32(x, g):
    return (x.astype(np.float64) * np.float64(g)).astype(np.float32)


def premix(l, r, channels_out, scale, scale_left=0.0, scale_right=0.0):
    """(left, right) as the encoder core sees them; `scale` is the value in force after the preset (the user's, or the preset's)."""
    a = np.asarray(l).astype(np.float32)
    b = None if r is None else np.asarray(r).astype(np.float32)
    if in_force(scale):
        a = mul32(a, scale)
        if b is not None and channels_out == 2:
            b = mul32(b, scale)
    if in_force(scale_left):
        a = mul32(a, scale_left)
    if b is not None and in_force(scale_right):
        b = mul32(b, scale_right)
    if b is not None and channels_out == 1:
        return (0.5 * (a.astype(np.float64) + b.astype(np.float64))).astype(np.float32), None      # one rounding
    return a, b


def preset_scale(kbps, samplerate=44100):
    import subprocess
    js = "const t = require(process.argv[1]); console.log(t.resolveParams(1, +process.argv[2], +process.argv[3], { fractionalResample: true }).scale);"
    return float(subprocess.run(["node", "-e", js, str(ROOT / "lamejs_amd" / "js" / "tables.js"), str(samplerate), str(kbps)], capture_output=True, text=True, check=True).stdout)


def oracle_bytes(channels_out, samplerate, kbps, lens, L, R, frac=False):
    """The unchanged oracle on a blob built with scale: 1, fed whole-number Float32 planes as Int16, call by call, then its flush (not for
    non-integer ratios: it aborts there by design)."""
    import lamejs_amd
    from oracle_py import oracle_calls
    blob = lamejs_amd.tables_blob(channels_out, samplerate, kbps, fractional_resample=frac, scale=1.0)
    l16 = np.ascontiguousarray(L, dtype=np.int16)
    r16 = None if R is None else np.ascontiguousarray(R, dtype=np.int16)
    assert np.array_equal(l16.astype(np.float32), L) and (R is None or np.array_equal(r16.astype(np.float32), R)), "premix is not whole Int16 numbers"
    return oracle_calls(blob, l16, r16, lens, flush=not frac)


# ---- the seeded random family ----
# (channels in, samplerate, kbps, frac, recipe).  Recipes choose gains AND the shape of the samples so that the premix is whole numbers:
#   down       downmix, no gain in force (scale 1 by the preset above 128 kbps, or the user's 1): l + r even
#   quirk      downmix under the preset's 0.95: l = 20 k, so that fround(l * 0.95) = 19 k exactly; r of k's parity (r never sees the 0.95)
#   lr         two channels out, scaleLeft 0.5 / scaleRight 0.25, user scale 1: l even, r a multiple of 4
#   flip       downmix, scaleLeft -1 / scaleRight 2, user scale 1: l even, |l|, |r| <= 10000
#   scale2     user scale 2 (|x| <= 16000); scale_half: user scale 0.5 on even samples
FAMILY_CONFIGS = [
    (2, 44100, 320, 0, "down"), (2, 44100, 128, 0, "quirk"), (2, 44100, 128, 0, "lr"), (2, 44100, 128, 0, "flip"), (1, 44100, 128, 0, "scale2"),
    (2, 44100, 192, 0, "scale_half"), (2, 16000, 32, 0, "quirk"), (2, 44100, 32, 0, "quirk"), (2, 48000, 64, 0, "down1"), (2, 44100, 48, 1, "quirk"),
    (2, 8000, 8, 0, "flip"), (2, 44100, 32, 0, "flip"), (2, 22050, 64, 0, "lr"),
]


def family(seed, count, max_frames=5):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        cfg = FAMILY_CONFIGS[i % len(FAMILY_CONFIGS)]
        n = int(rng.randint(600, max_frames * 1152))
        lens, p = [], 0
        while p < n:
            m = 576 if cfg[3] else int(rng.choice([1, 7, 333, 777, 1151, 1152, 1153, 2305, int(rng.randint(1, 4001))]))
            m = min(m, n - p)
            lens.append(m)
            p += m
        out.append({"cfg": cfg, "corpus": ["sine", "bursts"][int(rng.randint(0, 2))], "seed": int(rng.randint(1, 1 << 30)), "n": n, "lens": lens,
                    "fmts": [FORMATS[int(rng.randint(0, 4))] for _ in lens]})
    return out


def family_pcm(fc):
    """(L, R as int64 whole numbers, encoder options, premix arguments)."""
    ch, sr, kb, frac, recipe = fc["cfg"]
    A, B = pcm.CORPORA[fc["corpus"]](fc["n"], 2, fc["seed"])
    l, r = np.asarray(A).astype(np.int64), np.asarray(B).astype(np.int64)
    if recipe in ("down", "down1"):
        r = r - ((l + r) & 1)
        r[r < -32768] += 2
        opts = {"downmix": True, "scale": 1.0 if recipe == "down1" else None}
        mix = (1, 1.0 if recipe == "down1" else None, 0.0, 0.0)
    elif recipe == "quirk":
        k = l // 20
        l = 20 * k
        r = r - ((k + r) & 1)
        r[r < -32768] += 2
        opts, mix = {"downmix": True}, (1, None, 0.0, 0.0)
    elif recipe == "lr":
        l, r = l & ~1, r & ~3
        opts, mix = {"scale": 1.0, "scale_left": 0.5, "scale_right": 0.25}, (2, 1.0, 0.5, 0.25)
    elif recipe == "flip":
        l, r = (l // 4) & ~1, r // 4
        opts, mix = {"downmix": True, "scale": 1.0, "scale_left": -1.0, "scale_right": 2.0}, (1, 1.0, -1.0, 2.0)
    elif recipe == "scale2":
        l, r = l // 3, None
        opts, mix = {"scale": 2.0}, (1, 2.0, 0.0, 0.0)
    elif recipe == "scale_half":
        l, r = l & ~1, r & ~1
        opts, mix = {"scale": 0.5}, (2, 0.5, 0.0, 0.0)
    else:
        raise AssertionError(recipe)
    return l, r, opts, mix


def family_want(fc):
    ch, sr, kb, frac, recipe = fc["cfg"]
    l, r, opts, (cout, scale, sl, sr_) = family_pcm(fc)
    scale = preset_scale(kb, sr) if scale is None else scale
    if recipe == "quirk":
        assert scale == 0.95
    pl, pr = premix(l, r, cout, scale, sl, sr_)
    return oracle_bytes(cout, sr, kb, fc["lens"], pl, pr, frac=bool(frac))


def family_encode(lib, fc):
    ch, sr, kb, frac, recipe = fc["cfg"]
    import lamejs_amd
    l, r, opts, _ = family_pcm(fc)
    enc = lamejs_amd.Mp3Encoder(ch, sr, kb, lib=lib, fractional_resample=bool(frac), **opts)
    try:
        p, parts = 0, []
        for n, fmt in zip(fc["lens"], fc["fmts"]):
            parts.append(encode_fmt(lib, enc, fmt, l[p:p + n], None if r is None else r[p:p + n]))
            p += n
        return parts, enc.flush()
    finally:
        enc.close()


def family_check(lib, cases):
    for fc in cases:
        want_parts, want_flush = family_want(fc)
        parts, flush = family_encode(lib, fc)
        assert parts == want_parts, (fc["cfg"], fc["lens"], fc["fmts"])
        if not fc["cfg"][3]:
            assert flush == want_flush, (fc["cfg"], fc["lens"])
    return len(cases)


def golden_premix_check(c):
    """The oracle on a scale-1 blob fed the premix equals the golden -- for the golden cases whose premix is whole numbers (what makes the
    family's reference a reference).  Returns False where the premix has fractions (the Int16 oracle cannot take it)."""
    L, R = case_pcm(c)
    cout = c["ref_channels_out"]
    pl, pr = premix(L, R, cout, c["ref_scale"], c.get("scaleLeft", 0.0), c.get("scaleRight", 0.0))
    whole = np.array_equal(pl, np.rint(pl)) and np.abs(pl).max() <= 32767 and (pr is None or (np.array_equal(pr, np.rint(pr)) and np.abs(pr).max() <= 32767))
    if not whole:
        return False
    parts, fl = oracle_bytes(cout, c["samplerate"], c["kbps"], c["call_lens"], pl, pr, frac=c["name"].endswith("_frac"))
    assert [len(p) for p in parts] == c["call_bytes"] and hashlib.md5(b"".join(parts)).hexdigest() == c["enc_md5"], c["name"]
    if not c["name"].endswith("_frac"):
        assert hashlib.md5(fl).hexdigest() == c["flush_md5"], c["name"]
    return True


def device_downmix_check(lib, call):
    """The device-pointer entry in all four formats on a downmix stream: two out-of-contract Float32 samples in the RIGHT channel are read as zero
    before gain and mix and counted (source positions); Int16 formats count nothing.  `call`: pcmformats_cases.sim_device_call / gpu_device_call."""
    c = next(x for x in goldens() if x["name"] == "downmix_f32")
    L, R = case_pcm(c)
    n = 3 * 1152
    for fmt in FORMATS:
        dirty, clean = make_encoder(lib, c), make_encoder(lib, c)
        l, r = (L[:n], R[:n].copy()) if fmt & F32 else (np.rint(L[:n]), np.rint(R[:n]))
        zr, nbad = r.copy(), 0
        if fmt & F32:
            r[[5, 2000]] = [float("inf"), 131073.0]
            zr[[5, 2000]] = 0.0
            nbad = 2
        got, rejected = call(lib, dirty, fmt, l, r)
        want, zero = call(lib, clean, fmt, l, zr)
        assert got == want and len(got) > 0 and (rejected, zero) == (nbad, 0), (fmt, rejected)
        assert dirty.flush() == clean.flush()
        dirty.close()
        clean.close()
    return len(FORMATS)


if __name__ == "__main__":
    # the check that holds torch tensors runs in a process of its own: torch initialises the GPU first, then the library is loaded
    import sys
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")
    sys.path.insert(0, str(ROOT))
    import lamejs_amd
    from pcmformats_cases import gpu_device_call
    if sys.argv[1:] == ["--device-downmix"]:
        print(json.dumps({"device_downmix_formats": device_downmix_check(lamejs_amd.load_library(), gpu_device_call)}))
    else:
        sys.exit(2)
