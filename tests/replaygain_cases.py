"""TEST SUPPORT for the ReplayGain analysis (extension { replayGain }).

1. A restatement in Python of the reference's analysis (GainAnalysis.js, BitStream.js:781-787, VBRTag.js:640-661): serial, IEEE f64 with the Float32 stores,
   ``math.log10``.  tests/test_replaygain_cpu.py holds it to tests/golden/golden_replaygain.json -- recorded from the live reference by
   tests/tools/gen_golden_replaygain.js -- exactly; only then is it the reference where the live module cannot go (44100 / 22050 Hz at full length).
   The filter coefficients are read from the library's own table (lamejs_amd/csrc/k_gain.h): the exact comparison with the live reference pins them.
2. The sample streams of the golden cases as the reference's analysis sees them (behind gains, downmix and resampler), and the checks the three tiers
   share: the exact anchor, cut independence, the comparison with the reference beyond the anchor, the tag.
"""
import ctypes
import functools
import json
import math
import re
import struct

import numpy as np

import pcm
from conftest import ROOT

RATES = (48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000)
BINS = 12000
F32 = np.float32


@functools.lru_cache(maxsize=None)
def rate_table():
    """{fs: (window, wf, yule[21], butter[5])} from k_gain.h"""
    src = (ROOT / "lamejs_amd" / "csrc" / "k_gain.h").read_text()
    rows = re.findall(r"\{(\d+), (\d+), (\d+),\s*\{([^}]*)\},\s*\{([^}]*)\}\}", src)
    t = {int(fs): (int(w), int(wf), [float(v) for v in y.split(",")], [float(v) for v in b.split(",")]) for fs, w, wf, y, b in rows}
    assert tuple(t) == RATES and all(len(v[2]) == 21 and len(v[3]) == 5 and v[0] == -(-fs // 20) and v[1] % 64 == 0 for fs, v in t.items())
    return t


def window_of(fs):
    return rate_table()[fs][0]


def wf_of(fs):
    return rate_table()[fs][1]


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def filter_channel(fs, x, start=0, stop=None):
    """Both filters over x[start:stop] from zero state at `start`, in the reference's operation order with its Float32 stores: (yule, butter) as float lists."""
    _, _, ky, kb = rate_table()[fs]
    stop = len(x) if stop is None else stop
    xs = [0.0] * 10 + [float(v) for v in x[start:stop]]
    ys = [0.0] * (len(xs))
    os_ = [0.0] * (len(xs))
    for n in range(10, len(xs)):
        v = (1e-10 + xs[n] * ky[0] - ys[n - 1] * ky[1] + xs[n - 1] * ky[2] - ys[n - 2] * ky[3] + xs[n - 2] * ky[4] - ys[n - 3] * ky[5] + xs[n - 3] * ky[6]
             - ys[n - 4] * ky[7] + xs[n - 4] * ky[8] - ys[n - 5] * ky[9] + xs[n - 5] * ky[10] - ys[n - 6] * ky[11] + xs[n - 6] * ky[12] - ys[n - 7] * ky[13]
             + xs[n - 7] * ky[14] - ys[n - 8] * ky[15] + xs[n - 8] * ky[16] - ys[n - 9] * ky[17] + xs[n - 9] * ky[18] - ys[n - 10] * ky[19] + xs[n - 10] * ky[20])
        ys[n] = _f32(v)
        o = ys[n] * kb[0] - os_[n - 1] * kb[1] + ys[n - 1] * kb[2] - os_[n - 2] * kb[3] + ys[n - 2] * kb[4]
        os_[n] = _f32(o)
    return ys[10:], os_[10:]


def window_sum(o, a, window):
    """sum of squares of o[a : a + window]: groups of eight from the window's first sample, each as one sum, then the rest one by one"""
    s = 0.0
    k = 0
    while k + 8 <= window:
        q = [o[a + k + j] * o[a + k + j] for j in range(8)]
        s += q[0] + q[1] + q[2] + q[3] + q[4] + q[5] + q[6] + q[7]
        k += 8
    while k < window:
        s += o[a + k] * o[a + k]
        k += 1
    return s


def bin_of(energy, window):
    val = 100.0 * 10.0 * math.log10(energy / window * 0.5 + 1.0e-37)
    return 0 if val <= 0 else min(int(val), BINS - 1)


def analyse(fs, chans, restart=None):
    """The reference's analysis of the channel streams `chans` (1 or 2 float32 arrays) run through: (per-window energies lsum + rsum, per-window bins).
    restart = wf: every window from zero state wf samples in front of it (or from sample 0) instead -- what the kernels compute."""
    window = window_of(fs)
    n = len(chans[0])
    nwin = n // window
    if restart is None:
        outs = [filter_channel(fs, c)[1] for c in chans]
        sums = [[window_sum(o, k * window, window) for k in range(nwin)] for o in outs]
    else:
        sums = []
        for c in chans:
            row = []
            for k in range(nwin):
                a = max(0, k * window - restart)
                o = filter_channel(fs, c, a, (k + 1) * window)[1]
                row.append(window_sum(o, k * window - a, window))
            sums.append(row)
    energies = [sums[0][k] + sums[-1][k] for k in range(nwin)]
    return energies, [bin_of(e, window) for e in energies]


def result(hist_or_bins, from_bins=True):
    """GetTitleGain + RadioGain: (tenth_db or None, percentile bin)"""
    A = [0] * BINS
    if from_bins:
        for b in hist_or_bins:
            A[b] += 1
    else:
        A = list(hist_or_bins)
    elems = sum(A)
    if elems == 0:
        return None, None
    upper = int(math.ceil(elems * (1.0 - 0.95)))
    i = BINS
    while i > 0:
        i -= 1
        upper -= A[i]
        if upper <= 0:
            break
    return int(math.floor((64.82 - i / 100.0) * 10.0 + 0.5)), i


def tenth_at(i):
    """RadioGain if the percentile bin were i"""
    return int(math.floor((64.82 - i / 100.0) * 10.0 + 0.5))


def tag_field(tenth_db):
    g = max(-0x1FE, min(0x1FE, tenth_db))
    return 0x2000 | 0x0C00 | (0x200 if g < 0 else 0) | abs(g)


def bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


# ---- the golden file and its cases' sample streams ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    return json.loads((ROOT / "tests" / "golden" / "golden_replaygain.json").read_text())


def corpus(case):
    return pcm.CORPORA[case["corpus"]](case["nsamples"], case["channels"])


def make_encoder(lib, case, replay_gain=True, info_tag=False, **kw):
    import lamejs_amd
    return lamejs_amd.Mp3Encoder(case["channels"], case["samplerate"], case["kbps"], lib=lib, downmix=bool(case.get("downmix")), joint=bool(case.get("jointStereo")),
                                 reservoir=bool(case.get("reservoir")), protect=bool(case.get("protect")), replay_gain=replay_gain, info_tag=info_tag, **kw)


def histogram(lib, enc):
    A = np.zeros(BINS, np.uint32)
    rc = lib.lhip_debug_gain_histogram(enc._h, A.ctypes.data)
    assert rc == 0, lib.lhip_last_error()
    return A


def nonzero(A):
    return {int(i): int(A[i]) for i in np.nonzero(A)[0]}


def gain_windows(lib, fs, chans):
    """lhip_debug_gain_windows: (energies, bins) of the kernels over one array as one stream"""
    n = len(chans[0])
    nwin = n // window_of(fs)
    l = np.ascontiguousarray(chans[0], F32)
    r = np.ascontiguousarray(chans[-1], F32)
    b = np.zeros(max(nwin, 1), np.int32)
    e = np.zeros(max(nwin, 1), np.float64)
    rc = lib.lhip_debug_gain_windows(fs, len(chans), l.ctypes.data, r.ctypes.data, n, b.ctypes.data, e.ctypes.data)
    assert rc == nwin, (rc, lib.lhip_last_error())
    return e[:nwin], b[:nwin]


def signal_for(fs, n, channels, seed=1):
    """A float32 test stream at any rate: the corpora's formulas are rate-free (sample index based), so the Int16 corpora serve as they are."""
    L, R = (pcm.sine if seed % 2 else pcm.bursts)(n, 2, seed=1000 + seed)
    return [L.astype(F32), R.astype(F32)][:channels]


def ragged_cuts(n, window):
    """call lengths 1, 7, 9, 11, window - 1, window + 1, 1152 and the rest"""
    cuts, left = [], n
    for m in (1, 7, 9, 11, window - 1, window + 1, 1152):
        if left > m:
            cuts.append(m)
            left -= m
    cuts.append(left)
    return cuts


def encode_cut(enc, L, R, cuts, flush=True):
    """the stream in calls of the given lengths; returns the bytes"""
    out, p = [], 0
    for m in cuts:
        out.append(enc.encodeBuffer(L[p:p + m], None if R is None else R[p:p + m]))
        p += m
    assert p == len(L)
    if flush:
        out.append(enc.flush())
    return b"".join(out)


# ---- the samples the analysis sees: behind `scale`, the downmix and the integer-ratio resampler (Lame.js:1551-1584, 1719-1843), flush zeros included --------
def blob_entries(blob):
    """{name: numpy array} of a table blob"""
    n = struct.unpack_from("<I", blob, 8)[0]
    out = {}
    for k in range(n):
        e = 16 + 48 * k
        name = blob[e:e + 32].split(b"\0", 1)[0].decode()
        dtype, count, off = struct.unpack_from("<III", blob, e + 32)
        out[name] = np.frombuffer(blob, {1: "<i4", 2: "<f4", 3: "<f8"}[dtype], count, off)
    return out


def blob_cfg(blob):
    e = blob_entries(blob)
    names = lambda k: bytes(int(c) for c in e[k] if c).decode().split(",")
    cfg = dict(zip(names("cfg_i_names"), (int(v) for v in e["cfg_i"])))
    cfg.update(zip(names("cfg_d_names"), (float(v) for v in e["cfg_d"])))
    return cfg, e


def analysed_stream(case, fed=None):
    """The Float32 samples per output channel that the reference hands its analysis for a golden case: `fed` of them (the case's own count by default)."""
    import lamejs_amd
    fed = case["fed"] if fed is None else fed
    blob = lamejs_amd.tables_blob(case["channels"], case["samplerate"], case["kbps"], joint=bool(case.get("jointStereo")), reservoir=bool(case.get("reservoir")), downmix=bool(case.get("downmix")))
    cfg, ent = blob_cfg(blob)
    L, R = corpus(case)
    scale = cfg["scale"]
    do_scale = cfg.get("do_scale", int(scale != 0.0 and scale != 1.0))
    sc = lambda a: (a.astype(np.float64) * scale).astype(F32) if do_scale else a
    a = sc(L.astype(F32))
    if case.get("downmix"):      # the right samples never see `scale` in a downmix (Lame.js:1551-1584)
        chans = [(0.5 * (a.astype(np.float64) + R.astype(F32).astype(np.float64))).astype(F32)]
    elif cfg["channels_out"] == 2:
        chans = [a, sc(R.astype(F32))]
    else:
        chans = [a]
    ratio = cfg["in_samplerate"] // cfg["out_samplerate"]
    out = []
    for c in chans:
        if ratio == 1:
            assert fed >= len(c)
            out.append(np.concatenate([c, np.zeros(fed - len(c), F32)]))
            continue
        coef = ent["rs_blackfilt"][33:66].astype(np.float64)          # window 1 of the 2 bpc + 1 (bpc = 1): the one an integer ratio always uses
        x = np.concatenate([np.zeros(16, np.float64), c.astype(np.float64), np.zeros(fed * ratio + 64, np.float64)])
        acc = np.zeros(fed, np.float64)
        idx = np.arange(fed) * ratio
        for i in range(33):
            acc = acc + x[idx + i] * coef[i]
        out.append(acc.astype(F32))
    return out


def analysed_md5(chans):
    import hashlib
    h = hashlib.md5()
    for c in chans:
        h.update(np.ascontiguousarray(c, "<f4").tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """(energies, bins) of the run-through restatement for a golden case, computed once and shared"""
    case = next(c for c in golden()["cases"] if c["name"] == name)
    chans = analysed_stream(case)
    assert analysed_md5(chans) == case["analysed_md5"], name
    return analyse(case["out_samplerate"], chans)


def run_case(lib, case, cuts=None, **kw):
    """The case's PCM through an encoder with the option, in calls of `cuts` (default: the case's own 1152), flushed: (histogram, (tenth_db, windows, samples), bytes)"""
    L, R = corpus(case)
    enc = make_encoder(lib, case, **kw)
    if cuts is None:
        cuts = [case["call"]] * (case["nsamples"] // case["call"])
    data = encode_cut(enc, L, R, cuts)
    A = histogram(lib, enc)
    res = enc.replay_gain()
    enc.close()
    return A, res, data


def cap_windows(nwin, worst_share=0.0):
    """(c): at most four times the largest share of windows in which the reference restarted wf samples ahead differs from the reference run through
    (golden: restart_diff -- zero on every case), with a floor of two windows per case"""
    return max(2, int(math.floor(4 * worst_share * nwin)))


def check_against_reference(lib, case, A, res, ref_bins=None, analysed=None):
    """5 (a) - (d) for one case; the per-window bins of the device come from the kernels over the analysed stream (lhip_debug_gain_windows), and the stream's own
    histogram must be exactly the histogram of those bins -- that ties the encoder's path to them."""
    fs = case["out_samplerate"]
    tenth, windows, samples = res
    if ref_bins is None:
        ref_bins = reference_of(case["name"])[1]
        analysed = analysed_stream(case)
        assert samples == case["fed"] and windows == case["windows"] == len(ref_bins), (case["name"], res)          # (a)
    _, dev_bins = gain_windows(lib, fs, analysed)
    assert nonzero(A) == nonzero(np.bincount(dev_bins, minlength=BINS)), case["name"]
    d = [abs(int(x) - int(y)) for x, y in zip(dev_bins, ref_bins)]
    print(case["name"], "windows", windows, "bins differing", sum(1 for v in d if v), "worst", max(d), "tenth_db", tenth)
    assert max(d) <= 1, (case["name"], d)                                                                             # (b)
    worst_share = max(c["restart_diff"] / c["windows"] for c in golden()["cases"])
    assert sum(1 for v in d if v) <= cap_windows(len(d), worst_share), (case["name"], d)                              # (c)
    return dev_bins


def cut_independence(lib, case, with_batch=True):
    """4: one stream as one call, as 1152-sample calls and as ragged calls -- the same histogram, count and bytes; then two streams of different lengths in one batch"""
    import lamejs_amd
    N = case["nsamples"]
    window = window_of(case["out_samplerate"])
    ratio = case["samplerate"] // case["out_samplerate"]
    A0, r0, b0 = run_case(lib, case, [N])
    A1, r1, b1 = run_case(lib, case)
    A2, r2, b2 = run_case(lib, case, ragged_cuts(N, window * ratio))
    assert r0 == r1 == r2 and r0[1] > 0 and (A0 == A1).all() and (A0 == A2).all() and b0 == b1 == b2, (case["name"], r0, r1, r2)
    if with_batch:
        L, R = corpus(case)
        M = N - 3 * 1152 - 77
        a, b = make_encoder(lib, case), make_encoder(lib, case)
        res = lamejs_amd.encode_streams([a, b], [L, L[:M]], None if R is None else [R, R[:M]])
        Aa, Ab = histogram(lib, a), histogram(lib, b)
        ra, rb = a.replay_gain(), b.replay_gain()
        a.close(), b.close()
        c = make_encoder(lib, case)
        bc = encode_cut(c, L[:M], None if R is None else R[:M], [M])
        Ac, rc_ = histogram(lib, c), c.replay_gain()
        c.close()
        assert ra == r0 and (Aa == A0).all() and res[0] == b0 and rb == rc_ and (Ab == Ac).all() and res[1] == bc, (case["name"], ra, rb, rc_)
    return r0
