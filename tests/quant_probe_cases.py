"""TEST INFRASTRUCTURE shared by tests/test_quant_probe_cpu.py and tests/test_quant_probe_gpu.py: the differential probe of the quantization search's
pure functions (lhip_debug_quant_probe, include/lamejs_hip.h: init_outer_loop with the analog-silence rule, init_xrpow, calc_xmin, pecalc, one quantize +
count at a gain with the full and with the short round count, calc_noise eight times) against the oracle's lo_quant_probe, bit for bit.

Every record is built from the oracle's taps and numpy alone, never from the library under test.

harvested   the oracle with taps over pcm.CORPORA["sine"] and ["bursts"], 40 frames each, at 44100/128 stereo and mono, 44100/320 stereo, 48000/192 stereo,
            32000/64 mono, 22050/64 stereo, 8000/16 mono (joint stereo is out of scope: its lines are formed from two spectra).  Every active
            granule-channel gives two records: its FINAL state (the scalefactors, gains and quantized lines the search kept: ix_in = the tap's l3_enc) and
            its BIN-SEARCH state (the final global_gain, zero scalefactors, no ix_in).
synthetic   on 44100/128 stereo, 32000/64 mono and 22050/64 stereo: a gain sweep 0..255 of a full-scale noise granule per block type (44100/128; quantized
            values up to IXMAX_VAL, the LARGE_BITS refusal on both sides of its bound); spectra with one non-zero line at the borders of max_nonzero_coeff,
            tail0 and the 3-, 7- and 9-line bodies; noise floors just below and just above the analog-silence thresholds; maskings with en = 0, thm = 0,
            thm = en, thm / en = 1e-12 and 1e+6, ath_adjust 1, 1e-3 and the smallest value the oracle reaches on digital silence followed by a burst; and
            scalefactor corners (every scalefactor at its slen maximum, preflag with scalefac_scale, subblock_gain 7, steps at both edges of the pow20 table).

census(...) asserts, from the oracle's outputs alone, that the set holds what it is meant to hold."""
import functools

import numpy as np

SFBMAX = 39
LARGE_BITS = 100000
IXMAX_VAL = 8206
Q_MAX, Q_MAX2 = 257, 116
NCALLS = 8
NEED_MAX = (1, 0, 0, 1, 0, 1, 0, 1)      # calls a .. h: the caller reads max_noise whatever over_count is

REC_IN = np.dtype([("xr", "<f4", (576,)), ("ratio", "<f4", (122,)), ("ath_adjust", "<f8"), ("block_type", "<i4"), ("global_gain", "<i4"),
                   ("scalefac_scale", "<i4"), ("preflag", "<i4"), ("subblock_gain", "<i4", (3,)), ("scalefac", "<i4", (SFBMAX,)), ("flags", "<i4"),
                   ("pad", "<i4"), ("ix_in", "<i2", (576,))], align=True)
EVAL = np.dtype([("bits", "<i4"), ("big_values", "<i4"), ("count1", "<i4"), ("count1table_select", "<i4"), ("table_select", "<i4", (3,)),
                 ("region0_count", "<i4"), ("region1_count", "<i4"), ("ran", "<i4"), ("ix", "<i2", (576,))], align=True)
NOISE = np.dtype([("max_noise", "<f8"), ("over_count", "<i4"), ("over_SSD", "<i4"), ("ran", "<i4"), ("pad", "<i4"), ("distort", "<f4", (SFBMAX + 1,))],
                 align=True)
REC_OUT = np.dtype([("xrpow_max", "<f8"), ("pe", "<f8"), ("active", "<i4"), ("max_nonzero_coeff", "<i4"), ("tail0", "<i4"), ("pad", "<i4"),
                    ("xr", "<f4", (576,)), ("xmin", "<f4", (SFBMAX + 1,)), ("ev", EVAL, (2,)), ("nz", NOISE, (NCALLS,))], align=True)
assert REC_IN.itemsize == 4144 and REC_OUT.itemsize == 6352 and EVAL.itemsize == 1192 and NOISE.itemsize == 184

# (sample rate, kbps, channels)
CONFIGS = ((44100, 128, 2), (44100, 128, 1), (44100, 320, 2), (48000, 192, 2), (32000, 64, 1), (22050, 64, 2), (8000, 16, 1))
SYNTH_ON = ((44100, 128, 2), (32000, 64, 1), (22050, 64, 2))
FRAMES = 40
SINGLE_LINES = (0, 1, 2, 190, 191, 192, 193, 446, 447, 448, 449, 510, 511, 512, 513, 574, 575)
# E layout (lhip_debug_read(2)): en.l[22] en.s[13][3] thm.l[22] thm.s[13][3]
EN = np.r_[0:61]
THM = np.r_[61:122]


def config_name(cfg):
    return f"{cfg[0]}/{cfg[1]}/{'stereo' if cfg[2] == 2 else 'mono'}"


def blob_of(cfg):
    import lamejs_amd
    return lamejs_amd.tables_blob(cfg[2], cfg[0], cfg[1])


@functools.lru_cache(maxsize=None)
def tables_of(cfg):
    from replaygain_cases import blob_cfg
    return blob_cfg(blob_of(cfg))


def expected_nln(cfg):
    """The rule of lhip_tables.h (Tables::noise_nln) on the configuration's own blob, as noise_lines_cases.expected_nln."""
    _, e = tables_of(cfg)
    return 7 if max(int(e["sfb_l"][21]), 3 * int(e["sfb_s"][12])) <= 64 * 7 else 9


def psymax_of(block_type):
    return 36 if block_type == 2 else 21


def steps_of(cfg, rec):
    """The band steps of a record in the three scalefactor states the probe visits (as given; the lowest bit of every scalefactor flipped covers e and f)."""
    _, e = tables_of(cfg)
    n = psymax_of(int(rec["block_type"]))
    sfb = np.arange(n)
    pre = np.asarray(e["pretab"][:22], dtype=np.int64)
    out = []
    for flip in (0, 1):
        sf = np.asarray(rec["scalefac"][:n], dtype=np.int64) ^ flip
        if rec["preflag"]:
            assert rec["block_type"] != 2
            sf = sf + pre[:n]
        sbg = np.asarray(rec["subblock_gain"], dtype=np.int64)[sfb % 3] * 8 if rec["block_type"] == 2 else 0
        out.append(int(rec["global_gain"]) - (sf << (int(rec["scalefac_scale"]) + 1)) - sbg)
    return np.concatenate(out)


def _blank(n=1):
    r = np.zeros(n, dtype=REC_IN)
    r["ath_adjust"] = 1.0
    return r


@functools.lru_cache(maxsize=None)
def harvest(cfg):
    """(records, names, checks) of a configuration: checks[i] = (l3_xmin, pe or None) of the tap for the final-state records, None otherwise."""
    import pcm
    from stage_taps import oracle_stages
    sr, kb, ch = cfg
    gr_n = 2 if sr >= 32000 else 1
    cfgd, _ = tables_of(cfg)
    ml = {False: cfgd["masking_lower_long"], True: cfgd["masking_lower_short"]}
    recs, names, checks = [], [], []
    for material in ("sine", "bursts"):
        L, R = pcm.CORPORA[material]((1152 if gr_n == 2 else 576) * FRAMES, ch)
        taps = oracle_stages(ch, sr, kb, L, R)
        assert len(taps) >= FRAMES - 2, (cfg, len(taps))
        ml_prev = 1.0                          # gfc.masking_lower: 1 before the first frame, then what the previous frame's last channel set
        for k, t in enumerate(taps):
            for gr in range(gr_n):
                for c in range(ch):
                    if not t["active"][gr, c]:
                        continue
                    bt = int(t["block_type"][gr, c])
                    r = _blank()[0]
                    r["xr"], r["ratio"], r["ath_adjust"], r["block_type"] = t["xr"][gr, c], t["ratio"][gr, c], t["ath_adjust"], bt
                    r["global_gain"] = t["global_gain"][gr, c]
                    b = r.copy()                                    # the bin-search state
                    r["scalefac_scale"], r["preflag"] = t["scalefac_scale"][gr, c], t["preflag"][gr, c]
                    r["subblock_gain"], r["scalefac"] = t["subblock_gain"][gr, c], t["scalefac"][gr, c]
                    r["flags"], r["ix_in"] = 1, t["l3_enc"][gr, c]
                    assert t["l3_enc"][gr, c].max() <= IXMAX_VAL and t["l3_enc"][gr, c].min() >= 0
                    where = f"{config_name(cfg)} {material} frame {k} gr {gr} ch {c} bt {bt}"
                    # The tap's pe is pecalc of this granule's maskings (the slot the quantizer is handed: lo_tap.ratio) with the masking_lower the
                    # frame BEFORE left behind; the probe uses the block type's own.  Where the two differ the tap's pe is not the probe's.
                    pe = float(t["pe"][gr, c]) if ml_prev == ml[bt == 2] else None
                    recs += [r, b]
                    names += [where + " final", where + " binsearch"]
                    checks += [(t["l3_xmin"][gr, c].copy(), pe), None]
            last = int(t["block_type"][gr_n - 1, ch - 1])
            ml_prev = ml[last == 2]
    return np.array(recs, dtype=REC_IN), names, checks


@functools.lru_cache(maxsize=None)
def smallest_ath_adjust():
    """The smallest ATH adjustment the oracle's adjust_ATH reaches on digital silence followed by a burst (44100/128 mono)."""
    import pcm
    from stage_taps import oracle_stages
    L, _ = pcm.CORPORA["bursts"](1152 * 10, 1)
    L = np.concatenate([np.zeros(1152 * 30, dtype=L.dtype), L])
    taps = oracle_stages(1, 44100, 128, L, None)
    v = min(float(t["ath_adjust"]) for t in taps)
    assert 0.0 < v < 1e-2, v
    return v


def _ath_adjusted(cfg, a, x):
    """athAdjust (QuantizePVT.js:541-561) in numpy: only to place lines a per mille below and above a threshold, never compared."""
    cfgd, _ = tables_of(cfg)
    o, p, fl = 90.30873362, 94.82444863, cfgd["ATH_floor"]
    u = np.log10(x) * 10.0 - fl
    v = a * a
    w = max(0.0, 1.0 + np.log10(v) * (10.0 / o)) if v > 1e-20 else 0.0
    return 10.0 ** (0.1 * (u * w + fl + o - p))


def _silence_records(cfg, base):
    """Noise floors whose pseudo-band lines lie a per mille below / above the analog-silence thresholds; returns (records, names, expectations), an
    expectation being (first natural-order line that must come out zero in every window, or None: nothing is zeroed)."""
    _, e = tables_of(cfg)
    recs, names = [], []
    rng = np.random.default_rng(99)
    for adj in (1.0, 0.03):
        # long blocks: the pseudo bands of sfb21
        b21 = [int(v) for v in e["psfb21"][:7]]
        thr = [float(_ath_adjusted(cfg, adj, float(e["ATH_psfb21"][g])) * (float(e["longfact"][21]) if float(e["longfact"][21]) > 1e-12 else 1.0)) for g in range(6)]
        for bt in (0, 1, 3):
            for kind in ("below", "above", "mixed"):
                r = base.copy()
                r["block_type"], r["ath_adjust"], r["flags"] = bt, adj, 0
                xr = (rng.standard_normal(576) * 50).astype(np.float32)
                for g in range(6):
                    f = 1 - 1e-3 if kind == "below" or (kind == "mixed" and g > 2) else 1 + 1e-3
                    xr[b21[g]:b21[g + 1]] = np.float32(thr[g] * f) * np.where(rng.random(b21[g + 1] - b21[g]) < 0.5, -1, 1)
                r["xr"] = xr
                recs.append(r)
                names.append(f"{config_name(cfg)} analog silence {kind} ath_adjust {adj} bt {bt}")
        # short blocks: the pseudo bands of sfb12, per window
        s12, w12 = int(e["sfb_s"][12]), int(e["sfb_s"][13]) - int(e["sfb_s"][12])
        b12 = [int(v) - int(e["psfb12"][0]) for v in e["psfb12"][:7]]
        thr = [float(_ath_adjusted(cfg, adj, float(e["ATH_psfb12"][g])) * (float(e["shortfact"][12]) if float(e["shortfact"][12]) > 1e-12 else 1.0)) for g in range(6)]
        for kind in ("below", "above", "mixed"):
            r = base.copy()
            r["block_type"], r["ath_adjust"], r["flags"] = 2, adj, 0
            r["subblock_gain"], r["preflag"] = 0, 0
            xr = (rng.standard_normal(576) * 50).astype(np.float32)
            for win in range(3):
                for g in range(6):
                    f = 1 - 1e-3 if kind == "below" or (kind == "mixed" and g > 1 + win) else 1 + 1e-3
                    for l in range(b12[g], min(b12[g + 1], w12)):
                        xr[3 * (s12 + l) + win] = np.float32(thr[g] * f)
            r["xr"] = xr
            recs.append(r)
            names.append(f"{config_name(cfg)} analog silence {kind} ath_adjust {adj} bt 2")
    return recs, names


def _synthetic(cfg, final, binsearch):
    """Synthetic records on a configuration.  final / binsearch: a harvested long-block record of each kind to build on."""
    recs, names = [], []
    cn = config_name(cfg)
    rng = np.random.default_rng(1234)

    def add(r, name):
        recs.append(r)
        names.append(f"{cn} {name}")

    if cfg == SYNTH_ON[0]:
        noise = (rng.standard_normal(576) * 9000).clip(-32000, 32000).astype(np.float32)
        for bt in range(4):
            for gain in range(256):
                r = binsearch.copy()
                r["xr"], r["block_type"], r["global_gain"] = noise, bt, gain
                add(r, f"gain sweep bt {bt} gain {gain}")
    for bt in (0, 2):
        for line in SINGLE_LINES:
            for amp, gain in ((1e-3, 150), (1.0, 190), (3e4, 230)):
                r = binsearch.copy()
                xr = np.zeros(576, dtype=np.float32)
                xr[line] = amp
                r["xr"], r["block_type"], r["global_gain"] = xr, bt, gain
                add(r, f"single line {line} amplitude {amp} bt {bt}")
    s, n = _silence_records(cfg, binsearch)
    recs += s
    names += n
    for bt in range(4):
        for what in ("en=0", "thm=0", "thm=en", "thm/en=1e-12", "thm/en=1e+6"):
            r = binsearch.copy()
            r["block_type"] = bt
            ratio = r["ratio"].copy()
            if what == "en=0":
                ratio[EN] = 0
            elif what == "thm=0":
                ratio[THM] = 0
            elif what == "thm=en":
                ratio[THM] = ratio[EN]
            else:
                ratio[EN] = np.maximum(ratio[EN], np.float32(1e-3))
                ratio[THM] = (ratio[EN].astype(np.float64) * float(what.split("=")[1])).astype(np.float32)
            r["ratio"] = ratio
            add(r, f"masking {what} bt {bt}")
        for adj in (1.0, 1e-3, smallest_ath_adjust()):
            r = binsearch.copy()
            r["block_type"], r["ath_adjust"] = bt, adj
            add(r, f"ath_adjust {adj!r} bt {bt}")
    # scalefactor corners, on the final state's lines (c-h run whatever the gain)
    slen_max = {False: np.r_[np.full(11, 15), np.full(10, 7), np.zeros(18)], True: np.r_[np.full(18, 15), np.full(18, 7), np.zeros(3)]}
    for bt in range(4):
        sh = bt == 2
        for what, gain, scale, pre, sbg in (("slen maximum", 200, 0, 0, 0), ("slen maximum scalefac_scale", 200, 1, 0, 0), ("preflag scalefac_scale", 200, 1, 1, 0),
                                            ("subblock_gain 7", 200, 1, 0, 7), ("lowest step", 0, 1, 0, 7), ("highest step", 255, 0, 0, 0)):
            if (pre and sh) or (sbg and not sh and what != "lowest step"):
                continue
            r = final.copy()
            r["block_type"], r["global_gain"], r["scalefac_scale"], r["preflag"] = bt, gain, scale, pre
            r["subblock_gain"] = sbg if sh else 0
            r["scalefac"] = 0 if what == "highest step" else slen_max[sh].astype(np.int32)
            if what == "lowest step" and not sh:
                r["scalefac"] = np.r_[np.full(21, 28), np.zeros(18)].astype(np.int32)       # 0 - (28 << 2) = -112, flipped 29: -116
            add(r, f"scalefactors {what} bt {bt}")
    return recs, names


@functools.lru_cache(maxsize=None)
def record_set(cfg):
    """(records, names, checks) of a configuration: harvested, then synthetic.  Every record's steps lie inside the pow20 table (asserted)."""
    recs, names, checks = harvest(cfg)
    if cfg in SYNTH_ON:
        longs = [i for i in range(0, len(recs), 2) if recs[i]["block_type"] == 0]
        assert longs, cfg
        i = longs[len(longs) // 2]
        s, n = _synthetic(cfg, recs[i], recs[i + 1])
        recs = np.concatenate([recs, np.array(s, dtype=REC_IN)])
        names = names + n
        checks = checks + [None] * len(s)
    for r, nm in zip(recs, names):
        st = steps_of(cfg, r)
        assert st.min() >= -Q_MAX2 and st.max() <= Q_MAX, (nm, int(st.min()), int(st.max()))
    assert len(recs) == len(names) == len(checks)
    return recs, names, checks


@functools.lru_cache(maxsize=None)
def oracle_outputs(cfg):
    """The oracle's lo_quant_probe over the configuration's records (computed once, shared, read-only), with max_noise zeroed where the reference's caller
    may not read it (need_max clear and over_count > 0): the library writes 0 there."""
    from oracle_py import OracleStream
    recs, _, _ = record_set(cfg)
    with OracleStream(blob_of(cfg)) as o:
        out = o.quant_probe(recs, REC_OUT)
    for k in range(NCALLS):
        if not NEED_MAX[k]:
            hide = out["nz"]["over_count"][:, k] > 0
            out["nz"]["max_noise"][hide, k] = 0.0
    out.setflags(write=False)
    return out


def census():
    """What the whole set holds, from the oracle's outputs alone; asserts the conditions the set is built for."""
    n = dict(bt=[0, 0, 0, 0], tail0=0, notail0=0, over0=0, over=0, big=0, large=0, ath=0, inactive=0, cached=0, records=0)
    for cfg in CONFIGS:
        recs, names, _ = record_set(cfg)
        out = oracle_outputs(cfg)
        _, e = tables_of(cfg)
        for r, o in zip(recs, out):
            n["records"] += 1
            if not o["active"]:
                n["inactive"] += 1
                continue
            n["bt"][int(r["block_type"])] += 1
            n["tail0" if o["tail0"] else "notail0"] += 1
            n["over0" if o["nz"][0]["over_count"] == 0 else "over"] += 1
            n["large"] += int(o["ev"][0]["bits"] == LARGE_BITS)
            n["big"] += int(max(int(o["ev"][0]["ix"].max()), int(r["ix_in"].max()) if r["flags"] & 1 else 0) >= 256)
            n["cached"] += int(o["nz"][5]["ran"])
            if r["block_type"] != 2:
                ath = (np.float64(r["ath_adjust"]) * e["ATH_l"][:21].astype(np.float64) * e["longfact"][:21].astype(np.float64)).astype(np.float32)
                n["ath"] += int(np.array_equal(ath.view(np.uint32), o["xmin"][:21].view(np.uint32)))
    assert min(n["bt"]) >= 8, n
    assert n["tail0"] >= 8 and n["notail0"] >= 8 and n["over0"] >= 8 and n["over"] >= 8, n
    assert n["big"] >= 1 and n["large"] >= 1 and n["ath"] >= 1 and n["inactive"] >= 1, n
    forms = {expected_nln(cfg) for cfg in CONFIGS}
    assert forms == {7, 9}, forms
    # the analog-silence records do what they are named for (the oracle's own rule on them)
    for cfg in SYNTH_ON:
        recs, names, _ = record_set(cfg)
        out = oracle_outputs(cfg)
        _, e = tables_of(cfg)
        lo = int(e["psfb21"][0])
        for r, o, nm in zip(recs, out, names):
            if " analog silence " in nm and not nm.endswith("bt 2"):
                zeros = int((o["xr"][lo:] == 0).sum())
                if " below " in nm:
                    assert zeros == 576 - lo, (nm, zeros)
                elif " above " in nm:
                    assert zeros == 0, (nm, zeros)
                else:
                    assert 0 < zeros < 576 - lo, (nm, zeros)
    return n


def compare(cfg, got, want, names, label):
    """Bit-for-bit comparison of probe outputs; returns human-readable mismatches naming record, step, field and band (at most 12)."""
    bad = []
    if got.tobytes() == want.tobytes():
        return bad

    def bits(a):
        a = np.ascontiguousarray(a)
        return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize]) if a.dtype.kind == "f" else a

    def field(i, step, name, g, w):
        g, w = bits(np.atleast_1d(g)), bits(np.atleast_1d(w))
        d = np.nonzero(g != w)[0]
        if len(d):
            j = int(d[0])
            bad.append(f"{label}: record {i} ({names[i]}): {step}: {name}[{j}] {np.atleast_1d(g)[j]!r} != {np.atleast_1d(w)[j]!r} ({len(d)} differ)")

    for i in range(len(want)):
        if got[i].tobytes() == want[i].tobytes():
            continue
        g, w = got[i], want[i]
        for f in ("active", "xrpow_max", "xr"):
            field(i, "1 init", f, g[f], w[f])
        for f in ("xmin", "max_nonzero_coeff", "tail0", "pe"):
            field(i, "2 xmin", f, g[f], w[f])
        for e in range(2):
            for f in EVAL.names:
                field(i, f"3 evaluation {'full' if e == 0 else 'short'} round count", f, g["ev"][e][f], w["ev"][e][f])
        for k in range(NCALLS):
            for f in ("ran", "over_count", "over_SSD", "max_noise", "distort"):
                field(i, f"4 calc_noise {'abcdefgh'[k]}", f, g["nz"][k][f], w["nz"][k][f])
        if len(bad) >= 12:
            break
    return bad


def run_probe(lib, cfg, recs, max_workgroups=0, stream=None):
    """The library's lhip_debug_quant_probe over records of a configuration -> REC_OUT array.  Raises LhipError on a refusal."""
    import ctypes
    import lamejs_amd
    enc = stream or lamejs_amd.Mp3Encoder(cfg[2], cfg[0], cfg[1], lib=lib)
    try:
        recs = np.ascontiguousarray(recs)
        out = np.full(len(recs), 0, dtype=REC_OUT)
        out.view(np.uint8)[:] = 0xa5                     # the library writes every byte
        rc = enc._lib.lhip_debug_quant_probe(enc._h, recs.ctypes.data_as(ctypes.c_void_p), len(recs), out.ctypes.data_as(ctypes.c_void_p), max_workgroups)
        if rc < 0:
            raise lamejs_amd.LhipError(enc._lib.lhip_last_error().decode())
        return out
    finally:
        if stream is None:
            enc.close()
