"""TEST INFRASTRUCTURE shared by tests/test_bits_probe_cpu.py and tests/test_bits_probe_gpu.py: the differential probe of the bitstream formatter
(lhip_debug_bits_probe, include/lamejs_hip.h: kb_bits and kb_bits_mw of k_bits.h over caller-supplied frames) against the oracle's lo_bits_probe, byte for byte,
and against the main-data decoder of tests/maindata.py, which goes from bits back to values.

Every record is built from the oracle and numpy alone, never from the library under test; part2_length and part2_3_length are computed here, in numpy, from the
configuration's own table blob (hlen, slen1 / slen2, the LSF partition rule).

harvested   the oracle's complete side state (stage_taps.TAP: the s_ fields) over pcm.CORPORA["sine"], ["bursts"] and two fixed-seed streams of
            tests/tools/fuzz_gpu.py's material, 40 frames each; lo_bits_probe of record k must equal frame k of the same lo_encode run.
synthetic   table sweep (every (x, y) of every selectable table under the four sign combinations; 15 with linbits values 0, 1, 2^linbits - 1 in x, y, both;
            8206/8206 under tables 23 and 31; table_select 14), word alignment (the longest codes of tables 13, 15, 24 and a 28-bit ext starting at each of the
            32 bit offsets of a word), trip geometry (big_values and quad counts around the 64-lane trips, region counts at their ends, short blocks around
            3 sfb_s[3]), scalefactors (MPEG-1: the 16 scalefac_compress values at slen maximum and 0, the 16 scfsi patterns; LSF: every partition width at its
            maximum, long and short, the preflag range, a negative scalefactor; side fields at their extremes) and frame filling (empty frame, chosen
            numbers of stuffing bits, the 12-bit length field at 4095, a frame filled to its last bit).

census(...) asserts, from the records and the oracle's outputs alone, that the set holds what it is meant to hold."""
import functools
import sys
from pathlib import Path

import numpy as np

from stage_taps import GRSIDE, SFBMAX, TAP

IXMAX_VAL = 8206
FRAMES = 40
REC_OUT = np.dtype([("bytes", "u1", (1448,)), ("nbytes", "<i4"), ("status", "<i4"), ("offset", "<i8")], align=True)
assert REC_OUT.itemsize == 1464 and GRSIDE.itemsize == 464

# name -> (sample rate, kbps, channels, tables_blob options)
CONFIGS = {
    "44100/128/stereo": (44100, 128, 2, {}), "44100/128/mono": (44100, 128, 1, {}), "44100/320/stereo": (44100, 320, 2, {}), "48000/192/stereo": (48000, 192, 2, {}),
    "32000/64/mono": (32000, 64, 1, {}), "22050/64/stereo": (22050, 64, 2, {}), "8000/16/mono": (8000, 16, 1, {}),
    "32000/320/stereo": (32000, 320, 2, {}),                                                   # the 1440-byte frame
    "44100/128/stereo/protect": (44100, 128, 2, {"protect": True}), "44100/128/mono/protect": (44100, 128, 1, {"protect": True}),
    "22050/64/stereo/protect": (22050, 64, 2, {"protect": True}),
    "44100/128/stereo/joint": (44100, 128, 2, {"joint": True}),
}
SYNTH_FULL = "44100/320/stereo"                                   # room for everything
SYNTH_ALSO = ("22050/64/stereo", "44100/128/mono")                # the table sweep and the scalefactor cases again: LSF, one channel
SELECTABLE = tuple(t for t in range(1, 32) if t not in (4, 14))
BIG_VALUES = (0, 2, 126, 128, 130, 254, 256, 258, 574, 576)
QUADS = (0, 1, 63, 64, 65, 143, 144)
STUFFING = (0, 1, 7, 8, 31, 32, 33, 39)


class Cfg:
    """A configuration's constants and Huffman / scalefactor tables, read from its own table blob."""

    def __init__(self, name):
        import lamejs_amd
        from replaygain_cases import blob_cfg
        sr, kbps, ch, opts = CONFIGS[name]
        self.name, self.sr, self.kbps, self.ch, self.opts = name, sr, kbps, ch, opts
        self.blob = lamejs_amd.tables_blob(ch, sr, kbps, **opts)
        c, e = blob_cfg(self.blob)
        self.c = c
        self.GR, self.C = int(c["mode_gr"]), int(c["channels_out"])
        self.NGC = self.GR * self.C
        self.sideinfo_len, self.frac, self.out_sr = int(c["sideinfo_len"]), int(c["frac_SpF"]), int(c["out_samplerate"])
        self.base = (int(c["version"]) + 1) * 72000 * int(c["brate"]) // self.out_sr
        self.joint = int(c["mode"]) == 1
        self.xlen, self.linmax, self.off = (np.asarray(e[k], dtype=np.int64) for k in ("ht_xlen", "ht_linmax", "ht_off"))
        self.hlen, self.code = np.asarray(e["ht_hlen"], dtype=np.int64), np.asarray(e["ht_code"], dtype=np.int64)
        self.sfb_l, self.sfb_s = np.asarray(e["sfb_l"], dtype=np.int64), np.asarray(e["sfb_s"], dtype=np.int64)
        self.slen1, self.slen2 = np.asarray(e["slen1_tab"], dtype=np.int64), np.asarray(e["slen2_tab"], dtype=np.int64)
        self.n_version = len(e["version_bytes"])
        self.rec_in = np.dtype([("side", GRSIDE, (self.NGC,)), ("l3", "<i2", (self.NGC, 576))])
        assert self.rec_in.itemsize == self.NGC * 1616

    def table(self, t):
        """(hlen, code) of table t as (n, n) arrays (n = 16 for the ESC tables), linbits."""
        t = 16 if t == 14 else t
        n = 16 if t > 15 else int(self.xlen[t])
        o = int(self.off[t])
        return self.hlen[o:o + n * n].reshape(n, n), self.code[o:o + n * n].reshape(n, n), (int(self.xlen[t]) if t > 15 else 0)

    def vmax(self, t):
        t = 16 if t == 14 else t
        return 0 if t == 0 else min(IXMAX_VAL, 15 + int(self.linmax[t])) if t > 15 else int(self.xlen[t]) - 1

    def paddings(self, n):
        """Padding bit of frames 0 .. n-1 of a fresh stream (Encoder.js:442-446; slot_lag starts at frac_SpF)."""
        lag, out = self.frac, []
        for _ in range(n):
            lag -= self.frac
            pad = 0
            if lag < 0:
                lag += self.out_sr
                pad = 1
            out.append(pad if self.frac else 0)
        return out


@functools.lru_cache(maxsize=None)
def cfg_of(name):
    return Cfg(name)


# ---------------------------------------------------------------- lengths, in numpy, from the blob's tables
def lsf_partitions(sc, short):
    """MPEG-2 LSF: (widths, entries) of the four scalefactor partitions, as a decoder derives them from scalefac_compress (no intensity stereo)."""
    if sc < 400:
        return ((sc >> 4) // 5, (sc >> 4) % 5, (sc & 15) >> 2, sc & 3), ((9, 9, 9, 9) if short else (6, 5, 5, 5))
    assert 500 <= sc < 512, sc
    return ((sc - 500) // 3, (sc - 500) % 3, 0, 0), ((18, 18, 0, 0) if short else (11, 10, 0, 0))


def regions_of(cfg, s):
    """[(table, start, end)] of the big-value regions of a side record."""
    bv = int(s["big_values"])
    ts = [int(s[f"table_select{i}"]) for i in range(3)]
    if int(s["block_type"]) == 2:
        r1 = min(3 * int(cfg.sfb_s[3]), bv)
        return [(ts[0], 0, r1), (ts[1], r1, bv)]
    r1 = min(int(cfg.sfb_l[int(s["region0_count"]) + 1]), bv)
    r2 = min(int(cfg.sfb_l[int(s["region0_count"]) + int(s["region1_count"]) + 2]), bv)
    return [(ts[0], 0, r1), (ts[1], r1, r2), (ts[2], r2, bv)]


def pair_bits(cfg, t, x, y):
    """(code bits, ext bits: signs and linbits values) per pair of magnitudes under table t -- the two fields the packer writes (hlen counts the sign bits)."""
    t = 16 if t == 14 else t                        # (the formatter writes, and codes, table 14 as 16)
    hl, _, lin = cfg.table(t)
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    xb = np.where(x > 14, lin, 0) + np.where(y > 14, lin, 0) if t > 15 else np.zeros_like(x)
    signs = (x != 0).astype(np.int64) + (y != 0)
    cx, cy = (np.minimum(x, 15), np.minimum(y, 15)) if t > 15 else (x, y)
    return hl[cx, cy] - signs, xb + signs


def part2_bits(cfg, s, gr):
    if cfg.GR == 2:
        sc = int(s["scalefac_compress"])
        n = 0
        for sfb in range(int(s["sfbmax"])):
            if int(s["scalefac"][sfb]) == -1 and gr == 1:
                continue
            n += int(cfg.slen1[sc] if sfb < int(s["sfbdivide"]) else cfg.slen2[sc])
        return n
    w, cnt = lsf_partitions(int(s["scalefac_compress"]), int(s["block_type"]) == 2)
    return sum(a * b for a, b in zip(w, cnt))


def part3_bits(cfg, s, l3):
    a = np.abs(l3.astype(np.int64))
    n = 0
    for t, lo, hi in regions_of(cfg, s):
        if t == 0 or lo >= hi:
            continue
        c, x = pair_bits(cfg, t, a[lo:hi:2], a[lo + 1:hi:2])
        n += int(c.sum() + x.sum())
    bv, c1 = int(s["big_values"]), int(s["count1"])
    if c1 > bv:
        q = (a[bv:c1] != 0).reshape(-1, 4)
        hl = cfg.hlen[int(cfg.off[32 + int(s["count1table_select"])]):][:16]
        n += int(hl[q[:, 0] * 8 + q[:, 1] * 4 + q[:, 2] * 2 + q[:, 3]].sum())
    return n


def frame_record(cfg, gcs, mode_ext=0):
    """A frame record from NGC (side dict, l3) pairs (None: an empty granule-channel); the lengths are computed here."""
    rec = np.zeros((), dtype=cfg.rec_in)
    gcs = list(gcs) + [None] * (cfg.NGC - len(gcs))
    assert len(gcs) == cfg.NGC
    for gc, item in enumerate(gcs):
        s = rec["side"][gc]
        side, l3 = item if item is not None else ({}, np.zeros(576, dtype=np.int16))
        side = dict(side)
        bt = side.get("block_type", 0)
        side.setdefault("sfbmax", 21 if bt != 2 else 36)
        side.setdefault("sfbdivide", 11 if bt != 2 else 18)
        if bt in (1, 3):                                          # not transmitted: what a decoder assumes, regions ending at sfb_l[8] and at 576
            side["region0_count"], side["region1_count"] = 7, 13
        for k, v in side.items():
            if k == "table_select":
                for i in range(3):
                    s[f"table_select{i}"] = v[i]
            elif k == "subblock_gain":
                for i in range(3):
                    s[f"subblock_gain{i}"] = v[i]
            else:
                s[k] = v
        s["mode_ext"] = mode_ext if cfg.joint else 0
        rec["l3"][gc] = l3
        if "count1" not in side:
            s["count1"] = s["big_values"]
        s["part2_length"] = part2_bits(cfg, s, gc // cfg.C)
        s["part2_3_length"] = part3_bits(cfg, s, rec["l3"][gc])
    return rec


def frame_used_bits(cfg, rec):
    return 8 * cfg.sideinfo_len + int(rec["side"]["part2_length"].sum() + rec["side"]["part2_3_length"].sum())


# ---------------------------------------------------------------- synthetic records
def _gc_pairs(t, xs, ys, tables=None, r0=0, r1=0, **side):
    """A granule-channel whose big values are the signed pairs (xs, ys) under table t (all three regions)."""
    l3 = np.zeros(576, dtype=np.int16)
    n = len(xs)
    assert n <= 288
    l3[0:2 * n:2], l3[1:2 * n:2] = xs, ys
    d = {"big_values": 2 * n, "count1": 2 * n, "table_select": tables or (t, t, t), "region0_count": r0, "region1_count": r1, "global_gain": 100 + t}
    d.update(side)
    return d, l3


def _pack_items(cfg, t, xs, ys, budget):
    """Cut the signed pairs into granule-channels of at most `budget` bits and 288 pairs."""
    c, x = pair_bits(cfg, t, np.abs(xs), np.abs(ys))
    bits = c + x
    out, lo, acc = [], 0, 0
    for i in range(len(xs)):
        if acc + bits[i] > budget or i - lo == 288:
            out.append(_gc_pairs(t, xs[lo:i], ys[lo:i]))
            lo, acc = i, 0
        acc += int(bits[i])
    out.append(_gc_pairs(t, xs[lo:], ys[lo:]))
    return out


def _frames_of(cfg, gcs, label, out):
    for i in range(0, len(gcs), cfg.NGC):
        out.append((label, frame_record(cfg, gcs[i:i + cfg.NGC])))


def table_sweep(cfg, out):
    budget = min(3800, (8 * (cfg.base - cfg.sideinfo_len)) // cfg.NGC - 8)
    gcs = []
    for t in SELECTABLE:
        n = 16 if t > 15 else int(cfg.xlen[t])
        lin = int(cfg.xlen[t]) if t > 15 else 0
        x, y = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
        xs = np.concatenate([x * sx for sx in (1, 1, -1, -1)])
        ys = np.concatenate([y * sy for sy in (1, -1, 1, -1)])
        if t > 15:
            # 15 stands for 15 + the linbits value: 0, 1 and 2^linbits - 1, in x, in y and in both
            ex = sorted({15, 16, min(15 + (1 << lin) - 1, IXMAX_VAL)})
            ax = [(a, b) for a in ex for b in (0, 1, 14)] + [(b, a) for a in ex for b in (0, 1, 14)] + [(a, b) for a in ex for b in ex]
            axs, ays = np.array([p[0] for p in ax]), np.array([p[1] for p in ax])
            xs = np.concatenate([xs] + [axs * sx for sx in (1, -1)] + [axs])
            ys = np.concatenate([ys] + [ays * sy for sy in (1, -1)] + [-ays])
        gcs += _pack_items(cfg, t, xs.astype(np.int16), ys.astype(np.int16), budget)
    for t in (23, 31):
        gcs.append(_gc_pairs(t, np.array([IXMAX_VAL, -IXMAX_VAL, IXMAX_VAL], dtype=np.int16), np.array([IXMAX_VAL, -IXMAX_VAL, -IXMAX_VAL], dtype=np.int16)))
    x, y = (a.ravel() for a in np.meshgrid(np.arange(16), np.arange(16), indexing="ij"))
    gcs.append(_pack_items(cfg, 14, x[:64].astype(np.int16), (-y[:64]).astype(np.int16), budget)[0])      # table_select 14: written, and coded, as 16
    _frames_of(cfg, gcs, "table sweep", out)


def longest(cfg, t):
    hl, _, _ = cfg.table(t)
    i = int(np.argmax(hl))
    return i // hl.shape[1], i % hl.shape[1], int(hl.max())


def word_alignment(cfg, out):
    """gc 0: `shift` pairs (0, 0) under table 1, one bit each; gc 1 starts with the item, so the item starts at every offset of a word over 32 shifts."""
    items = []
    for t in (13, 15, 24):
        x, y, _ = longest(cfg, t)
        items.append((f"longest code of table {t}", t, x, y))
    items.append(("28-bit ext", 23, IXMAX_VAL, IXMAX_VAL))
    for label, t, x, y in items:
        for shift in range(32):
            filler = _gc_pairs(1, np.zeros(shift, dtype=np.int16), np.zeros(shift, dtype=np.int16))
            body = _gc_pairs(t, np.array([-x, x, 1], dtype=np.int16), np.array([-y, y, 0], dtype=np.int16))
            out.append((f"word alignment: {label}, shift {shift}", frame_record(cfg, [filler, body][:cfg.NGC] if cfg.NGC >= 2 else [body])))


def trip_geometry(cfg, out):
    rng = np.random.default_rng(20260)
    for bv in BIG_VALUES:
        for t, tabs in ((1, (1, 1, 1)), (7, (5, 7, 9)), (16, (16, 13, 24))):
            l3 = np.zeros(576, dtype=np.int16)
            for tt, lo, hi in regions_of(cfg, {"big_values": bv, "block_type": 0, "region0_count": 3, "region1_count": 2, "table_select0": tabs[0], "table_select1": tabs[1], "table_select2": tabs[2]}):
                m = min(cfg.vmax(tt), 2 if tt < 16 else 17)
                l3[lo:hi] = rng.integers(-m, m + 1, hi - lo)
            # (keep the granule within the 12-bit length: small values)
            rest = (576 - bv) // 4 * 4
            nq = min(rest // 4, 3)
            l3[bv:bv + 4 * nq] = rng.integers(-1, 2, 4 * nq)
            out.append((f"trip geometry: big_values {bv}, tables {tabs}", frame_record(cfg, [({"big_values": bv, "count1": bv + 4 * nq, "table_select": tabs, "region0_count": 3, "region1_count": 2, "global_gain": 150}, l3)])))
    for c1t in (0, 1):
        for nq in QUADS:
            # all 16 patterns with all their sign combinations, cycled over the quads
            pats = [(p, sg) for p in range(16) for sg in range(1 << bin(p).count("1"))]
            l3 = np.zeros(576, dtype=np.int16)
            for k in range(nq):
                p, sg = pats[(k * 7 + c1t) % len(pats)]
                b = 0
                for j in range(4):
                    if (p >> (3 - j)) & 1:
                        l3[4 * k + j] = -1 if (sg >> b) & 1 else 1
                        b += 1
            out.append((f"trip geometry: {nq} quads, count1 table {c1t}", frame_record(cfg, [({"big_values": 0, "count1": 4 * nq, "count1table_select": c1t, "global_gain": 160}, l3)])))
        # every pattern under every sign combination, in one granule-channel
        l3 = np.zeros(576, dtype=np.int16)
        pats = [(p, sg) for p in range(16) for sg in range(1 << bin(p).count("1"))]
        assert len(pats) == 81
        for k, (p, sg) in enumerate(pats):
            b = 0
            for j in range(4):
                if (p >> (3 - j)) & 1:
                    l3[2 + 4 * k + j] = -1 if (sg >> b) & 1 else 1
                    b += 1
        l3[0:2] = (1, -1)
        out.append((f"trip geometry: the 81 signed quad patterns, count1 table {c1t}", frame_record(cfg, [({"big_values": 2, "count1": 2 + 4 * 81, "count1table_select": c1t, "table_select": (1, 0, 0), "global_gain": 161}, l3)])))
    # region counts: (0, 0), the largest pair with a valid sfb_l index, regions clipped by big_values
    for r0, r1, bv in ((0, 0, 40), (15, 5, 576), (13, 7, 576), (15, 5, 20), (7, 7, 100), (0, 7, 6)):
        l3 = np.zeros(576, dtype=np.int16)
        l3[:bv] = np.random.default_rng(r0 * 100 + r1).integers(-1, 2, bv)
        out.append((f"trip geometry: region counts {r0}, {r1}, big_values {bv}", frame_record(cfg, [None, ({"big_values": bv, "count1": bv, "table_select": (2, 3, 1), "region0_count": r0, "region1_count": r1, "global_gain": 170}, l3)][-min(2, cfg.NGC):])))
    # short blocks below, at and above 3 sfb_s[3]
    e = 3 * int(cfg.sfb_s[3])
    for bv in (e - 2, e, e + 2, 0, 2, 190):
        l3 = np.zeros(576, dtype=np.int16)
        l3[:bv] = np.random.default_rng(bv).integers(-3, 4, bv)
        out.append((f"trip geometry: short block, big_values {bv} (3 sfb_s[3] = {e})", frame_record(cfg, [({"big_values": bv, "count1": bv, "block_type": 2, "table_select": (8, 24, 0), "subblock_gain": (1, 0, 7), "global_gain": 180}, l3)])))
    # start and stop blocks (window switching without short windows: two tables, the regions a decoder assumes)
    for bt in (1, 3):
        l3 = np.zeros(576, dtype=np.int16)
        l3[:100] = np.random.default_rng(bt).integers(-2, 3, 100)
        out.append((f"trip geometry: block type {bt}", frame_record(cfg, [({"big_values": 100, "count1": 100, "block_type": bt, "table_select": (5, 6, 0), "global_gain": 181}, l3)])))


def scalefactor_cases(cfg, out):
    l3 = np.zeros(576, dtype=np.int16)
    l3[:8] = (1, -1, 0, 1, 1, 0, -1, -1)
    body = {"big_values": 4, "count1": 8, "table_select": (1, 1, 1), "global_gain": 120}
    if cfg.GR == 2:
        for sc in range(16):
            for short in (0, 1):
                nmax, div = (36, 18) if short else (21, 11)
                for top in (1, 0):
                    sf = np.zeros(SFBMAX, dtype=np.int32)
                    if top:
                        sf[:div], sf[div:nmax] = (1 << int(cfg.slen1[sc])) - 1, (1 << int(cfg.slen2[sc])) - 1
                    gc = dict(body, scalefac_compress=sc, scalefac=sf, block_type=2 if short else 0, sfbmax=nmax, sfbdivide=div)
                    out.append((f"scalefactors: scalefac_compress {sc}, {'short' if short else 'long'}, {'slen maximum' if top else 'zero'}", frame_record(cfg, [(gc, l3)] * min(2, cfg.NGC))))
        # scfsi: the 16 patterns, -1 in the shared bands of granule 1 (scfsi_band 0, 6, 11, 16, 21)
        band = (0, 6, 11, 16, 21)
        for pat in range(16):
            gcs = []
            for gr in range(2):
                for ch in range(cfg.C):
                    sf = (np.arange(SFBMAX, dtype=np.int32) * 3 + ch) % 4
                    sf[21:] = 0
                    p = pat if ch == 0 else (pat * 7 + 3) % 16
                    if gr == 1:
                        for i in range(4):
                            if (p >> i) & 1:
                                sf[band[i]:band[i + 1]] = -1
                    gcs.append((dict(body, scalefac_compress=9, scalefac=sf, scfsi=p if gr == 1 else 0), l3))      # slen 2, 2... see slen tables
            out.append((f"scalefactors: scfsi pattern {pat}", frame_record(cfg, gcs)))
    else:
        for short in (0, 1):
            # every partition width at its maximum (below 400: 4, 4, 3, 3), each partition alone and all together; the preflag range 500 .. 511
            for w in ((4, 0, 0, 0), (0, 4, 0, 0), (0, 0, 3, 0), (0, 0, 0, 3), (4, 4, 3, 3), (1, 2, 3, 1), (0, 0, 0, 0)):
                sc = (w[0] * 5 + w[1]) * 16 + w[2] * 4 + w[3]
                widths, cnt = lsf_partitions(sc, short)
                assert tuple(widths) == w
                sf, i = np.zeros(SFBMAX, dtype=np.int32), 0
                for a, n in zip(widths, cnt):
                    sf[i:i + n] = (1 << a) - 1
                    i += n
                gc = dict(body, scalefac_compress=sc, scalefac=sf, block_type=2 if short else 0, table_select=(1, 1, 0) if short else (1, 1, 1))
                out.append((f"scalefactors: LSF widths {w}, {'short' if short else 'long'}", frame_record(cfg, [(gc, l3)] * cfg.NGC)))
            for sc in range(500, 512):
                widths, cnt = lsf_partitions(sc, short)
                sf, i = np.zeros(SFBMAX, dtype=np.int32), 0
                for a, n in zip(widths, cnt):
                    sf[i:i + n] = (1 << a) - 1
                    i += n
                gc = dict(body, scalefac_compress=sc, preflag=1, scalefac=sf, block_type=2 if short else 0, table_select=(1, 1, 0) if short else (1, 1, 1))
                out.append((f"scalefactors: LSF preflag scalefac_compress {sc}, {'short' if short else 'long'}", frame_record(cfg, [(gc, l3)] * cfg.NGC)))
        sf = np.zeros(SFBMAX, dtype=np.int32)
        sf[:21] = (np.arange(21) % 3) - 1                                      # -1, 0, 1: a negative scalefactor is written as 0
        out.append(("scalefactors: LSF negative scalefactor", frame_record(cfg, [(dict(body, scalefac_compress=(1 * 5 + 1) * 16 + 1 * 4 + 1, scalefac=sf), l3)] * cfg.NGC)))
    # side fields at their extremes
    ext = dict(body, global_gain=255, scalefac_scale=1, count1table_select=1, block_type=2, table_select=(31, 31, 0), subblock_gain=(7, 7, 7), big_values=4, count1=8)
    if cfg.GR == 2:
        ext.update(preflag=1, scalefac_compress=15, scfsi=15)
        sf = np.zeros(SFBMAX, dtype=np.int32)
        sf[:18], sf[18:36] = (1 << int(cfg.slen1[15])) - 1, (1 << int(cfg.slen2[15])) - 1
        ext.update(scalefac=sf, sfbmax=36, sfbdivide=18)
    else:
        ext.update(preflag=1, scalefac_compress=511)
    out.append(("side fields at their extremes", frame_record(cfg, [(ext, l3)] * cfg.NGC, mode_ext=2)))
    ext2 = dict(body, global_gain=255, scalefac_scale=1, count1table_select=1, table_select=(31, 31, 31), region0_count=15, region1_count=5, big_values=4, count1=8)
    out.append(("side fields at their extremes, long block", frame_record(cfg, [(ext2, l3)] * cfg.NGC, mode_ext=3)))


def exact_gc(cfg, n):
    """A granule-channel whose main data is exactly n bits (0 .. 4095): table 13 over [0, e), e a band border -- na pairs of its longest code, (0, 0) pairs for the
    rest --, then nb pairs (0, 0) under table 1, one bit each."""
    x13, y13, l13 = longest(cfg, 13)
    z13 = int(cfg.table(13)[0][0, 0])
    assert int(cfg.table(1)[0][0, 0]) == 1 and 0 <= n <= 4095
    for k in range(2, 23):
        e = int(cfg.sfb_l[k])
        if e % 2:
            continue
        for na in range(e // 2, -1, -1):
            nb = n - na * l13 - (e // 2 - na) * z13
            if 0 <= nb <= (576 - e) // 2:
                r0 = min(15, k - 2)
                l3 = np.zeros(576, dtype=np.int16)
                l3[0:2 * na:2], l3[1:2 * na:2] = x13, -y13
                bv = e + 2 * nb
                return {"big_values": bv, "count1": bv, "table_select": (13, 13, 1), "region0_count": r0, "region1_count": k - 2 - r0, "global_gain": 142}, l3
    raise AssertionError(f"no granule-channel of {n} bits")


def filled_frame(cfg, nbits):
    """A frame whose main data is exactly nbits, dealt over its granule-channels."""
    gcs, left = [], nbits
    for gc in range(cfg.NGC):
        take = min(left, 4095, -(-left // (cfg.NGC - gc)) + 37 * gc)
        gcs.append(exact_gc(cfg, take))
        left -= take
    assert left == 0, (cfg.name, nbits)
    rec = frame_record(cfg, gcs)
    assert frame_used_bits(cfg, rec) == 8 * cfg.sideinfo_len + nbits
    return rec


def frame_filling(cfg, out):
    """A record's padding comes from its place in the set: empty frames are put in until the place has the padding a case asks for."""
    def at_padding(pad):
        while cfg.paddings(len(out) + 1)[-1] != pad:
            out.append(("frame filling: the empty frame", frame_record(cfg, [])))
        return 8 * (cfg.base + pad) - 8 * cfg.sideinfo_len

    out.append(("frame filling: the empty frame", frame_record(cfg, [])))
    for pad in (0, 1) if cfg.frac else (0,):
        for st in STUFFING + (8 * cfg.n_version + 32, 8 * cfg.n_version + 33):
            room = at_padding(pad)
            if room - st <= 4095 * cfg.NGC:
                out.append((f"frame filling: {st} stuffing bits on a{' padded' if pad else 'n unpadded'} frame", filled_frame(cfg, room - st)))
    if 8 * cfg.base - 8 * cfg.sideinfo_len >= 4095:
        out.append(("frame filling: the 12-bit length field at 4095", frame_record(cfg, [exact_gc(cfg, 4095)])))


@functools.lru_cache(maxsize=None)
def synthetic(name):
    """[(label, record)] of a configuration's synthetic records, in a fixed order."""
    cfg = cfg_of(name)
    out = []
    if name == SYNTH_FULL or name in SYNTH_ALSO:
        table_sweep(cfg, out)
        scalefactor_cases(cfg, out)
    if name == SYNTH_FULL:
        word_alignment(cfg, out)
        trip_geometry(cfg, out)
    if name in (SYNTH_FULL, "32000/320/stereo", "44100/128/mono", "22050/64/stereo", "8000/16/mono"):
        frame_filling(cfg, out)                                   # (32000/320: 0 stuffing bits = the 1440-byte frame filled completely)
    if cfg.joint:                                                 # the header's mode_ext comes from the record
        for me in (2, 0, 2):
            out.append((f"joint stereo: mode_ext {me}", frame_record(cfg, [exact_gc(cfg, 300 + 7 * gc + me) for gc in range(cfg.NGC)], mode_ext=me)))
    return out


# ---------------------------------------------------------------- harvested records
def _materials(cfg):
    import pcm
    n = 1152 * FRAMES // (2 // cfg.GR) + 2000
    yield "sine", pcm.CORPORA["sine"](n, cfg.ch)
    yield "bursts", pcm.CORPORA["bursts"](n, cfg.ch)
    sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
    import fuzz_gpu
    for seed in (11, 12):
        yield f"fuzz material seed {seed}", fuzz_gpu.material(np.random.default_rng(seed), n, cfg.ch)


@functools.lru_cache(maxsize=None)
def harvested(name):
    """[(material, records, frames)]: per material the oracle's side state of frames 0 .. FRAMES-1 as records, and the bytes lo_encode gave for each frame."""
    from oracle_py import OracleStream
    cfg = cfg_of(name)
    out = []
    for label, (L, R) in _materials(cfg):
        recs, frames = [], []
        with OracleStream(cfg.blob, tap=True) as o:
            for p in range(0, len(L), 576):
                b = o.encode(L[p:p + 576], None if (cfg.ch == 1 or R is None) else R[p:p + 576])
                if not b or len(recs) == FRAMES:
                    continue
                t = np.frombuffer(o.tap(), dtype=TAP)[0]
                rec = np.zeros((), dtype=cfg.rec_in)
                for gc in range(cfg.NGC):
                    gr, ch = divmod(gc, cfg.C)
                    s = rec["side"][gc]
                    for f in ("big_values", "count1", "region0_count", "region1_count", "scalefac_compress", "count1table_select", "sfbmax", "sfbdivide", "preflag",
                              "scalefac_scale", "block_type", "global_gain", "part2_3_length", "part2_length"):
                        s[f] = t["s_" + f][gr, ch]
                    for i in range(3):
                        s[f"table_select{i}"], s[f"subblock_gain{i}"] = t["s_table_select"][gr, ch, i], t["s_subblock_gain"][gr, ch, i]
                    s["scalefac"] = t["s_scalefac"][gr, ch]
                    s["scfsi"] = t["s_scfsi"][ch] if gr == 1 else 0
                    s["mode_ext"] = t["mode_ext"]
                    rec["l3"][gc] = t["s_l3"][gr, ch]
                    # the lengths the oracle's search kept are the ones numpy computes from the tables
                    assert int(s["part2_length"]) == part2_bits(cfg, s, gr) and int(s["part2_3_length"]) == part3_bits(cfg, s, rec["l3"][gc]), \
                        (name, label, len(recs), gc, int(s["part2_length"]), part2_bits(cfg, s, gr), int(s["part2_3_length"]), part3_bits(cfg, s, rec["l3"][gc]), s)
                recs.append(rec)
                frames.append(b)
        assert len(recs) == FRAMES, (name, label, len(recs))
        out.append((label, np.array(recs, dtype=cfg.rec_in), frames))
    return out


@functools.lru_cache(maxsize=None)
def groups(name):
    """[(group label, record labels, records)]: one probe call each -- a record's padding and offset come from its place in the call, so every material's
    harvested records are a call of their own (record k is frame k, as in the lo_encode run they come from), and so are the synthetic records."""
    cfg = cfg_of(name)
    out = [(label, [f"harvested {label} frame {k}" for k in range(len(r))], r) for label, r, _ in harvested(name)]
    syn = synthetic(name)
    if syn:
        out.append(("synthetic", [label for label, _ in syn], np.array([r for _, r in syn], dtype=cfg.rec_in)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_outputs(name):
    """lo_bits_probe over every group of groups(name): computed once, shared, read-only."""
    from oracle_py import OracleStream
    cfg = cfg_of(name)
    outs = []
    with OracleStream(cfg.blob) as o:
        for _, _, recs in groups(name):
            out = o.bits_probe(recs, REC_OUT)
            out.setflags(write=False)
            outs.append(out)
    return outs


def oracle_probe(name, recs):
    from oracle_py import OracleStream
    with OracleStream(cfg_of(name).blob) as o:
        return o.bits_probe(recs, REC_OUT)


def run_probe(lib, name, recs, form=0, max_workgroups=0, stream=None):
    """The library's lhip_debug_bits_probe over records of a configuration -> REC_OUT array.  Raises LhipError on a refusal."""
    import ctypes
    import lamejs_amd
    cfg = cfg_of(name)
    enc = stream or lamejs_amd.Mp3Encoder(cfg.ch, cfg.sr, cfg.kbps, lib=lib, **cfg.opts)
    try:
        recs = np.ascontiguousarray(recs)
        assert recs.dtype == cfg.rec_in
        out = np.zeros(len(recs), dtype=REC_OUT)
        out.view(np.uint8)[:] = 0xa5                     # the library writes every byte
        rc = enc._lib.lhip_debug_bits_probe(enc._h, recs.ctypes.data_as(ctypes.c_void_p), len(recs), out.ctypes.data_as(ctypes.c_void_p), form, max_workgroups)
        if rc < 0:
            raise lamejs_amd.LhipError(enc._lib.lhip_last_error().decode())
        return out
    finally:
        if stream is None:
            enc.close()


# ---------------------------------------------------------------- comparison
def locate_bit(cfg, rec, bit):
    """What a bit position of a frame belongs to: header, side field, scalefactor, region and pair, count1 quad, or stuffing."""
    if bit < 32:
        return "header"
    pos = 32
    if cfg.c["error_protection"]:
        if bit < 48:
            return "CRC"
        pos = 48
    head = (9 + (3 if cfg.C == 2 else 5) + 4 * cfg.C) if cfg.GR == 2 else (8 + cfg.C)
    if bit < pos + head:
        return "side info: main_data_begin / private bits / scfsi"
    pos += head
    per = 59 if cfg.GR == 2 else 63
    if bit < pos + per * cfg.NGC:
        gc, o = divmod(bit - pos, per)
        names = [("part2_3_length", 12), ("big_values", 9), ("global_gain", 8), ("scalefac_compress", 4 if cfg.GR == 2 else 9), ("window_switching_flag", 1),
                 ("block type / table_select / region counts / subblock_gain", 22)] + ([("preflag", 1)] if cfg.GR == 2 else []) + [("scalefac_scale", 1), ("count1table_select", 1)]
        for nm, w in names:
            if o < w:
                return f"granule-channel {gc} side field {nm}"
            o -= w
    pos = 8 * cfg.sideinfo_len
    for gc in range(cfg.NGC):
        s, l3 = rec["side"][gc], rec["l3"][gc]
        p2, p3 = int(s["part2_length"]), int(s["part2_3_length"])
        if bit < pos + p2:
            return f"granule-channel {gc} scalefactors (bit {bit - pos} of part 2)"
        if bit < pos + p2 + p3:
            q = pos + p2
            a = np.abs(l3.astype(np.int64))
            for ri, (t, lo, hi) in enumerate(regions_of(cfg, s)):
                if t == 0 or lo >= hi:
                    continue
                c, x = pair_bits(cfg, t, a[lo:hi:2], a[lo + 1:hi:2])
                ends = q + np.cumsum(c + x)
                if bit < ends[-1]:
                    k = int(np.searchsorted(ends, bit, side="right"))
                    return f"granule-channel {gc} region {ri} (table {t}) pair {k} = lines {lo + 2 * k}, {lo + 2 * k + 1}: values {int(l3[lo + 2 * k])}, {int(l3[lo + 2 * k + 1])}"
                q = int(ends[-1])
            return f"granule-channel {gc} count1 region (bit {bit - q} of it)"
        pos += p2 + p3
    return f"stuffing (bit {bit - pos} of it)"


def compare(cfg, labels, recs, got, want):
    """Byte-for-byte comparison; returns human-readable mismatches naming record, field and the first differing bit (at most 12)."""
    bad = []
    for r in range(len(recs)):
        g, w = got[r], want[r]
        if int(w["status"]) != 0:
            bad.append(f"record {r} ({labels[r]}): the oracle refused the record (status {int(w['status'])})")
        elif int(g["status"]) != 0 or int(g["nbytes"]) != int(w["nbytes"]) or int(g["offset"]) != int(w["offset"]):
            bad.append(f"record {r} ({labels[r]}): status / bytes / offset {int(g['status'])} / {int(g['nbytes'])} / {int(g['offset'])}, the oracle's 0 / {int(w['nbytes'])} / {int(w['offset'])}")
        elif not np.array_equal(g["bytes"], w["bytes"]):
            i = int(np.nonzero(g["bytes"] != w["bytes"])[0][0])
            x = int(g["bytes"][i]) ^ int(w["bytes"][i])
            bit = 8 * i + (7 - (x.bit_length() - 1))
            bad.append(f"record {r} ({labels[r]}): first differing bit {bit} (byte {i}: {int(g['bytes'][i]):02x}, the oracle's {int(w['bytes'][i]):02x}): {locate_bit(cfg, recs[r], bit)}")
        if len(bad) >= 12:
            break
    return bad


# ---------------------------------------------------------------- census
def item_positions(cfg, rec):
    """(start bit in the frame, bits, kind) of every field of the main data of a record: kind 'code' / 'ext' / 'quad'."""
    pos = 8 * cfg.sideinfo_len
    out = []
    for gc in range(cfg.NGC):
        s, l3 = rec["side"][gc], rec["l3"][gc]
        q = pos + int(s["part2_length"])
        a = np.abs(l3.astype(np.int64))
        for t, lo, hi in regions_of(cfg, s):
            if t == 0 or lo >= hi:
                continue
            c, x = pair_bits(cfg, t, a[lo:hi:2], a[lo + 1:hi:2])
            # the packer's two fields: code with the signs that precede... it writes `code` (hlen bits) and `ext` (linbits values and signs)
            starts = q + np.concatenate([[0], np.cumsum(c + x)[:-1]])
            out += [(int(st), int(n), "code") for st, n in zip(starts, c)]
            out += [(int(st + n), int(m), "ext") for st, n, m in zip(starts, c, x) if m]
            q += int((c + x).sum())
        bv, c1 = int(s["big_values"]), int(s["count1"])
        if c1 > bv:
            z = (a[bv:c1] != 0).reshape(-1, 4)
            hl = cfg.hlen[int(cfg.off[32 + int(s["count1table_select"])]):][:16]
            n = hl[z[:, 0] * 8 + z[:, 1] * 4 + z[:, 2] * 2 + z[:, 3]]
            starts = q + np.concatenate([[0], np.cumsum(n)[:-1]])
            out += [(int(st), int(m), "quad") for st, m in zip(starts, n)]
        pos += int(s["part2_length"]) + int(s["part2_3_length"])
    return out


def census(names=None):
    """What the record sets hold, counted from the records and the oracle's outputs alone; asserts that nothing the set is meant to hold is missing."""
    names = list(names or CONFIGS)
    seen_pairs, seen_quads, straddle, lens_seen = set(), set(), set(), set()
    bvs, quads, scfsi, lsf_ranges, stuffing, pads = set(), set(), set(), set(), set(), set()
    align = {k: set() for k in ("13", "15", "24", "ext28")}
    versions, channels, sidelens, mode_exts = set(), set(), set(), set()
    for name in names:
        cfg = cfg_of(name)
        versions.add("1" if cfg.GR == 2 else "2.5" if cfg.out_sr < 16000 else "2")
        channels.add(cfg.C)
        sidelens.add(cfg.sideinfo_len)
        long13, long15, long24 = (longest(cfg, t) for t in (13, 15, 24))
        for (_, _, recs), want in zip(groups(name), oracle_outputs(name)):
            assert (want["status"] == 0).all(), (name, np.nonzero(want["status"])[0][:5])
            padding = cfg.paddings(len(recs))
            for r, rec in enumerate(recs):
                assert int(want["nbytes"][r]) == cfg.base + padding[r]
                pads.add((bool(cfg.frac), padding[r]))
                if cfg.joint:
                    mode_exts.add((int(rec["side"][0]["mode_ext"]), (int(want["bytes"][r][3]) >> 4) & 3))
                left = 8 * int(want["nbytes"][r]) - frame_used_bits(cfg, rec)
                assert left >= 0
                stuffing.add(left)
                for gc in range(cfg.NGC):
                    s, l3 = rec["side"][gc], rec["l3"][gc]
                    a = np.abs(l3.astype(np.int64))
                    bv, c1 = int(s["big_values"]), int(s["count1"])
                    bvs.add(bv)
                    quads.add((c1 - bv) // 4)
                    if cfg.GR == 2 and gc // cfg.C == 1:
                        scfsi.add(int(s["scfsi"]))
                    if cfg.GR == 1:
                        lsf_ranges.add(int(s["scalefac_compress"]) >= 500)
                    for t, lo, hi in regions_of(cfg, s):
                        if t == 0 or lo >= hi:
                            continue
                        tt = 16 if t == 14 else t
                        x, y = a[lo:hi:2], a[lo + 1:hi:2]
                        if tt > 15:
                            x, y = np.minimum(x, 15), np.minimum(y, 15)
                        sx, sy = l3[lo:hi:2] < 0, l3[lo + 1:hi:2] < 0
                        seen_pairs.update(zip([tt] * len(x), x.tolist(), y.tolist(), sx.tolist(), sy.tolist()))
                    if c1 > bv:
                        z = l3[bv:c1].reshape(-1, 4)
                        seen_quads.update((int(s["count1table_select"]),) + tuple(q) for q in z.tolist())
                for st, n, kind in item_positions(cfg, rec):
                    lens_seen.add((kind, n))
                    if (st & 31) + n > 32:
                        straddle.add((kind, n))
                if name == SYNTH_FULL:
                    # the alignment items: the first field of granule-channel 1
                    pos = 8 * cfg.sideinfo_len + int(rec["side"][0]["part2_length"]) + int(rec["side"][0]["part2_3_length"])
                    s1, l1 = rec["side"][1], rec["l3"][1]
                    if int(s1["big_values"]) >= 2 and int(s1["part2_length"]) == 0:
                        t, x, y = int(s1["table_select0"]), abs(int(l1[0])), abs(int(l1[1]))
                        for key, (lx, ly, _), tab in (("13", long13, 13), ("15", long15, 15), ("24", long24, 24)):
                            if t == tab and (x, y) == (lx, ly):
                                align[key].add(pos & 31)
                        if t == 23 and x == IXMAX_VAL and y == IXMAX_VAL:
                            c, _ = pair_bits(cfg, 23, [15], [15])
                            align["ext28"].add((pos + int(c[0])) & 31)
    missing = []
    full = cfg_of(SYNTH_FULL if SYNTH_FULL in names else names[0])
    for t in SELECTABLE:
        n = 16 if t > 15 else int(full.xlen[t])
        for x in range(n):
            for y in range(n):
                for sx in ((False, True) if x else (False,)):
                    for sy in ((False, True) if y else (False,)):
                        if (t, x, y, sx, sy) not in seen_pairs:
                            missing.append(f"table {t} pair ({x}, {y}) signs ({sx}, {sy})")
    for c1t in (0, 1):
        for p in range(81):
            q, v = [], p
            for _ in range(4):
                q.append((0, 1, -1)[v % 3])
                v //= 3
            if (c1t,) + tuple(q) not in seen_quads:
                missing.append(f"count1 table {c1t} quad {q}")
    for item in sorted(lens_seen):
        if item[1] >= 2 and item not in straddle:
            missing.append(f"{item[0]} field of {item[1]} bits never straddles a word")
    missing += [f"big_values {b}" for b in BIG_VALUES if b not in bvs] + [f"{q} quads" for q in QUADS if q not in quads]
    missing += [f"scfsi pattern {p}" for p in range(16) if p not in scfsi]
    missing += [f"LSF scalefac_compress range {'500 up' if r else 'below 500'}" for r in (False, True) if r not in lsf_ranges]
    missing += [f"{s} stuffing bits" for s in STUFFING + (8 * full.n_version + 32,) if s not in stuffing]
    missing += [f"frames with padding {p} in a configuration {'with' if f else 'without'} a fractional slot" for f, p in ((True, 0), (True, 1), (False, 0)) if (f, p) not in pads]
    for key, offs in align.items():
        missing += [f"alignment item {key} at offset {o}" for o in range(32) if o not in offs]
    missing += [f"MPEG-{v}" for v in ("1", "2", "2.5") if v not in versions] + [f"{c} channels" for c in (1, 2) if c not in channels]
    missing += [f"side information of {n} bytes" for n in (13, 38) if n not in sidelens]
    missing += [f"joint stereo frame with mode_ext {m} in record and header" for m in (0, 2) if (m, m) not in mode_exts]
    return {"missing": missing, "pairs": len(seen_pairs), "quads": len(seen_quads), "stuffing": sorted(stuffing)[:50], "straddling": sorted(straddle)}
