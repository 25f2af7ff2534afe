"""TEST INFRASTRUCTURE shared by tests/test_path_matrix_cpu.py and tests/test_path_matrix_gpu.py: every quantization launch path on every
configuration family.

run_pipeline picks its kernels from the batch's shape and the device's CU count alone; the library records the choice per batch
(lhip_debug_last_paths) and two switches, read once per process, force it at small shapes: LAMEJS_HIP_PAIR_MAX_FRAMES=0 sends two-channel
batches through the persistent kernel g_quant with its tail help instead of g_quant_pair, LAMEJS_HIP_NO_FRAME_KERNEL=1 sends one-frame calls
through the separate kernels instead of g_frame.  The case list below is encoded by tests/tools/path_matrix_worker.py, a fresh process per
environment (ENVS); every stream is compared with the oracle byte for byte and every call's path set with ``expected_paths``.

Shapes are frames completed by ONE call (SEQS): 1 (g_frame, or the separate kernels when forced), 2 (the smallest pair / persistent batch),
9 (one more than a workgroup's eight waves), 17, 33, 62 / 63 / 64 (63 / 64 / 65 frame slots: g_fixup's single-to-cooperative boundary,
(nfs + 63) / 64), 150, and 0 (a remainder that completes no frame).  A stream is fed as a sequence of such calls, so the state one kernel
family saves is consumed by another.

Fractional resampling is not in the matrix: a non-integer-ratio stream takes at most call_limit() samples per call, which is less than one
frame of output, so one call never completes two frames and the family cannot reach the pair or the persistent kernel through a stream's own
calls (its one-frame calls are tests/test_fracresample_*.py).

Material is tests/tools/fuzz_gpu.material under fixed seeds (SEED + the case's index).  ``census_ok`` states what the material of each
two-channel family must contain, read from the ORACLE's bytes by tests/sideinfo.py; the CPU tier checks it with every count >= 2.

Quality 7 (the fast mode, g_quant_fast) is the family ``fast``, appended behind the 37 quality-3 cases so that those keep their seeds, their
material and their census: five two-channel and four one-channel configurations and the feature cases, on call sequences of SEQS.  Its
reference is the unchanged oracle on a quality-7 blob, which the CPU tier first holds against the unmodified reference's goldens
(tests/golden/golden_quality.json).  Two more switches belong to it: LAMEJS_HIP_NO_FAST_QUANT=1 sends a fast batch through the general
kernels, LAMEJS_HIP_QUANT_GRID_MAX=1 launches the persistent quantization kernels (g_quant_fast, g_quant) as ONE workgroup, so that a
wave or a pair of waves takes frame after frame -- the handshake, the parity of the bits words, the seeds of a wave's previous frame -- at
the matrix's small shapes.  Every call's launch (workgroups, waves, frame slots, kernel, template form: lhip_debug_read(11)) is recorded
and checked by ``check_launch``.  The census is not asked of quality-7 material: the fast mode has no scalefac_scale / subblock_gain."""
import json
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, str(ROOT / "tests" / "tools"))

SEED = 4100
ENVS = {"default": {}, "pair0": {"LAMEJS_HIP_PAIR_MAX_FRAMES": "0"}, "noframe": {"LAMEJS_HIP_NO_FRAME_KERNEL": "1"},
        "both": {"LAMEJS_HIP_PAIR_MAX_FRAMES": "0", "LAMEJS_HIP_NO_FRAME_KERNEL": "1"},
        "nofast": {"LAMEJS_HIP_NO_FAST_QUANT": "1"}, "grid1": {"LAMEJS_HIP_QUANT_GRID_MAX": "1", "LAMEJS_HIP_PAIR_MAX_FRAMES": "0"}}
SWITCHES = ("LAMEJS_HIP_PAIR_MAX_FRAMES", "LAMEJS_HIP_NO_FRAME_KERNEL", "LAMEJS_HIP_NO_FAST_QUANT", "LAMEJS_HIP_QUANT_GRID_MAX")
SHAPES = (1, 2, 9, 17, 33, 62, 63, 64, 150)
SEQS = [(9, 1, 1, 1, 64, 0, 2), (2, 33, 1, 62, 0, 17), (17, 1, 63, 0, 2, 150), (1, 150, 2, 9, 0, 33), (9, 2, 62, 1, 64, 0, 17), (33, 1, 17, 63, 0, 2, 9)]
TWO_CHANNEL = {"mpeg1": [(44100, 128), (48000, 256), (32000, 160), (44100, 320)],
               "lsf": [(22050, 64), (24000, 128), (16000, 64), (8000, 24), (11025, 64), (12000, 48)],
               "resample": [(44100, 48), (48000, 64), (32000, 8), (24000, 16)]}
ONE_CHANNEL = {"mpeg1": (44100, 128), "lsf": (22050, 64), "resample": (44100, 32)}
FEATURE_CFG = {"mpeg1": (44100, 128), "lsf": (22050, 64)}
FLAGS = {"protect": True, "copyright": True, "original": False, "private_bit": True, "emphasis": 3}
GAINS = {"scale": 0.5, "scale_left": 0.5, "scale_right": 0.25}
TWO_OUT = ("stereo", "joint", "protect", "f32gain")
# quality 7: 44100/320 keeps the polyphase bands 28..31 (the SKIP = 0 kernels), at 32 kHz band 20 straddles line 512, 22050 has one granule per frame
# (the waves of a pair never meet between granules), 44100/48 and 44100/32 resample.  One channel: the lowpass of a one-channel stream lies higher, so
# 44100/128, 22050/64 and 32000/96 keep the polyphase bands 28..31 (TableSet::skip_tail false: g_quant_fast<0, 0>) and only 44100/32 -- and the downmix
# case, a two-channel blob -- takes <0, 1>; 48000/320 has skip_tail TRUE, as every one-channel 48 kHz configuration (tests/test_path_matrix_cpu.py)
FAST_STEREO = [(44100, 128), (44100, 320), (32000, 160), (22050, 64), (44100, 48)]
FAST_MONO = [(44100, 128), (22050, 64), (44100, 32), (32000, 96)]
FAST_TWO_OUT = ("fast_stereo", "fast_joint", "fast_protect", "fast_f32gain")
BATCH_QUANT = ("QUANT_FAST", "QUANT_PAIR", "QUANT_PERSISTENT")
RESV_SHAPES = {"helpers": (8, (12, 1), 1), "nohelpers": (300, (3,), 23)}       # streams, frames per call, every n-th stream against the oracle


def cases():
    out = []

    def add(family, kind, ch, sr, kb, seq, **kw):
        out.append(dict({"name": f"{family}/{kind}/{ch}x{sr}@{kb}", "family": family, "kind": kind, "ch": ch, "sr": sr, "kb": kb, "seq": list(seq), "seed": SEED + len(out),
                         "opts": {}, "resv": None}, **kw))

    for fam, cfgs in TWO_CHANNEL.items():
        for i, (sr, kb) in enumerate(cfgs):
            add(fam, "stereo", 2, sr, kb, SEQS[i % len(SEQS)])
    for i, (fam, (sr, kb)) in enumerate(ONE_CHANNEL.items()):
        add(fam, "mono", 1, sr, kb, SEQS[i])
    for i, (fam, (sr, kb)) in enumerate(FEATURE_CFG.items()):
        add(fam, "joint", 2, sr, kb, SEQS[4 + i], opts={"joint": True})
        add(fam, "protect", 2, sr, kb, SEQS[i], opts=dict(FLAGS))
        add(fam, "f32gain", 2, sr, kb, SEQS[5 - i], opts=dict(GAINS))
        add(fam, "downmix", 2, sr, kb, SEQS[2 + i], opts={"downmix": True, "scale": 1.0})
    for fam, (sr, kb) in FEATURE_CFG.items():
        for kind, ch, opts in (("resv_mono", 1, {}), ("resv_stereo", 2, {}), ("resv_joint", 2, {"joint": True})):
            for shape in RESV_SHAPES:
                add(fam, kind, ch, sr, kb, RESV_SHAPES[shape][1], opts=dict(opts, reservoir=True), resv=shape)
                out[-1]["name"] += "/" + shape
    assert len(out) == 37          # quality 7 goes BEHIND these: a case's seed is SEED + its index
    q7 = lambda **o: dict(o, quality=7)
    for i, (sr, kb) in enumerate(FAST_STEREO):          # (from SEQS[2] on: the 150-frame calls go to 44100/128 and 44100/320, the forms <1, 1> and <1, 0>)
        add("fast", "fast_stereo", 2, sr, kb, SEQS[(i + 2) % len(SEQS)], opts=q7())
    for i, (sr, kb) in enumerate(FAST_MONO):
        add("fast", "fast_mono", 1, sr, kb, SEQS[i], opts=q7())
    add("fast", "fast_joint", 2, 44100, 128, SEQS[4], opts=q7(joint=True))
    add("fast", "fast_joint", 2, 22050, 64, SEQS[5], opts=q7(joint=True))
    add("fast", "fast_protect", 2, 44100, 128, SEQS[0], opts=q7(**FLAGS))
    add("fast", "fast_f32gain", 2, 44100, 128, SEQS[5], opts=q7(**GAINS))
    add("fast", "fast_downmix", 2, 44100, 128, SEQS[2], opts=q7(downmix=True, scale=1.0))
    add("fast", "fast_resv_stereo", 2, 44100, 128, RESV_SHAPES["helpers"][1], opts=q7(reservoir=True), resv="helpers")
    out[-1]["name"] += "/helpers"
    return out


def is_fast(c):
    return c["opts"].get("quality") == 7


def base_kind(c):
    """The kind without the fast family's prefix: what decides a case's material, its input format and its oracle blob."""
    return c["kind"][5:] if c["kind"].startswith("fast_") else c["kind"]


def select(cs, which):
    """The case lists a child can run: 'all', 'fast', or 'grid1' -- the fast cases and the quality-3 stereo and mono cases of family mpeg1."""
    keep = {"all": lambda c: True, "fast": is_fast, "grid1": lambda c: is_fast(c) or (c["family"] == "mpeg1" and c["kind"] in ("stereo", "mono"))}[which]
    return [c for c in cs if keep(c)]


def for_wavesim(cs):
    """The wave simulation's fibers are slow (tests/tools/fuzz_gpu.py: keep its cases short): shapes capped at 17 frames, each shape once per
    stream, three streams of a twelve-frame and a one-frame call for the reservoir (it always runs the count helpers, whatever the stream count)."""
    out = []
    for c in cs:
        c = dict(c)
        if c["resv"]:
            if c["resv"] != "helpers":
                continue
            c["seq"], c["streams"] = [12, 1], 3
        else:
            seq = []
            for f in c["seq"]:
                if min(f, 17) not in seq:
                    seq.append(min(f, 17))
            c["seq"] = seq
        out.append(c)
    return out


# ---- blobs, material, the oracle's bytes ----
def cfg_of(c):
    """(channels out, frame length in output samples, integer resampling ratio) of a case, from its table blob."""
    import lamejs_amd
    from protection_cases import cfg_entry
    blob = lamejs_amd.tables_blob(c["ch"], c["sr"], c["kb"], **c["opts"])
    g = lambda k: cfg_entry(blob, k)[1]
    assert g("in_samplerate") % g("out_samplerate") == 0
    return g("channels_out"), 576 * g("mode_gr"), g("in_samplerate") // g("out_samplerate")


def blob_array(blob, name, fmt):
    """A named array of an LHTB blob (16-byte header, 48-byte entries: name[32], dtype, count, offset, pad)."""
    import struct
    for k in range(struct.unpack_from("<I", blob, 8)[0]):
        e = 16 + 48 * k
        if blob[e:e + 32].split(b"\0", 1)[0].decode() == name:
            cnt, off = struct.unpack_from("<II", blob, e + 36)
            return struct.unpack_from(f"<{cnt}{fmt}", blob, off)
    raise KeyError(name)


def skip_tail_of(c):
    """The rule of lhip_tables.h (TableSet::skip_tail) on the case's own blob: the lowpass zeroes the polyphase bands 28..31, so the device launches
    the SKIP = 1 form of the batch quantization kernels."""
    import lamejs_amd
    if c["name"] not in _skip_tail:
        af = blob_array(lamejs_amd.tables_blob(c["ch"], c["sr"], c["kb"], **c["opts"]), "amp_filter", "f")
        _skip_tail[c["name"]] = all(float(af[b]) < 1e-12 for b in (28, 29, 30, 31))
    return _skip_tail[c["name"]]


_skip_tail = {}



def fast_form(c):
    """(PAIR, SKIP) of the g_quant_fast launch a fast case takes: PAIR by its output channels."""
    return (1 if c["kind"] in FAST_TWO_OUT else 0, 1 if skip_tail_of(c) else 0)


def plan_calls(seq, frame, ratio, rng):
    """Input samples per call so that call i completes exactly seq[i] frames (lhip_batch.h: call_frames, rs_outputs)."""
    mf_needed, mf, n_in, lens = 1024 + frame - 272, 528, 0, []      # (a fresh stream holds 528 samples: MF_INIT, the encoder delay)
    outs = lambda n: (n - 16 + ratio - 1) // ratio if n > 16 else 0
    for F in seq:
        total = mf_needed + (F - 1) * frame + int(rng.integers(0, frame - 2)) if F > 0 else mf + max(1, (mf_needed - mf) // 2)
        assert (F > 0 or total < mf_needed) and total > mf
        n = max(1, (total - mf) * ratio - 2 * ratio - 16) if ratio > 1 else total - mf
        while ratio > 1 and outs(n_in + n) - outs(n_in) != total - mf:
            n += 1
        lens.append(n)
        n_in += n
        mf = total - frame * F
    return lens


def stream_pcm(c, seed, n):
    """Whole-number planes (int64) the encoder under test is fed, and the Int16 planes the oracle is fed for them."""
    from fuzz_gpu import material
    from inputmix_cases import premix
    rng = np.random.default_rng(seed)
    L, R = material(rng, n, c["ch"])
    if c["opts"].get("joint"):          # strongly correlated channels in the first half of the stream: the M/S decision goes both ways
        h = n // 2
        d = R[:h].astype(np.int32) >> 3
        a = L[:h].astype(np.int32)
        L, R = L.copy(), R.copy()
        L[:h], R[:h] = np.clip(a + d, -32768, 32767).astype(np.int16), np.clip(a - d, -32768, 32767).astype(np.int16)
    l, r = L.astype(np.int64), None if R is None else R.astype(np.int64)
    if base_kind(c) == "f32gain":                          # scale 0.5, then 0.5 / 0.25, on multiples of four / eight: the premix is whole numbers
        l, r = l & ~3, r & ~7
        ol, orr = premix(l, r, 2, GAINS["scale"], GAINS["scale_left"], GAINS["scale_right"])
    elif base_kind(c) == "downmix":                        # l + r even
        r = r - ((l + r) & 1)
        r[r < -32768] += 2
        ol, orr = premix(l, r, 1, 1.0)
    else:
        return l, r, L, R
    o16 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int16)
    assert np.array_equal(o16(ol).astype(np.float32), ol) and (orr is None or np.array_equal(o16(orr).astype(np.float32), orr))
    return l, r, o16(ol), o16(orr)


def oracle_blob(c):
    import lamejs_amd
    o = dict(c["opts"])
    q = {"quality": o["quality"]} if "quality" in o else {}      # (where the options are rewritten, the quality stays)
    if base_kind(c) == "f32gain":
        o = dict({"scale": 1.0}, **q)
    ch = c["ch"]
    if base_kind(c) == "downmix":
        o, ch = dict({"scale": 1.0}, **q), 1
    return lamejs_amd.tables_blob(ch, c["sr"], c["kb"], **o)


def oracle_stream(blob, L, R):
    """The oracle on this blob: all samples in one call, then its flush (any chunking gives the same stream)."""
    from oracle_py import oracle_calls
    (part,), tail = oracle_calls(blob, L, R, [len(L)])
    return part + tail


def case_streams(c):
    """[(stream index, call lengths, l, r, oracle's bytes or None)] of a case; the oracle runs for the streams that are checked."""
    C, frame, ratio = cfg_of(c)
    blob = oracle_blob(c)
    S, every = (c.get("streams") or RESV_SHAPES[c["resv"]][0], RESV_SHAPES[c["resv"]][2]) if c["resv"] else (1, 1)
    out = []
    for s in range(S):
        seed = c["seed"] * 1000 + s
        lens = plan_calls(c["seq"], frame, ratio, np.random.default_rng(seed))
        l, r, ol, orr = stream_pcm(c, seed, sum(lens))
        out.append((s, lens, l, r, oracle_stream(blob, ol, orr) if s % every == 0 else None))
    return out


# ---- the expectation table ----
def expected_paths(c, C, ratio, S, F, flush, env, backend, num_cus):
    """The path set of one batch of S streams completing F frames each (SMALL_CALL left out: it follows the byte sizes, not the shape)."""
    no_frame = env.get("LAMEJS_HIP_NO_FRAME_KERNEL") == "1"
    resv = bool(c["resv"])
    if F <= 1 and not no_frame and S <= num_cus:
        return {"FRAME_RESV" if resv else "FRAME"} | ({"RESV_FLUSH"} if resv and flush else set())
    p = {"SEPARATE"} | ({"PREP"} if ratio != 1 else set()) | ({"PSY4"} if c["opts"].get("joint") else set())
    if resv:      # the count helpers: the device decides by S <= CUs; the wave simulation always runs them, the scalar one has none
        return p | {"RESV_STREAM_HELPERS" if (backend == "wavesim" or (backend == "gpu" and S <= num_cus)) else "RESV_STREAM_NOHELPERS"}
    nfs, pm = S * (F + 1), env.get("LAMEJS_HIP_PAIR_MAX_FRAMES")
    pair_max = -1 if backend == "hostsim" else int(pm) if pm is not None else (6 * num_cus if backend == "gpu" else 12)
    if is_fast(c) and env.get("LAMEJS_HIP_NO_FAST_QUANT") != "1":      # g_quant_fast at every batch size, whatever the pair threshold says
        p |= {"QUANT_FAST"}
    else:
        p |= {"QUANT_PAIR" if C == 2 and nfs <= pair_max else "QUANT_PERSISTENT"}
    if backend == "gpu" and S * F > 0:      # (the simulations repair in a host loop: no g_fixup launch, no bit)
        p |= {"FIXUP_SINGLE" if (nfs + 63) // 64 == 1 else "FIXUP_COOP"}
    return p


def required_cells(cs, env, backend, num_cus):
    """(required, impossible): sets of cells that must / cannot be observed in this environment.  A cell is (what, path, shape) with `what` a
    case name, a family, '2ch' (the cases with two output channels and no reservoir) or '*', and shape a frame count or None (any)."""
    req, imp = set(), {}
    forced = env.get("LAMEJS_HIP_PAIR_MAX_FRAMES") == "0"
    no_frame = env.get("LAMEJS_HIP_NO_FRAME_KERNEL") == "1"
    pair_max = -1 if backend == "hostsim" else 0 if forced else (6 * num_cus if backend == "gpu" else 12)
    two = [c for c in cs if c["kind"] in TWO_OUT]
    shapes = sorted({f for c in two for f in c["seq"] if f >= 2})
    for f in shapes:
        if f + 1 <= pair_max:
            req.add(("2ch", "QUANT_PAIR", f))
            imp[("2ch", "QUANT_PERSISTENT", f)] = "two channels: the batch is below the pair threshold of this environment"
        else:
            req.add(("2ch", "QUANT_PERSISTENT", f))
            imp[("2ch", "QUANT_PAIR", f)] = "forced off (LAMEJS_HIP_PAIR_MAX_FRAMES=0), above the threshold, or a simulation without the pair program"
    for c in two:          # every two-channel configuration and feature, at some shape >= 2
        fs = [f for f in c["seq"] if f >= 2]
        if any(f + 1 <= pair_max for f in fs):
            req.add((c["name"], "QUANT_PAIR", None))
        if any(f + 1 > pair_max for f in fs):
            req.add((c["name"], "QUANT_PERSISTENT", None))
    for c in cs:
        if not c["resv"] and c["kind"] in ("mono", "downmix"):      # one channel out: g_quant whatever the switches say
            req.add((c["name"], "QUANT_PERSISTENT", None))
            imp[(c["name"], "QUANT_PAIR", None)] = "one channel always takes g_quant"
    # quality 7: g_quant_fast at every shape >= 2 and, with the separate kernels forced, on one frame; with LAMEJS_HIP_NO_FAST_QUANT=1 the rule above
    nofast = env.get("LAMEJS_HIP_NO_FAST_QUANT") == "1"
    quant_of = lambda f, two_ch: "QUANT_FAST" if not nofast else "QUANT_PAIR" if two_ch and f + 1 <= pair_max else "QUANT_PERSISTENT"
    fast = [c for c in cs if is_fast(c) and not c["resv"]]
    for f in sorted({f for c in fast if c["kind"] in FAST_TWO_OUT for f in c["seq"] if f >= 2}):
        req.add(("fast2ch", quant_of(f, True), f))
        for q in set(BATCH_QUANT) - {quant_of(f, True)}:
            imp[("fast2ch", q, f)] = "quality 7: g_quant_fast unless LAMEJS_HIP_NO_FAST_QUANT=1, then the pair threshold of this environment"
    for c in fast:
        took = {quant_of(f, c["kind"] in FAST_TWO_OUT) for f in c["seq"] if f >= 2}
        req |= {(c["name"], q, None) for q in took}
        if no_frame:
            req.add((c["name"], quant_of(1, c["kind"] in FAST_TWO_OUT), 1))
        for q in set(BATCH_QUANT) - took - ({quant_of(1, c["kind"] in FAST_TWO_OUT)} if no_frame else set()):
            imp[(c["name"], q, None)] = "quality 7: one batch quantization kernel per shape, see fast2ch"
    if fast and no_frame and not nofast:
        req.add(("fast", "QUANT_FAST", 1))      # the separate kernels on one frame: two frame slots, one of them a stream's slot -1
    if nofast:
        imp[("*", "QUANT_FAST", None)] = "LAMEJS_HIP_NO_FAST_QUANT=1"
    else:
        for c in cs:
            if not is_fast(c):
                imp[(c["name"], "QUANT_FAST", None)] = "not a quality-7 stream"
    for c in cs:
        if is_fast(c) and c["resv"]:
            for q in BATCH_QUANT:
                imp[(c["name"], q, None)] = "the bit reservoir: g_resv_stream, no batch quantization kernel"
    fams = sorted({c["family"] for c in cs if not c["resv"]})
    for fam in fams:
        req.add((fam, "SEPARATE" if no_frame else "FRAME", 1))
        imp[(fam, "FRAME" if no_frame else "SEPARATE", 1)] = "LAMEJS_HIP_NO_FRAME_KERNEL decides one-frame calls"
        if backend == "gpu":
            fam_shapes = {f for c in cs if c["family"] == fam and not c["resv"] for f in c["seq"]}
            for f in fam_shapes & {62, 63}:
                req.add((fam, "FIXUP_SINGLE", f))
            for f in fam_shapes & {64, 150}:
                req.add((fam, "FIXUP_COOP", f))
        else:
            imp[(fam, "FIXUP_SINGLE", None)] = imp[(fam, "FIXUP_COOP", None)] = "the simulations repair in a host loop"
    if any(c["family"] == "resample" for c in cs):
        req.add(("resample", "PREP", None))
    if any(c["resv"] for c in cs):
        for fam in [fam for fam in FEATURE_CFG if any(c["resv"] and c["family"] == fam for c in cs)]:
            req.add((fam, "FRAME_RESV" if not no_frame else "SEPARATE", 1))
            imp[(fam, "RESV_FLUSH", None)] = ("g_resv_flush behind the one-frame program needs a flush that completes at most one frame; a stream's flush pads the "
                                              "encoder delay and a whole frame (576 + 1152 samples and the remainder): it always completes two frames or more")
            helpers = backend == "wavesim" or (backend == "gpu" and RESV_SHAPES["helpers"][0] <= num_cus)
            nohelpers = backend == "hostsim" or (backend == "gpu" and RESV_SHAPES["nohelpers"][0] > num_cus)
            for flag, path in ((helpers, "RESV_STREAM_HELPERS"), (nohelpers, "RESV_STREAM_NOHELPERS")):
                if flag:
                    req.add((fam, path, None))
                else:
                    imp[(fam, path, None)] = "the scalar simulation has no count helpers, the wave simulation always runs them; the device decides by streams <= CUs"
    if any(c["kind"] in ("joint", "resv_joint") for c in cs):
        req.add(("*", "PSY4", None))
    return req, imp


def observed_cells(records):
    obs = set()
    for r in records:
        if "paths" not in r:
            continue
        for p in r["paths"]:
            for what in (r["case"], r["family"], "*") + (("2ch",) if r["kind"] in TWO_OUT else ()) + (("fast2ch",) if r["kind"] in FAST_TWO_OUT else ()):
                obs.add((what, p, r["frames"]))
                obs.add((what, p, None))
    return obs


# ---- what the material must contain (read from the oracle's bytes) ----
def census_ok(fam, cen, joint_cen, at_least=1):
    bad = []
    need = lambda ok, what: bad.append(f"{fam}: {what}") if not ok else None
    for bt in range(4):
        need(cen["block_type"][bt] >= at_least, f"block type {bt}: {cen['block_type'][bt]}")
    for t in range(2):
        need(cen["count1table"][t] >= at_least, f"count1 table {t}: {cen['count1table'][t]}")
    need(cen["esc_table"] >= at_least, f"ESC tables: {cen['esc_table']}")
    need(cen["scalefac_scale"] >= at_least, f"scalefac_scale: {cen['scalefac_scale']}")
    need(cen["subblock_gain"] >= at_least, f"subblock_gain: {cen['subblock_gain']}")
    need(cen["empty"] >= at_least, f"part2_3_length = 0: {cen['empty']}")
    if fam == "mpeg1":
        need(cen["preflag"] >= at_least, f"preflag: {cen['preflag']}")
        need(cen["scfsi"] >= at_least, f"scfsi: {cen['scfsi']}")
    if joint_cen is not None:
        for me in (0, 2):
            need(joint_cen["mode_ext"].get(me, 0) >= at_least, f"joint mode_ext {me}: {joint_cen['mode_ext'].get(me, 0)}")
    return bad


# ---- the children ----
HIP_ERROR_WORDS = ("hipError", "HIP error", "illegal memory access", "HSA_STATUS_ERROR", "Memory access fault")
FATAL_STATUS = {124, 134, 137, 139, -6, -9, -11}


def launch_record(lib):
    """lhip_debug_read(11): the speculative quantization launch of this thread's last batch, or None when it launched none."""
    import ctypes
    v = (ctypes.c_int32 * 8)()
    assert lib.lhip_debug_read(11, v, 32) == 32
    if not any(v):
        return None
    assert v[3] in (1, 2, 3) and v[6] == 0 and v[7] == 0, list(v)
    return {"wg": v[0], "waves": v[1], "nfs": v[2], "kernel": (None, "fast", "pair", "persistent")[v[3]], "pair": v[4], "skip": v[5]}


def run_child(env_name, backend, limit, args=()):
    """One environment in a fresh process (the switches are read once per process), under a time limit of its own; returns (status, records, text).
    ``args``: the CU count (gpu) and, optionally, ``--cases=fast|grid1`` (``select``)."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES + ("PATH_MATRIX_ONLY",)}      # (the by-hand filter of the worker never reaches a test's child)
    env.update(ENVS[env_name])
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(ROOT / "tests" / "tools" / "path_matrix_worker.py"), backend, env_name] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    recs = []
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            recs.append(json.loads(line))
    return r.returncode, recs, r.stdout[-3000:] + r.stderr[-3000:], child_is_fatal(r.returncode, r.stdout + r.stderr)


def child_is_fatal(status, text):
    return status in FATAL_STATUS or any(w in text for w in HIP_ERROR_WORDS)


def check_records(cs, recs, env_name, backend, num_cus):
    """The three assertions on one child's records; returns a list of failures (empty = fine)."""
    env, bad = ENVS[env_name], []
    done = [r for r in recs if r.get("done")]
    if len(done) != 1 or done[0]["cases"] != len(cs):
        return [f"{env_name}: the worker did not finish its case list ({done})"]
    for r in recs:
        if r.get("diff") is not None:
            bad.append(f"{env_name}: MISMATCH {r['case']} stream {r.get('stream', 0)} call {r['call']}: first differing byte {r['diff']} (paths {r.get('paths')})")
        if "expected" in r and set(r["paths"]) - {"SMALL_CALL"} != set(r["expected"]):
            bad.append(f"{env_name}: {r['case']} call {r['call']} ({r['frames']} frames): paths {sorted(r['paths'])}, expected {sorted(r['expected'])}")
        if r.get("planned") is not None and r["planned"] != r["frames"]:
            bad.append(f"{env_name}: {r['case']} call {r['call']}: {r['frames']} frames, planned {r['planned']}")
    obs = observed_cells(recs)
    req, imp = required_cells(cs, env, backend, num_cus)
    bad += [f"{env_name}: never observed {cell}" for cell in sorted(req - obs, key=str)]
    bad += [f"{env_name}: observed {cell}, listed as impossible ({why})" for cell, why in imp.items() if cell in obs]
    return bad + check_launch(cs, recs, env_name, backend, num_cus)


def check_launch(cs, recs, env_name, backend, num_cus):
    """Every call's launch record against its path set, its shape and the backend's grid rule; over the fast cases, every (PAIR, SKIP) form the case
    list reaches was launched; with LAMEJS_HIP_QUANT_GRID_MAX=1 on the device, ``check_one_workgroup``."""
    by_name, bad = {c["name"]: c for c in cs}, []
    forms = set()
    cap = ENVS[env_name].get("LAMEJS_HIP_QUANT_GRID_MAX") if backend == "gpu" else None      # (the switch exists in the HIP build only)
    for r in recs:
        if "paths" not in r:
            continue
        c, L, where = by_name[r["case"]], r["launch"], f"{env_name}: {r['case']} call {r['call']} ({r['frames']} frames)"
        bit = set(r["paths"]) & set(BATCH_QUANT)
        if bit != ({"QUANT_" + L["kernel"].upper()} if L else set()):
            bad.append(f"{where}: launch record {L}, paths {sorted(r['paths'])}")
            continue
        if not L:
            continue
        S = r.get("nstreams", 1)
        ceil = lambda per: (L["nfs"] + per - 1) // per
        if backend == "hostsim":
            want = (1, 3)
        elif backend == "wavesim":
            want = (L["nfs"], 2) if L["kernel"] == "pair" else (1, 8)
        elif L["kernel"] == "pair":
            want = (L["nfs"], 2)
        elif L["kernel"] == "fast":          # as many workgroups as the device holds of the kernel, at least one per CU: exact while the batch is below that
            want = (ceil(4 if L["pair"] else 8), 8) if ceil(4 if L["pair"] else 8) <= num_cus else (L["wg"], 8)
        else:
            want = (min(ceil(8), 2 * num_cus), 8)
        if cap is not None and L["kernel"] != "pair":
            want = (min(want[0], int(cap)), want[1])
        form = (fast_form(c) if L["kernel"] == "fast" else (1 if L["kernel"] == "pair" else 0, 1 if skip_tail_of(c) else 0))
        if (L["wg"], L["waves"]) != want or L["nfs"] != S * (r["frames"] + 1) or (L["pair"], L["skip"]) != form:
            bad.append(f"{where}: launch record {L}, expected (workgroups, waves) {want}, {S * (r['frames'] + 1)} frame slots, form {form}")
        if L["kernel"] == "fast":
            forms.add((L["pair"], L["skip"]))
    if ENVS[env_name].get("LAMEJS_HIP_NO_FAST_QUANT") != "1":
        reach = {fast_form(c) for c in cs if is_fast(c) and not c["resv"]}
        bad += [f"{env_name}: g_quant_fast form (PAIR, SKIP) = {f} never launched" for f in sorted(reach - forms)]
    elif forms:
        bad.append(f"{env_name}: g_quant_fast launched {sorted(forms)}")
    if cap == "1":
        bad += check_one_workgroup(recs, env_name)
    return bad


def check_one_workgroup(recs, env_name, max_shape=150):
    """One workgroup per persistent quantization launch, and calls in which -- by counting alone -- some pair of waves (two channels: four pairs) or
    some wave (one channel: eight waves) took at least two frames; with the full shapes, 150 frames: 37 rounds and more per pair."""
    L = [(r, r["launch"]) for r in recs if r.get("launch") and r["launch"]["kernel"] in ("fast", "persistent")]
    bad = [f"{env_name}: {r['case']} call {r['call']}: {l['wg']} workgroups" for r, l in L if l["wg"] != 1]
    n = lambda kernel, pair, frames: sum(1 for r, l in L if l["kernel"] == kernel and l["pair"] == pair and r.get("nstreams", 1) == 1 and r["frames"] >= frames)
    need = {"fast calls of >= 9 frames on two channels": n("fast", 1, 9), "fast calls of >= 17 frames on one channel": n("fast", 0, 17),
            f"fast calls of {max_shape} frames on two channels": n("fast", 1, max_shape), f"fast calls of {max_shape} frames on one channel": n("fast", 0, max_shape),
            "g_quant calls of >= 9 frames (one workgroup and its tail help)": sum(1 for r, l in L if l["kernel"] == "persistent" and r["kind"] in TWO_OUT and r["frames"] >= 9)}
    return bad + [f"{env_name}: no {what}" for what, k in need.items() if k == 0]

