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
two-channel family must contain, read from the ORACLE's bytes by tests/sideinfo.py; the CPU tier checks it with every count >= 2."""
import json
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, str(ROOT / "tests" / "tools"))

SEED = 4100
ENVS = {"default": {}, "pair0": {"LAMEJS_HIP_PAIR_MAX_FRAMES": "0"}, "noframe": {"LAMEJS_HIP_NO_FRAME_KERNEL": "1"},
        "both": {"LAMEJS_HIP_PAIR_MAX_FRAMES": "0", "LAMEJS_HIP_NO_FRAME_KERNEL": "1"}}
SWITCHES = ("LAMEJS_HIP_PAIR_MAX_FRAMES", "LAMEJS_HIP_NO_FRAME_KERNEL")
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
    return out


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
    if c["kind"] == "f32gain":                             # scale 0.5, then 0.5 / 0.25, on multiples of four / eight: the premix is whole numbers
        l, r = l & ~3, r & ~7
        ol, orr = premix(l, r, 2, GAINS["scale"], GAINS["scale_left"], GAINS["scale_right"])
    elif c["kind"] == "downmix":                           # l + r even
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
    if c["kind"] == "f32gain":
        o = {"scale": 1.0}
    ch = c["ch"]
    if c["kind"] == "downmix":
        o, ch = {"scale": 1.0}, 1
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
        for fam in FEATURE_CFG:
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
            for what in (r["case"], r["family"], "*") + (("2ch",) if r["kind"] in TWO_OUT else ()):
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


def run_child(env_name, backend, limit, args=()):
    """One environment in a fresh process (the switches are read once per process), under a time limit of its own; returns (status, records, text)."""
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
    return bad

