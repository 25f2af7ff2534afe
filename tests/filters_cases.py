"""TEST INFRASTRUCTURE shared by tests/test_filters_cpu.py and tests/test_filters_gpu.py: the output sample rate and the polyphase filter settings
(``out_samplerate``, ``lowpass``, ``lowpass_width``, ``highpass``, ``highpass_width``).  Yardsticks: the unmodified reference's bytes and resolved values
with the five gfp fields set (tests/golden/golden_filters.json, tests/tools/gen_golden_filters.js), and -- only once it has reproduced those goldens
itself -- the unchanged CPU oracle, which reads amp_filter, the resampler and the stream's rate from the blob, for a seeded random family.  Four cases run
through the launch-path environments of tests/path_matrix_cases.py in fresh child processes (``python tests/filters_cases.py matrix <backend> <env>``)."""
import ctypes
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np

from conftest import ROOT
from golden_cases import check_stream, feed_calls, load, pinned

PY_NAME = {"outSampleRate": "out_samplerate", "lowpass": "lowpass", "lowpassWidth": "lowpass_width", "highpass": "highpass", "highpassWidth": "highpass_width"}
CLI_WORD = {"outSampleRate": "outrate", "lowpass": "lowpass", "lowpassWidth": "lowpasswidth", "highpass": "highpass", "highpassWidth": "highpasswidth"}
BATCH_QUANT_BITS = {"QUANT_FAST", "QUANT_PAIR", "QUANT_PERSISTENT"}
# the launch-path matrix: the states no configuration without the options reaches
MATRIX_CASES = ("hp2000_w500_128",            # zero bands at the bottom of the spectrum
                "lp_off_128",                 # a full 32-band spectrum at 128 kbps: the full-round kernels at a bitrate that always took the round-skip form
                "lp16000_320",                # 320 kbps in the round-skip form
                "out22050_44100_320")         # MPEG-2 frames from 44.1 kHz input, 320 clamped to 160
MATRIX_ENVS = ("default", "pair0", "noframe", "grid1")


def goldens():
    return load("golden_filters")["cases"]


def filter_opts(settings):
    return {PY_NAME[k]: v for k, v in settings.items()}


def case_opts(c, host_side=True):
    """The Python keywords of a case; ``host_side=False`` leaves out info_tag / replay_gain (the oracle's blob)."""
    o = {"joint": bool(c.get("jointStereo")), "reservoir": bool(c.get("reservoir")), "downmix": bool(c.get("downmix")), "protect": bool(c.get("protect")), "quality": c.get("quality", 3)}
    if host_side:
        o.update(info_tag=bool(c.get("infoTag")), replay_gain=bool(c.get("replayGain")))
    return dict(o, **filter_opts(c["settings"]))


def case_pcm(c):
    from quality_cases import material
    return pinned(material(c["corpus"], c["nsamples"], c["channels"]), c["pcm_md5"])


def make_encoder(lib, c, **kw):
    import lamejs_amd
    return lamejs_amd.Mp3Encoder(c["channels"], c["samplerate"], c["kbps"], lib=lib, **dict(case_opts(c), **kw))


def amp_filter_of(c):
    return np.array(c["amp_filter_bits"], dtype="<u4").view("<f4")


def expected_skip_tail(c):
    """The rule of lhip_tables.h (TableSet::skip_tail) on the values the REFERENCE resolved."""
    af = amp_filter_of(c)
    return all(float(af[b]) < 1e-12 for b in (28, 29, 30, 31))


def blob_cfg(blob, key):
    from protection_cases import cfg_entry
    return cfg_entry(blob, key)[1]


def blob_array(blob, name, fmt):
    from path_matrix_cases import blob_array as ba
    return ba(blob, name, fmt)


def launch_record(lib):
    from path_matrix_cases import launch_record as lr
    return lr(lib)


def run_golden_case(lib, c, lens=None, on_call=None):
    """The case through encodeBuffer in calls of ``lens`` samples (default: its own calls), then flush, against the golden.  Returns the union of the
    path names its calls took.  ``on_call(i, samples, paths)`` sees every call.  An info_tag stream's placeholder is taken off the front first: the audio
    behind it is what the reference recorded."""
    import lamejs_amd
    L, R = case_pcm(c)
    enc = make_encoder(lib, c)
    seen = set()
    try:
        def call(i, l, r):
            out = enc.encodeBuffer(l, r)
            p = lamejs_amd.last_batch_paths(lib)
            if on_call:
                on_call(i, len(l), p)
            seen.update(p)
            return out
        parts = feed_calls(lens or c["call_lens"], L, R, call)
        tail = enc.flush()
        if c.get("infoTag"):
            cut = enc.stream_info()["tag_bytes"]
            k = next(i for i, p in enumerate(parts) if p)
            assert cut > 0 and len(parts[k]) >= cut
            parts[k] = parts[k][cut:]
        resv = bool(c.get("reservoir"))      # (a reservoir stream's split into calls and flush is the library's: checked as a whole)
        check_stream(c, parts, tail, call_bytes=lens is None and not resv, enc_md5=not resv, flush_md5=not resv, all_md5=resv)
        assert hashlib.md5(b"".join(parts) + tail).hexdigest() == c["all_md5"], c["name"]
        if resv:
            assert not (BATCH_QUANT_BITS & seen), (c["name"], sorted(seen))
        return seen
    finally:
        enc.close()


def encode_whole(lib, channels, samplerate, kbps, L, R, lens=None, **opts):
    import lamejs_amd
    enc = lamejs_amd.Mp3Encoder(channels, samplerate, kbps, lib=lib, **opts)
    try:
        parts = feed_calls(lens or [len(L)], L, R, lambda i, l, r: enc.encodeBuffer(l, r))
        return b"".join(parts) + enc.flush()
    finally:
        enc.close()


# ---- the unchanged oracle on a blob built with the options ----
def oracle_takes(c):
    """The oracle encodes Int16 planes as they are: it has no downmix."""
    return not c.get("downmix")


def oracle_stream(cfg, L, R, lens, **opts):
    import lamejs_amd
    from oracle_py import oracle_calls
    ch, sr, kb = cfg
    return oracle_calls(lamejs_amd.tables_blob(ch, sr, kb, **opts), L, R if ch == 2 else None, lens)


def oracle_reproduces(c):
    L, R = case_pcm(c)
    parts, tail = oracle_stream((c["channels"], c["samplerate"], c["kbps"]), L, R, c["call_lens"], **case_opts(c, host_side=False))
    resv = bool(c.get("reservoir"))
    check_stream(c, parts, tail, call_bytes=not resv, enc_md5=not resv, flush_md5=not resv, all_md5=resv)
    return True


# ---- the seeded random family: reference = the oracle (only behind oracle_reproduces on every golden it takes) ----
# (channels, input rate, kbps, output rate): one and two channels; MPEG-1, MPEG-2 and MPEG-2.5 streams; ratios 1, 2, 3, 4 and 6
FAMILY_CONFIGS = [(2, 44100, 128, 44100), (1, 44100, 64, 44100), (2, 48000, 192, 48000), (2, 32000, 96, 32000), (2, 44100, 96, 44100), (1, 48000, 112, 48000),
                  (2, 44100, 64, 22050), (1, 24000, 32, 24000), (2, 48000, 64, 16000), (2, 16000, 32, 16000), (1, 44100, 32, 11025), (2, 48000, 24, 12000),
                  (1, 48000, 16, 8000), (2, 11025, 24, 11025), (2, 44100, 320, 22050), (2, 88200, 160, 44100)]


def highpass_minimum(out):
    """The smallest highpass + width tables.js accepts for a stream of ``out`` Hz (Lame.js:508-515)."""
    m = 1
    while 2.0 * m / out < 0.9 * (0.75 / 31.0):
        m += 1
    return m


def family(seed, count=16):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        ch, sr, kb, o = FAMILY_CONFIGS[i % len(FAMILY_CONFIGS)]
        s = {"out_samplerate": o}
        kind = int(rng.randint(0, 4))          # 0: lowpass; 1: highpass; 2: both; 3: no lowpass, a highpass
        lp = int(rng.randint(o // 8, o // 2 + 1))
        if kind in (0, 2):
            s["lowpass"] = lp
            if rng.randint(0, 2):
                s["lowpass_width"] = int(rng.randint(0, lp // 2))
        if kind == 3:
            s["lowpass"], lp = -1, o // 2
        if kind in (1, 2, 3):
            lo = highpass_minimum(o)
            top = max(lo + 1, min(lp, o // 4) // 2)          # (kind 1: below the automatic lowpass as well, whatever it is -- it is never under out / 8)
            if kind == 1:
                top = max(lo + 1, o // 20)
            s["highpass"] = int(rng.randint(lo, top + 1))
            if rng.randint(0, 2):
                s["highpass_width"] = int(rng.randint(0, s["highpass"] // 2 + 1))
        frame, ratio = (1152 if o > 24000 else 576), sr // o
        n = int(rng.randint(8 * frame * ratio, 14 * frame * ratio + 1))
        cuts, p = [], 0
        while p < n:                      # random call cuts: single samples, odd lengths, several frames at once
            m = min(int(rng.choice([1, 17, 777, 1152, 2305, 4096, n])), n - p)
            cuts.append(m)
            p += m
        out.append({"cfg": (ch, sr, kb), "opts": s, "corpus": ["bursts", "sine", "silent3"][int(rng.randint(0, 3))], "seed": int(rng.randint(1, 1 << 30)), "n": n, "lens": cuts})
    return out


def family_check(lib, cases):
    """Every case of the family on ``lib`` against the oracle: none is skipped (a setting tables.js refuses fails the check)."""
    import lamejs_amd
    from quality_cases import material
    for fc in cases:
        ch, sr, kb = fc["cfg"]
        L, R = material(fc["corpus"], fc["n"], ch, fc["seed"])
        parts, tail = oracle_stream(fc["cfg"], L, R, fc["lens"], **fc["opts"])
        got = encode_whole(lib, ch, sr, kb, L, R, lens=fc["lens"], **fc["opts"])
        assert got == b"".join(parts) + tail, (fc["cfg"], fc["opts"], fc["corpus"], fc["lens"][:6], len(got))
    return len(cases)


def mixed_batch(lib, names, G=None):
    """One encode_streams over encoders of DIFFERENT option sets (the goldens ``names``): each stream gets its golden's bytes.  Returns the path set."""
    import lamejs_amd
    by = {c["name"]: c for c in (G or goldens())}
    cs = [by[n] for n in names]
    pcms = [case_pcm(c) for c in cs]
    encs = [make_encoder(lib, c) for c in cs]
    try:
        got = lamejs_amd.encode_streams(encs, [p[0] for p in pcms], [p[1] if p[1] is not None else p[0] for p in pcms], flush=False)
        paths = lamejs_amd.last_batch_paths(lib)
        got = [g + e.flush() for g, e in zip(got, encs)]
    finally:
        for e in encs:
            e.close()
    for c, g in zip(cs, got):
        assert hashlib.md5(g).hexdigest() == c["all_md5"], c["name"]
    return paths


def check_js_result(res, G):
    """The JSON line of tests/js_filters_check.js."""
    assert res["mismatches"] == 0 and res["goldens"] == len(G) and res["range_errors"] == 23 and res["refusals"] == 2, res
    assert set(res["families"]) >= {"goldens", "batch_mixed", "refusals"} and res["families"]["batch_mixed"]["calls"] == 5
    assert res["live"] in (0, 3) and (res["live"] == 0 or res["families"]["live"]["calls"] == 30)


# ---- the four matrix cases in a child process per environment (the switches are read once per process) ----
def matrix_child(backend, env_name):
    """Runs in the child: every matrix case in its own calls, in one call, and in a call of five frames' input followed by the rest; one record per call."""
    import libs
    import path_matrix_cases as pm
    env = {k: os.environ[k] for k in pm.SWITCHES if k in os.environ}
    assert env == pm.ENVS[env_name], (env, env_name)
    lib = libs.gpu_library() if backend == "gpu" else libs.sim_library(backend)
    by = {c["name"]: c for c in goldens()}
    for name in MATRIX_CASES:
        c = by[name]
        per = c["call_lens"][0]
        for how, lens in (("own", None), ("whole", [c["nsamples"]]), ("split", [5 * per + 3, c["nsamples"] - 5 * per - 3])):
            def on_call(i, n, paths, how=how):
                a, b, d = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
                lib.lhip_last_batch_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(d))
                print(json.dumps({"case": name, "how": how, "call": i, "samples": n, "frames": int(a.value), "paths": sorted(paths), "launch": launch_record(lib)}), flush=True)
            run_golden_case(lib, c, lens=lens, on_call=on_call)
    print(json.dumps({"done": True, "cases": len(MATRIX_CASES)}), flush=True)


def run_matrix(backend, env_name, limit):
    """One environment in a fresh process under a time limit of its own; returns (status, records, text, fatal)."""
    import path_matrix_cases as pm
    env = {k: v for k, v in os.environ.items() if k not in pm.SWITCHES}
    env.update(pm.ENVS[env_name])
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(ROOT / "tests" / "filters_cases.py"), "matrix", backend, env_name]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    return r.returncode, recs, r.stdout[-2000:] + r.stderr[-3000:], pm.child_is_fatal(r.returncode, r.stdout + r.stderr)


def run_nofast(backend, limit=600):
    """The quality-7 goldens in a child process with the general kernels forced; returns the child's JSON result."""
    import path_matrix_cases as pm
    env = dict({k: v for k, v in os.environ.items() if k not in pm.SWITCHES}, LAMEJS_HIP_NO_FAST_QUANT="1")
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, str(ROOT / "tests" / "filters_cases.py"), "nofast", backend], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def check_matrix(recs, env_name, backend):
    """Every call's launch (lhip_debug_read(11)) and path set (lhip_debug_last_paths) against the environment and the case's expected form."""
    import path_matrix_cases as pm
    env, bad = pm.ENVS[env_name], []
    by = {c["name"]: c for c in goldens()}
    if [r for r in recs if r.get("done")] != [{"done": True, "cases": len(MATRIX_CASES)}]:
        return [f"{env_name}: the child did not finish"]
    no_frame, forced, cap = env.get("LAMEJS_HIP_NO_FRAME_KERNEL") == "1", env.get("LAMEJS_HIP_PAIR_MAX_FRAMES") == "0", env.get("LAMEJS_HIP_QUANT_GRID_MAX")
    seen = {n: set() for n in MATRIX_CASES}
    for r in (r for r in recs if "paths" in r):
        c, L, paths, where = by[r["case"]], r["launch"], set(r["paths"]), f"{env_name}: {r['case']} {r['how']} call {r['call']} ({r['frames']} frames)"
        skip = 1 if expected_skip_tail(c) else 0
        if (BATCH_QUANT_BITS & paths) != ({"QUANT_" + L["kernel"].upper()} if L else set()):
            bad.append(f"{where}: launch record {L}, paths {sorted(paths)}")
            continue
        if r["frames"] == 0:
            continue
        if r["frames"] == 1 and not no_frame:
            if "FRAME" not in paths or L:
                bad.append(f"{where}: a one-frame call must take g_frame, paths {sorted(paths)}")
            seen[r["case"]].add("FRAME")
            continue
        if "SEPARATE" not in paths or not L or "FRAME" in paths:
            bad.append(f"{where}: the separate kernels with a quantization launch expected, paths {sorted(paths)}, launch {L}")
            continue
        if c["ref"]["resample_ratio"] != 1 and "PREP" not in paths:
            bad.append(f"{where}: a resampling stream without PREP")
        if L["skip"] != skip or L["nfs"] != r["frames"] + 1 or L["kernel"] == "fast":
            bad.append(f"{where}: launch {L}, expected the SKIP = {skip} form over {r['frames'] + 1} frame slots")
        if backend == "hostsim" and L["kernel"] != "persistent" or forced and L["kernel"] != "persistent":
            bad.append(f"{where}: launch {L}, expected the persistent kernel")
        if backend == "gpu" and not forced and L["kernel"] != "pair":          # two channels, at most 13 frame slots: below the pair threshold of any device
            bad.append(f"{where}: launch {L}, expected the pair kernel")
        if backend == "gpu" and cap == "1" and L["kernel"] == "persistent" and L["wg"] != 1:
            bad.append(f"{where}: launch {L}, expected one workgroup")
        seen[r["case"]].add((L["kernel"], L["skip"], r["frames"] == 1))
    for n in MATRIX_CASES:
        if not any(isinstance(s, tuple) and not s[2] for s in seen[n]) or (no_frame and not any(isinstance(s, tuple) and s[2] for s in seen[n])) or (not no_frame and "FRAME" not in seen[n]):
            bad.append(f"{env_name}: {n}: not every kind of call was seen ({sorted(map(str, seen[n]))})")
    return bad


if __name__ == "__main__":          # the child of run_matrix
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    sys.path.insert(0, str(ROOT / "tests" / "tools"))
    if sys.argv[1] == "matrix":
        matrix_child(sys.argv[2], sys.argv[3])
    else:          # "nofast" <backend>: the quality-7 goldens through the general kernels (LAMEJS_HIP_NO_FAST_QUANT=1, read once per process)
        import libs
        assert sys.argv[1] == "nofast" and os.environ.get("LAMEJS_HIP_NO_FAST_QUANT") == "1"
        lib = libs.gpu_library() if sys.argv[2] == "gpu" else libs.sim_library(sys.argv[2])
        seen, fast = set(), [c for c in goldens() if c.get("quality") == 7]
        for c in fast:
            seen |= run_golden_case(lib, c) | run_golden_case(lib, c, lens=[c["nsamples"]])
        print(json.dumps({"cases": len(fast), "paths": sorted(seen)}))
