"""TEST INFRASTRUCTURE shared by tests/test_round_skip_cpu.py, tests/test_round_skip_gpu.py and tests/tools/round_skip_worker.py: the
quantization search without its dead last round of pairs.

A granule-channel whose lines 512..575 are all zero (GI::tail0, set from its own spectrum by q_calc_xmin) runs the per-pair functions of the
batch kernels with four rounds instead of five; the words 256..287 of the wave's working spectrum are zeroed once per granule-channel
instead.  What can go wrong is small and specific: the flag on the wrong granule-channel (short blocks keep lines up there at bitrates whose
long blocks do not, 320 kbps keeps them everywhere), stale words of a five-round unit surviving into a four-round unit of the same wave or
the reverse, and a kernel taking the wrong form.  The cases are the smallest that reach each of those:

configurations   44100/128 stereo (flag set on long blocks, clear on short ones, both in one workgroup), 44100/320 stereo (clear on long
                 blocks too), 44100/128 mono, 22050/64 stereo (LSF: one granule per frame), 44100/128 joint stereo with identical channels in
                 the first half of the stream (the side channel is an all-zero spectrum), 44100/128 stereo with the bit reservoir (the
                 five-round kernels on the changed shared code)
material         tests/tools/fuzz_gpu.material under fixed seeds (attacks, hence short blocks), pcm.CORPORA["bursts"], full-scale noise with
                 two stretches of digital silence of four and five frames (a silent granule-channel makes no evaluation and leaves an all-zero
                 working spectrum; the noise's onset is a short block -- five rounds -- and the long blocks behind it run four), and
                 pcm.CORPORA["sine"] at 320 kbps (no granule-channel may take the short form)
quality 7        the twins of six cases (Q7_TWINS) with { quality: 7 }: a batch call takes kb_quant_fast / g_quant_fast, whose unit (q_unit_fast) decides the
                 flag and zeroes the words itself
the stale words  At 44.1 / 48 kHz the lines 512..575 lie in the last band, beyond big_values, count1 and every band the search evaluates: nothing reads
                 the words 256..287 there, with or without the zeroing.  At 32 kHz band 20 straddles line 512, and the simulations poison those
                 words at the entry of every granule-channel (q_unit, host-only): with the zeroing statement removed from q_unit, 32000/96 stereo
                 differs from the oracle from its 9-frame call on and 32000/48 mono from its 2-frame call on (checked on the one-lane simulation).
calls            completing 1, 2, 9 and 17 frames (the one-frame kernel, the pair kernel, one more than a workgroup's eight waves, two
                 workgroups and a wave), each in the default environment and with LAMEJS_HIP_PAIR_MAX_FRAMES=0, which sends 9 and 17 through
                 g_quant and its tail help

Every stream is compared with the oracle byte for byte (oracle_py.oracle_calls); the oracle alone decides the expected bytes."""
import functools
import json
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT
from path_matrix_cases import ENVS, SWITCHES, child_is_fatal, plan_calls

sys.path.insert(0, str(ROOT / "tests" / "tools"))

SEQ = (1, 2, 9, 17)
SEED = 7312                          # (chosen on the CPU: with it the fuzz material of the first case has short blocks inside its 2-, 9- and 17-frame calls)
SILENT = ((5, 9), (16, 21))          # frames of input samples that are digital silence in the `silence` material: inside the 9- and the 17-frame call

CASES = [
    dict(name="stereo128/fuzz", ch=2, sr=44100, kb=128, opts={}, material="fuzz"),
    dict(name="stereo128/bursts", ch=2, sr=44100, kb=128, opts={}, material="bursts"),
    dict(name="stereo128/silence", ch=2, sr=44100, kb=128, opts={}, material="silence"),
    dict(name="stereo320/fuzz", ch=2, sr=44100, kb=320, opts={}, material="fuzz"),
    dict(name="stereo320/sine", ch=2, sr=44100, kb=320, opts={}, material="sine"),
    dict(name="mono128/fuzz", ch=1, sr=44100, kb=128, opts={}, material="fuzz"),
    dict(name="lsf64/fuzz", ch=2, sr=22050, kb=64, opts={}, material="fuzz"),
    dict(name="joint128/fuzz", ch=2, sr=44100, kb=128, opts={"joint": True}, material="fuzz"),
    dict(name="resv128/fuzz", ch=2, sr=44100, kb=128, opts={"reservoir": True}, material="fuzz"),
    # 32 kHz: band 20 is lines 448..549, so calc_noise and the scalefactor store READ the lines 512..549 of a unit that ran without the last round
    dict(name="stereo32k96/fuzz", ch=2, sr=32000, kb=96, opts={}, material="fuzz", seed=7400),
    dict(name="mono32k48/fuzz", ch=1, sr=32000, kb=48, opts={}, material="fuzz", seed=7400),
]
for _i, _c in enumerate(CASES):
    _c.setdefault("seed", SEED + _i)
# quality 7: the fast unit has code of its own for the skipped round (q_search_limits' tail0, the zeroing statement of q_unit_fast).  Each case is the twin of
# a quality-3 one: same configuration, same material, same seed.  `silence`: an inactive unit leaves an all-zero working spectrum in front of a four-round
# unit of the same wave.
Q7_TWINS = ("stereo128/fuzz", "stereo128/silence", "stereo320/fuzz", "lsf64/fuzz", "stereo32k96/fuzz", "mono32k48/fuzz")
CASES += [dict(next(c for c in CASES if c["name"] == _n), name="q7/" + _n, opts={"quality": 7}) for _n in Q7_TWINS]
# ... and the stream in which the fast unit's zeroing statement decides bytes.  Behind the bin search the fast mode reads the lines 512..549 in one place
# only, the empty-band scan of q_best_scalefac_store (the count of a tail0 search never reads them, g_bits stops at big_values + count1 <= 512).  All
# scalefactors are zero there, so whether band 20 is marked empty matters to the preflag test alone: preflag is set when the bands 11..20 are ALL empty, that
# is when an active long-block granule quantizes to zero from line 66 (1.8 kHz) up.  The fuzz material never does; loud noise cut off at 1.5 kHz does in half
# of its granules, and with the statement removed from q_unit_fast this case differs from the oracle from its 2-frame call on (both simulations; 32000/48
# one channel from the 9-frame call on).  32000/80 is the two-channel 32 kHz configuration whose lowpass zeroes the lines 512..575 (96 kbps keeps them).
CASES.append(dict(name="q7/stereo32k80/lownoise", ch=2, sr=32000, kb=80, opts={"quality": 7}, material="lownoise", seed=7400))


def case(name):
    return next(c for c in CASES if c["name"] == name)


def frame_len(c):
    return 1152 if c["sr"] >= 32000 else 576


def case_pcm(c, n):
    """The Int16 planes of a case (the second is None for one channel)."""
    import pcm
    from fuzz_gpu import material
    rng = np.random.default_rng(c["seed"])
    if c["material"] == "fuzz":
        L, R = material(rng, n, c["ch"])
    elif c["material"] == "silence":
        L, R = (rng.integers(-32768, 32768, n).astype(np.int16) for _ in range(2))
        for a, b in SILENT:
            L[1152 * a:1152 * b] = 0
            R[1152 * a:1152 * b] = 0
    elif c["material"] == "lownoise":     # white noise without its bins above 1.5 kHz, peak 30000
        def plane():
            X = np.fft.rfft(rng.standard_normal(n))
            X[int(1500.0 * n / c["sr"]):] = 0
            x = np.fft.irfft(X, n)
            return np.round(x * (30000 / np.abs(x).max())).astype(np.int16)
        L, R = plane(), plane()
    else:
        L, R = pcm.CORPORA[c["material"]](n, c["ch"])
        L, R = np.asarray(L, dtype=np.int16), None if R is None else np.asarray(R, dtype=np.int16)
    if c["opts"].get("joint"):          # identical channels in the first half: the side channel's spectrum is all zero there
        L, R = L.copy(), R.copy()
        R[:n // 2] = L[:n // 2]
    return L, (R if c["ch"] == 2 else None)


@functools.lru_cache(maxsize=None)
def case_stream(name):
    """(call lengths, left, right, the oracle's bytes) of a case: computed once per process and shared."""
    import lamejs_amd
    from oracle_py import oracle_calls
    c = case(name)
    lens = plan_calls(SEQ, frame_len(c), 1, np.random.default_rng(c["seed"]))
    L, R = case_pcm(c, sum(lens))
    (part,), tail = oracle_calls(lamejs_amd.tables_blob(c["ch"], c["sr"], c["kb"], **c["opts"]), L, R, [len(L)])
    for a in (L, R):
        if a is not None:
            a.setflags(write=False)
    return lens, L, R, part + tail


def first_diff(got, want):
    if got == want:
        return None
    return next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))


def encode_case(lib, c, before_call=None):
    """The case through the library under test, call by call, then its flush: [{call, frames, planned, paths, diff}] (planned None: the flush).
    before_call(k), if given, runs in front of call k (the CPU tier reads the simulations' counters there)."""
    import lamejs_amd
    lens, L, R, want = case_stream(c["name"])
    enc = lamejs_amd.Mp3Encoder(c["ch"], c["sr"], c["kb"], lib=lib, **c["opts"])
    out, p, off = [], 0, 0
    for k, n in enumerate(list(lens) + [None]):
        if before_call:
            before_call(k)
        got = enc.flush() if n is None else enc.encodeBuffer(L[p:p + n], None if R is None else R[p:p + n])
        w = want[off:] if n is None else want[off:off + len(got)]
        out.append({"case": c["name"], "call": k, "frames": enc.last_batch_stats()["frames"], "planned": None if n is None else SEQ[k],
                    "paths": sorted(enc.last_batch_paths()), "diff": first_diff(got, w)})
        p, off = p + (n or 0), off + len(got)
    if before_call:
        before_call(len(lens) + 1)
    enc.close()
    return out


def round_counts(lib):
    """(evaluations without the last round of pairs, evaluations with it) this process has made in a simulation library: lhip_debug_read(10)."""
    import ctypes
    v = (ctypes.c_int64 * 2)()
    assert lib.lhip_debug_read(10, v, 16) == 16
    return int(v[0]), int(v[1])


def run_child(env_name, backend, limit):
    """tests/tools/round_skip_worker.py for one environment in a fresh process (the switch is read once per process) under a time limit of its
    own; returns (status, records, text, fatal)."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(ENVS[env_name])
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(ROOT / "tests" / "tools" / "round_skip_worker.py"), backend, env_name]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    return r.returncode, recs, r.stdout[-3000:] + r.stderr[-3000:], child_is_fatal(r.returncode, r.stdout + r.stderr)


def check_records(recs, env_name):
    """What one child's records must show; returns a list of failures (empty = fine)."""
    done = [r for r in recs if r.get("done")]
    if len(done) != 1 or done[0]["cases"] != len(CASES):
        return [f"{env_name}: the worker did not finish its case list ({done})"]
    bad = []
    for r in recs:
        if r.get("done"):
            continue
        if r["diff"] is not None:
            bad.append(f"{env_name}: MISMATCH {r['case']} call {r['call']}: first differing byte {r['diff']} (paths {r['paths']})")
        if r["planned"] is not None and r["planned"] != r["frames"]:
            bad.append(f"{env_name}: {r['case']} call {r['call']}: {r['frames']} frames, planned {r['planned']}")
    return bad
