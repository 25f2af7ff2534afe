"""TEST INFRASTRUCTURE shared by tests/test_noise_lines_cpu.py, tests/test_noise_lines_gpu.py and tests/tools/noise_lines_worker.py: calc_noise's
line pass and fold over the lines the evaluated bands reach.

calc_noise reads the sums of the bands below psymax only (21 long bands or 36 short ones), so its 64-lane program gives every lane 7 lines
(lines 0..447) where sfb_l[21] and 3 * sfb_s[12] both lie at or below 448, and 9 lines (the whole spectrum) elsewhere (Tables::noise_nln,
lhip_tables.h).  What can go wrong is specific: the wrong form for a table set, band marks laid out for the other form, the band that straddles
the last lane's border stored, a short block's last evaluated band (3 * sfb_s[12] - 1 = line 407 at 44.1 kHz, 377 at 48 kHz) cut off, and long
band 20 -- lines 342..417 at 44.1 kHz, through lane 59 of the 7-line layout -- losing its tail.  The cases:

configurations   44100/128 stereo and mono (7 lines; borders 418 / 408), 48000/192 stereo (7 lines; 384 / 378: short band 36 ends at line 443, inside
                 the 448 lines, and is stored though never read), 32000/64 mono (9 lines: sfb_l[21] = 550), 22050/64 stereo (MPEG-2, 9 lines:
                 sfb_l[21] = 522), 44100/128 stereo with the bit reservoir (the per-stream kernel)
material         pcm.CORPORA["sine"] and pcm.CORPORA["bursts"] (attacks, hence short blocks)
calls            completing 1, 2, 9 and 12 frames (the one-frame program, the pair program, one more than a workgroup's eight waves, a workgroup and
                 a half) -- 24 frames, the CPU tier -- or 1, 2, 9, 17 and 20 frames on the device, 49 frames; there each in the default environment
                 and with LAMEJS_HIP_PAIR_MAX_FRAMES=0, which sends the two-channel calls through the persistent kernel and its tail help

A call whose fresh bands all end at or below line 192 (bands 0..15 at 44.1 kHz; the others come from the cache) takes a third body whatever the table set:
3 lines per lane over the lines 0..191 (Tables::noise_hib3).  Every case has such calls beside the full ones.

expected_nln(c) applies the rule to the case's own table blob; every stream is compared with the oracle byte for byte (oracle_py.oracle_calls)."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT
from path_matrix_cases import ENVS, SWITCHES, blob_array, child_is_fatal, plan_calls
from round_skip_cases import first_diff

SEQ_CPU = (1, 2, 9, 12)
SEQ_GPU = (1, 2, 9, 17, 20)

CASES = [
    dict(name="stereo128/sine", ch=2, sr=44100, kb=128, opts={}, material="sine"),
    dict(name="stereo128/bursts", ch=2, sr=44100, kb=128, opts={}, material="bursts"),
    dict(name="mono128/sine", ch=1, sr=44100, kb=128, opts={}, material="sine"),
    dict(name="mono128/bursts", ch=1, sr=44100, kb=128, opts={}, material="bursts"),
    dict(name="stereo48k192/sine", ch=2, sr=48000, kb=192, opts={}, material="sine"),
    dict(name="stereo48k192/bursts", ch=2, sr=48000, kb=192, opts={}, material="bursts"),
    dict(name="mono32k64/sine", ch=1, sr=32000, kb=64, opts={}, material="sine"),
    dict(name="lsf64/sine", ch=2, sr=22050, kb=64, opts={}, material="sine"),
    dict(name="resv128/bursts", ch=2, sr=44100, kb=128, opts={"reservoir": True}, material="bursts"),
]
SEVEN = ("stereo128/sine", "stereo128/bursts", "mono128/sine", "mono128/bursts", "stereo48k192/sine", "stereo48k192/bursts", "resv128/bursts")
NINE = ("mono32k64/sine", "lsf64/sine")


def case(name):
    return next(c for c in CASES if c["name"] == name)


def frame_len(c):
    return 1152 if c["sr"] >= 32000 else 576


def band_borders(c):
    """(sfb_l[21], 3 * sfb_s[12]) of the case's table blob: the first lines calc_noise never needs in a long and in a short block."""
    import lamejs_amd
    blob = lamejs_amd.tables_blob(c["ch"], c["sr"], c["kb"], **c["opts"])
    return int(blob_array(blob, "sfb_l", "i")[21]), 3 * int(blob_array(blob, "sfb_s", "i")[12])


def expected_nln(c):
    """The rule of lhip_tables.h (Tables::noise_nln) on the case's own blob."""
    return 7 if max(band_borders(c)) <= 64 * 7 else 9


@functools.lru_cache(maxsize=None)
def case_stream(name, seq):
    """(call lengths, left, right, the oracle's bytes) of a case for a call sequence: computed once per process and shared."""
    import lamejs_amd
    import pcm
    from oracle_py import oracle_calls
    c = case(name)
    lens = plan_calls(seq, frame_len(c), 1, np.random.default_rng(4100 + CASES.index(c)))
    L, R = pcm.CORPORA[c["material"]](sum(lens), c["ch"])
    L, R = np.asarray(L, dtype=np.int16), None if (R is None or c["ch"] == 1) else np.asarray(R, dtype=np.int16)
    (part,), tail = oracle_calls(lamejs_amd.tables_blob(c["ch"], c["sr"], c["kb"], **c["opts"]), L, R, [len(L)])
    for a in (L, R):
        if a is not None:
            a.setflags(write=False)
    return lens, L, R, part + tail


def encode_case(lib, c, seq, after_call=None):
    """The case through the library under test, call by call, then its flush: [{case, call, frames, planned, paths, diff}] (planned None: the
    flush).  after_call(k, enc), if given, runs behind call k (the CPU tier reads the simulation's counters and side records there)."""
    import lamejs_amd
    lens, L, R, want = case_stream(c["name"], seq)
    enc = lamejs_amd.Mp3Encoder(c["ch"], c["sr"], c["kb"], lib=lib, **c["opts"])
    out, p, off = [], 0, 0
    for k, n in enumerate(list(lens) + [None]):
        got = enc.flush() if n is None else enc.encodeBuffer(L[p:p + n], None if R is None else R[p:p + n])
        w = want[off:] if n is None else want[off:off + len(got)]
        out.append({"case": c["name"], "call": k, "frames": enc.last_batch_stats()["frames"], "planned": None if n is None else seq[k],
                    "paths": sorted(enc.last_batch_paths()), "diff": first_diff(got, w)})
        if after_call:
            after_call(k, enc)
        p, off = p + (n or 0), off + len(got)
    enc.close()
    return out


def line_counts(lib):
    """(calc_noise calls with 7 lines per lane, with 9, with the short window's 3) this process has made in the 64-lane simulation: lhip_debug_read(12)."""
    v = (ctypes.c_int64 * 3)()
    assert lib.lhip_debug_read(12, v, 24) == 24
    return int(v[0]), int(v[1]), int(v[2])


def run_child(env_name, limit):
    """tests/tools/noise_lines_worker.py on the device for one environment in a fresh process (the switch is read once per process) under a
    time limit of its own; returns (status, records, text, fatal)."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(ENVS[env_name])
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(ROOT / "tests" / "tools" / "noise_lines_worker.py"), env_name]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    return r.returncode, recs, r.stdout[-3000:] + r.stderr[-3000:], child_is_fatal(r.returncode, r.stdout + r.stderr)


def check_records(recs, env_name, ncases=None):
    """What a run's records must show; returns a list of failures (empty = fine)."""
    done = [r for r in recs if r.get("done")]
    if len(done) != 1 or done[0]["cases"] != (len(CASES) if ncases is None else ncases):
        return [f"{env_name}: the case list was not finished ({done})"]
    bad = []
    for r in recs:
        if r.get("done"):
            continue
        if r["diff"] is not None:
            bad.append(f"{env_name}: MISMATCH {r['case']} call {r['call']}: first differing byte {r['diff']} (paths {r['paths']})")
        if r["planned"] is not None and r["planned"] != r["frames"]:
            bad.append(f"{env_name}: {r['case']} call {r['call']}: {r['frames']} frames, planned {r['planned']}")
    return bad
