"""TEST TOOL: one environment of the launch-path matrix (tests/path_matrix_cases.py), in a process of its own because the library reads
its switches (path_matrix_cases.SWITCHES) once per process.

usage: path_matrix_worker.py gpu|hostsim|wavesim <environment name> [num_cus] [--cases=all|fast|grid1]

Encodes the whole case list through the Python mirror, compares every stream with the oracle byte for byte and prints one JSON line per
call: the case, the call index, the frames it completed, the path set the library reports for it (Mp3Encoder.last_batch_paths), the set
path_matrix_cases.expected_paths gives for it, the launch record of its speculative quantization (path_matrix_cases.launch_record: workgroups,
waves, frame slots, kernel, template form; null = none launched) and the first differing byte, if any (null = equal).  The last line is
{"done": true, ...}.
Exit status 0 unless the program itself failed: mismatches are for the parent to judge."""
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np

import lamejs_amd
import libs
import path_matrix_cases as pm
from pcmformats_cases import interleave


def first_diff(got, want):
    if got == want:
        return None
    return next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))


def main():
    backend, env_name = sys.argv[1], sys.argv[2]
    argv = [a for a in sys.argv[3:] if not a.startswith("--cases=")]
    which = next((a[8:] for a in sys.argv[3:] if a.startswith("--cases=")), "all")
    t0 = time.time()
    if backend == "gpu":
        lib = libs.gpu_library()
        num_cus = int(argv[0])
    else:
        lib = libs.sim_library(backend)
        num_cus = 256                                  # (the simulations' context keeps the default)
    env = {k: os.environ[k] for k in pm.SWITCHES if k in os.environ}
    assert env == pm.ENVS[env_name], (env, env_name)
    cs = pm.select(pm.cases(), which)
    if backend == "wavesim":
        cs = pm.for_wavesim(cs)
    only = os.environ.get("PATH_MATRIX_ONLY")          # (for locating a failure by hand: a substring of the case names to run)
    frames_total = ran = 0
    for c in cs:
        if only and only not in c["name"]:
            continue
        ran += 1
        C, frame, ratio = pm.cfg_of(c)
        streams = pm.case_streams(c)
        S = len(streams)
        encs = [lamejs_amd.Mp3Encoder(c["ch"], c["sr"], c["kb"], lib=lib, **c["opts"]) for _ in streams]
        rec = lambda **kw: print(json.dumps(dict({"case": c["name"], "family": c["family"], "kind": c["kind"]}, **kw)), flush=True)

        def note(call, planned, flush, got=None, want=None, stream=0, nstreams=S):
            fr = encs[0].last_batch_stats()["frames"] // nstreams
            paths = sorted(encs[0].last_batch_paths())
            rec(call=call, stream=stream, nstreams=nstreams, frames=fr, planned=planned, paths=paths, launch=pm.launch_record(lib), diff=None if got is None else first_diff(got, want),
                expected=sorted(pm.expected_paths(c, C, ratio, nstreams, fr, flush, env, backend, num_cus)))
            return fr

        if not c["resv"]:
            (_, lens, l, r, want), enc, p, off = streams[0], encs[0], 0, 0
            for k, n in enumerate(lens):
                if pm.base_kind(c) == "f32gain":             # Float32, interleaved, gains in force
                    got = enc.encode_interleaved(interleave(l[p:p + n], r[p:p + n]).astype(np.float32))
                else:
                    got = enc.encodeBuffer(l[p:p + n], None if r is None else r[p:p + n])
                frames_total += note(k, c["seq"][k], False, got, want[off:off + len(got)])
                p, off = p + n, off + len(got)
            got = enc.flush()
            frames_total += note(len(lens), None, False, got, want[off:])
        else:
            # the bit reservoir: all streams in one batch per call; then each checked stream's own flush
            acc, p = [b""] * S, 0
            for k in range(len(c["seq"])):
                ns = [st[1][k] for st in streams]
                ps = [sum(st[1][:k]) for st in streams]
                part = lamejs_amd.encode_streams(encs, [st[2][q:q + n] for st, q, n in zip(streams, ps, ns)],
                                                 None if c["ch"] == 1 else [st[3][q:q + n] for st, q, n in zip(streams, ps, ns)], flush=False)
                acc = [a + b for a, b in zip(acc, part)]
                frames_total += S * note(k, c["seq"][k], False)
            for (s, _, _, _, want), enc in zip(streams, encs):
                if want is None:
                    continue
                got = acc[s] + enc.flush()
                frames_total += note(len(c["seq"]), None, True, got, want, stream=s, nstreams=1)
        for e in encs:
            e.close()
    print(json.dumps({"done": True, "cases": ran, "frames": frames_total, "seconds": round(time.time() - t0, 2), "only": only, "which": which}), flush=True)


if __name__ == "__main__":
    main()
