"""TEST INFRASTRUCTURE shared by tests/test_quality_cpu.py and tests/test_quality_gpu.py: the fast encoding mode, quality 7 (LAME's -f).
Yardsticks: the unmodified reference's bytes with gfp.quality = 7 (tests/golden/golden_quality.json, tests/tools/gen_golden_quality.js), and --
only once it has reproduced those goldens itself -- the unchanged CPU oracle, which reads the quality switches from the blob, for a seeded
random family.  Every stream can be run twice: through the bin-search-only kernel body (path bit QUANT_FAST) and, in a child process with
LAMEJS_HIP_NO_FAST_QUANT=1, through the general quantization kernels."""
import os
import subprocess
import sys

import numpy as np

import pcm
from conftest import ROOT
from golden_cases import check_stream, feed_calls, load, pinned

SWITCHES = ("noise_shaping", "noise_shaping_amp", "noise_shaping_stop", "use_best_huffman", "subblock_gain", "full_outer_loop")
BATCH_QUANT_BITS = {"QUANT_FAST", "QUANT_PAIR", "QUANT_PERSISTENT"}


def goldens():
    return load("golden_quality")["cases"]


def case_opts(c):
    return {"joint": bool(c.get("jointStereo")), "reservoir": bool(c.get("reservoir")), "downmix": bool(c.get("downmix")), "protect": bool(c.get("protect")), "quality": c["quality"]}


def _wav(n, ch):
    L = np.fromfile(ROOT / "tests" / "golden" / "left44100_full.s16", dtype="<i2")[:n]
    return L, (np.fromfile(ROOT / "tests" / "golden" / "right44100_full.s16", dtype="<i2")[:n] if ch == 2 else None)


def material(corpus, n, ch, seed=None):
    """The corpora of tests/tools/gen_golden_quality.js by name; ``seed``: another draw of the synthetic ones (the random family)."""
    kw = {} if seed is None else {"seed": seed}
    if corpus == "wavexcerpt":
        return _wav(n, ch)
    if corpus == "mixed":          # six frames' worth of the centre variant, then independent channels: M/S and L/R frames in one stream
        (A, B), (CL, CR), h = pcm.bursts(n, 2, **kw), pcm.CORPORA["centre_bursts"](n, 2, **kw), n // 2
        return np.concatenate([CL[:h], A[h:]]), np.concatenate([CR[:h], B[h:]])
    if corpus == "silent3":        # three frames of digital silence in front: granules without energy
        A, B = pcm.bursts(n, ch, **kw)
        A = A.copy()
        A[:3 * 1152] = 0
        if B is not None:
            B = B.copy()
            B[:3 * 1152] = 0
        return A, B
    return pcm.CORPORA[corpus](n, ch, **kw)


def case_pcm(c):
    return pinned(material(c["corpus"], c["nsamples"], c["channels"]), c["pcm_md5"])


def make_encoder(lib, c, **kw):
    import lamejs_amd
    return lamejs_amd.Mp3Encoder(c["channels"], c["samplerate"], c["kbps"], lib=lib, **dict(case_opts(c), **kw))


def run_golden_case(lib, c, lens=None, want_fast=None):
    """The case through encodeBuffer in calls of ``lens`` samples (default: its own calls), then flush, against the golden.  Returns the
    union of the path names its calls took.  ``want_fast``: True / False asserts that every call which took the separate kernels without the
    reservoir quantized through QUANT_FAST / through the general kernels."""
    import lamejs_amd
    L, R = case_pcm(c)
    enc = make_encoder(lib, c)
    seen = set()
    try:
        def call(i, l, r):
            out = enc.encodeBuffer(l, r)
            p = lamejs_amd.last_batch_paths(lib)
            if want_fast is not None and BATCH_QUANT_BITS & p:
                assert (BATCH_QUANT_BITS & p) == ({"QUANT_FAST"} if want_fast else (BATCH_QUANT_BITS & p) - {"QUANT_FAST"}) != set(), (c["name"], i, sorted(p))
            seen.update(p)
            return out
        parts = feed_calls(lens or c["call_lens"], L, R, call)
        check_stream(c, parts, enc.flush(), call_bytes=lens is None)
        if c.get("reservoir"):
            assert not (BATCH_QUANT_BITS & seen), (c["name"], sorted(seen))
        return seen
    finally:
        enc.close()


def encode_whole(lib, channels, samplerate, kbps, L, R, lens=None, **opts):
    import lamejs_amd
    enc = lamejs_amd.Mp3Encoder(channels, samplerate, kbps, lib=lib, **opts)
    try:
        n = len(L)
        lens = lens or [n]
        parts = feed_calls(lens, L, R, lambda i, l, r: enc.encodeBuffer(l, r))
        return b"".join(parts) + enc.flush()
    finally:
        enc.close()


# ---- the unchanged oracle on a quality-7 blob ----
def oracle_takes(c):
    """The oracle encodes Int16 planes as they are: it has no downmix (tests/inputmix_cases.py says the same of its family)."""
    return not c.get("downmix")


def oracle_stream(c_or_cfg, L, R, lens, **opts):
    import lamejs_amd
    from oracle_py import oracle_calls
    ch, sr, kb = c_or_cfg
    parts, tail = oracle_calls(lamejs_amd.tables_blob(ch, sr, kb, **opts), L, R if ch == 2 else None, lens)
    return parts, tail


def oracle_reproduces(c):
    L, R = case_pcm(c)
    o = case_opts(c)
    parts, tail = oracle_stream((c["channels"], c["samplerate"], c["kbps"]), L, R, c["call_lens"], **o)
    # (a reservoir stream's split into calls and flush is the library's; the oracle's is checked as a whole)
    check_stream(c, parts, tail, call_bytes=not c.get("reservoir"), enc_md5=not c.get("reservoir"), flush_md5=not c.get("reservoir"), all_md5=bool(c.get("reservoir")))
    return True


# ---- the seeded random family: reference = the oracle (only behind oracle_reproduces on every golden it takes) ----
CONFIGS = [(2, 44100, 128, {}), (1, 44100, 64, {}), (2, 48000, 320, {}), (2, 22050, 48, {}), (1, 16000, 32, {}), (1, 8000, 8, {}), (2, 44100, 48, {}),
           (2, 44100, 128, {"joint": True}), (2, 44100, 192, {"joint": True}), (2, 44100, 128, {"reservoir": True}), (1, 32000, 96, {}), (2, 24000, 64, {"joint": True}),
           (2, 44100, 128, {"protect": True})]


def family(seed, count, min_frames=8, max_frames=20):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        ch, sr, kb, o = CONFIGS[int(rng.randint(0, len(CONFIGS)))] if i >= 4 else CONFIGS[(0, 1, 7, 3)[i]]
        n = int(rng.randint(min_frames * 1152, max_frames * 1152 + 1))
        corpus = ("mixed" if ch == 2 and o.get("joint") else ["bursts", "sine", "silent3"][int(rng.randint(0, 3))])
        n -= n % 2 if corpus == "mixed" else 0
        cuts, p = [], 0
        while p < n:                      # random call cuts: single samples, odd lengths, several frames at once
            m = int(rng.choice([1, 17, 777, 1152, 2305, 4096, n]))
            m = min(m, n - p)
            cuts.append(m)
            p += m
        out.append({"cfg": (ch, sr, kb), "opts": dict(o), "corpus": corpus, "seed": int(rng.randint(1, 1 << 30)), "n": n, "lens": cuts})
    return out


def family_check(lib, cases, want_fast=None):
    import lamejs_amd
    for fc in cases:
        ch, sr, kb = fc["cfg"]
        L, R = material(fc["corpus"], fc["n"], ch, fc["seed"])
        parts, tail = oracle_stream(fc["cfg"], L, R, fc["lens"], quality=7, **fc["opts"])
        want = b"".join(parts) + tail
        enc = lamejs_amd.Mp3Encoder(ch, sr, kb, lib=lib, quality=7, **fc["opts"])
        got, p = b"", 0
        for m in fc["lens"]:
            got += enc.encodeBuffer(L[p:p + m], None if R is None else R[p:p + m])
            paths = lamejs_amd.last_batch_paths(lib)
            if want_fast is not None and BATCH_QUANT_BITS & paths:
                assert ("QUANT_FAST" in paths) == bool(want_fast) and not fc["opts"].get("reservoir"), (fc["cfg"], fc["opts"], sorted(paths))
            p += m
        got += enc.flush()
        enc.close()
        assert got == want, (fc["cfg"], fc["opts"], fc["corpus"], fc["lens"][:6], len(got), len(want))
    return len(cases)


# ---- a check in a child process with the general kernels forced (LAMEJS_HIP_NO_FAST_QUANT is read once per process) ----
def run_forced_general(what, lib_path=None, timeout=None):
    """`python tests/quality_cases.py <what>` with LAMEJS_HIP_NO_FAST_QUANT=1 (and LAMEJS_HIP_LIB = a simulation, if given); the child's
    last line of output is its JSON result."""
    import json
    e = dict(os.environ, LAMEJS_HIP_NO_FAST_QUANT="1")
    if lib_path is not None:
        e["LAMEJS_HIP_LIB"] = str(lib_path)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "quality_cases.py"), what], capture_output=True, text=True, env=e, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def batch64(lib, want_fast):
    """64 two-channel streams of up to 16 frames with different lengths, quality 7, in ONE lhip_encode_batch: per stream the oracle's bytes.
    Returns the path names of the batch."""
    import lamejs_amd
    rng = np.random.RandomState(20300)
    lens = [int(rng.randint(9 * 1152, 16 * 1152 + 1)) for _ in range(64)]
    lens[0], lens[1] = 16 * 1152, 9 * 1152 + 1
    pcms = [material(["bursts", "sine", "silent3"][i % 3], n, 2, 1000 + i) for i, n in enumerate(lens)]
    encs = [lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, quality=7) for _ in lens]
    got = lamejs_amd.encode_streams(encs, [p[0] for p in pcms], [p[1] for p in pcms], flush=False)
    paths = lamejs_amd.last_batch_paths(lib)
    assert ("QUANT_FAST" in paths) == bool(want_fast) and (BATCH_QUANT_BITS & paths) - {"QUANT_FAST"} == (set() if want_fast else (BATCH_QUANT_BITS & paths)), sorted(paths)
    got = [g + e.flush() for g, e in zip(got, encs)]
    for e in encs:
        e.close()
    for i, (n, (L, R)) in enumerate(zip(lens, pcms)):
        parts, tail = oracle_stream((2, 44100, 128), L, R, [n], quality=7)
        assert got[i] == b"".join(parts) + tail, (i, n)
    return paths


if __name__ == "__main__":          # the child of run_forced_general
    import json
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import lamejs_amd
    assert os.environ.get("LAMEJS_HIP_NO_FAST_QUANT") == "1"
    lib = lamejs_amd.load_library()
    what = sys.argv[1]
    res = {"what": what, "sim": b"HOST SIMULATION" in lib.lhip_version()}
    if what == "goldens":
        seen = set()
        for c in goldens():
            seen |= run_golden_case(lib, c, want_fast=False)
            seen |= run_golden_case(lib, c, lens=[c["nsamples"]], want_fast=False)
        res.update(cases=len(goldens()), paths=sorted(seen))
    elif what == "family":
        res.update(cases=family_check(lib, family(20301, 12), want_fast=False))
    elif what == "batch64":
        res.update(paths=sorted(batch64(lib, False)))
    print(json.dumps(res))
