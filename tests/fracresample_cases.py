"""TEST helper for the { fractionalResample } extension: the golden cases of tests/golden/golden_fracresample.json (written by
tests/tools/gen_golden_fracresample.js from the unmodified reference) driven through the C ABI -- the HIP library or a simulation of it."""
import ctypes
import hashlib

import numpy as np

import golden_cases
from conftest import load_case_pcm


def golden_frac():
    return golden_cases.load("golden_fracresample")


def triples(cases):
    return sorted({(c["channels"], c["samplerate"], c["kbps"]) for c in cases})


def frames_of(data: bytes, lengths):
    out, p = [], 0
    for n in lengths:
        out.append(data[p:p + n])
        p += n
    assert p == len(data)
    return out


def predict(lib, enc, nsamples):
    """(k, frames, rc) of the next call by the host arithmetic alone"""
    k, f = ctypes.c_int32(), ctypes.c_int32()
    rc = lib.lhip_debug_frac_call(enc._h, nsamples, ctypes.byref(k), ctypes.byref(f))
    return k.value, f.value, rc


def predict_flush(lib, enc):
    b, c = (ctypes.c_int32 * 16)(), (ctypes.c_int32 * 16)()
    n = lib.lhip_debug_frac_flush(enc._h, b, c, 16)
    assert 0 <= n <= 16
    return [(b[i], bool(c[i])) for i in range(n)]


def check_flush(case, data: bytes):
    """frame count, each frame's length and header; a frame the reference made of finite samples byte for byte (md5), every other one
    with all-zero main data (here: everything behind the header)"""
    want = case["flush"]
    assert len(data) == sum(f["bytes"] for f in want), (case["kind"], case["channels"], case["samplerate"], case["kbps"], len(data))
    for f, got in zip(want, frames_of(data, [f["bytes"] for f in want])):
        assert got[:4].hex() == f["header_hex"], case
        if not f["nan_in_window"]:
            assert hashlib.md5(got).hexdigest() == f["md5"], case
        else:
            assert not any(got[4:]), case


def run_case(lib, case, host_arithmetic=True, with_flush=True):
    """One golden case call by call.  Returns the encodeBuffer() bytes per call."""
    import lamejs_amd
    L, R = load_case_pcm(case)
    enc = lamejs_amd.Mp3Encoder(case["channels"], case["samplerate"], case["kbps"], lib=lib, fractional_resample=True)
    assert enc.call_limit() == case["call_limit"]
    outs, p, good = [], 0, 0
    try:
        for c, n in enumerate(case["call_lens"]):
            l, r = L[p:p + n], None if R is None else R[p:p + n]
            p += n
            if c == case.get("bad_call", -1):
                # the reference turns fractional here: refused, the limit named, nothing consumed
                k, f, rc = predict(lib, enc, n)
                assert rc == -4 and f == -1
                try:
                    enc.encodeBuffer(l, r)
                    raise AssertionError("a call the reference does not consume whole was accepted")
                except lamejs_amd.LhipError as e:
                    assert "-4" in str(e) and str(case["call_limit"]) in str(e), str(e)
                continue
            if host_arithmetic:
                k, f, rc = predict(lib, enc, n)
                assert rc == 0 and k == case["call_k"][good] and f == (1 if case["call_bytes"][good] else 0), (case, c, k, f)
            o = enc.encodeBuffer(l, r)
            assert len(o) == case["call_bytes"][good], (case["kind"], case["channels"], case["samplerate"], case["kbps"], c, len(o))
            outs.append(o)
            good += 1
        assert hashlib.md5(b"".join(outs)).hexdigest() == case["enc_md5"], (case["kind"], case["channels"], case["samplerate"], case["kbps"])
        if with_flush:
            if host_arithmetic:
                plan = predict_flush(lib, enc)
                assert [b for b, _ in plan] == [f["bytes"] for f in case["flush"]], (case, plan)
                assert [c for _, c in plan] == [not f["nan_in_window"] for f in case["flush"]], (case, plan)
            check_flush(case, enc.flush())
            assert enc.flush() == b""
    finally:
        enc.close()
    return outs


def np_i16(a):
    return np.ascontiguousarray(a, dtype=np.int16)


def batch_all_configurations(lib, G, rounds=12):
    """lhip_encode_batch over one stream of every one of the 49 configurations at once -- different configurations in one launch call --
    `rounds` rounds of 576 samples: every stream gets what it gets alone (the golden's bytes per call)."""
    import lamejs_amd
    cases = [c for c in G["cases"] if c["kind"] == "calls576"]
    assert len(cases) == 49
    pcm = [load_case_pcm(c) for c in cases]
    encs = [lamejs_amd.Mp3Encoder(c["channels"], c["samplerate"], c["kbps"], lib=lib, fractional_resample=True) for c in cases]
    got = [b""] * len(cases)
    try:
        for rnd in range(rounds):
            lefts = [L[576 * rnd:576 * (rnd + 1)] for L, _ in pcm]
            rights = [(L if R is None else R)[576 * rnd:576 * (rnd + 1)] for L, R in pcm]
            outs = lamejs_amd.encode_streams(encs, lefts, rights, flush=False)
            for i, (c, o) in enumerate(zip(cases, outs)):
                assert len(o) == c["call_bytes"][rnd], (c["channels"], c["samplerate"], c["kbps"], rnd)
                got[i] += o
        singles = 0
        for c, g, (L, R) in zip(cases, got, pcm):
            e = lamejs_amd.Mp3Encoder(c["channels"], c["samplerate"], c["kbps"], lib=lib, fractional_resample=True)
            alone = b"".join(e.encodeBuffer(L[576 * r:576 * (r + 1)], None if R is None else R[576 * r:576 * (r + 1)]) for r in range(rounds))
            e.close()
            assert g == alone, (c["channels"], c["samplerate"], c["kbps"])
            if len(c["call_lens"]) == rounds:
                assert hashlib.md5(g).hexdigest() == c["enc_md5"]
                singles += 1
        # the streams end through lhip_flush_batch: the same frames as each stream's own flush (checked against the golden where the case ends here)
        tails = lamejs_amd.encode_streams(encs, [np.zeros(0, np.int16)] * len(encs), None, flush=True)
        for c, t in zip(cases, tails):
            if len(c["call_lens"]) == rounds:
                check_flush(c, t)
        return singles
    finally:
        for e in encs:
            e.close()
