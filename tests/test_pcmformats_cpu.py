"""Sample formats of the C ABI -- Int16 / Float32, planar / interleaved (lhip_encode_pcm, lhip_encode_batch_pcm,
lhip_encode_batch_device_pcm) -- CPU tier: the kernel bodies in both simulations against the goldens of the unmodified reference
(Float32Array input, tests/tools/gen_golden_floatpcm.js) and against the unchanged oracle on integer-valued input."""
import hashlib

import numpy as np
import pytest

import pcmformats_cases as pc
from conftest import load_case_pcm
from libs import ADDON, HOSTSIM_SO, NODE, run_js_check, sim, wavesim  # noqa: F401
from pcmformats_cases import F32, INTER, S16


@pytest.fixture(scope="module")
def G():
    return pc.golden_floatpcm()


def test_golden_set_is_the_one_asked_for(G):
    kinds = [c["kind"] for c in G]
    assert all(kinds.count(k) == 11 for k in pc.KINDS) and len(G) == 44
    for k in pc.KINDS:
        mine = [c for c in G if c["kind"] == k]
        assert {c["channels"] for c in mine} == {1, 2}
        assert {(c["channels"], c["samplerate"], c["kbps"]) for c in mine} >= {(1, 44100, 128), (2, 44100, 128), (2, 44100, 320), (2, 48000, 192), (1, 16000, 32), (1, 44100, 32), (2, 44100, 96)}
        assert any(c["joint"] for c in mine) and any(c["reservoir"] for c in mine) and any(c["frac"] and set(c["call_lens"]) == {576} for c in mine)
        assert {c["pattern"] for c in mine} >= {"one", "calls1152", "odd"}
        assert any({1, 777} <= set(c["call_lens"]) for c in mine)
    assert all(65536 < c["peak"] <= 131072 for c in G if c["kind"] == "hot") and all(c["peak"] <= 1 for c in G if c["kind"] == "unit")


def test_hostsim_every_golden_case_f32_planar(sim, G):
    assert pc.run_all_goldens(sim, G) == {k: 11 for k in pc.KINDS}


def test_wavesim_golden_cases_f32_planar(wavesim, G):
    """The wave programs (64 lanes as fibers): every kind over one-channel and two-channel configurations, resamplers, joint stereo and the reservoir."""
    names = {"m1_128_mono", "m1_128_stereo", "resample_int_mono", "resample_frac_stereo", "joint_stereo", "reservoir_stereo"}
    ran = pc.run_all_goldens(wavesim, [c for c in G if c["name"] in names])
    assert ran == {k: 6 for k in pc.KINDS}


def test_hostsim_interleaved_equals_planar_for_frac_cases(sim, G):
    n = 0
    for case in G:
        if case["kind"] == "frac":
            pc.run_golden_case(sim, case, F32 | INTER)      # same goldens: byte for byte the planar result
            n += 1
    assert n == 11


def test_wavesim_interleaved_frac_cases(wavesim, G):
    n = 0
    for case in G:
        if case["kind"] == "frac" and case["name"] in ("m1_320_stereo", "resample_frac_stereo", "m1_48k_stereo"):
            pc.run_golden_case(wavesim, case, F32 | INTER)
            n += 1
    assert n == 3


def test_hostsim_ints_cases_equal_the_oracle(sim, G):
    """Integer-valued floats inside the Int16 range: the reference's goldens and the unchanged oracle on the Int16 values agree, so the
    oracle is the reference of the random family below."""
    from oracle_py import oracle_encode
    n = 0
    for case in G:
        if case["kind"] != "ints" or case["frac"]:
            continue
        _, _, A, B = pc.case_pcm(case)
        want = oracle_encode(case["channels"], case["samplerate"], case["kbps"], A, B, joint=bool(case["joint"]), reservoir=bool(case["reservoir"]))
        assert hashlib.md5(want).hexdigest() == case["all_md5"], case["name"]
        n += 1
    assert n == 10


@pytest.mark.parametrize("fmt", ["f32_planar", "f32_interleaved", "s16_interleaved"])
def test_hostsim_random_family_equals_the_oracle(sim, fmt):
    fam = pc.family(20261, 112)
    for fc in fam:
        assert pc.family_encode(sim, fc, lambda c: pc.FORMATS[fmt]) == pc.family_oracle(fc), (fmt, fc["cfg"], fc["n"], fc["lens"][:4])


def test_wavesim_random_family_equals_the_oracle(wavesim):
    fam = pc.family(20262, 28, max_frames=3)
    for i, fc in enumerate(fam):
        fmt = [F32, F32 | INTER, S16 | INTER][i % 3]
        assert pc.family_encode(wavesim, fc, lambda c: fmt) == pc.family_oracle(fc), (fmt, fc["cfg"], fc["n"])


def test_hostsim_formats_mixed_from_call_to_call(sim, wavesim):
    order = [S16, F32 | INTER, F32, S16 | INTER]
    for lib, fam in ((sim, pc.family(20263, 42)), (wavesim, pc.family(20264, 14, max_frames=3))):
        for i, fc in enumerate(fam):
            assert pc.family_encode(lib, fc, lambda c: order[(c + i) % 4]) == pc.family_oracle(fc), (fc["cfg"], fc["n"], fc["lens"][:4])


def test_hostsim_batch_entry_in_all_four_formats(sim, G):
    """lhip_encode_batch_pcm over several streams at once == the streams one by one (oracle), in every format; a frac-valued batch in both
    Float32 layouts == the golden calls."""
    import pcm
    from oracle_py import oracle_encode
    for cfg in ((2, 44100, 128), (1, 44100, 128), (2, 44100, 48)):
        lens = [1152 * 3 + 5, 1, 777, 1152 * 6, 2305]
        pcms = [pcm.bursts(n, cfg[0], seed=100 + i) if i % 2 else pcm.sine(n, cfg[0], seed=100 + i) for i, n in enumerate(lens)]
        want = [oracle_encode(*cfg, l, r) for l, r in pcms]
        for name, fmt in pc.FORMATS.items():
            encs = [pc.make_encoder(sim, cfg) for _ in lens]
            got, _ = pc.batch_pcm(sim, encs, fmt, [p[0] for p in pcms], [p[1] for p in pcms])
            assert [g + e.flush() for g, e in zip(got, encs)] == want, (cfg, name)
            for e in encs:
                e.close()
    cases = [c for c in G if c["kind"] in ("frac", "hot") and c["name"] == "m1_128_stereo"]
    for fmt in (F32, F32 | INTER):
        data = [pc.case_pcm(c) for c in cases]
        encs = [pc.make_encoder(sim, c) for c in cases]
        got = [b""] * len(cases)
        for k in range(len(cases[0]["call_lens"])):
            part, _ = pc.batch_pcm(sim, encs, fmt, [d[0][1152 * k:1152 * (k + 1)] for d in data], [d[1][1152 * k:1152 * (k + 1)] for d in data])
            got = [g + p for g, p in zip(got, part)]
        for c, g, e in zip(cases, got, encs):
            assert hashlib.md5(g).hexdigest() == c["enc_md5"] and hashlib.md5(e.flush()).hexdigest() == c["flush_md5"], (c["kind"], fmt)
            e.close()


BAD = pc.BAD


@pytest.mark.parametrize("libname", ["sim", "wavesim"])
def test_refused_samples_on_the_host_entries(libname, request, G):
    """NaN, +inf, 131072.5 and -1e9: -4, the text names index and value, the stream is untouched -- the next good calls give the bytes of a
    run without the bad call.  131072.0 itself is inside the contract."""
    lib = request.getfixturevalue(libname)
    case = next(c for c in G if c["kind"] == "frac" and c["name"] == "m1_128_stereo")
    L, R, _, _ = pc.case_pcm(case)
    for fmt in (F32, F32 | INTER):
        enc = pc.make_encoder(lib, case)
        got = b""
        for k, n in enumerate(case["call_lens"]):
            l, r = L[1152 * k:1152 * k + n], R[1152 * k:1152 * k + n]
            if k in (0, 2, 5, 9):
                v = BAD[(0, 2, 5, 9).index(k)]
                bl, br = l.copy(), r.copy()
                idx = 100 + 7 * k
                (br if k % 2 else bl)[idx] = v
                state = enc.state_get()
                assert pc.encode_fmt(lib, enc, fmt, bl, br, strict=False) == -4
                msg = lib.lhip_last_error().decode()
                assert f"index {idx}" in msg and f"channel {k % 2}" in msg and ("nan" in msg.lower() or "inf" in msg.lower() or "131072" in msg or "-1e+09" in msg), msg
                assert enc.state_get() == state
            got += pc.encode_fmt(lib, enc, fmt, l, r)
        assert hashlib.md5(got).hexdigest() == case["enc_md5"] and hashlib.md5(enc.flush()).hexdigest() == case["flush_md5"]
        enc.close()
    # the batch entry: a bad sample in one stream refuses the whole batch, no stream consumes anything
    encs = [pc.make_encoder(lib, case) for _ in range(3)]
    states = [e.state_get() for e in encs]
    bad = L[:1152].copy()
    bad[5] = np.float32("nan")
    rc, wr = pc.batch_pcm(lib, encs, F32, [L[:1152], bad, L[:1152]], [R[:1152]] * 3)
    assert rc == -4 and wr == [-4, -4, -4] and "stream 1" in lib.lhip_last_error().decode() and "index 5" in lib.lhip_last_error().decode()
    assert [e.state_get() for e in encs] == states
    edge = pc.make_encoder(lib, case)
    top = np.full(1152, 131072.0, np.float32)
    assert isinstance(pc.encode_fmt(lib, edge, F32, top, -top), bytes)
    for e in encs + [edge]:
        e.close()


@pytest.mark.parametrize("libname", ["sim", "wavesim"])
def test_device_entry_reads_refused_samples_as_zero(libname, request):
    """The simulated device-pointer entry: pcmformats_cases.device_sanitise_check, the body the GPU tier runs, through the simulation's
    device entry (its device pointers are host pointers)."""
    lib = request.getfixturevalue(libname)
    assert pc.device_sanitise_check(lib, pc.sim_device_call, long_call=5 * 1152) == 60
    # nothing is counted, and nothing is refused, in an Int16 call
    enc = pc.make_encoder(lib, (2, 44100, 128))
    _, rejected = pc.sim_device_call(lib, enc, S16 | INTER, np.arange(1152), np.arange(1152))
    assert rejected == 0
    # a two-channel planar call without a right plane: both channels read the left one, each of its samples counts once
    l = np.zeros(1152, np.float32)
    l[[3, 700]] = np.float32("nan"), np.float32(2e5)
    _, rejected = pc.sim_device_call(lib, enc, F32, l, l, right_is_left=True)
    assert rejected == 2
    enc.close()


def test_existing_entries_are_the_s16_planar_case(sim, golden, golden_joint, golden_resv):
    """lhip_encode / lhip_encode_batch give the bytes they gave (a golden of each family), and lhip_encode_pcm(LHIP_PCM_S16) the same."""
    import lamejs_amd
    n = 0
    for fam, opts in ((golden, {}), (golden_joint, {"joint": True}), (golden_resv, {"reservoir": True})):
        case = next(c for c in fam if c["nsamples"] <= 400 * 1152 and c["channels"] == 2 and c.get("samplerate", 44100) == 44100 and c["corpus"] in ("sine", "bursts"))
        L, R = load_case_pcm(case)
        enc = lamejs_amd.Mp3Encoder(2, 44100, case["kbps"], lib=sim, joint=bool(case.get("joint")) or bool(opts.get("joint")), reservoir=bool(opts.get("reservoir")))
        chunk = case.get("chunk") or 1152
        got = b"".join(enc.encodeBuffer(L[p:p + chunk], R[p:p + chunk]) for p in range(0, len(L), chunk)) + enc.flush()
        enc.close()
        assert hashlib.md5(got).hexdigest() == case["mp3_md5"], case
        enc = lamejs_amd.Mp3Encoder(2, 44100, case["kbps"], lib=sim, joint=bool(case.get("joint")) or bool(opts.get("joint")), reservoir=bool(opts.get("reservoir")))
        got2 = b"".join(pc.encode_fmt(sim, enc, S16, L[p:p + chunk], R[p:p + chunk]) for p in range(0, len(L), chunk)) + enc.flush()
        enc.close()
        assert got2 == got
        n += 1
    assert n == 3


def test_python_mirror_dispatches_on_dtype(sim, G):
    """encodeBuffer / encode_streams: integer dtypes as always, floating dtypes through the Float32 entries (float64 is rounded to Float32, as the
    reference's store into its Float32Array does); encode_interleaved."""
    import lamejs_amd
    case = next(c for c in G if c["kind"] == "frac" and c["name"] == "m1_128_stereo")
    L, R, A, B = pc.case_pcm(case)
    enc = pc.make_encoder(sim, case)
    got = b"".join(enc.encodeBuffer(L[p:p + 1152].astype(np.float64), R[p:p + 1152]) for p in range(0, len(L), 1152))
    assert hashlib.md5(got).hexdigest() == case["enc_md5"] and hashlib.md5(enc.flush()).hexdigest() == case["flush_md5"]
    enc.close()
    enc = pc.make_encoder(sim, case)
    got = b"".join(enc.encode_interleaved(pc.interleave(L[p:p + 1152], R[p:p + 1152])) for p in range(0, len(L), 1152))
    assert hashlib.md5(got).hexdigest() == case["enc_md5"]
    enc.close()
    from oracle_py import oracle_encode
    want = oracle_encode(2, 44100, 128, A, B)
    a, b = pc.make_encoder(sim, case), pc.make_encoder(sim, case)
    assert a.encode_interleaved(pc.interleave(A, B)) + a.flush() == want
    res = lamejs_amd.encode_streams([a2 := pc.make_encoder(sim, case), b], [A, A.astype(np.float32)], [B, B])      # mixed dtypes: one Float32 batch
    assert res == [want, want]
    res = lamejs_amd.encode_streams([c2 := pc.make_encoder(sim, case)], [pc.interleave(A, B)], interleaved=True)
    assert res == [want]
    with pytest.raises(lamejs_amd.LhipError, match="index 3"):
        bad = L[:1152].copy()
        bad[3] = np.inf
        c2.encodeBuffer(bad, R[:1152])
    for e in (a, b, a2, c2):
        e.close()


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_beside_the_live_reference_hostsim(sim):
    """lamejs_amd/js on the one-lane simulation beside the live unmodified reference (tests/js_pcmformats_check.js): Float32Array, Float64Array and
    Array with fractional and beyond-16-bit values, Int16Array, encodeInterleaved, encodeBatch with mixed array types and { interleaved },
    a { pendingFrames } encoder that switches from Int16 to Float32 mid-stream, refused samples.  Call by call the reference's bytes -- which
    for Float32Array input are NOT the bytes of Int16Array.from(input), what the drop-in used to encode."""
    res = run_js_check("js_pcmformats_check.js", 20261, lib=HOSTSIM_SO)
    assert res["calls"] == 223 and res["batch_range_errors"] == 1 and res["mismatches"] == 0 and res["range_errors"] == 4 and res["differs_from_int16_coercion"] >= 3
    assert res["families"]["Float32Array"]["calls"] == 52 and 1 <= res["pending_nonempty_calls"] <= 4
