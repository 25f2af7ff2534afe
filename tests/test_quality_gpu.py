"""The fast encoding mode (quality 7) on the GPU: the goldens of the unmodified reference through the bin-search-only kernel g_quant_fast (path
bit QUANT_FAST) and through the paths that keep the general program (one-frame calls: g_frame; the bit reservoir: g_resv_stream), a 64-stream
batch with the validation + repair pass behind the fast kernel, checked per stream against the oracle and repeated with the general kernels
forced in a child process, the random family, and a quality-3 stream beside them.  Streams of 12 to 20 frames.  Reads tests/golden/ only."""
import hashlib

import pytest

import quality_cases as qc
from libs import lib  # noqa: F401


@pytest.fixture(scope="module")
def G():
    G = qc.goldens()
    assert len(G) == 25
    return G


@pytest.mark.gpu
def test_gpu_goldens_through_the_batch_path(lib, G):
    """One call with all twelve frames' samples: g_psyA ... g_quant_fast, g_validate_fast, g_fixup, g_bits (reservoir streams: g_resv_stream)."""
    seen = set()
    for c in G:
        p = qc.run_golden_case(lib, c, lens=[c["nsamples"]], want_fast=True)
        assert ("QUANT_FAST" in p) == (not c.get("reservoir")), (c["name"], sorted(p))
        seen |= p
    assert {"QUANT_FAST", "PSY4", "PREP", "RESV_STREAM_HELPERS"} <= seen and seen & {"FIXUP_SINGLE", "FIXUP_COOP"} and not ({"QUANT_PAIR", "QUANT_PERSISTENT"} & seen)


@pytest.mark.gpu
def test_gpu_goldens_in_their_own_calls(lib, G):
    """Twelve calls of 1152 samples (g_frame: the general program, given the option), and the uneven ones, whose long calls are batches."""
    seen = set()
    for c in G:
        seen |= qc.run_golden_case(lib, c, want_fast=True)
    assert {"FRAME", "FRAME_RESV", "QUANT_FAST"} <= seen


@pytest.mark.gpu
def test_gpu_batch_of_64_streams_with_the_repair_pass_behind_the_fast_kernel(lib):
    """64 two-channel streams of 9 to 16 frames in one lhip_encode_batch: g_quant_fast, then g_validate_fast + g_fixup (the FIXUP bit), every stream
    the oracle's bytes; the same batch in a child process with LAMEJS_HIP_NO_FAST_QUANT=1 takes the general kernels and passes the same check."""
    paths = qc.batch64(lib, True)
    assert "QUANT_FAST" in paths and paths & {"FIXUP_SINGLE", "FIXUP_COOP"} and "SEPARATE" in paths, sorted(paths)
    res = qc.run_forced_general("batch64", timeout=300)
    assert not res["sim"] and "QUANT_FAST" not in res["paths"] and set(res["paths"]) & {"QUANT_PAIR", "QUANT_PERSISTENT"} and set(res["paths"]) & {"FIXUP_SINGLE", "FIXUP_COOP"}


@pytest.mark.gpu
def test_gpu_random_family_against_the_oracle(lib, G):
    """(the oracle is this family's reference because it reproduces the goldens: tests/test_quality_cpu.py makes that check; here on two of them)"""
    by = {c["name"]: c for c in G}
    assert qc.oracle_reproduces(by["q7_stereo_44100_128"]) and qc.oracle_reproduces(by["q7_joint_mixed_128"])
    assert qc.family_check(lib, qc.family(20301, 12), want_fast=True) == 12


@pytest.mark.gpu
def test_gpu_reservoir_batch_and_one_frame_calls_keep_the_general_program(lib, G):
    """A batch of eight reservoir streams (g_resv_stream) and a stream fed one frame per call (g_frame) do NOT take QUANT_FAST; their bytes are the
    reference's."""
    import lamejs_amd
    by = {c["name"]: c for c in G}
    c = by["q7_resv_stereo_128"]
    L, R = qc.case_pcm(c)
    encs = [qc.make_encoder(lib, c) for _ in range(8)]
    got = lamejs_amd.encode_streams(encs, [L] * 8, [R] * 8, flush=False)
    paths = lamejs_amd.last_batch_paths(lib)
    got = [g + e.flush() for g, e in zip(got, encs)]
    for e in encs:
        e.close()
    assert not (qc.BATCH_QUANT_BITS & paths) and paths & {"RESV_STREAM_HELPERS", "RESV_STREAM_NOHELPERS"}, sorted(paths)
    assert all(hashlib.md5(g).hexdigest() == c["all_md5"] for g in got)
    c = by["q7_stereo_44100_128"]
    L, R = qc.case_pcm(c)
    enc, out = qc.make_encoder(lib, c), b""
    for p in range(0, c["nsamples"], 1152):
        out += enc.encodeBuffer(L[p:p + 1152], R[p:p + 1152])
        paths = lamejs_amd.last_batch_paths(lib)
        assert "FRAME" in paths and not (qc.BATCH_QUANT_BITS & paths), sorted(paths)
    out += enc.flush()
    enc.close()
    assert hashlib.md5(out).hexdigest() == c["all_md5"]


@pytest.mark.gpu
def test_gpu_quality_3_stream_beside_the_fast_ones(lib, G):
    """The existing path in the same process, between two quality-7 batches: the reference's quality-3 bytes of the same input, through
    QUANT_PAIR / QUANT_PERSISTENT as always; and one batch call over encoders of both qualities."""
    import lamejs_amd
    by = {c["name"]: c for c in G}
    for name in ("q7_stereo_44100_128", "q7_mono_44100_64", "q7_joint_mixed_128"):
        c = by[name]
        L, R = qc.case_pcm(c)
        assert hashlib.md5(qc.encode_whole(lib, c["channels"], c["samplerate"], c["kbps"], L, R, **dict(qc.case_opts(c), quality=7))).hexdigest() == c["all_md5"]
        enc = qc.make_encoder(lib, c, quality=3)
        out = enc.encodeBuffer(L, R)
        paths = lamejs_amd.last_batch_paths(lib)
        out += enc.flush()
        enc.close()
        assert hashlib.md5(out).hexdigest() == c["q3_all_md5"] and "QUANT_FAST" not in paths and paths & {"QUANT_PAIR", "QUANT_PERSISTENT"}, (name, sorted(paths))
        assert hashlib.md5(qc.encode_whole(lib, c["channels"], c["samplerate"], c["kbps"], L, R, **dict(qc.case_opts(c), quality=8))).hexdigest() == c["all_md5"]
    c7, cj = by["q7_stereo_44100_128"], by["q7_joint_mixed_128"]
    (L, R), (JL, JR) = qc.case_pcm(c7), qc.case_pcm(cj)
    encs = [lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib), lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, quality=7), lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, quality=7, joint=True)]
    got = lamejs_amd.encode_streams(encs, [L, L, JL], [R, R, JR])
    for e in encs:
        e.close()
    assert [hashlib.md5(g).hexdigest() for g in got] == [c7["q3_all_md5"], c7["all_md5"], cj["all_md5"]]
