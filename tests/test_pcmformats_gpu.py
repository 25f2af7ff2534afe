"""Sample formats of the C ABI -- Int16 / Float32, planar / interleaved -- on the GPU: the goldens of the unmodified reference (Float32Array
input), the random family against the oracle in every format on every launch path, device-resident batches per format, and the device
entry's sanitising.  Reads tests/golden/ and oracle/_ref/ only."""
import hashlib
import sys

import numpy as np
import pytest

import pcmformats_cases as pc
from conftest import ROOT
from libs import ADDON, NODE, lib, run_check, run_js_check  # noqa: F401
from pcmformats_cases import F32, INTER, S16


@pytest.mark.gpu
def test_gpu_every_golden_case(lib):
    """Float32 planar and Float32 interleaved: every call and the flush of all 44 cases; no case is skipped."""
    G = pc.golden_floatpcm()
    assert pc.run_all_goldens(lib, G, F32) == {k: 11 for k in pc.KINDS}
    assert pc.run_all_goldens(lib, G, F32 | INTER) == {k: 11 for k in pc.KINDS}


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["f32_planar", "f32_interleaved", "s16_interleaved", "mixed"])
def test_gpu_random_family_equals_the_oracle(lib, fmt):
    """Per-stream calls: 1152-sample calls are one-frame launches (g_frame<0>, with the reservoir g_frame<1>), a few frames of two channels in
    one call the pair kernel (g_quant_pair) -- the family's calls stay at or below 60 frames, far below the pair threshold of 6 x CUs frame slots, so
    its two-channel cases never reach the persistent kernel; its one-channel cases always take it (g_quant) --, several reservoir frames in one call
    g_resv_stream.  (The two-channel persistent kernel on every configuration family: tests/test_path_matrix_gpu.py.)"""
    order = [S16, F32 | INTER, F32, S16 | INTER]
    fam = pc.family(20271, 84) + pc.family(20272, 28, max_frames=60)
    for i, fc in enumerate(fam):
        pick = (lambda c: order[(c + i) % 4]) if fmt == "mixed" else (lambda c: pc.FORMATS[fmt])
        assert pc.family_encode(lib, fc, pick) == pc.family_oracle(fc), (fmt, fc["cfg"], fc["n"], fc["lens"][:4])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", sorted(pc.FORMATS))
def test_gpu_device_resident_batch(fmt):
    """lhip_encode_batch_device_pcm with sync = 0 over torch tensors (float32 / int16, planar / interleaved): many streams of many frames
    (two channels: about 100 frame slots, g_quant_pair; one channel: g_quant), one frame per stream (g_frame), reservoir streams (g_resv_stream)
    == the oracle (pcmformats_cases.device_batch_check, in a
    process of its own: torch initialises the GPU before the library is loaded)."""
    assert run_check([sys.executable, ROOT / "tests" / "pcmformats_cases.py", "--device-batch", fmt], timeout=600)["device_batches"] == 12


@pytest.mark.gpu
def test_gpu_host_batch_and_refused_samples(lib):
    G = pc.golden_floatpcm()
    case = next(c for c in G if c["kind"] == "hot" and c["name"] == "m1_128_stereo")
    L, R, _, _ = pc.case_pcm(case)
    for fmt in (F32, F32 | INTER):
        encs = [pc.make_encoder(lib, case) for _ in range(3)]
        got = [b""] * 3
        for k in range(len(case["call_lens"])):
            s = slice(1152 * k, 1152 * (k + 1))
            if k == 4:
                bad = L[s].copy()
                bad[17] = np.float32("inf")
                states = [e.state_get() for e in encs]
                rc, wr = pc.batch_pcm(lib, encs, fmt, [L[s], L[s], bad], [R[s]] * 3)
                msg = lib.lhip_last_error().decode()
                assert rc == -4 and wr == [-4] * 3 and "stream 2" in msg and "index 17" in msg and "inf" in msg.lower(), msg
                assert [e.state_get() for e in encs] == states
            part, _ = pc.batch_pcm(lib, encs, fmt, [L[s]] * 3, [R[s]] * 3)
            got = [g + p for g, p in zip(got, part)]
        for g, e in zip(got, encs):
            assert hashlib.md5(g).hexdigest() == case["enc_md5"] and hashlib.md5(e.flush()).hexdigest() == case["flush_md5"]
            e.close()
    # a long host call goes through the chunked path: Float32 planar and interleaved == the oracle on the same integers
    import pcm
    from oracle_py import oracle_encode
    A, B = pcm.sine(1152 * 17000, 2)
    want = hashlib.md5(oracle_encode(2, 44100, 128, A, B)).hexdigest()
    for fmt in (F32, F32 | INTER, S16 | INTER):
        enc = pc.make_encoder(lib, (2, 44100, 128))
        got = pc.encode_fmt(lib, enc, fmt, A, B) + enc.flush()
        enc.close()
        assert hashlib.md5(got).hexdigest() == want, fmt


@pytest.mark.gpu
def test_gpu_device_entry_reads_refused_samples_as_zero():
    """Once, in a process and under a time limit of its own (the CPU tier runs the same check on both simulations first)."""
    assert run_check([sys.executable, ROOT / "tests" / "pcmformats_cases.py", "--device-sanitise"], timeout=600)["device_sanitise_calls"] == 60


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_gpu_js_beside_the_live_reference():
    """lamejs_amd/js on the real library beside the live unmodified reference (tests/js_pcmformats_check.js), fresh seed: every family of
    array types call by call the reference's bytes."""
    res = run_js_check("js_pcmformats_check.js", 90417, timeout=600)
    assert res["calls"] == 223 and res["batch_range_errors"] == 1 and res["mismatches"] == 0 and res["range_errors"] == 4 and res["differs_from_int16_coercion"] >= 3
