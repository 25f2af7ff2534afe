"""The output sample rate and the polyphase filter settings on the GPU: the goldens of the unmodified reference (tests/golden/golden_filters.json) through the
batch kernels and through one-frame calls, four cases -- zero bands at the bottom of the spectrum, a full 32-band spectrum at 128 kbps, 320 kbps in the
round-skip form, MPEG-2 frames from 44.1 kHz input at a clamped bitrate -- through the launch-path environments in fresh child processes with every
call's launch and path set checked, an 8-stream batch of mixed option sets, the reservoir case through g_resv_stream and the one-frame call through
g_frame.  Streams of 12 output frames.  Reads tests/golden/ only."""
import hashlib

import pytest

import filters_cases as fc
from libs import lib  # noqa: F401


@pytest.fixture(scope="module")
def G():
    return fc.goldens()


@pytest.mark.gpu
def test_gpu_goldens_through_the_batch_path(lib, G):
    """One call with all twelve frames' samples: g_prep where the stream resamples, g_poly ... g_quant_pair (quality 7: g_quant_fast), g_fixup, g_bits; reservoir
    streams g_resv_stream."""
    seen = set()
    for c in G:
        p = fc.run_golden_case(lib, c, lens=[c["nsamples"]])
        assert "SEPARATE" in p and ("PREP" in p) == (c["ref"]["resample_ratio"] != 1), (c["name"], sorted(p))
        if not c.get("reservoir"):
            rec = fc.launch_record(lib)          # (the flush's launch: the last batch of this thread)
            assert rec is None or rec["skip"] == (1 if fc.expected_skip_tail(c) else 0), (c["name"], rec)
        seen |= p
    assert {"QUANT_PAIR", "QUANT_FAST", "PSY4", "PREP", "RESV_STREAM_HELPERS"} <= seen and seen & {"FIXUP_SINGLE", "FIXUP_COOP"}


@pytest.mark.gpu
def test_gpu_goldens_in_their_own_calls(lib, G):
    """Twelve calls of one output frame's input each (g_frame; the reservoir: its one-frame program), and the uneven ones, whose long calls are batches."""
    seen = set()
    for c in G:
        seen |= fc.run_golden_case(lib, c)
    assert {"FRAME", "FRAME_RESV", "QUANT_PAIR"} <= seen


@pytest.mark.gpu
@pytest.mark.parametrize("env_name", fc.MATRIX_ENVS)
def test_gpu_launch_path_environments_on_the_four_new_states(env_name):
    """A fresh process per environment (the switches are read once per process): the four cases in their own calls, in one call and in two, bytes against the
    goldens, and per call the launch (lhip_debug_read(11)) and the paths (lhip_debug_last_paths)."""
    status, recs, text, fatal = fc.run_matrix("gpu", env_name, 120)
    assert status == 0 and not fatal, (env_name, status, text)
    assert fc.check_matrix(recs, env_name, "gpu") == [], env_name


@pytest.mark.gpu
def test_gpu_quality_7_goldens_through_the_general_kernels(G):
    res = fc.run_nofast("gpu", limit=120)
    assert res["cases"] == sum(1 for c in G if c.get("quality") == 7) and "QUANT_FAST" not in res["paths"] and set(res["paths"]) & {"QUANT_PAIR", "QUANT_PERSISTENT"}


@pytest.mark.gpu
def test_gpu_batch_of_eight_streams_with_mixed_option_sets(lib, G):
    """One lhip_encode_batch over eight blobs: highpass, no lowpass, a width, three output rates (MPEG-1 and MPEG-2, ratios 1, 2 and 4), one channel, quality 7 and a
    reservoir stream -- each stream its golden's bytes."""
    paths = fc.mixed_batch(lib, ["hp2000_w500_128", "lp_off_128", "lp12000_w2000_out44100_128", "out22050_44100_320", "out48000_lp15000_192000_64_mono", "lp16000_320",
                                 "q7_hp500_128", "resv_hp500_128"], G)
    assert "SEPARATE" in paths, sorted(paths)          # (each configuration gets launches of its own inside the call; the path word is the last group's)


@pytest.mark.gpu
def test_gpu_reservoir_batch_and_one_frame_calls(lib, G):
    """Eight reservoir streams with a highpass in one batch (g_resv_stream), a resampling reservoir stream, and a highpass stream fed one frame per call (g_frame)."""
    import lamejs_amd
    by = {c["name"]: c for c in G}
    for name in ("resv_hp500_128", "resv_out22050_44100_128"):
        c = by[name]
        L, R = fc.case_pcm(c)
        encs = [fc.make_encoder(lib, c) for _ in range(8)]
        got = lamejs_amd.encode_streams(encs, [L] * 8, [R] * 8, flush=False)
        paths = lamejs_amd.last_batch_paths(lib)
        got = [g + e.flush() for g, e in zip(got, encs)]
        for e in encs:
            e.close()
        assert not (fc.BATCH_QUANT_BITS & paths) and paths & {"RESV_STREAM_HELPERS", "RESV_STREAM_NOHELPERS"}, sorted(paths)
        assert all(hashlib.md5(g).hexdigest() == c["all_md5"] for g in got), name
    for name in ("hp2000_w500_128", "lp_off_128", "out22050_44100_320"):
        c = by[name]
        L, R = fc.case_pcm(c)
        enc, out, per, frames = fc.make_encoder(lib, c), b"", c["call_lens"][0], 0
        for p in range(0, c["nsamples"], per):
            part = enc.encodeBuffer(L[p:p + per], R[p:p + per])
            paths = lamejs_amd.last_batch_paths(lib)
            assert not part or ("FRAME" in paths and not (fc.BATCH_QUANT_BITS & paths)), (name, sorted(paths))
            frames += bool(part)
            out += part
        out += enc.flush()
        enc.close()
        assert hashlib.md5(out).hexdigest() == c["all_md5"] and frames >= 11, name
