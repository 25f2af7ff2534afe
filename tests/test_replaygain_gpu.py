"""ReplayGain analysis (extension { replayGain }) on the GPU: the kernels g_gain_stage and g_gain.  The same bodies the CPU tier runs on the simulations
(tests/replaygain_cases.py): the exact anchor against the restatement of the reference, per-window energies and bins equal to the host simulation's bit for bit,
cut independence, the comparison with the reference beyond the anchor, the tag, the path bit.  Shapes are small: each test takes a few seconds."""
import numpy as np
import pytest

import infotag_cases as ic
import replaygain_cases as rc
from libs import lib, sim  # noqa: F401

G = rc.golden()
CASES = {c["name"]: c for c in G["cases"]}


@pytest.mark.gpu
@pytest.mark.parametrize("fs", rc.RATES)
def test_gpu_exact_anchor_and_simulation(lib, sim, fs):
    """Every rate, one and two channels, wf + 4 windows (at 8 kHz: 12 windows, 4800 samples): the windows whose warm-up starts at sample 0 have the restatement's
    lsum + rsum bit for bit and its bins; EVERY window's energy and bin equal the host simulation's bit for bit (the same C++, IEEE f64, no contraction)."""
    window, wf = rc.window_of(fs), rc.wf_of(fs)
    n = 4800 if fs == 8000 else wf + 4 * window + 13
    nanchor = wf // window + 1
    for ch in (1, 2):
        chans = rc.signal_for(fs, n, ch, seed=fs % 5 + ch)
        e, b = rc.gain_windows(lib, fs, chans)
        es, bs = rc.gain_windows(sim, fs, chans)
        assert len(e) == n // window >= nanchor
        assert [rc.bits(x) for x in e] == [rc.bits(x) for x in es] and list(b) == list(bs), (fs, ch)
        er, br = rc.analyse(fs, [c[:nanchor * window] for c in chans])
        assert [rc.bits(x) for x in e[:nanchor]] == [rc.bits(x) for x in er] and list(b[:nanchor]) == br, (fs, ch)


@pytest.mark.gpu
def test_gpu_second_wave_and_stream_bisection(lib, sim):
    """More than 64 windows of one stream (a second wave), and three streams of one batch with different lengths (the waves find their stream by bisection)."""
    import lamejs_amd
    fs = 8000
    chans = rc.signal_for(fs, 70 * 400 + 3, 2, seed=4)
    e, b = rc.gain_windows(lib, fs, chans)
    es, bs = rc.gain_windows(sim, fs, chans)
    assert len(e) == 70 and [rc.bits(x) for x in e] == [rc.bits(x) for x in es] and list(b) == list(bs)
    c = CASES["stereo_8000_24_mpeg25"]
    L, R = rc.corpus(c)
    res = {}
    for name, l in (("gpu", lib), ("sim", sim)):
        encs = [rc.make_encoder(l, c) for _ in range(3)]
        cut = [len(L), 3000, 399]
        lamejs_amd.encode_streams(encs, [L[:m] for m in cut], [R[:m] for m in cut], flush=False)
        res[name] = [(rc.nonzero(rc.histogram(l, e)), e.replay_gain()) for e in encs]
        if name == "gpu":
            assert "GAIN" in encs[0].last_batch_paths()
        for e in encs:
            e.close()
    assert res["gpu"] == res["sim"] and [r[1][1:] for r in res["gpu"]] == [(len(L) // 400, len(L)), (7, 3000), (0, 399)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stereo_48000_128", "resample_48000_24000_stereo_64", "mono_8000_16_mpeg25"])
def test_gpu_cut_independence(lib, name):
    """One call, 1152-sample calls, ragged calls; a two-stream batch of unequal lengths: the same histogram, count and bytes."""
    c = CASES[name]
    res = rc.cut_independence(lib, c)
    assert res[1:] == (c["windows"], c["fed"]) and (res[0] == c["RadioGain"] or not c["margin_ok"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_against_reference(lib, name):
    """5 (a) - (d) for every golden case: windows and samples, every bin within one, at most cap_windows() differing, tenth_db on the margin_ok cases."""
    c = CASES[name]
    A, res, _ = rc.run_case(lib, c)
    rc.check_against_reference(lib, c, A, res)
    if c["margin_ok"]:
        assert res[0] == c["RadioGain"]


@pytest.mark.gpu
@pytest.mark.parametrize("fs,ch,kbps,frames", [(44100, 2, 128, 30), (22050, 1, 32, 20)])
def test_gpu_against_restatement_44100_22050(lib, sim, fs, ch, kbps, frames):
    """44.1 kHz stereo, 30 frames in 1152-sample calls with flush (and 22.05 kHz mono): the restatement is the reference at these two rates; the stream's
    histogram also equals the host simulation's exactly."""
    c = {"name": f"full_{fs}", "channels": ch, "samplerate": fs, "kbps": kbps, "corpus": "sine", "nsamples": frames * 1152, "call": 1152, "out_samplerate": fs}
    A, res, data = rc.run_case(lib, c)
    As, ress, datas = rc.run_case(sim, c)
    assert (A == As).all() and res == ress and data == datas
    tenth, windows, samples = res
    assert samples > c["nsamples"] and windows == samples // rc.window_of(fs)
    analysed = rc.analysed_stream(c, fed=samples)
    _, ref_bins = rc.analyse(fs, analysed)
    rc.check_against_reference(lib, c, A, res, ref_bins, analysed)
    want, i = rc.result(ref_bins)
    if rc.tenth_at(i - 2) == want == rc.tenth_at(i + 2):
        assert tenth == want


@pytest.mark.gpu
def test_gpu_tag_and_path_bit(lib):
    """The radio field with infoTag (joint stereo, reservoir), the audio bytes identical with and without the option, LHIP_PATH_GAIN only with it; a
    device-pointer call stays asynchronous and still gives the histogram of the host call."""
    import lamejs_amd
    from test_replaygain_cpu import TAG_CASES, tag_check
    for name, c in TAG_CASES[:2]:
        tag_check(lib, dict(c, nsamples=8 * 1152))
    L, R = rc.pcm.sine(6 * 1152, 2)
    plain = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib)
    plain.encodeBuffer(L, R)
    assert "GAIN" not in plain.last_batch_paths()
    enc = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, replay_gain=True)
    enc.encodeBuffer(L, R)
    assert "GAIN" in enc.last_batch_paths() and enc.replay_gain()[1:] == (3, 6 * 1152)
    enc.encodeBuffer(L[:1152], R[:1152])
    assert {"GAIN", "FRAME"} <= enc.last_batch_paths()
    plain.close(), enc.close()
