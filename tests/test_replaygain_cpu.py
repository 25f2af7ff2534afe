"""ReplayGain analysis (extension { replayGain }) -- CPU tier: the kernel bodies of g_gain_stage and g_gain in both simulations.  The restatement of the
reference's analysis (replaygain_cases.py) is first held to the live reference's golden exactly; then the kernels are held to it: bit for bit where a window's
warm-up reaches the stream's first sample, within one histogram step (and almost always equal) elsewhere; any cut of a stream into calls gives the same
histogram; the Info tag's radio field; blobs, refusals, the path bit; and the bounds of every load and store under AddressSanitizer in a stand-alone program."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import infotag_cases as ic
import replaygain_cases as rc
from conftest import ROOT
from libs import sim, wavesim  # noqa: F401

G = rc.golden()
CASES = {c["name"]: c for c in G["cases"]}
F32 = np.float32


# ---- 1. the restatement against the live reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_live_reference(name):
    """Exact: every histogram, every per-window bin where recorded, RadioGain, the window count."""
    c = CASES[name]
    energies, bins = rc.reference_of(name)
    assert len(bins) == c["windows"] == c["fed"] // rc.window_of(c["out_samplerate"])
    assert rc.nonzero(np.bincount(bins, minlength=rc.BINS)) == {int(k): v for k, v in c["histogram"].items()}
    if "bins" in c:
        assert bins == c["bins"]
    tenth, i = rc.result(bins)
    assert tenth == c["RadioGain"] and i == c["percentile_bin"]
    assert c["margin_ok"] == int(rc.tenth_at(i - 2) == tenth == rc.tenth_at(i + 2))


def test_golden_file_is_what_the_checks_assume():
    assert set(int(k) for k in G["wf"]) == set(rc.RATES) and all(G["wf"][str(fs)] == rc.wf_of(fs) for fs in rc.RATES)          # the counts were taken with the library's warm-up
    assert {c["out_samplerate"] for c in G["cases"]} == {48000, 32000, 24000, 16000, 12000, 11025, 8000} and sum(1 for c in G["cases"] if "bins" in c) == 2
    assert 4 * sum(c["margin_ok"] for c in G["cases"]) >= 3 * len(G["cases"])
    worst = max(c["restart_diff"] / c["windows"] for c in G["cases"])
    assert all(2 * c["restart_diff"] <= rc.cap_windows(c["windows"], worst) for c in G["cases"])          # the reference's own share stays below half the cap
    assert any(c.get("downmix") for c in G["cases"]) and any(c["samplerate"] != c["out_samplerate"] for c in G["cases"]) and any(c.get("jointStereo") for c in G["cases"])


@pytest.mark.parametrize("p", G["partial"], ids=lambda p: p["name"])
def test_restatement_equals_live_reference_44100_22050(p):
    """The two rates whose window is no multiple of eight: both filters' Float32 outputs and the running sums after 2200 / 1096 samples, bit for bit."""
    fs, n = p["out_samplerate"], p["fed"]
    chans = rc.analysed_stream(p)
    assert rc.analysed_md5(chans) == p["analysed_md5"] and fs in (44100, 22050) and n < rc.window_of(fs) and n % 8 == 0
    md5 = lambda a: hashlib.md5(np.asarray(a, "<f4").tobytes()).hexdigest()
    sums = []
    for c, side in zip(chans, "lr"):
        step, out = rc.filter_channel(fs, c)
        assert md5(step) == p[side + "step_md5"] and md5(out) == p[side + "out_md5"], side
        if side == "l":
            assert [int(v) for v in np.asarray(out[-16:], "<f4").view("<i4")] == p["lout_tail_bits"]
        sums.append(rc.window_sum(out, 0, n))
    hexof = lambda x: np.float64(x).tobytes().hex()
    assert hexof(sums[0]) == p["lsum_hex"] and hexof(sums[-1]) == p["rsum_hex"]


# ---- 2. the exact anchor ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("libname", ["sim", "wavesim"])
@pytest.mark.parametrize("fs", rc.RATES)
def test_exact_anchor(libname, fs, request):
    """Every rate, one and two channels: the windows whose warm-up starts at sample 0 have the restatement's lsum + rsum bit for bit and its bins; the window
    behind them equals the restatement restarted wf samples ahead bit for bit (the kernels' own definition)."""
    lib = request.getfixturevalue(libname)
    window, wf = rc.window_of(fs), rc.wf_of(fs)
    nanchor = wf // window + 1
    n = (nanchor + 1) * window + 5
    for ch in (1, 2):
        chans = rc.signal_for(fs, n, ch, seed=fs % 7 + ch)
        e, b = rc.gain_windows(lib, fs, chans)
        er, br = rc.analyse(fs, chans)
        ek, bk = rc.analyse(fs, chans, restart=wf)
        assert len(e) == nanchor + 1
        assert [rc.bits(x) for x in e[:nanchor]] == [rc.bits(x) for x in er[:nanchor]] and list(b[:nanchor]) == br[:nanchor], (fs, ch)
        assert [rc.bits(x) for x in e] == [rc.bits(x) for x in ek] and list(b) == bk, (fs, ch)


# ---- 4. cut independence ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stereo_48000_128", "resample_48000_24000_stereo_64", "downmix_48000_96", "mono_8000_16_mpeg25", "resv_stereo_48000_128"])
def test_cut_independence_hostsim(sim, name):
    """One call, 1152-sample calls (shorter than wf at 48 kHz), ragged calls of 1, 7, 9, 11, window - 1, window + 1, 1152 samples and the rest; two streams of
    different lengths in one batch: the same histogram, count and bytes."""
    res = rc.cut_independence(sim, CASES[name])
    assert res == (CASES[name]["RadioGain"] if CASES[name]["margin_ok"] else res[0], CASES[name]["windows"], CASES[name]["fed"])


def test_cut_independence_wavesim(wavesim):
    c = dict(CASES["stereo_8000_24_mpeg25"], nsamples=5 * 1152)
    rc.cut_independence(wavesim, c, with_batch=False)


def test_stream_shorter_than_one_window(sim):
    """No window complete: lhip_replay_gain returns 1 (None here) and the count.  (A flushed stream always has one: the flush alone feeds 2528 samples to a
    stream of a few samples at 48 kHz, more than the longest window -- so the tag, which exists only after the flush, never meets the case; its zero radio
    field is what test_tag_radio_field sees on the stream without the option.)"""
    import lamejs_amd
    enc = lamejs_amd.Mp3Encoder(1, 48000, 64, lib=sim, replay_gain=True, info_tag=True)
    L, _ = rc.pcm.sine(700, 1)
    enc.encodeBuffer(L[:300])
    assert enc.replay_gain() == (None, 0, 300)
    enc.encodeBuffer(L[300:])
    assert enc.replay_gain() == (None, 0, 700)
    enc.flush()
    tenth, windows, samples = enc.replay_gain()
    assert tenth is not None and windows == 1 and samples == 2528
    assert ic.parse_tag(enc.info_tag_frame())["radio_gain"] == rc.tag_field(tenth)
    enc.close()


# ---- 5. against the reference, beyond the anchor -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_against_reference_hostsim(sim, name):
    """(a) windows and samples equal the reference's (which pins what the flush feeds), (b) every window's bin within one of the reference's, (c) at most
    cap_windows() of them differ at all, (d) tenth_db equal where the case is margin_ok."""
    c = CASES[name]
    A, res, _ = rc.run_case(sim, c)
    rc.check_against_reference(sim, c, A, res)
    if c["margin_ok"]:
        assert res[0] == c["RadioGain"]


@pytest.mark.parametrize("fs,ch,kbps,frames", [(44100, 2, 128, 12), (22050, 1, 32, 12)])
def test_against_restatement_44100_22050(sim, fs, ch, kbps, frames):
    """At full length the restatement is the reference for these two rates.  The samples the flush adds are zeros whose number the seven other rates pin."""
    c = {"name": f"full_{fs}", "channels": ch, "samplerate": fs, "kbps": kbps, "corpus": "sine", "nsamples": frames * 1152, "call": 1152, "out_samplerate": fs}
    A, res, _ = rc.run_case(sim, c)
    tenth, windows, samples = res
    assert samples > c["nsamples"] and windows == samples // rc.window_of(fs)
    analysed = rc.analysed_stream(c, fed=samples)
    _, ref_bins = rc.analyse(fs, analysed)
    rc.check_against_reference(sim, c, A, res, ref_bins, analysed)
    want, i = rc.result(ref_bins)
    if rc.tenth_at(i - 2) == want == rc.tenth_at(i + 2):          # (margin_ok, as the generator defines it)
        assert tenth == want


def test_against_reference_wavesim(wavesim):
    c = CASES["stereo_8000_24_mpeg25"]
    A, res, _ = rc.run_case(wavesim, c)
    rc.check_against_reference(wavesim, c, A, res)
    assert res[0] == c["RadioGain"]


# ---- 6. the tag ------------------------------------------------------------------------------------------------------------------------------------------------
TAG_CASES = [("joint", dict(channels=2, samplerate=44100, kbps=128, jointStereo=1, corpus="centre_bursts")), ("reservoir", dict(channels=2, samplerate=44100, kbps=128, reservoir=1, corpus="sine")),
             ("protect", dict(channels=2, samplerate=48000, kbps=128, protect=1, corpus="bursts")), ("downmix", dict(channels=2, samplerate=44100, kbps=128, downmix=1, corpus="sine"))]


def tag_check(lib, c, encode=None):
    """With infoTag and replayGain the radio field is the encoding of lhip_replay_gain's value, peak and audiophile are zero, every other byte (the tag CRC aside)
    is the frame of the same stream without replayGain, and the audio bytes are identical with and without the option."""
    L, R = rc.corpus(c)
    out = {}
    for rg in (True, False):
        enc = rc.make_encoder(lib, c, replay_gain=rg, info_tag=True)
        data = encode(enc, L, R) if encode else rc.encode_cut(enc, L, R, [1152] * (len(L) // 1152), flush=False)
        data += enc.flush()
        out[rg] = (data, enc.info_tag_frame(), enc.replay_gain() if rg else None)
        if not rg:
            with pytest.raises(Exception, match="replayGain option"):
                enc.replay_gain()
        enc.close()
    (d1, f1, res), (d0, f0, _) = out[True], out[False]
    t1, t0 = ic.parse_tag(f1), ic.parse_tag(f0)
    assert d1 == d0 and res[0] is not None
    assert t1["radio_gain"] == rc.tag_field(res[0]) and t0["radio_gain"] == 0 and t1["peak"] == t1["audiophile_gain"] == 0
    at = t1["offset"] + 116 + 19          # the radio field
    crc = t1["tag_crc_offset"]
    assert f1[:at] == f0[:at] and f1[at + 2:crc] == f0[at + 2:crc] and f1[crc + 2:] == f0[crc + 2:] and len(f1) == len(f0)
    assert t1["tag_crc"] == ic.crc16(f1[:crc])
    return res


@pytest.mark.parametrize("name,c", TAG_CASES, ids=[n for n, _ in TAG_CASES])
def test_tag_radio_field(sim, name, c):
    tag_check(sim, dict(c, nsamples=8 * 1152))


def test_tag_radio_field_s24_interleaved(sim):
    import lamejs_amd
    import wavpcm_cases as wc
    c = dict(channels=2, samplerate=44100, kbps=128, corpus="sine", nsamples=8 * 1152)

    def encode(enc, L, R):
        return b"".join(enc.encode_pcm(wc.pack(wc.S24, wc.interleave(L[p:p + 2304].astype(np.int32) * 256, R[p:p + 2304].astype(np.int32) * 256)), lamejs_amd.PCM_S24) for p in range(0, len(L), 2304))
    res = tag_check(sim, c, encode)
    # 24-bit samples that are Int16 values times 256 are the Int16 stream: the same analysis
    L, R = rc.corpus(c)
    enc = rc.make_encoder(sim, c)
    rc.encode_cut(enc, L, R, [len(L)])
    assert enc.replay_gain() == res
    enc.close()


def test_tag_field_encoding():
    assert rc.tag_field(0) == 0x2C00 and rc.tag_field(-22) == 0x2C00 | 0x200 | 22 and rc.tag_field(600) == 0x2C00 | 0x1FE and rc.tag_field(-600) == 0x2E00 | 0x1FE


# ---- 7. blobs, refusals, the path bit ------------------------------------------------------------------------------------------------------------------------------
def test_blobs_without_the_option_are_unchanged():
    """All 324 triples: a blob built without the option is the blob the generator made before the option existed (the digests the Info tag change recorded
    from its parent, the generator's own hash entry zeroed), whether the option is absent, null or false; with it every entry keeps its bytes and cfg_i gains
    one named entry, replay_gain, at its end -- no array is added."""
    js = ("const t = require(process.argv[1]), crypto = require('crypto'); const out = {};"
          "const ents = (b) => { const n = b.readUInt32LE(8), e = {}; for (let i = 0; i < n; i++) { const p = 16 + 48 * i; e[b.toString('ascii', p, p + 32).replace(/\\0.*$/, '')] = [b.readUInt32LE(p + 36), b.readUInt32LE(p + 40)]; } return e; };"
          "const names = (b, e) => { let s = ''; for (let k = 0; k < e.cfg_i_names[0]; k++) { const c = b.readInt32LE(e.cfg_i_names[1] + 4 * k); if (!c) break; s += String.fromCharCode(c); } return s.split(','); };"
          "const body = (b, e, k, n) => b.slice(e[k][1], e[k][1] + n).toString('hex');"
          "for (const ch of [1, 2]) for (const sr of %s) for (const kb of %s) {"
          " const F = { fractionalResample: true };"
          " const a = Buffer.from(t.buildBlob(ch, sr, kb, F).blob), same = [null, false].every((v) => Buffer.compare(a, Buffer.from(t.buildBlob(ch, sr, kb, Object.assign({ replayGain: v }, F)).blob)) == 0);"
          " const g = Buffer.from(t.buildBlob(ch, sr, kb, Object.assign({ replayGain: true }, F)).blob), ea = ents(a), eg = ents(g), na = names(a, ea), ng = names(g, eg);"
          " let kept = Object.keys(eg).join(',') == Object.keys(ea).join(',') && ng.slice(0, na.length).join(',') == na.join(',') && ng.slice(na.length).join(',') == 'replay_gain';"
          " for (const k of Object.keys(ea)) { if (k == 'cfg_i_names') continue; const w = k == 'cfg_i' || k == 'cfg_d_names' || k == 'cfg_d' ? 4 : 1; kept = kept && ea[k][0] <= eg[k][0] && body(a, ea, k, Math.min(ea[k][0], 64) * w) == body(g, eg, k, Math.min(ea[k][0], 64) * w); }"
          " const z = Buffer.from(a); z.fill(0, ea.src_sha256_64[1], ea.src_sha256_64[1] + 8);"
          " out[ch + '_' + sr + '_' + kb] = [crypto.createHash('md5').update(z).digest('hex'), same ? 1 : 0, kept ? 1 : 0]; }"
          "console.log(JSON.stringify(out));" % (json.dumps(list(rc.RATES)), json.dumps([8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 192, 224, 256, 320])))
    r = subprocess.run(["node", "-e", js, str(ROOT / "lamejs_amd" / "js" / "tables.js")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = json.loads(r.stdout)
    parent = json.loads((ROOT / "tests" / "golden" / "infotag_blob_md5.json").read_text())["md5"]
    assert len(rows) == 324 == len(parent)
    for k, (md5, same, kept) in rows.items():
        assert md5 == parent[k] and same == 1 and kept == 1, k


def test_refusals_and_path_bit(sim):
    import lamejs_amd
    hdr = (ROOT / "include" / "lamejs_hip.h").read_text()
    assert re.search(r"#define LHIP_PATH_GAIN \(1u << 15\)", hdr) and lamejs_amd.PATH_BITS_ALL == lamejs_amd.PATH_BITS + ("GAIN",) and lamejs_amd.PATH_BITS_ALL.index("GAIN") == 15
    # -3: a stream that resamples by a non-integer ratio
    with pytest.raises(lamejs_amd.LhipError, match=r"\(-3\).*ReplayGain cannot be combined with fractionalResample"):
        lamejs_amd.Mp3Encoder(2, 22050, 32, lib=sim, fractional_resample=True, replay_gain=True)
    lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, fractional_resample=True, replay_gain=True).close()          # (harmless where nothing is resampled)
    # -4: no option; moved
    L, R = rc.pcm.sine(6 * 1152, 2)
    plain = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim)
    plain.encodeBuffer(L, R)
    assert "GAIN" not in plain.last_batch_paths()
    t, w, n = (rc.ctypes.c_int32(), rc.ctypes.c_int64(), rc.ctypes.c_int64())
    assert sim.lhip_replay_gain(plain._h, rc.ctypes.byref(t), rc.ctypes.byref(w), rc.ctypes.byref(n)) == -4 and b"replayGain option" in sim.lhip_last_error()
    enc = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, replay_gain=True)
    enc.encodeBuffer(L, R)
    assert "GAIN" in enc.last_batch_paths() and enc.replay_gain()[1] == 3
    enc.encodeBuffer(L[:1152], R[:1152])          # the one-frame call
    assert {"GAIN", "FRAME"} <= enc.last_batch_paths()
    plain.encodeBuffer(L[:1152], R[:1152])
    assert "GAIN" not in plain.last_batch_paths()
    state = plain.state_get()
    assert len(state) == len(enc.state_get())          # the state blob does not know the option
    enc.state_set(enc.state_get())
    with pytest.raises(lamejs_amd.LhipError, match=r"\(-4\).*moved"):
        enc.replay_gain()
    fresh = lamejs_amd.Mp3Encoder(1, 44100, 128, lib=sim, replay_gain=True)
    tail = np.zeros(fresh.seek_tail_samples(), np.int16)
    fresh.seek(4 * 1152, tail)
    with pytest.raises(lamejs_amd.LhipError, match=r"\(-4\).*moved"):
        fresh.replay_gain()
    for e in (plain, enc, fresh):
        e.close()


# ---- 8. bounds: a stand-alone program under AddressSanitizer, both simulations --------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave", [False, True], ids=["one_lane", "wave"])
def test_bounds_under_asan(tmp_path, wave):
    """tests/tools/replaygain_bounds.c with lhip_api.cpp, -fsanitize=address, the flags of tests/hostsim/Makefile: the kernels' bodies on heap blocks that end with
    the data -- history that shifts, a call of one sample, a call ending on a window boundary.  Nothing goes through Python, nothing is preloaded."""
    mk = (ROOT / "tests" / "hostsim" / "Makefile").read_text()
    flags = re.search(r"^CXXFLAGS = (.*)$", mk, flags=re.M).group(1).split()
    flags = [f for f in flags if f not in ("-shared", "-fPIC", "-O2")]
    exe = tmp_path / "replaygain_bounds"
    blob = tmp_path / "t.bin"
    import lamejs_amd
    blob.write_bytes(lamejs_amd.tables_blob(2, 8000, 24, replay_gain=True))
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-fsanitize=address", "-static-libasan", *flags] + (["-DLHIP_WAVESIM"] if wave else []) + \
          ["-I", str(ROOT / "include"), "-x", "c++", str(ROOT / "tests" / "tools" / "replaygain_bounds.c"), str(ROOT / "lamejs_amd" / "csrc" / "lhip_api.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "replaygain_bounds OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
