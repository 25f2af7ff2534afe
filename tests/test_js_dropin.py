"""The JavaScript host (lamejs_amd/js: Mp3Encoder + N-API addon) must be a drop-in for the reference API:
same calls as the reference's Tests.js, same bytes as the goldens.  CPU run uses the host-simulation
library (logic only); the GPU run uses the real HIP library."""
import pytest

from libs import ADDON, HOSTSIM_SO, NODE, run_js_check


def _run(env_lib, corpus, ch, kbps, nfr, chunk, sr=44100, joint=False, reservoir=False):
    return run_js_check("js_dropin_check.js", corpus, ch, kbps, nfr, chunk, sr, *(["joint"] if joint else []), *(["reservoir"] if reservoir else []), lib=env_lib)


def _joint_cases(golden_joint):
    """Joint-stereo extension of the drop-in: an all-M/S stream, a mixed one, and an MPEG-2 one."""
    pick = [c for c in golden_joint if (c["corpus"], c["kbps"], c["nsamples"] // 1152, c.get("samplerate", 44100)) in
            (("centre_sine", 128, 300, 44100), ("bursts", 128, 400, 44100), ("centre_bursts", 64, 150, 22050))]
    assert len(pick) == 3
    return pick


def _cases(golden):
    """Three MPEG-1 cases, one MPEG-2 (22.05 kHz) and one that resamples 48 -> 24 kHz in front of the encoder."""
    ok = [c for c in golden if c["corpus"] in ("sine", "bursts") and not c.get("outside_envelope")]
    mpeg1 = [c for c in ok if 1152 * 200 <= c["nsamples"] <= 1152 * 400 and c.get("samplerate", 44100) == 44100 and c["kbps"] >= 128][:3]
    lsf = [c for c in ok if c.get("samplerate") == 22050 and c["nsamples"] <= 1152 * 150][:1]
    rs = [c for c in ok if c.get("samplerate") == 48000 and c["kbps"] == 64][:1]
    assert len(mpeg1) == 3 and lsf and rs
    return mpeg1 + lsf + rs


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_dropin_hostsim(golden):
    for c in _cases(golden):
        got = _run(HOSTSIM_SO, c["corpus"], c["channels"], c["kbps"], c["nsamples"] // 1152, c["chunk"], c.get("samplerate", 44100))
        assert got["md5"] == c["mp3_md5"] and got["bytes"] == c["mp3_len"], c


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_dropin_gpu(golden):
    for c in _cases(golden):
        got = _run(None, c["corpus"], c["channels"], c["kbps"], c["nsamples"] // 1152, c["chunk"], c.get("samplerate", 44100))
        assert got["md5"] == c["mp3_md5"] and got["bytes"] == c["mp3_len"], c


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_joint_stereo_extension_hostsim(golden_joint):
    """new Mp3Encoder(2, sr, kbps, { jointStereo: true }) == the reference core asked for MPEGMode.JOINT_STEREO (golden_joint.json)."""
    for c in _joint_cases(golden_joint):
        got = _run(HOSTSIM_SO, c["corpus"], 2, c["kbps"], c["nsamples"] // 1152, c["chunk"], c.get("samplerate", 44100), joint=True)
        assert got["md5"] == c["mp3_md5"] and got["bytes"] == c["mp3_len"], c


def _resv_cases(golden_resv):
    pick = [c for c in golden_resv if (c["corpus"], c["channels"], c["kbps"], c["nsamples"] // 1152, c.get("samplerate", 44100), bool(c.get("joint"))) in
            (("bursts", 2, 128, 400, 44100, False), ("sine", 1, 128, 300, 44100, False), ("centre_bursts", 2, 64, 150, 22050, True))]
    assert len(pick) == 3
    return pick


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_bit_reservoir_extension_hostsim(golden_resv):
    """new Mp3Encoder(ch, sr, kbps, { reservoir: true }) == the reference core with gfp.disable_reservoir = false (golden_resv.json)."""
    for c in _resv_cases(golden_resv):
        got = _run(HOSTSIM_SO, c["corpus"], c["channels"], c["kbps"], c["nsamples"] // 1152, c["chunk"], c.get("samplerate", 44100),
                   joint=bool(c.get("joint")), reservoir=True)
        assert got["md5"] == c["mp3_md5"] and got["bytes"] == c["mp3_len"], c


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_bit_reservoir_extension_gpu(golden_resv):
    for c in _resv_cases(golden_resv):
        got = _run(None, c["corpus"], c["channels"], c["kbps"], c["nsamples"] // 1152, c["chunk"], c.get("samplerate", 44100), joint=bool(c.get("joint")), reservoir=True)
        assert got["md5"] == c["mp3_md5"] and got["bytes"] == c["mp3_len"], c


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_joint_stereo_extension_gpu(golden_joint):
    for c in _joint_cases(golden_joint):
        got = _run(None, c["corpus"], 2, c["kbps"], c["nsamples"] // 1152, c["chunk"], c.get("samplerate", 44100), joint=True)
        assert got["md5"] == c["mp3_md5"] and got["bytes"] == c["mp3_len"], c


def _run_batch(env_lib, ch, kbps, nstreams, nfr, chunk):
    return run_js_check("js_batch_check.js", ch, kbps, nstreams, nfr, chunk, lib=env_lib)


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_batch_extension_hostsim():
    """encodeBatch / flushBatch (many independent streams per launch, BASELINE config 5 shape) == every stream on its own."""
    for ch, kbps, ns, nfr, chunk in ((1, 128, 3, 10, 3000), (2, 128, 2, 6, 1152)):
        got = _run_batch(HOSTSIM_SO, ch, kbps, ns, nfr, chunk)
        assert got["single"] == got["batch"] and len(got["batch"]) == ns


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_batch_extension_gpu():
    for ch, kbps, ns, nfr, chunk in ((1, 128, 16, 60, 5000), (2, 320, 5, 40, 1152 * 7)):
        got = _run_batch(None, ch, kbps, ns, nfr, chunk)
        assert got["single"] == got["batch"] and len(got["batch"]) == ns


def _shard(env_lib, corpus, ch, kbps, nfr, H, cuts):
    return run_js_check("js_shard_check.js", corpus, ch, kbps, nfr, H, *cuts, lib=env_lib)


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_frame_range_shards_hostsim():
    """The sharding extension through the JavaScript surface (seek / getState / setState; setDevices): pieces == whole == oracle."""
    import hashlib
    import pcm
    from oracle_py import oracle_encode
    for corpus, ch, nfr, H, cuts in (("sine", 2, 40, 8, [14, 27]), ("bursts", 1, 60, 2, [20, 41])):
        got = _shard(HOSTSIM_SO, corpus, ch, 128, nfr, H, cuts)
        L, R = pcm.CORPORA[corpus](1152 * nfr, ch)
        want = oracle_encode(ch, 44100, 128, L, R)
        assert got["whole"] == got["pieces"] == hashlib.md5(want).hexdigest() and got["bytes"] == len(want), got
        assert got["devices_allowed"] >= 1
        assert (got["missed"] == 0) if corpus == "sine" else (got["missed"] >= 1)


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_frame_range_shards_gpu():
    got = _shard(None, "sine", 2, 128, 300, 8, [100, 200])
    assert got["whole"] == got["pieces"] and got["missed"] == 0 and got["devices_allowed"] >= 1, got


def _pending(env_lib, corpus, ch):
    d = run_js_check("js_pending_check.js", corpus, ch, 128, 150, lib=env_lib)
    for k in ("pending64", "pending7", "pending5_odd_chunks", "pending3_big_chunks"):
        assert d[k]["md5"] == d["plain"]["md5"] and d[k]["bytes"] == d["plain"]["bytes"] and d[k]["second_flush_bytes"] == 0, (k, d)
    assert d["pending64"]["nonempty"] <= 3 < d["plain"]["nonempty"]


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_pending_frames_extension_hostsim():
    """{ pendingFrames: N } (extension): the 1152-sample call pattern with input held back until N frames are pending -- same byte stream as
    without it, whatever N and whatever the call sizes; flush() returns the rest and a second flush() nothing."""
    for corpus, ch in (("bursts", 2), ("sine", 1)):
        _pending(HOSTSIM_SO, corpus, ch)


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_pending_frames_extension_gpu():
    for corpus, ch in (("bursts", 2), ("sine", 1)):
        _pending(None, corpus, ch)


def _interleaved(env_lib, nfr):
    """tests/js_interleaved_check.js: seven live encoders of five configurations called in turn (two plain Mp3Encoder objects alternately, an encodeBatch group
    in between, joint stereo + reservoir, { pendingFrames } incl. its passage through encodeBatch / flushBatch); every stream == itself alone == the oracle."""
    import hashlib
    import pcm
    from oracle_py import oracle_encode
    d = run_js_check("js_interleaved_check.js", nfr, lib=env_lib)
    assert d["interleaved"] == d["alone"] and len(d["alone"]) == 7, d
    for name, corpus, ch, kbps, n, seed, kw in (("mono", "sine", 1, 128, 1152 * nfr + 100, 9001, {}), ("stereo", "bursts", 2, 128, 1152 * nfr + 200, 9002, {}),
                                                ("jr", "bursts", 2, 192, 1152 * nfr + 300, 9006, dict(joint=True, reservoir=True)), ("pend", "sine", 2, 128, 1152 * nfr + 50, 9007, {})):
        L, R = pcm.CORPORA[corpus](n, ch, seed=seed)
        want = oracle_encode(ch, 44100, kbps, L, R, **kw)
        assert d["alone"][name] == hashlib.md5(want).hexdigest() and d["bytes"][name] == len(want), name


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_interleaved_live_encoders_hostsim():
    _interleaved(HOSTSIM_SO, 14)


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_interleaved_live_encoders_gpu():
    _interleaved(None, 60)
