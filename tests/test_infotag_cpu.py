"""The Info/LAME tag frame ({ infoTag }; extension).  CPU tier: both simulations are built from the kernel sources (tests/hostsim), so the music CRC
of a large call comes from the device functions of k_crc.h -- walked by one lane in the host simulation, spread over 64 lanes with an XOR
reduction in the wave simulation -- and that of a small call from the host's table CRC.  Yardsticks: tests/infotag_cases.py."""
import ctypes
import hashlib
import json
import re
import subprocess

import numpy as np
import pytest

import infotag_cases as ic
import pcm
from conftest import ROOT
from libs import NODE, sim, wavesim  # noqa: F401

RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000]
KBPS = [8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 192, 224, 256, 320]
TABLES_JS = str(ROOT / "lamejs_amd" / "js" / "tables.js")
# the wave simulation runs 64 fibers per wave: a subset that still has both granule counts, the reservoir with joint stereo, protection and calls without bytes
WAVESIM_CASES = ("mono_16000_40_mpeg2", "joint_resv_128", "protect_mono_22050_56", "calls_of_100")


@pytest.fixture(scope="module")
def G():
    return ic.goldens()


def test_yardstick_crc_is_crc16_arc():
    """The bitwise CRC of the tests: the catalogued check value of CRC-16/ARC over "123456789" is 0xbb3d; and the two properties the kernel
    stands on -- crc(A ++ B) follows from crc(A), crc(B) and |B| alone (shown on the bytes), leading zero bytes change nothing."""
    assert ic.crc16(b"123456789") == 0xBB3D and ic.crc16(b"") == 0
    a, b = b"\x01\x80\xff\x10 something", b"\x00\x7f and more"
    assert ic.crc16(a + b) == ic.crc16(bytes(len(b)), ic.crc16(a)) ^ ic.crc16(b)
    assert ic.crc16(bytes(77) + a) == ic.crc16(a)


def test_golden_set_is_the_one_asked_for(G):
    by = {c["name"]: c for c in G}
    assert {c["channels"] for c in G} == {1, 2}
    assert {(c["out_samplerate"] >= 32000, c["out_samplerate"] < 16000) for c in G} == {(True, False), (False, False), (False, True)}      # MPEG-1, MPEG-2, MPEG-2.5
    assert by["stereo_48000_64_resample_int"]["out_samplerate"] * 2 == by["stereo_48000_64_resample_int"]["samplerate"]
    for opts in ({"jointStereo"}, {"reservoir"}, {"jointStereo", "reservoir"}, {"protect"}, {"downmix"}):
        assert any(opts <= {k for k in ("jointStereo", "reservoir", "protect", "downmix") if c.get(k)} for c in G), opts
    d = by["downmix_unequal_gains"]
    assert d["downmix"] and d["scaleLeft"] != d["scaleRight"] and d["ref_channels_out"] == 1
    assert set(by["calls_of_100"]["call_lens"]) <= {100, by["calls_of_100"]["nsamples"] % 100} and by["calls_of_100"]["call_bytes"].count(0) > 100
    assert by["one_call"]["call_lens"] == [by["one_call"]["nsamples"]]
    assert {c["encoder_padding"] for c in G} == {1691, 1115} and {c["encoder_delay"] for c in G} == {576} and {c["version_string"] for c in G} == {"LAME3.98r"}
    for c in G:
        assert 12 <= c["frameNum"] <= 20 and c["nsamples"] % 576 in (37, 74) and c["total_bytes"] == sum(c["call_bytes"]) + c["flush_len"]


def test_hostsim_crc_kernel_body_against_the_bitwise_crc(sim):
    assert ic.check_crc_table(sim, 20290) == 12 * 16


def test_wavesim_crc_kernel_body_against_the_bitwise_crc(wavesim):
    assert ic.check_crc_table(wavesim, 20291) == 12 * 16


def test_crc_entry_refuses_bad_arguments(sim):
    r = ctypes.c_uint32()
    buf = np.zeros(4, dtype=np.uint8)
    assert sim.lhip_debug_crc16(buf.ctypes.data, 4, 16, ctypes.byref(r)) < 0 and sim.lhip_debug_crc16(None, 4, 0, ctypes.byref(r)) < 0
    assert sim.lhip_debug_crc16(buf.ctypes.data, 4, 0, None) < 0 and b"lhip_debug_crc16" in sim.lhip_last_error()


def test_hostsim_every_golden(sim, G):
    for c in G:
        ic.run_golden_case(sim, c)


def test_hostsim_every_golden_in_one_call(sim, G):
    """One call with the whole stream: large enough, for the bigger configurations, to leave the small-call path -- the CRC then comes from the
    kernel body, and must be the one the recorded call lengths gave."""
    import lamejs_amd
    seen = set()
    for c in G:
        ic.run_golden_case(sim, c, lens=[c["nsamples"]])
        seen |= lamejs_amd.last_batch_paths(sim)
    assert "SMALL_CALL" in seen


def test_wavesim_goldens(wavesim, G):
    for c in G:
        if c["name"] in WAVESIM_CASES:
            ic.run_golden_case(wavesim, c)


def _device_path_stream(lib, kw, frames, ch=2, kbps=128, sr=44100):
    """A stream through the NO-SMALL-CALLS path is not available from a test; a device-pointer batch is: in the simulations device memory is
    host memory, so the kernel body runs over the call's bytes where the formatter left them (the placeholder in front, at an odd address)."""
    import lamejs_amd
    L, R = pcm.bursts(frames * 1152, ch)
    enc = lamejs_amd.Mp3Encoder(ch, sr, kbps, lib=lib, info_tag=True, **kw)
    cap = lib.lhip_max_output_bytes(enc._h, len(L))
    out = np.zeros(cap, dtype=np.uint8)
    H, lp, rp = (ctypes.c_void_p * 1)(enc._h), (ctypes.c_void_p * 1)(L.ctypes.data), (ctypes.c_void_p * 1)((R if R is not None else L).ctypes.data)
    ns, op, cp, wr = (ctypes.c_size_t * 1)(len(L)), (ctypes.c_void_p * 1)(out.ctypes.data), (ctypes.c_size_t * 1)(cap), (ctypes.c_int64 * 1)()
    assert lib.lhip_encode_batch_device(H, 1, lp, rp, ns, op, cp, wr, 0) == 0, lib.lhip_last_error()
    paths = lamejs_amd.last_batch_paths(lib)
    body = out[:wr[0]].tobytes()
    nt = enc.stream_info()["tag_bytes"]
    tail = enc.flush()
    si, frame = enc.stream_info(), enc.info_tag_frame()
    enc.close()
    return body[:nt], body[nt:] + tail, si, frame, paths


@pytest.mark.parametrize("kind", ["hostsim", "wavesim"])
def test_device_pointer_call_takes_the_kernel_path(kind, request):
    lib = request.getfixturevalue("sim" if kind == "hostsim" else "wavesim")
    for kw in ({}, {"reservoir": True}):
        ph, audio, si, frame, paths = _device_path_stream(lib, kw, 5 if kind == "wavesim" else 45)
        assert "OUT_CRC" in paths and "SMALL_CALL" not in paths, paths
        assert si["music_crc"] == ic.crc16(audio) and si["audio_bytes"] == len(audio) and ic.parse_tag(frame)["music_crc"] == si["music_crc"], kw
        assert ic.header_fields(int.from_bytes(ph[:4], "big"))["frame_bytes"] == len(ph) == si["tag_bytes"]


def test_untagged_batches_do_not_take_the_new_path(sim):
    import lamejs_amd
    L, R = pcm.sine(3 * 1152, 2)
    enc = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim)
    enc.encodeBuffer(L, R)
    assert "OUT_CRC" not in enc.last_batch_paths()
    with pytest.raises(lamejs_amd.LhipError, match="infoTag"):
        enc.stream_info()
    with pytest.raises(lamejs_amd.LhipError, match="infoTag"):
        enc.info_tag_frame()
    enc.close()


def test_path_bit_is_declared_and_mirrored():
    import lamejs_amd
    hdr = (ROOT / "include" / "lamejs_hip.h").read_text()
    assert re.search(r"#define LHIP_PATH_OUT_CRC \(1u << 13\)", hdr)
    assert lamejs_amd.PATH_NAMES_ALL[:13] == lamejs_amd.PATH_NAMES and lamejs_amd.PATH_NAMES_ALL[13] == "OUT_CRC" and len(lamejs_amd.PATH_NAMES_ALL) == 14


def test_long_host_call_keeps_its_crcs_in_the_call_log(sim):
    """A host call long enough to be cut into units (chunk schedule overridden in a child): the pieces' CRCs are logged on the device and folded
    into the stream's total after the last unit -- the same totals as frame-sized calls give."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import json, lamejs_amd, pcm, infotag_cases as ic\n"
            "from libs import HOSTSIM_SO\n"
            "lib = lamejs_amd.load_library(HOSTSIM_SO)\n"
            "L, R = pcm.bursts(40 * 1152 + 5, 2)\n"
            "a, b = (lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, info_tag=True) for _ in range(2))\n"
            "x = a.encodeBuffer(L, R); paths = sorted(a.last_batch_paths()); x += a.flush()\n"
            "y = b''.join(b.encodeBuffer(L[p:p + 1152], R[p:p + 1152]) for p in range(0, len(L), 1152)) + b.flush()\n"
            "nt = a.stream_info()['tag_bytes']\n"
            "print(json.dumps({'same': x == y, 'info': a.stream_info() == b.stream_info(), 'crc': a.stream_info()['music_crc'] == ic.crc16(x[nt:]), 'tag': a.info_tag_frame() == b.info_tag_frame(), 'paths': paths}))\n"
            % (str(ROOT), str(ROOT / "tests")))
    import os
    import sys
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, LAMEJS_HIP_HOST_CHUNK_FRAMES="8"))
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["same"] and res["info"] and res["crc"] and res["tag"] and "OUT_CRC" in res["paths"], res


def test_batch_of_tagged_beside_untagged_streams(sim):
    """encode_streams over 1, 2 and 37 frames, tagged and untagged mixed (infotag_cases.mixed_batch_check), and a batch of tagged reservoir
    streams of unequal lengths."""
    ic.mixed_batch_check(sim)
    ic.resv_batch_check(sim)


def test_long_stream_in_one_call_and_in_frame_sized_calls(sim):
    """As on the GPU, shorter: one call whose bytes span several workgroups of the kernel body against frame-sized calls on the host path."""
    one_call, small_calls = ic.long_stream_check(sim, 250)
    assert "OUT_CRC" in one_call and "OUT_CRC" not in small_calls and "SMALL_CALL" in small_calls


def test_output_size_calculators_count_the_pending_placeholder(sim):
    import lamejs_amd
    L, R = pcm.sine(4 * 1152, 2)
    for kw in ({}, {"reservoir": True}):
        a, b = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, **kw), lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, info_tag=True, **kw)
        nt = b.stream_info()["tag_bytes"]
        assert nt == 417
        for n in (1, 1152, 100000):
            assert sim.lhip_encode_output_bytes(b._h, n) == sim.lhip_encode_output_bytes(a._h, n) + nt and sim.lhip_max_output_bytes(b._h, n) == sim.lhip_max_output_bytes(a._h, n) + nt
        if not kw:      # (with the reservoir the entry returns the upper bound, which counts the pending placeholder whatever the length)
            assert sim.lhip_encode_output_bytes(b._h, 0) == sim.lhip_encode_output_bytes(a._h, 0)
        x, y = a.encodeBuffer(L[:100], R[:100]), b.encodeBuffer(L[:100], R[:100])          # the first call: no frame yet, the placeholder alone
        assert x == b"" and len(y) == nt
        for n in (1, 1152, 100000):
            assert sim.lhip_encode_output_bytes(b._h, n) == sim.lhip_encode_output_bytes(a._h, n) and sim.lhip_max_output_bytes(b._h, n) == sim.lhip_max_output_bytes(a._h, n)
        assert a.encodeBuffer(L[100:], R[100:]) + a.flush() == b.encodeBuffer(L[100:], R[100:]) + b.flush()
        a.close()
        b.close()
    # a buffer that cannot hold the placeholder: -1, and nothing is consumed
    e = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, info_tag=True)
    out = np.zeros(100, dtype=np.uint8)
    assert sim.lhip_encode(e._h, L.ctypes.data, R.ctypes.data, 100, out.ctypes.data, 100) == -1
    assert len(e.encodeBuffer(L[:100], R[:100])) == 417
    e.close()


def test_toc_bookkeeping_past_400_and_800_frames(sim):
    """The seek table's bag (at most 400 entries, halved when full) fed in batches against the frame-by-frame walk: below 400 frames, just
    across 400 and 800, far beyond, and in one batch of 1e5 frames."""
    for calls in ([1] * 399, [1] * 401, [399, 1, 1], [401], [37] * 25, [800, 1], [801], [1152, 3, 700], [100000], [1] * 850, [7, 100000, 13]):
        toc = (ctypes.c_uint8 * 100)()
        fr = (ctypes.c_int64 * len(calls))(*calls)
        pos = sim.lhip_debug_info_toc(fr, len(calls), 128, toc)
        want, want_pos = ic.toc_by_frames(sum(calls), 128)
        assert pos == want_pos and list(toc) == want, calls[:4]
        assert toc[0] == 0 and all(a <= b for a, b in zip(toc, list(toc)[1:]))
    toc = (ctypes.c_uint8 * 100)()
    assert sim.lhip_debug_info_toc(None, 0, 128, toc) == 0 and list(toc) == [0] * 100


def test_refusals(sim):
    import lamejs_amd
    # a frame too small for the tag: 8 kHz at 8 kbps is 72 bytes, the tag needs 13 + 156
    with pytest.raises(lamejs_amd.LhipError, match=r"\(-3\).*Info tag.*72 bytes"):
        lamejs_amd.Mp3Encoder(1, 8000, 8, lib=sim, info_tag=True)
    lamejs_amd.Mp3Encoder(1, 8000, 8, lib=sim).close()
    # a stream that resamples by a non-integer ratio
    with pytest.raises(lamejs_amd.LhipError, match=r"\(-3\).*fractionalResample"):
        lamejs_amd.Mp3Encoder(2, 22050, 32, lib=sim, fractional_resample=True, info_tag=True)
    lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, fractional_resample=True, info_tag=True).close()       # (harmless where nothing is resampled)
    with pytest.raises(ValueError):
        lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, info_tag=2)
    # the tag of a stream that was moved: the state entries do not carry the totals
    L, R = pcm.sine(8 * 1152, 2)
    e = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, info_tag=True)
    nt = e.seek_tail_samples()
    e.seek(4 * 1152, L[4 * 1152 - nt:4 * 1152], R[4 * 1152 - nt:4 * 1152])
    e.encodeBuffer(L[4 * 1152:], R[4 * 1152:])
    e.flush()
    with pytest.raises(lamejs_amd.LhipError, match=r"\(-4\).*lhip_seek or lhip_state_set"):
        e.info_tag_frame()
    e.close()
    a, b = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, info_tag=True), lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, info_tag=True)
    a.encodeBuffer(L[:4 * 1152], R[:4 * 1152])
    b.state_set(a.state_get())
    b.flush()
    with pytest.raises(lamejs_amd.LhipError, match=r"\(-4\)"):
        b.info_tag_frame()
    # before the flush
    with pytest.raises(lamejs_amd.LhipError, match=r"\(-4\).*not been flushed"):
        a.info_tag_frame()
    a.flush()
    assert len(a.info_tag_frame()) == 417
    a.close()
    b.close()


def test_state_blobs_do_not_change(sim):
    import lamejs_amd
    a, b = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim), lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, info_tag=True)
    assert sim.lhip_state_bytes(a._h) == sim.lhip_state_bytes(b._h) and a.state_get() == b.state_get()
    a.close()
    b.close()


@pytest.mark.skipif(NODE is None, reason="node not available")
def test_blob_without_the_option_is_unchanged():
    """All 324 triples: a blob built without the option is the blob the generator made before the option existed (its digest recorded from the
    parent's generator, the generator's own hash entry zeroed), whether the option is absent, null or false; with it, every existing
    entry keeps its bytes, cfg_i gains the tag's named entries at its end and the blob one array, tag_version."""
    js = ("const t = require(process.argv[1]), crypto = require('crypto'); const out = {};"
          "const ents = (b) => { const n = b.readUInt32LE(8), e = {}; for (let i = 0; i < n; i++) { const p = 16 + 48 * i; e[b.toString('ascii', p, p + 32).replace(/\\0.*$/, '')] = [b.readUInt32LE(p + 36), b.readUInt32LE(p + 40)]; } return e; };"
          "const names = (b, e) => { let s = ''; for (let k = 0; k < e.cfg_i_names[0]; k++) { const c = b.readInt32LE(e.cfg_i_names[1] + 4 * k); if (!c) break; s += String.fromCharCode(c); } return s.split(','); };"
          "const body = (b, e, k, n) => b.slice(e[k][1], e[k][1] + n).toString('hex');"
          "for (const ch of [1, 2]) for (const sr of %s) for (const kb of %s) {"
          " const F = { fractionalResample: true };"
          " const a = Buffer.from(t.buildBlob(ch, sr, kb, F).blob), same = [null, false].every((v) => Buffer.compare(a, Buffer.from(t.buildBlob(ch, sr, kb, Object.assign({ infoTag: v }, F)).blob)) == 0);"
          " const g = Buffer.from(t.buildBlob(ch, sr, kb, Object.assign({ infoTag: true }, F)).blob), ea = ents(a), eg = ents(g), na = names(a, ea), ng = names(g, eg);"
          " let kept = Object.keys(eg).filter((k) => !(k in ea)).join(',') == 'tag_version' && ng.slice(0, na.length).join(',') == na.join(',') && ng.slice(na.length).join(',') == 'info_tag,tag_quality,tag_method,tag_lowpass,tag_flags,tag_misc,tag_preset,tag_delay';"
          " for (const k of Object.keys(ea)) { if (k == 'cfg_i_names') continue; const w = k == 'cfg_i' || k == 'cfg_d_names' || k == 'cfg_d' ? 4 : 1; kept = kept && ea[k][0] <= eg[k][0] && body(a, ea, k, Math.min(ea[k][0], 64) * w) == body(g, eg, k, Math.min(ea[k][0], 64) * w); }"
          " const z = Buffer.from(a); z.fill(0, ea.src_sha256_64[1], ea.src_sha256_64[1] + 8);"
          " out[ch + '_' + sr + '_' + kb] = [crypto.createHash('md5').update(z).digest('hex'), same ? 1 : 0, kept ? 1 : 0]; }"
          "console.log(JSON.stringify(out));" % (json.dumps(RATES), json.dumps(KBPS)))
    r = subprocess.run([NODE, "-e", js, TABLES_JS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = json.loads(r.stdout)
    parent = json.loads((ROOT / "tests" / "golden" / "infotag_blob_md5.json").read_text())["md5"]
    assert len(rows) == 324 == len(parent)
    for k, (md5, same, kept) in rows.items():
        assert md5 == parent[k] and same == 1 and kept == 1, k


@pytest.mark.skipif(NODE is None, reason="node not available")
def test_tables_resolve_the_recorded_settings(G):
    """The tag's named entries of tables.js for every golden case against what the reference's own settings give (VBRTag.js:576-732)."""
    import lamejs_amd
    from protection_cases import cfg_entry
    for c in G:
        blob = lamejs_amd.tables_blob(c["channels"], c["samplerate"], c["kbps"], info_tag=True, **ic.case_opts(c))
        got = {k: cfg_entry(blob, k)[1] for k in ("info_tag", "tag_quality", "tag_method", "tag_lowpass", "tag_flags", "tag_misc", "tag_preset", "tag_delay")}
        assert got == {"info_tag": 1, "tag_quality": 100 - 10 * c["VBR_q"] - c["quality"], "tag_method": 1, "tag_lowpass": min(255, int(c["lowpassfreq"] / 100.0 + .5)),
                       "tag_flags": c["ATHtype"] + (c["exp_nspsytune"] << 4), "tag_misc": ic.expected_misc(c), "tag_preset": c["preset"], "tag_delay": c["encoder_delay"]}, c["name"]
    assert hashlib.md5(lamejs_amd.tables_blob(2, 44100, 128)).hexdigest() != hashlib.md5(lamejs_amd.tables_blob(2, 44100, 128, info_tag=True)).hexdigest()
