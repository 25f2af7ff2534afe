"""The fast encoding mode, quality 7 (LAME's -f; extension: the reference's wrapper always asks for 3).  CPU tier: the blob and the resolved
switches, refusals, the unmodified reference's goldens on both simulations -- through the bin-search-only body (kb_quant_fast, path bit
QUANT_FAST) and, in a child process with LAMEJS_HIP_NO_FAST_QUANT=1, through the general quantization -- the unchanged oracle on the goldens and
then as the reference of a random family, mixed batches, seek and state, the Info tag."""
import hashlib
import json
import re
import subprocess

import pytest

import quality_cases as qc
from conftest import ROOT
from libs import ADDON, HOSTSIM_SO, NODE, WAVESIM_SO, run_js_check, sim, wavesim  # noqa: F401

RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000]
KBPS = [8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 192, 224, 256, 320]
TABLES_JS = str(ROOT / "lamejs_amd" / "js" / "tables.js")


@pytest.fixture(scope="module")
def G():
    return qc.goldens()


def test_golden_set_is_the_one_asked_for(G):
    by = {c["name"]: c for c in G}
    assert len(G) == 25 and {"q7_stereo_44100_128", "q7_mono_44100_64", "q7_stereo_48000_320", "q7_stereo_22050_48", "q7_mono_16000_32", "q7_mono_8000_8",
                             "q7_stereo_44100_48_resample_int", "q7_joint_centre_bursts_128", "q7_joint_mixed_128", "q7_resv_mono_128", "q7_resv_stereo_128", "q7_resv_joint_mixed_128",
                             "q7_downmix_128", "q7_protect_128", "q7_uneven_calls", "q7_silent3_stereo_128", "q7_wavexcerpt_stereo_128", "q8_stereo_44100_128"} <= set(by)
    assert {c["corpus"] for c in G} >= {"bursts", "sine", "wavexcerpt", "mixed", "silent3", "centre_bursts"}
    for c in G:
        assert sum(c["call_lens"]) == 12 * 1152 and c["frames"] >= 13 and c["flush_len"] > 0
        assert c["all_md5"] != c["q3_all_md5"], c["name"]                              # the generator insisted; the file says so
        assert c["ref_switches"] == {"noise_shaping": 0, "noise_shaping_amp": 0, "noise_shaping_stop": 0, "use_best_huffman": 0, "subblock_gain": -1, "psymodel": 1, "full_outer_loop": 0}
    assert by["q7_joint_mixed_128"]["ms_frames"] > 0 and by["q7_joint_mixed_128"]["lr_frames"] > 0 and by["q7_resv_joint_mixed_128"]["ms_frames"] > 0 < by["q7_resv_joint_mixed_128"]["lr_frames"]
    assert by["q7_stereo_22050_48"]["frames"] == 26 and by["q7_mono_16000_32"]["frames"] == 26 and by["q7_stereo_44100_48_resample_int"]["out_samplerate"] == 22050
    assert by["q7_downmix_128"]["ref_channels_out"] == 1 and by["q7_uneven_calls"]["call_lens"][:4] == [1, 17, 777, 4096]
    assert by["q8_stereo_44100_128"]["quality"] == 8 and by["q8_stereo_44100_128"]["all_md5"] == by["q7_stereo_44100_128"]["all_md5"] == by["q7_uneven_calls"]["all_md5"]


@pytest.mark.skipif(NODE is None, reason="node not available")
def test_blob_without_the_option_is_unchanged_and_with_it_only_the_switches_move():
    """All 324 triples: without the option -- absent, undefined, null or 3 -- the blob is the one the generator made before the option existed (the
    digests recorded then, the generator's own hash entry zeroed); with 7 no entry appears or changes size and cfg_i differs in the quality
    switches alone, at lame_init_qval's values; 8 gives the bytes of 7."""
    js = ("const t = require(process.argv[1]), crypto = require('crypto'); const out = {};"
          "const ents = (b) => { const n = b.readUInt32LE(8), e = {}; for (let i = 0; i < n; i++) { const p = 16 + 48 * i; e[b.toString('ascii', p, p + 32).replace(/\\0.*$/, '')] = [b.readUInt32LE(p + 36), b.readUInt32LE(p + 40)]; } return e; };"
          "const cfg = (b, e) => { let s = ''; for (let k = 0; k < e.cfg_i_names[0]; k++) { const c = b.readInt32LE(e.cfg_i_names[1] + 4 * k); if (!c) break; s += String.fromCharCode(c); }"
          " const o = {}; s.split(',').forEach((nm, k) => { o[nm] = b.readInt32LE(e.cfg_i[1] + 4 * k); }); return o; };"
          "for (const ch of [1, 2]) for (const sr of %s) for (const kb of %s) {"
          " const F = { fractionalResample: true };"
          " const a = Buffer.from(t.buildBlob(ch, sr, kb, F).blob), same = [undefined, null, 3].every((v) => Buffer.compare(a, Buffer.from(t.buildBlob(ch, sr, kb, Object.assign({ quality: v }, F)).blob)) == 0);"
          " const q = Buffer.from(t.buildBlob(ch, sr, kb, Object.assign({ quality: 7 }, F)).blob), q8 = Buffer.from(t.buildBlob(ch, sr, kb, Object.assign({ quality: 8 }, F)).blob);"
          " const ea = ents(a), eq = ents(q), ca = cfg(a, ea), cq = cfg(q, eq);"
          " const diff = Object.keys(ca).filter((k) => ca[k] != cq[k]).join(',');"
          " let moved = 0; for (let i = 0; i < a.length; i++) if (a[i] != q[i]) moved++;"
          " const z = Buffer.from(a); z.fill(0, ea.src_sha256_64[1], ea.src_sha256_64[1] + 8);"
          " out[ch + '_' + sr + '_' + kb] = [crypto.createHash('md5').update(z).digest('hex'), same ? 1 : 0, JSON.stringify(ea) == JSON.stringify(eq) && a.length == q.length && Buffer.compare(q, q8) == 0 ? 1 : 0, diff,"
          "  [cq.noise_shaping, cq.noise_shaping_amp, cq.noise_shaping_stop, cq.subblock_gain, cq.use_best_huffman, cq.full_outer_loop], ca.noise_shaping, moved]; }"
          "console.log(JSON.stringify(out));" % (json.dumps(RATES), json.dumps(KBPS)))
    r = subprocess.run([NODE, "-e", js, TABLES_JS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = json.loads(r.stdout)
    parent = json.loads((ROOT / "tests" / "golden" / "infotag_blob_md5.json").read_text())["md5"]
    assert len(rows) == 324 == len(parent)
    preset_type2 = 0
    for k, (md5, same, shape, diff, sw, ns3, moved) in rows.items():
        assert md5 == parent[k] and same == 1 and shape == 1, k
        assert diff == "noise_shaping,noise_shaping_amp,noise_shaping_stop,subblock_gain,use_best_huffman" and sw == [0, 0, 0, -1, 0, 0], (k, diff, sw)
        assert moved <= 5 * 4, (k, moved)                  # nothing but those five words differs in the whole blob
        preset_type2 += ns3 == 2
    assert preset_type2 > 0                                # (rows whose preset asks for noise shaping type 2: quality 7 clears it as well)


@pytest.mark.skipif(NODE is None, reason="node not available")
def test_tables_resolve_the_switches_the_reference_resolved(G):
    """Every golden's configuration: the quality switches in the blob are the ones the generator read from the reference's gfc after lame_init_params."""
    import lamejs_amd
    from protection_cases import cfg_entry
    for c in G:
        blob = lamejs_amd.tables_blob(c["channels"], c["samplerate"], c["kbps"], **qc.case_opts(c))
        assert {k: cfg_entry(blob, k)[1] for k in qc.SWITCHES} == {k: c["ref_switches"][k] for k in qc.SWITCHES}, c["name"]
    js = "const t = require(process.argv[1]); const p = t.resolveParams(2, 44100, 128, { quality: 8 }); console.log(JSON.stringify([p.quality, p.psymodel]));"
    r = subprocess.run([NODE, "-e", js, TABLES_JS], capture_output=True, text=True)
    assert r.returncode == 0 and json.loads(r.stdout) == [7, 1], r.stderr[-1000:]


@pytest.mark.skipif(NODE is None, reason="node not available")
def test_tables_refuse_other_levels_with_a_range_error_that_names_the_three(tmp_path):
    js = ("const t = require(process.argv[1]); const res = [];"
          "for (const q of [0, 1, 2, 4, 5, 6, 9, 10, -1, 7.5, '7', true, NaN])"
          " try { t.buildBlob(2, 44100, 128, { quality: q }); res.push('accepted'); } catch (e) { res.push(e instanceof RangeError && /\\b3\\b/.test(e.message) && /\\b7\\b/.test(e.message) && /\\b8\\b/.test(e.message) ? 'RangeError' : String(e)); }"
          "console.log(JSON.stringify(res));")
    r = subprocess.run([NODE, "-e", js, TABLES_JS], capture_output=True, text=True)
    assert r.returncode == 0 and json.loads(r.stdout) == ["RangeError"] * 13, (r.stdout, r.stderr[-1000:])
    # the command line's word
    a, b, c = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "c.bin"
    for out, words in ((a, ["quality=7"]), (b, ["quality=8", "joint"]), (c, [])):
        subprocess.run([NODE, TABLES_JS, "2", "44100", "128", str(out)] + words, check=True, capture_output=True)
    from protection_cases import cfg_entry
    assert cfg_entry(a.read_bytes(), "noise_shaping")[1] == 0 and cfg_entry(b.read_bytes(), "use_best_huffman")[1] == 0 and cfg_entry(b.read_bytes(), "mode")[1] == 1
    assert cfg_entry(c.read_bytes(), "noise_shaping")[1] >= 1 and cfg_entry(c.read_bytes(), "use_best_huffman")[1] == 1
    assert subprocess.run([NODE, TABLES_JS, "2", "44100", "128", str(a), "quality=5"], capture_output=True).returncode != 0


def test_python_refuses_other_levels_and_names_the_cache_file_by_the_option(sim):
    import lamejs_amd
    for q in (0, 2, 4, 5, 6, 9, 10, -1, 7.5, "7", True, None):
        with pytest.raises(ValueError, match="3, 7 or 8"):
            lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, quality=q)
        with pytest.raises(ValueError, match="3, 7 or 8"):
            lamejs_amd.tables_blob(2, 44100, 128, quality=q)
    plain, fast = lamejs_amd.tables_blob(1, 44100, 64), lamejs_amd.tables_blob(1, 44100, 64, quality=7)
    assert plain == lamejs_amd.tables_blob(1, 44100, 64, quality=3) and fast == lamejs_amd.tables_blob(1, 44100, 64, quality=8) and plain != fast
    tdir = ROOT / "lamejs_amd" / "tables"
    assert (tdir / "t_1_44100_64_quality7.bin").read_bytes() == fast and (tdir / "t_1_44100_64.bin").read_bytes() == plain


def test_abi_and_header_state_the_new_path_bit(sim):
    """No new C entry, no changed record: the header gains one path bit, Python a tuple of its own (PATH_BITS and PATH_BITS_ALL are pinned elsewhere)."""
    import lamejs_amd
    hdr = (ROOT / "include" / "lamejs_hip.h").read_text()
    assert re.search(r"#define LHIP_PATH_QUANT_FAST \(1u << 16\)", hdr)
    assert lamejs_amd.PATH_BITS_QUALITY == lamejs_amd.PATH_BITS_ALL + ("QUANT_FAST",) and lamejs_amd.PATH_BITS_QUALITY.index("QUANT_FAST") == 16
    a, b = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim), lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, quality=7)
    assert sim.lhip_state_bytes(a._h) == sim.lhip_state_bytes(b._h)
    a.close()
    b.close()


def test_hostsim_every_golden_through_the_fast_body(sim, G):
    seen = set()
    for c in G:
        seen |= qc.run_golden_case(sim, c, want_fast=True)                                   # the case's own calls: one-frame calls, and batches where a call holds more
        seen |= qc.run_golden_case(sim, c, lens=[c["nsamples"]], want_fast=True)             # one call: the batch path
    assert {"QUANT_FAST", "FRAME", "FRAME_RESV", "RESV_STREAM_NOHELPERS", "PSY4", "PREP"} <= seen and not ({"QUANT_PAIR", "QUANT_PERSISTENT"} & seen)


def test_wavesim_every_golden_through_the_fast_body(wavesim, G):
    seen = set()
    for c in G:
        seen |= qc.run_golden_case(wavesim, c, want_fast=True)
        seen |= qc.run_golden_case(wavesim, c, lens=[c["nsamples"]], want_fast=True)
    assert {"QUANT_FAST", "FRAME", "FRAME_RESV", "RESV_STREAM_HELPERS", "PSY4", "PREP"} <= seen and not ({"QUANT_PAIR", "QUANT_PERSISTENT"} & seen)


@pytest.mark.parametrize("which", ["hostsim", "wavesim"])
def test_every_golden_through_the_general_kernels(which, G):
    """LAMEJS_HIP_NO_FAST_QUANT=1 (read once per process: a child): the same goldens, no call takes QUANT_FAST."""
    res = qc.run_forced_general("goldens", lib_path={"hostsim": HOSTSIM_SO, "wavesim": WAVESIM_SO}[which], timeout=600)
    assert res["sim"] and res["cases"] == len(G) and "QUANT_FAST" not in res["paths"] and "QUANT_PERSISTENT" in res["paths"]
    assert ("QUANT_PAIR" in res["paths"]) == (which == "wavesim")


def test_oracle_reproduces_the_goldens_then_serves_the_random_family(sim, wavesim, G):
    """What makes the family's reference a reference: the unchanged oracle, given a quality-7 blob, gives the reference's bytes on every golden it can
    take (it has no downmix).  Only then: 12 seeded cases of 8 to 20 frames, random configuration, random call cuts, on both simulations."""
    took = [c["name"] for c in G if qc.oracle_takes(c) and qc.oracle_reproduces(c)]
    assert len(took) == len(G) - 1 and "q7_downmix_128" not in took
    fam = qc.family(20301, 12)
    assert len(fam) == 12 and all(8 * 1152 <= f["n"] <= 20 * 1152 for f in fam) and len({f["cfg"] for f in fam}) >= 5
    assert qc.family_check(sim, fam, want_fast=True) == 12
    assert qc.family_check(wavesim, fam, want_fast=True) == 12


def test_random_family_through_the_general_kernels():
    assert qc.run_forced_general("family", lib_path=HOSTSIM_SO, timeout=600)["cases"] == 12


@pytest.mark.parametrize("which", ["hostsim", "wavesim"])
def test_mixed_batch_of_three_encoders(which, request, G):
    """One encode_batch over a quality-3 stream, a quality-7 stream and a quality-7 joint-stereo stream: each gets its single-stream bytes."""
    import lamejs_amd
    lib = request.getfixturevalue("sim" if which == "hostsim" else "wavesim")
    by = {c["name"]: c for c in G}
    c7, cj = by["q7_stereo_44100_128"], by["q7_joint_mixed_128"]
    (L, R), (JL, JR) = qc.case_pcm(c7), qc.case_pcm(cj)
    encs = [lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib), lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, quality=7), lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, quality=7, joint=True)]
    got = lamejs_amd.encode_streams(encs, [L, L, JL], [R, R, JR])
    for e in encs:
        e.close()
    assert hashlib.md5(got[0]).hexdigest() == c7["q3_all_md5"] and hashlib.md5(got[1]).hexdigest() == c7["all_md5"] and hashlib.md5(got[2]).hexdigest() == cj["all_md5"]
    assert got[0] == qc.encode_whole(lib, 2, 44100, 128, L, R) and got[1] == qc.encode_whole(lib, 2, 44100, 128, L, R, quality=7)


def test_state_and_seek_on_a_fast_stream(sim):
    """lhip_state_get / lhip_state_set / lhip_seek on a quality-7 stream at a frame boundary: the state at the cut and the bytes after it equal the
    unbroken stream's; a quality-3 state is the same size but not the same stream."""
    import lamejs_amd
    import pcm
    L, R = pcm.sine(24 * 1152, 2)          # (steady material: the speculated state of a seek hits)
    cutpos, warm = 12 * 1152, 3 * 1152
    mk = lambda **kw: lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, quality=7, **kw)
    for kw in ({}, {"joint": True}):
        whole, graft, cut = mk(**kw), mk(**kw), mk(**kw)
        head = whole.encodeBuffer(L[:cutpos], R[:cutpos])
        assert "QUANT_FAST" in lamejs_amd.last_batch_paths(sim)
        state_at_cut = whole.state_get()
        rest = whole.encodeBuffer(L[cutpos:], R[cutpos:]) + whole.flush()
        assert head + rest == qc.encode_whole(sim, 2, 44100, 128, L, R, quality=7, **kw)
        graft.state_set(state_at_cut)
        assert graft.encodeBuffer(L[cutpos:], R[cutpos:]) + graft.flush() == rest
        nt, p0 = cut.seek_tail_samples(), cutpos - warm
        cut.seek(p0, L[p0 - nt:p0], R[p0 - nt:p0])
        cut.encodeBuffer(L[p0:cutpos], R[p0:cutpos])          # warm-up frames, output discarded
        got = cut.state_get()
        if got != state_at_cut:
            from state_fields import describe_diff
            raise AssertionError(describe_diff(got, state_at_cut))
        assert cut.encodeBuffer(L[cutpos:], R[cutpos:]) + cut.flush() == rest
        for e in (whole, graft, cut):
            e.close()


def test_info_tag_reports_quality_53_and_no_noise_shaping(sim, G):
    """With info_tag: the parser of tests/infotag_cases.py finds quality 100 - 40 - 7 and the noise-shaping bits of the misc byte 0 (57 and 1 at
    quality 3); the audio behind the placeholder is byte for byte the untagged stream."""
    import lamejs_amd
    from infotag_cases import parse_tag
    by = {c["name"]: c for c in G}
    for name, kw in (("q7_stereo_44100_128", {}), ("q7_joint_mixed_128", {"joint": True}), ("q7_resv_stereo_128", {"reservoir": True}), ("q8_stereo_44100_128", {})):
        c = by[name]
        L, R = qc.case_pcm(c)
        for quality, want_q, want_ns in ((c["quality"], 53, 0), (3, 57, None)):
            enc = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, info_tag=True, quality=quality, **kw)
            out = enc.encodeBuffer(L, R) + enc.flush()
            frame, info = enc.info_tag_frame(), enc.stream_info()
            enc.close()
            t = parse_tag(frame)
            assert t["magic"] == b"Info" and t["quality"] == want_q and (want_ns is None or t["misc"] & 3 == want_ns) and (want_ns is not None or t["misc"] & 3 in (1, 2)), (name, quality, t["quality"], t["misc"])
            audio = out[info["tag_bytes"]:]
            assert len(frame) == info["tag_bytes"] and hashlib.md5(audio).hexdigest() == (c["all_md5"] if quality != 3 else c["q3_all_md5"]), (name, quality)


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_option_hostsim():
    res = run_js_check("js_quality_check.js", 20302, lib=HOSTSIM_SO, timeout=600)
    assert res["mismatches"] == 0 and res["goldens"] == 25 and res["range_errors"] == 6 and set(res["families"]) >= {"goldens", "batch_mixed", "quality8", "pending", "refusals"}


@pytest.mark.parametrize("wave", [False, True], ids=["one_lane", "wave"])
def test_bounds_under_sanitizers(tmp_path, wave):
    """tests/tools/quality_bounds.c with lhip_api.cpp, -fsanitize=address,undefined, the flags of tests/hostsim/Makefile: quality-7 streams through the
    fast quantization body (the wave build: g_quant_fast's workgroup of wave pairs) on heap blocks that end with the input -- two channels, one channel,
    one granule per frame, joint stereo, a configuration without the dead last round of pairs.  Nothing goes through Python, nothing is preloaded."""
    import os
    import lamejs_amd
    mk = (ROOT / "tests" / "hostsim" / "Makefile").read_text()
    flags = re.search(r"^CXXFLAGS = (.*)$", mk, flags=re.M).group(1).split()
    flags = [f for f in flags if f not in ("-shared", "-fPIC", "-O2")]
    exe = tmp_path / "quality_bounds"
    args = []
    for i, (ch, sr, kb, kw) in enumerate(((2, 44100, 128, {}), (1, 44100, 64, {}), (2, 22050, 48, {}), (2, 44100, 128, {"joint": True}), (2, 48000, 320, {}))):
        blob = tmp_path / f"t{i}.bin"
        blob.write_bytes(lamejs_amd.tables_blob(ch, sr, kb, quality=7, **kw))
        args += [str(ch), str(sr), str(kb), str(blob)]
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", *flags] + (["-DLHIP_WAVESIM"] if wave else []) + \
          ["-I", str(ROOT / "include"), "-x", "c++", str(ROOT / "tests" / "tools" / "quality_bounds.c"), str(ROOT / "lamejs_amd" / "csrc" / "lhip_api.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=900)          # (the sanitizers' runtimes are linked statically: the environment is the inherited one)
    assert r.returncode == 0 and "quality_bounds OK: 15 streams" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
