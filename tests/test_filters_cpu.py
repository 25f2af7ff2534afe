"""The output sample rate and the polyphase filter settings (out_samplerate, lowpass, lowpass_width, highpass, highpass_width; extension: the
reference's wrapper leaves the five gfp fields at lame_init's values).  CPU tier: blobs without the options are unchanged, the resolved values and
amp_filter are the reference's bit for bit, every refusal in tables.js, its command line and Python, the unmodified reference's goldens on both
simulations, the unchanged oracle on the goldens and then as the reference of a random family, batches of different option sets, what follows the blob
on the host (frame counts, output sizes, the call limit, ReplayGain's rate, seek), the Info tag's lowpass byte, and INTEGRATION.md's list of the
formerly refused triples."""
import ctypes
import hashlib
import json
import re
import subprocess

import numpy as np
import pytest

import filters_cases as fc
from conftest import ROOT
from libs import ADDON, HOSTSIM_SO, NODE, run_js_check, sim, wavesim  # noqa: F401

RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000]
KBPS = [8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 192, 224, 256, 320]
TABLES_JS = str(ROOT / "lamejs_amd" / "js" / "tables.js")
needs_node = pytest.mark.skipif(NODE is None, reason="node not available")


@pytest.fixture(scope="module")
def G():
    return fc.goldens()


def node(js, *args):
    r = subprocess.run([NODE, "-e", js, TABLES_JS, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_golden_set_is_the_one_asked_for(G):
    by = {c["name"]: c for c in G}
    assert 38 <= len(G) <= 44 and len(by) == len(G)
    ref = lambda n: by[n]["ref"]
    bands = lambda n: by[n]["open_bands"]
    af = lambda n: fc.amp_filter_of(by[n])
    # the rows the issue states, as the reference resolved them
    assert bands("lp12000_out44100_128") == "1" * 17 + "0" * 15 and all(af("lp12000_out44100_128")[:17] == 1.0)
    assert abs(af("lp12000_w2000_out44100_128")[15] - 0.910) < 5e-4 and abs(af("lp12000_w2000_out44100_128")[16] - 0.541) < 5e-4
    assert bands("lp_off_128") == "1" * 32 and ref("lp_off_128")["out_samplerate"] == 44100 and ref("lp_off_128")["lowpassfreq"] == -1
    assert bands("lp19000_128") == "1" * 27 + "0" * 5 and bands("hp500_128")[:2] == "01"
    assert bands("hp2000_w500_128")[:4] == "0001" and abs(af("hp2000_w500_128")[3] - 0.782) < 5e-4
    assert ref("out44100_44100_96") == dict(ref("out44100_44100_96"), resample_ratio=1, lowpassfreq=15100) and ref("out48000_48000_112")["resample_ratio"] == 1
    assert ref("out22050_44100_128")["resample_ratio"] == 2 and ref("out22050_44100_320") == dict(ref("out22050_44100_320"), resample_ratio=2, version=0, brate=160)
    assert ref("out16000_48000_64")["resample_ratio"] == 3 and ref("out48000_192000_64")["resample_ratio"] == 4 == ref("out48000_lp15000_192000_64_mono")["resample_ratio"]
    assert ref("out8000_48000_16_mono")["resample_ratio"] == 6 and ref("out44100_88200_128")["resample_ratio"] == 2
    for c in G:
        assert c["frames"] in (13, 14, 15) and c["flush_len"] > 0 and c["all_md5"] != c["plain_all_md5"], c["name"]      # (plain_all_md5 null: the reference cannot encode the triple without the settings)
        if "highpass" in c["settings"]:
            assert fc.amp_filter_of(c)[0] < 1e-12, c["name"]
        if c["settings"].get("lowpassWidth", 0) > 0 or c["settings"].get("highpassWidth", 0) > 0:
            assert any(0 < v < 1 for v in fc.amp_filter_of(c)), c["name"]
    for k in ("jointStereo", "reservoir", "downmix", "protect", "infoTag", "replayGain"):
        assert any(c.get(k) for c in G), k
    assert any(c.get("quality") == 7 for c in G) and by["lp12000_uneven_calls"]["call_lens"][:4] == [1, 17, 777, 4096]
    assert by["lp12000_uneven_calls"]["all_md5"] == by["lp12000_out44100_128"]["all_md5"] and by["mono_lp8000_out44100_64"]["channels"] == 1
    assert {c["ref"]["version"] for c in G} == {0, 1} and {c["ref"]["out_samplerate"] for c in G} >= {8000, 11025, 16000, 22050, 24000, 44100, 48000}


@needs_node
def test_blobs_without_the_options_are_unchanged_over_all_324_triples():
    """Without the five options -- absent, undefined or null -- every blob is the one the generator made before they existed (the digests recorded then,
    the generator's own hash entry zeroed), and no option adds a blob entry."""
    js = ("const t = require(process.argv[1]), crypto = require('crypto'); const out = {};"
          "const ents = (b) => { const n = b.readUInt32LE(8), e = {}; for (let i = 0; i < n; i++) { const p = 16 + 48 * i; e[b.toString('ascii', p, p + 32).replace(/\\0.*$/, '')] = [b.readUInt32LE(p + 36), b.readUInt32LE(p + 40)]; } return e; };"
          "const K = ['outSampleRate', 'lowpass', 'lowpassWidth', 'highpass', 'highpassWidth'];"
          "for (const ch of [1, 2]) for (const sr of %s) for (const kb of %s) {"
          " const F = { fractionalResample: true };"
          " const a = Buffer.from(t.buildBlob(ch, sr, kb, F).blob), ea = ents(a);"
          " const same = [undefined, null].every((v) => { const o = Object.assign({}, F); K.forEach((k) => { o[k] = v; }); return Buffer.compare(a, Buffer.from(t.buildBlob(ch, sr, kb, o).blob)) == 0; });"
          " const w = Buffer.from(t.buildBlob(ch, sr, kb, { outSampleRate: sr, lowpass: -1 }).blob), ew = ents(w);"
          " const z = Buffer.from(a); z.fill(0, ea.src_sha256_64[1], ea.src_sha256_64[1] + 8);"
          " out[ch + '_' + sr + '_' + kb] = [crypto.createHash('md5').update(z).digest('hex'), same ? 1 : 0, Object.keys(ea).join() == Object.keys(ew).join() ? 1 : 0]; }"
          "console.log(JSON.stringify(out));" % (json.dumps(RATES), json.dumps(KBPS)))
    rows = node(js)
    parent = json.loads((ROOT / "tests" / "golden" / "infotag_blob_md5.json").read_text())["md5"]
    assert len(rows) == 324 == len(parent)
    for k, (md5, same, shape) in rows.items():
        assert md5 == parent[k] and same == 1 and shape == 1, k


@needs_node
def test_resolved_values_and_amp_filter_are_the_references_bit_for_bit(G):
    """Per golden: out_samplerate, lowpassfreq, brate, version, resample_ratio, mode_gr and all 32 amp_filter bit patterns as the reference resolved them;
    TableSet::skip_tail's rule on them flips both ways against the same triple without the options."""
    import lamejs_amd
    js = ("const t = require(process.argv[1]); const cs = JSON.parse(process.argv[2]); console.log(JSON.stringify(cs.map(([ch, sr, kb, o]) => { const p = t.resolveParams(ch, sr, kb, o);"
          " return { out_samplerate: p.out_samplerate, lowpassfreq: p.lowpassfreq, brate: p.brate, version: p.version, resample_ratio: p.resample_ratio, mode_gr: p.mode_gr }; })));")
    js_opts = lambda c: dict(c["settings"], **{k: True for k in ("jointStereo", "reservoir", "downmix", "protect") if c.get(k)})
    got = node(js, json.dumps([[c["channels"], c["samplerate"], c["kbps"], js_opts(c)] for c in G]))
    flips = set()
    for c, p in zip(G, got):
        assert p == c["ref"], (c["name"], p, c["ref"])
        blob = lamejs_amd.tables_blob(c["channels"], c["samplerate"], c["kbps"], **fc.case_opts(c))
        assert list(fc.blob_array(blob, "amp_filter", "I")) == c["amp_filter_bits"], c["name"]
        assert fc.blob_cfg(blob, "out_samplerate") == c["ref"]["out_samplerate"] and fc.blob_cfg(blob, "brate") == c["ref"]["brate"] and fc.blob_cfg(blob, "version") == c["ref"]["version"]
        if c["plain_all_md5"] is not None:
            o = {k: v for k, v in fc.case_opts(c).items() if k not in fc.PY_NAME.values()}
            plain = fc.blob_array(lamejs_amd.tables_blob(c["channels"], c["samplerate"], c["kbps"], **o), "amp_filter", "f")
            flips.add((all(float(plain[b]) < 1e-12 for b in (28, 29, 30, 31)), fc.expected_skip_tail(c)))
    by = {c["name"]: c for c in G}
    assert (True, False) in flips and (False, True) in flips
    assert not fc.expected_skip_tail(by["lp_off_128"]) and fc.expected_skip_tail(by["lp16000_320"]) and not fc.expected_skip_tail(by["out22050_44100_320"]) and fc.expected_skip_tail(by["hp2000_w500_128"])


REFUSED = [{"lowpass": "12000"}, {"lowpass": 0}, {"lowpass": -2}, {"lowpass": 12000.5}, {"lowpass": None, "lowpassWidth": -1}, {"lowpass": True}, {"lowpassWidth": "5"}, {"lowpassWidth": 0.5},
           {"highpass": 0}, {"highpass": -1}, {"highpass": 100}, {"highpass": 480}, {"highpass": 481.5}, {"highpass": "500"}, {"highpass": 17000}, {"highpass": 16000, "highpassWidth": 1000},
           {"highpass": 12000, "lowpass": 12000, "outSampleRate": 44100}, {"highpassWidth": 100}, {"highpass": 500, "highpassWidth": -1}, {"highpass": 500, "highpassWidth": True},
           {"outSampleRate": 44000}, {"outSampleRate": 0}, {"outSampleRate": 48000}, {"outSampleRate": 32000}, {"outSampleRate": 32000, "fractionalResample": True}, {"outSampleRate": "44100"},
           {"outSampleRate": 22050.5}, {"outSampleRate": False}]
ACCEPTED = [{"highpass": 481}, {"highpass": 300, "highpassWidth": 181}, {"lowpass": -1}, {"lowpass": 1, "outSampleRate": 44100}, {"lowpassWidth": 0}, {"outSampleRate": 11025}, {"highpass": 16999},
            {"lowpass": -1, "highpass": 20000}, {"outSampleRate": 44100, "fractionalResample": True}]


@needs_node
def test_tables_js_refuses_with_range_errors_and_accepts_the_edges():
    js = ("const t = require(process.argv[1]); const res = [];"
          "for (const o of JSON.parse(process.argv[2])) try { t.buildBlob(2, 44100, 128, o); res.push('accepted'); } catch (e) { res.push(e instanceof RangeError ? 'RangeError' : 'Error: ' + e.message); }"
          "for (const v of [NaN, Infinity, -Infinity]) for (const k of ['outSampleRate', 'lowpass', 'lowpassWidth', 'highpass']) try { t.buildBlob(2, 44100, 128, { [k]: v }); res.push('accepted'); } catch (e) { res.push(e instanceof RangeError ? 'RangeError' : String(e)); }"
          "console.log(JSON.stringify(res));")
    got = node(js, json.dumps(REFUSED + ACCEPTED))
    assert got[:len(REFUSED)] == ["RangeError"] * len(REFUSED), [(o, g) for o, g in zip(REFUSED, got) if g != "RangeError"]
    assert got[len(REFUSED):len(REFUSED) + len(ACCEPTED)] == ["accepted"] * len(ACCEPTED), list(zip(ACCEPTED, got[len(REFUSED):]))
    assert got[len(REFUSED) + len(ACCEPTED):] == ["RangeError"] * 12
    # the message names the minimum for the STREAM's rate; the reference's own non-integer choice stays today's refusal (an Error, not a RangeError)
    js = ("const t = require(process.argv[1]); const m = (ch, sr, kb, o) => { try { t.resolveParams(ch, sr, kb, o); return 'accepted'; } catch (e) { return (e instanceof RangeError ? 'R:' : 'E:') + e.message; } };"
          "console.log(JSON.stringify([m(2, 44100, 128, { highpass: 100 }), m(2, 44100, 128, { highpass: 100, outSampleRate: 22050 }), m(1, 48000, 16, { highpass: 50, outSampleRate: 8000 }), m(2, 44100, 128, { lowpass: 12000 }),"
          " m(2, 44100, 96, {}), m(2, 44100, 96, { lowpassWidth: 500, fractionalResample: true }), m(2, 44100, 128, { lowpass: 12000, fractionalResample: true })]));")
    msgs = node(js)
    for msg, out in zip(msgs[:3], (44100, 22050, 8000)):
        assert msg.startswith("R:") and f"at least {fc.highpass_minimum(out)} Hz" in msg and f"{out} Hz" in msg, msg
    assert fc.highpass_minimum(44100) == 481 and fc.highpass_minimum(8000) == 88
    assert all(m.startswith("E:") and "non-integer ratio" in m for m in msgs[3:]), msgs[3:]


@needs_node
def test_command_line_words_and_their_refusals(tmp_path, G):
    import lamejs_amd
    by = {c["name"]: c for c in G}
    for name in ("lp12000_w2000_out44100_128", "hp2000_w500_128", "lp_off_128", "out8000_48000_16_mono"):
        c = by[name]
        out = tmp_path / (name + ".bin")
        subprocess.run([NODE, TABLES_JS, str(c["channels"]), str(c["samplerate"]), str(c["kbps"]), str(out)] + [f"{fc.CLI_WORD[k]}={v}" for k, v in c["settings"].items()], check=True, capture_output=True)
        assert out.read_bytes() == lamejs_amd.tables_blob(c["channels"], c["samplerate"], c["kbps"], **fc.filter_opts(c["settings"])), name
    for words in (["lowpass=abc"], ["lowpass=0"], ["highpass=100"], ["highpasswidth=5"], ["outrate=32000"], ["outrate=44100.5"], ["lowpasswidth=-1"], ["outrate=32000", "fracresample"]):
        r = subprocess.run([NODE, TABLES_JS, "2", "44100", "128", str(tmp_path / "no.bin")] + words, capture_output=True, text=True)
        assert r.returncode != 0 and "RangeError" in r.stderr and not (tmp_path / "no.bin").exists(), words


def test_python_refuses_wrong_values_and_names_the_cache_file_by_the_options(sim):
    import lamejs_amd
    bad = [{"lowpass": "12000"}, {"lowpass": 0}, {"lowpass": -2}, {"lowpass": 12000.5}, {"lowpass": True}, {"lowpass": float("nan")}, {"lowpass_width": -1}, {"lowpass_width": 0.5}, {"highpass": 0}, {"highpass": "500"},
           {"highpass": 100}, {"highpass": 480}, {"highpass": 17000}, {"highpass_width": 100}, {"highpass": 500, "highpass_width": False}, {"out_samplerate": 44000}, {"out_samplerate": 48000},
           {"out_samplerate": 32000}, {"out_samplerate": 32000, "fractional_resample": True}, {"out_samplerate": "44100"}, {"out_samplerate": 22050.0}, {"out_samplerate": True}]
    for kw in bad:
        with pytest.raises(ValueError):
            lamejs_amd.tables_blob(2, 44100, 128, **kw)
        with pytest.raises(ValueError):
            lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, **kw)
    with pytest.raises(lamejs_amd.LhipError, match="non-integer ratio"):          # the reference's own choice for this lowpass is 32000 Hz: today's refusal
        lamejs_amd.tables_blob(2, 44100, 128, lowpass=12000)
    plain = lamejs_amd.tables_blob(1, 44100, 64)
    a = lamejs_amd.tables_blob(1, 44100, 64, out_samplerate=22050, lowpass=np.int64(9000), lowpass_width=500, highpass=300, highpass_width=0)
    b = lamejs_amd.tables_blob(1, 44100, 64, lowpass=-1, quality=7)
    tdir = ROOT / "lamejs_amd" / "tables"
    assert (tdir / "t_1_44100_64_outrate22050_lowpass9000_lowpasswidth500_highpass300_highpasswidth0.bin").read_bytes() == a and (tdir / "t_1_44100_64_quality7_lowpass-1.bin").read_bytes() == b
    assert (tdir / "t_1_44100_64.bin").read_bytes() == plain and len({plain, a, b}) == 3
    assert plain == lamejs_amd.tables_blob(1, 44100, 64, out_samplerate=None, lowpass=None, lowpass_width=None, highpass=None, highpass_width=None)


def test_lhip_create_checks_amp_filter(sim):
    """Every amp_filter value must be finite and in [0, 1]: anything else is -3 with a message that names the band."""
    import struct
    import lamejs_amd
    blob = lamejs_amd.tables_blob(2, 44100, 128, highpass=2000, highpass_width=500)
    off = next(struct.unpack_from("<I", blob, 16 + 48 * k + 40)[0] for k in range(struct.unpack_from("<I", blob, 8)[0]) if blob[16 + 48 * k:16 + 48 * k + 32].split(b"\0", 1)[0] == b"amp_filter")
    cfg = lamejs_amd._Config(2, 44100, 128, -1)

    def create(b):
        h = ctypes.c_void_p()
        rc = sim.lhip_create(ctypes.byref(cfg), ctypes.create_string_buffer(b, len(b)), len(b), ctypes.byref(h))
        if rc == 0:
            sim.lhip_destroy(h)
        return rc, sim.lhip_last_error().decode()
    assert create(blob)[0] == 0
    for band, v in ((0, float("nan")), (3, 1.5), (31, -0.25), (17, float("inf")), (5, -float("inf")), (30, 1.0000001)):
        rc, msg = create(blob[:off + 4 * band] + struct.pack("<f", v) + blob[off + 4 * band + 4:])
        assert rc == -3 and f"amp_filter[{band}]" in msg, (band, v, rc, msg)
    for band, v in ((0, 1.0), (3, 0.0), (31, 1e-30), (4, 0.5)):          # the edges of the interval are inside it
        assert create(blob[:off + 4 * band] + struct.pack("<f", v) + blob[off + 4 * band + 4:])[0] == 0, (band, v)


def test_hostsim_every_golden_in_its_own_calls_and_in_one_call(sim, G):
    seen = set()
    for c in G:
        seen |= fc.run_golden_case(sim, c)
        seen |= fc.run_golden_case(sim, c, lens=[c["nsamples"]])
    assert {"FRAME", "FRAME_RESV", "SEPARATE", "PREP", "PSY4", "QUANT_FAST", "QUANT_PERSISTENT", "RESV_STREAM_NOHELPERS"} <= seen


def test_wavesim_every_golden_in_its_own_calls_and_in_one_call(wavesim, G):
    seen = set()
    for c in G:
        seen |= fc.run_golden_case(wavesim, c)
        seen |= fc.run_golden_case(wavesim, c, lens=[c["nsamples"]])
    assert {"FRAME", "FRAME_RESV", "SEPARATE", "PREP", "PSY4", "QUANT_FAST", "QUANT_PERSISTENT", "RESV_STREAM_HELPERS"} <= seen


@pytest.mark.parametrize("which", ["hostsim", "wavesim"])
def test_quality_7_goldens_through_the_general_kernels(which, G):
    res = fc.run_nofast(which)
    assert res["cases"] == sum(1 for c in G if c.get("quality") == 7) >= 2 and "QUANT_FAST" not in res["paths"] and set(res["paths"]) & {"QUANT_PAIR", "QUANT_PERSISTENT"}


@pytest.mark.parametrize("which", ["hostsim", "wavesim"])
def test_launch_path_environments_on_the_four_new_states(which):
    """The four matrix cases under each environment's switches, a fresh process each: bytes against the goldens, and per call the launch record and the paths."""
    for env_name in fc.MATRIX_ENVS:
        status, recs, text, fatal = fc.run_matrix(which, env_name, 600)
        assert status == 0 and not fatal, (env_name, status, text)
        assert fc.check_matrix(recs, env_name, which) == [], env_name


def test_oracle_reproduces_the_goldens_then_serves_the_random_family(sim, wavesim, G):
    """What makes the family's reference a reference: the unchanged oracle, given a blob built with the options, gives the reference's bytes on every golden
    it can take (it has no downmix).  Only then: 16 seeded cases -- one and two channels, MPEG-1 / 2 / 2.5, ratios 1 to 6, random lowpass, widths and
    highpass, random call cuts -- on both simulations; a setting that tables.js refused would fail, not skip."""
    took = [c["name"] for c in G if fc.oracle_takes(c) and fc.oracle_reproduces(c)]
    assert len(took) == len(G) - 1 and "downmix_lp10000_out44100_64" not in took
    fam = fc.family(20400, 16)
    assert len(fam) == 16 and {f["cfg"][0] for f in fam} == {1, 2} and len({f["opts"]["out_samplerate"] for f in fam}) >= 8
    assert any("highpass" in f["opts"] for f in fam) and any(f["opts"].get("lowpass", 0) > 0 for f in fam) and any("lowpass_width" in f["opts"] or "highpass_width" in f["opts"] for f in fam)
    assert fc.family_check(sim, fam) == 16
    assert fc.family_check(wavesim, fam) == 16


def test_one_big_call_gives_the_stream_of_1152_sample_calls(sim, G):
    by = {c["name"]: c for c in G}
    for name in ("hp2000_w500_128", "out22050_44100_320", "out8000_48000_16_mono", "lp_off_128"):
        c = by[name]
        L, R = fc.case_pcm(c)
        o, n = fc.case_opts(c), c["nsamples"]
        whole = fc.encode_whole(sim, c["channels"], c["samplerate"], c["kbps"], L, R, **o)
        assert whole == fc.encode_whole(sim, c["channels"], c["samplerate"], c["kbps"], L, R, lens=[1152] * (n // 1152) + ([n % 1152] if n % 1152 else []), **o), name
        assert hashlib.md5(whole).hexdigest() == c["all_md5"]


@pytest.mark.parametrize("which", ["hostsim", "wavesim"])
def test_batch_of_three_encoders_with_different_option_sets(which, request, G):
    """One encode_batch over three blobs that differ in filters, output rate and MPEG version (and a second one with a reservoir stream): each stream gets its
    golden's bytes."""
    lib = request.getfixturevalue("sim" if which == "hostsim" else "wavesim")
    assert "SEPARATE" in fc.mixed_batch(lib, ["hp2000_w500_128", "out22050_44100_320", "mono_lp8000_out44100_64"], G)
    fc.mixed_batch(lib, ["lp_off_128", "resv_hp500_128", "q7_hp500_128"], G)


def test_what_follows_the_blob_on_the_host(sim, G):
    """Frame counts and lhip_encode_output_bytes (exact: Mp3Encoder._encode holds every call of every golden to it), the call limit, ReplayGain's rate and
    seek follow the blob's out_samplerate and ratio, not the (rate, kbps) table.  (ReplayGain counts the samples at the STREAM's rate that the encoder consumed: within one frame of
    frames x frame length, in windows of ceil(stream rate / 20).)"""
    import lamejs_amd
    by = {c["name"]: c for c in G}
    for name in ("out22050_44100_320", "out44100_44100_96", "out8000_48000_16_mono", "hp500_128"):
        c = by[name]
        L, R = fc.case_pcm(c)
        enc = fc.make_encoder(sim, c, replay_gain=True)
        assert sim.lhip_output_bytes_is_exact(enc._h) == 1 and enc.call_limit() == 0
        per, frame_bytes = c["call_lens"][0], c["call_bytes"][-1]
        assert sim.lhip_encode_output_bytes(enc._h, per) == c["call_bytes"][0]
        out = enc.encodeBuffer(L, R)
        assert len(out) == sum(c["call_bytes"]) and abs(frame_bytes - (144000 if c["ref"]["version"] else 72000) * c["ref"]["brate"] // c["ref"]["out_samplerate"]) <= 1
        out += enc.flush()
        tenth, windows, samples = enc.replay_gain()
        win = -(-c["ref"]["out_samplerate"] // 20)
        assert hashlib.md5(out).hexdigest() == c["all_md5"] and abs(samples - c["frames"] * 576 * c["ref"]["mode_gr"]) < 576 * c["ref"]["mode_gr"] and windows == samples // win and tenth is not None, (name, windows, samples)
        enc.close()
    # seek: refused on a stream the option makes resample, accepted on a formerly refused triple that no longer resamples -- and the bytes behind the cut are the unbroken stream's
    enc = lamejs_amd.Mp3Encoder(2, 44100, 320, lib=sim, out_samplerate=22050)
    with pytest.raises(lamejs_amd.LhipError, match="resampling"):
        enc.seek(4 * 1152, np.zeros(enc.seek_tail_samples(), np.int16), np.zeros(enc.seek_tail_samples(), np.int16))
    enc.close()
    import pcm
    L, R = pcm.sine(20 * 1152, 2)
    kw = {"out_samplerate": 44100, "highpass": 600}
    whole, cut = lamejs_amd.Mp3Encoder(2, 44100, 96, lib=sim, **kw), lamejs_amd.Mp3Encoder(2, 44100, 96, lib=sim, **kw)
    cutpos, p0 = 10 * 1152, 7 * 1152
    whole.encodeBuffer(L[:cutpos], R[:cutpos])
    state = whole.state_get()
    rest = whole.encodeBuffer(L[cutpos:], R[cutpos:]) + whole.flush()
    nt = cut.seek_tail_samples()
    cut.seek(p0, L[p0 - nt:p0], R[p0 - nt:p0])
    cut.encodeBuffer(L[p0:cutpos], R[p0:cutpos])
    assert cut.state_get() == state and cut.encodeBuffer(L[cutpos:], R[cutpos:]) + cut.flush() == rest
    whole.close()
    cut.close()


def test_info_tag_lowpass_byte_follows_the_setting(sim, G):
    """The parser of tests/infotag_cases.py on the finished tag frame: the lowpass byte is the setting in units of 100 Hz, rounded as VBRTag.js:595 does,
    0 with lowpass -1; the tag frame's header carries the stream's rate; the audio behind the placeholder is the golden's."""
    import lamejs_amd
    from infotag_cases import parse_tag
    by = {c["name"]: c for c in G}
    for name, want, rate in (("tag_gain_lp12000_w2000_out44100_128", 120, 44100), ("lp_off_128", 0, 44100), ("lp19000_128", 190, 44100), ("out22050_44100_128", 110, 22050), ("hp500_128", 170, 44100)):
        c = by[name]
        L, R = fc.case_pcm(c)
        enc = fc.make_encoder(sim, c, info_tag=True)
        out = enc.encodeBuffer(L, R) + enc.flush()
        frame, info = enc.info_tag_frame(), enc.stream_info()
        enc.close()
        t = parse_tag(frame)
        assert t["magic"] == b"Info" and t["lowpass"] == want == int(max(c["ref"]["lowpassfreq"], 0) / 100.0 + 0.5) and t["samplerate"] == rate, (name, t["lowpass"])
        assert hashlib.md5(out[info["tag_bytes"]:]).hexdigest() == c["all_md5"], name
        if c.get("replayGain"):
            assert t["radio_gain"] != 0


@needs_node
def test_integration_md_lists_the_49_formerly_refused_triples():
    """INTEGRATION.md "Sample rate and filters": every triple tables.js refuses by default for its non-integer ratio, with the outSampleRate values that make it
    encodable -- each the input rate or the input rate divided by a whole number -- and the highpass minimum per stream rate."""
    js = ("const t = require(process.argv[1]); const out = [];"
          "for (const ch of [1, 2]) for (const sr of %s) for (const kb of %s) { try { t.resolveParams(ch, sr, kb); continue; } catch (e) { if (!/non-integer ratio/.test(e.message)) throw e; }"
          " const dflt = t.resolveParams(ch, sr, kb, { fractionalResample: true }).out_samplerate;"
          " const ok = %s.filter((o) => { try { t.buildBlob(ch, sr, kb, { outSampleRate: o }); return true; } catch (e) { if (!(e instanceof RangeError)) throw e; return false; } });"
          " out.push([ch, sr, kb, dflt, ok.sort((a, b) => b - a)]); }"
          "console.log(JSON.stringify(out));" % (json.dumps(RATES), json.dumps(KBPS), json.dumps(RATES)))
    want = node(js)
    assert len(want) == 49 and all(vals and all(sr % v == 0 and v <= sr for v in vals) and sr in vals for _, sr, _, _, vals in want)
    text = (ROOT / "INTEGRATION.md").read_text()
    sect = text[text.index("### Sample rate and filters"):]
    sect = sect[:sect.index("\n## ", 5)]
    rows = [[int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), [int(v) for v in m.group(5).split(",")]]
            for m in re.finditer(r"^\| (\d) \| (\d+) \| (\d+) \| (\d+) \| ([\d, ]+) \|$", sect, flags=re.M)]
    assert sorted(rows) == sorted(want)
    mins = {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"^\| (\d+) Hz \| (\d+) Hz \|$", sect, flags=re.M)}
    assert mins == {r: fc.highpass_minimum(r) for r in RATES}


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_options_hostsim(G):
    fc.check_js_result(run_js_check("js_filters_check.js", 20401, lib=HOSTSIM_SO, timeout=900), G)


@pytest.mark.parametrize("wave", [False, True], ids=["one_lane", "wave"])
def test_bounds_under_sanitizers(tmp_path, wave):
    """tests/tools/filters_bounds.c with lhip_api.cpp, -fsanitize=address,undefined, the flags of tests/hostsim/Makefile: streams on heap blocks
    that end with the input, for the states the options add -- zero bands at the bottom, no lowpass at 128 kbps, MPEG-2 at a clamped bitrate from 44.1 kHz, ratio 4
    from 192 kHz on one channel, ratio 6 to 8 kHz.  Nothing goes through Python, nothing is preloaded."""
    import os
    import lamejs_amd
    mk = (ROOT / "tests" / "hostsim" / "Makefile").read_text()
    flags = [f for f in re.search(r"^CXXFLAGS = (.*)$", mk, flags=re.M).group(1).split() if f not in ("-shared", "-fPIC", "-O2")]
    exe = tmp_path / "filters_bounds"
    args = []
    for i, (ch, sr, kb, kw) in enumerate(((2, 44100, 128, {"highpass": 2000, "highpass_width": 500}), (2, 44100, 128, {"lowpass": -1}), (2, 44100, 320, {"out_samplerate": 22050}),
                                          (1, 192000, 64, {"out_samplerate": 48000, "lowpass": 15000}), (1, 48000, 16, {"out_samplerate": 8000}))):
        blob = tmp_path / f"t{i}.bin"
        blob.write_bytes(lamejs_amd.tables_blob(ch, sr, kb, **kw))
        args += [str(ch), str(sr), str(kb), str(blob)]
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", *flags] + (["-DLHIP_WAVESIM"] if wave else []) + \
          ["-I", str(ROOT / "include"), "-x", "c++", str(ROOT / "tests" / "tools" / "filters_bounds.c"), str(ROOT / "lamejs_amd" / "csrc" / "lhip_api.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=900)          # (the sanitizers' runtimes are linked statically: the environment is the inherited one)
    assert r.returncode == 0 and "filters_bounds OK: 15 streams" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
