"""CRC frame protection ({ protect }: the reference core's gfp.error_protection, LAME's -p) and the header's flag bits (extension;
BitStream.js:233-285, 406-409, Lame.js:1109-1110).  CPU tier: both simulations are built from the kernel sources (tests/hostsim), so the
stored CRC comes from the device function of k_bits.h -- walked by one lane in the host simulation, spread over 64 lanes with an XOR
reduction in the wave simulation.  Yardsticks: the unmodified reference's bytes and a CRC-16 as ISO 11172-3 defines it, written out in
protection_cases.iso_crc."""
import json
import subprocess

import pytest

import protection_cases as pc
from conftest import ROOT
from libs import ADDON, HOSTSIM_SO, NODE, run_js_check, sim, wavesim  # noqa: F401

RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000]
KBPS = [8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 192, 224, 256, 320]
TABLES_JS = str(ROOT / "lamejs_amd" / "js" / "tables.js")


@pytest.fixture(scope="module")
def G():
    return pc.goldens()


def test_iso_crc_is_the_standard_crc16():
    """The yardstick itself: polynomial 0x8005, preset 0xffff, MSB first, no final XOR -- the catalogued check value of that parametrisation
    (CRC-16/CMS) over "123456789" is 0xaee7, with a zero preset (CRC-16/UMTS) 0xfee8 -- and the linearity the kernel relies on."""
    assert pc.iso_crc(b"123456789") == 0xAEE7 and pc.iso_crc(b"") == 0xFFFF
    x, y = b"123456789", b"\x80\x00\x01\xff\x10\x20\x40\x08\x55"
    xor = bytes(p ^ q for p, q in zip(x, y))
    assert pc.iso_crc(x) ^ pc.iso_crc(y) ^ pc.iso_crc(bytes(9)) == pc.iso_crc(xor)
    assert pc.iso_crc(x) ^ pc.iso_crc(bytes(9)) == 0xFEE8          # the message's part alone is the zero-preset CRC


def test_golden_set_is_the_one_asked_for(G):
    by = {c["name"]: c for c in G}
    assert {"protect_stereo_44100_128", "protect_mono_44100_128", "protect_stereo_48000_320", "protect_stereo_22050_48", "protect_mono_22050_32", "protect_mono_8000_8",
            "protect_stereo_44100_48_resample_int", "protect_joint_128", "protect_joint_resv_128", "protect_mono_resv_128", "protect_downmix_128", "protect_uneven_calls",
            "flag_copyright", "flag_not_original", "flag_private", "flag_emphasis_1", "everything"} <= set(by)
    # every value of sideinfo_len of a protected stream and both granule counts; padding frames; an integer-ratio resampler in front
    assert {c["ref_sideinfo_len"] for c in G if c.get("protect")} == {38, 23, 15}
    assert {c["ref_sideinfo_len"] for c in G if not c.get("protect")} == {36, 21, 13}
    assert by["protect_stereo_44100_128"]["padded_frames"] > 0 and by["protect_stereo_48000_320"]["padded_frames"] == 0
    assert by["protect_stereo_44100_48_resample_int"]["out_samplerate"] == 22050 and by["protect_downmix_128"]["ref_channels_out"] == 1
    assert by["protect_uneven_calls"]["call_lens"] != by["protect_stereo_44100_128"]["call_lens"] and by["protect_uneven_calls"]["enc_md5"] == by["protect_stereo_44100_128"]["enc_md5"]
    e = by["everything"]
    assert (e["protect"], e["copyright"], e["original"], e["privateBit"], e["emphasis"], e["jointStereo"], e["reservoir"]) == (1, 1, 0, 1, 3, 1, 1)
    for c in G:
        assert sum(c["call_lens"]) == 12 * 1152 and c["frames"] >= 13 and c["flush_len"] > 0


def test_hostsim_every_golden_and_iso_crc(sim, G):
    for c in G:
        pc.run_golden_case(sim, c)


def test_wavesim_every_golden_and_iso_crc(wavesim, G):
    for c in G:
        pc.run_golden_case(wavesim, c)


def test_hostsim_one_call_gives_the_same_stream(sim, G):
    """The batch path of the simulation (one call with all twelve frames' samples) on every golden."""
    for c in G:
        pc.run_golden_case(sim, c, lens=[c["nsamples"]])


def test_wavesim_one_call_gives_the_same_stream(wavesim, G):
    for c in G:
        if c["name"] in ("protect_stereo_44100_128", "protect_mono_22050_32", "protect_joint_resv_128", "protect_mono_8000_8", "everything"):
            pc.run_golden_case(wavesim, c, lens=[c["nsamples"]])


def test_hostsim_flag_bits_against_the_oracle(sim):
    assert pc.flag_family_check(sim, pc.flag_family(20280, 21)) == 21


def test_wavesim_flag_bits_against_the_oracle(wavesim):
    assert pc.flag_family_check(wavesim, pc.flag_family(20281, 7, max_frames=3)) == 7


@pytest.mark.skipif(NODE is None, reason="node not available")
def test_blob_without_the_options_is_unchanged():
    """All 324 triples: a blob built without the options is the same bytes whether they are absent, undefined, null or at their defaults; with
    { protect } only error_protection and sideinfo_len (+2) change, with the flags only their four entries."""
    js = ("const t = require(process.argv[1]); const out = [];"
          "const cfg = (b) => { const n = b.readUInt32LE(8), ent = {}; for (let i = 0; i < n; i++) { const e = 16 + 48 * i; ent[b.toString('ascii', e, e + 32).replace(/\\0.*$/, '')] = [b.readUInt32LE(e + 36), b.readUInt32LE(e + 40)]; }"
          " let s = ''; for (let k = 0; k < ent.cfg_i_names[0]; k++) { const c = b.readInt32LE(ent.cfg_i_names[1] + 4 * k); if (!c) break; s += String.fromCharCode(c); }"
          " const o = {}; s.split(',').forEach((nm, k) => { o[nm] = b.readInt32LE(ent.cfg_i[1] + 4 * k); }); return o; };"
          "const diff = (a, b) => Object.keys(a).filter((k) => a[k] != b[k]).join(',');"
          "for (const ch of [1, 2]) for (const sr of %s) for (const kb of %s) {"
          " const F = { fractionalResample: true };"
          " const a = t.buildBlob(ch, sr, kb, F).blob, b = t.buildBlob(ch, sr, kb, Object.assign({ protect: undefined, copyright: null, original: undefined, privateBit: undefined, emphasis: null }, F)).blob;"
          " const d = t.buildBlob(ch, sr, kb, Object.assign({ protect: false, copyright: false, original: true, privateBit: false, emphasis: 0 }, F)).blob;"
          " const frac = t.fractionalCallLimit(t.resolveParams(ch, sr, kb, F)) > 0;"
          " let p = null; try { p = t.buildBlob(ch, sr, kb, Object.assign({ protect: true }, F)).blob; } catch (e) { p = null; }"
          " const f = t.buildBlob(ch, sr, kb, Object.assign({ copyright: true, original: false, privateBit: true, emphasis: 3 }, F)).blob;"
          " const ca = cfg(a), cp = p ? cfg(p) : null, cf = cfg(f);"
          " out.push([Buffer.compare(a, b) == 0 && Buffer.compare(a, d) == 0 ? 1 : 0, frac ? (p === null ? 1 : 0) : (p && p.length == a.length && diff(ca, cp) == 'sideinfo_len,error_protection' && cp.sideinfo_len == ca.sideinfo_len + 2 && cp.error_protection == 1 ? 1 : 0),"
          "  f.length == a.length && diff(ca, cf) == 'copyright,original,emphasis,extension' && cf.copyright == 1 && cf.original == 0 && cf.emphasis == 3 && cf.extension == 1 ? 1 : 0, frac ? 1 : 0]); }"
          "console.log(JSON.stringify(out));" % (json.dumps(RATES), json.dumps(KBPS)))
    r = subprocess.run([NODE, "-e", js, TABLES_JS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = json.loads(r.stdout)
    assert len(rows) == 324 and all(x[:3] == [1, 1, 1] for x in rows) and sum(x[3] for x in rows) == 49


@pytest.mark.skipif(NODE is None, reason="node not available")
def test_defaults_resolve_to_the_header_the_formatter_always_wrote():
    """All 324 triples without the options: copyright 0, original 1, emphasis 0, extension 0, error_protection 0 and the mode's sideinfo_len."""
    js = ("const t = require(process.argv[1]); let bad = 0, n = 0;"
          "for (const ch of [1, 2]) for (const sr of %s) for (const kb of %s) { const p = t.resolveParams(ch, sr, kb, { fractionalResample: true }); n++;"
          " const base = p.version == 1 ? (p.channels_out == 1 ? 21 : 36) : (p.channels_out == 1 ? 13 : 21);"
          " if (p.copyright != 0 || p.original != 1 || p.emphasis != 0 || p.extension != 0 || p.error_protection != 0 || p.sideinfo_len != base) bad++; }"
          "console.log(JSON.stringify([n, bad]));" % (json.dumps(RATES), json.dumps(KBPS)))
    r = subprocess.run([NODE, "-e", js, TABLES_JS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == [324, 0]


@pytest.mark.skipif(NODE is None, reason="node not available")
def test_tables_refuse_bad_values_with_a_range_error():
    js = ("const t = require(process.argv[1]); const res = [];"
          "for (const o of [{ emphasis: 2 }, { emphasis: 4 }, { emphasis: -1 }, { emphasis: '1' }, { emphasis: 1.5 }, { protect: 2 }, { copyright: 'yes' }, { original: 3 }, { privateBit: 0.5 }])"
          " try { t.buildBlob(2, 44100, 128, o); res.push('accepted'); } catch (e) { res.push(e instanceof RangeError ? 'RangeError' : e.constructor.name); }"
          "try { t.buildBlob(2, 22050, 32, { protect: true, fractionalResample: true }); res.push('accepted'); } catch (e) { res.push(/fractionalResample/.test(e.message) ? 'refused' : e.message); }"
          "res.push(t.resolveParams(2, 44100, 128, { protect: 1, copyright: 1, original: 0, privateBit: 1, emphasis: 1, fractionalResample: true }).sideinfo_len);"
          "console.log(JSON.stringify(res));")
    r = subprocess.run([NODE, "-e", js, TABLES_JS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == ["RangeError"] * 9 + ["refused", 38]


def test_python_refuses_bad_values_with_a_value_error(sim):
    import lamejs_amd
    for kw in ({"emphasis": 2}, {"emphasis": 4}, {"emphasis": True}, {"protect": 2}, {"copyright": "yes"}, {"original": None}, {"private_bit": 7}):
        with pytest.raises(ValueError):
            lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, **kw)


def test_create_refuses_inconsistent_blobs(sim):
    """lhip_create: -3 with a message for a sideinfo_len that does not fit the flag (both directions, and a wrong base), a reserved emphasis, a flag
    that is not a bit, and error_protection on a stream that resamples by a non-integer ratio."""
    import lamejs_amd
    plain, prot = lamejs_amd.tables_blob(2, 44100, 128), lamejs_amd.tables_blob(2, 44100, 128, protect=True)
    assert pc.cfg_entry(plain, "sideinfo_len")[1] == 36 and pc.cfg_entry(prot, "sideinfo_len")[1] == 38 and pc.cfg_entry(prot, "error_protection")[1] == 1
    assert pc.create_rc(sim, 2, 44100, 128, plain)[0] == 0 and pc.create_rc(sim, 2, 44100, 128, prot)[0] == 0
    for blob, pat in ((pc.patched(plain, error_protection=1), "sideinfo_len"), (pc.patched(prot, error_protection=0), "sideinfo_len"), (pc.patched(plain, sideinfo_len=38), "sideinfo_len"),
                      (pc.patched(prot, sideinfo_len=40), "sideinfo_len"), (pc.patched(plain, sideinfo_len=21), "sideinfo_len"), (pc.patched(prot, error_protection=2, sideinfo_len=40), "sideinfo_len"),
                      (pc.patched(plain, emphasis=2), "emphasis"), (pc.patched(prot, emphasis=4), "emphasis"), (pc.patched(plain, copyright=2), "copyright"), (pc.patched(plain, extension=-1), "extension")):
        rc, msg = pc.create_rc(sim, 2, 44100, 128, blob)
        assert rc == -3 and pat in msg, (rc, msg)
    frac = lamejs_amd.tables_blob(2, 22050, 32, fractional_resample=True)
    assert pc.create_rc(sim, 2, 22050, 32, frac)[0] == 0
    rc, msg = pc.create_rc(sim, 2, 22050, 32, pc.patched(frac, error_protection=1, sideinfo_len=pc.cfg_entry(frac, "sideinfo_len")[1] + 2))
    assert rc == -3 and "fractionalResample" in msg, (rc, msg)
    # the wrappers refuse the combination before a blob exists; the option is harmless where the configuration does not resample by such a ratio
    with pytest.raises(lamejs_amd.LhipError, match="fractionalResample"):
        lamejs_amd.Mp3Encoder(2, 22050, 32, lib=sim, protect=True, fractional_resample=True)
    lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, protect=True, fractional_resample=True).close()


def test_output_size_calculators_do_not_see_the_protection(sim):
    """Frame sizes do not change: lhip_encode_output_bytes and lhip_max_output_bytes give the same values with and without { protect }, call
    after call, and the exact ones are kept by the calls."""
    import lamejs_amd
    import pcm
    for ch, sr, kb, kw in ((2, 44100, 128, {}), (1, 44100, 64, {}), (2, 48000, 320, {}), (1, 22050, 32, {}), (1, 8000, 8, {}), (2, 44100, 48, {}), (2, 44100, 128, {"reservoir": True}),
                           (2, 44100, 128, {"joint": True}), (2, 44100, 128, {"downmix": True})):
        L, R = pcm.bursts(6 * 1152, ch)
        a, b = lamejs_amd.Mp3Encoder(ch, sr, kb, lib=sim, **kw), lamejs_amd.Mp3Encoder(ch, sr, kb, lib=sim, protect=True, **kw)
        p = 0
        for n in (1, 1151, 1152, 2305, 777, 1526):
            assert [sim.lhip_encode_output_bytes(a._h, m) for m in (n, 1, 1152, 100000)] == [sim.lhip_encode_output_bytes(b._h, m) for m in (n, 1, 1152, 100000)]
            assert [sim.lhip_max_output_bytes(a._h, m) for m in (n, 0, 4608, 100000)] == [sim.lhip_max_output_bytes(b._h, m) for m in (n, 0, 4608, 100000)]
            assert sim.lhip_output_bytes_is_exact(a._h) == sim.lhip_output_bytes_is_exact(b._h)
            x, y = (e.encodeBuffer(L[p:p + n], None if R is None else R[p:p + n]) for e in (a, b))
            if not kw.get("reservoir"):
                assert len(x) == len(y)                # (encodeBuffer itself checks each against the promise)
            p += n
        fa, fb = a.flush(), b.flush()
        assert p == 6 * 1152 and len(x + fa) > 0 and (kw.get("reservoir") or len(fa) == len(fb))
        a.close()
        b.close()


def test_seek_and_state_on_a_protected_stream(sim):
    """lhip_state_get / lhip_state_set on a protected 24-frame stream cut in two, without and with the reservoir (whose record holds the queued
    headers, CRC included), and lhip_seek without it (seek is not for reservoir streams): the state at the cut and the bytes after it equal the
    unbroken stream's."""
    import lamejs_amd
    import pcm
    L, R = pcm.sine(24 * 1152, 2)          # (steady material: the speculated state of a seek hits; on bursts the loudness adaptation has a longer memory than a test's warm-up)
    cutpos, warm = 12 * 1152, 3 * 1152
    for kw in ({}, {"reservoir": True}):
        mk = lambda: lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, protect=True, **kw)
        whole, graft = mk(), mk()
        head = whole.encodeBuffer(L[:cutpos], R[:cutpos])
        state_at_cut = whole.state_get()
        rest = whole.encodeBuffer(L[cutpos:], R[cutpos:]) + whole.flush()
        assert pc.check_crc(head + rest, True) == 25
        graft.state_set(state_at_cut)                      # a transplanted state continues the stream byte for byte
        assert graft.encodeBuffer(L[cutpos:], R[cutpos:]) + graft.flush() == rest
        if not kw:
            cut = mk()
            nt, p0 = cut.seek_tail_samples(), cutpos - warm
            cut.seek(p0, L[p0 - nt:p0], R[p0 - nt:p0])
            cut.encodeBuffer(L[p0:cutpos], R[p0:cutpos])          # warm-up frames, output discarded
            got = cut.state_get()
            if got != state_at_cut:
                from state_fields import describe_diff
                raise AssertionError(describe_diff(got, state_at_cut))
            assert cut.encodeBuffer(L[cutpos:], R[cutpos:]) + cut.flush() == rest
            cut.close()
        whole.close()
        graft.close()


@pytest.mark.skipif(NODE is None or not ADDON.exists() or not (ROOT / "oracle" / "_ref" / "lame.all.js").exists(),
                    reason="node / addon / reference bundle not available")
def test_js_beside_the_live_reference_hostsim():
    res = run_js_check("js_protection_check.js", 20282, lib=HOSTSIM_SO)
    assert res["mismatches"] == 0 and res["crc_bad"] == 0 and res["range_errors"] == 3 and set(res["families"]) >= {"protect", "flags", "everything", "batch_mixed", "pending"}
