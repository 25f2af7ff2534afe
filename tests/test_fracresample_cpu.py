"""{ fractionalResample } (extension): the 49 configurations the reference resamples by a non-integer ratio, call-sequence-exact.
CPU tier: tables, the unchanged oracle against the goldens of the unmodified reference, the kernel logic (host / wave simulation) and the
host arithmetic (outputs and frames per call, the flush plan)."""
import hashlib
import json
import subprocess

import numpy as np
import pytest

import fracresample_cases as fc
from conftest import ROOT, load_case_pcm
from libs import ADDON, HOSTSIM_SO, NODE, run_js_check, sim, wavesim  # noqa: F401

RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000]
KBPS = [8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 192, 224, 256, 320]


@pytest.fixture(scope="module")
def G():
    return fc.golden_frac()


def test_golden_set_is_the_one_asked_for(G):
    cases = G["cases"]
    kinds = [c["kind"] for c in cases]
    assert len(fc.triples(cases)) == 49 and G["ratios"] == len({c["samplerate"] / c["out_samplerate"] for c in cases})
    assert (kinds.count("calls576"), kinds.count("calls1152"), kinds.count("odd"), kinds.count("badcall")) == (49, 23, 12, G["ratios"])
    for c in cases:
        assert len(c["call_lens"]) >= (10 if c["kind"] == "badcall" else 12) and not c["flush"][0]["nan_in_window"]
        if c["kind"] == "odd":
            assert all(577 <= n <= c["call_limit"] and n % 2 for n in c["call_lens"]) and len(set(c["call_lens"])) >= 2
        if c["kind"] == "badcall":
            assert c["call_lens"][c["bad_call"]] == c["call_limit"] + 200 and c["bad_call"] == 3


@pytest.mark.skipif(NODE is None, reason="node not available")
def test_refused_without_the_option_accepted_with_it(G):
    """Without the option the 49 triples are refused as before (the text names the option); with it all 324 triples the reference accepts
    build; for the 275 others the blob is the same bytes with and without it."""
    import lamejs_amd
    for ch, sr, kb in fc.triples(G["cases"]):
        with pytest.raises(lamejs_amd.LhipError, match="resampl.*fractionalResample"):
            lamejs_amd.tables_blob(ch, sr, kb)
    js = ("const t = require(process.argv[1]); const out = [];"
          "for (const ch of [1, 2]) for (const sr of %s) for (const kb of %s) {"
          " const a = t.buildBlob(ch, sr, kb, { fractionalResample: true }); let b = null; try { b = t.buildBlob(ch, sr, kb); } catch (e) { if (!/resampl/.test(e.message)) throw e; }"
          " out.push([ch, sr, kb, a.params.rs_filter_l, a.params.rs_bpc, a.blob.length, b ? (Buffer.compare(a.blob, b.blob) == 0 ? 1 : 0) : -1]); }"
          "console.log(JSON.stringify(out));" % (json.dumps(RATES), json.dumps(KBPS)))
    r = subprocess.run([NODE, "-e", js, str(ROOT / "lamejs_amd" / "js" / "tables.js")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = json.loads(r.stdout)
    assert len(rows) == 324
    frac = [x for x in rows if x[6] == -1]
    assert sorted((x[0], x[1], x[2]) for x in frac) == fc.triples(G["cases"])
    assert all(x[3] == 31 and 1 <= x[4] <= 320 and x[5] < 400000 for x in frac)
    assert all(x[6] == 1 for x in rows if x[6] != -1) and len(rows) - len(frac) == 275


@pytest.mark.skipif(NODE is None, reason="node not available")
def test_blackfilt_rows_equal_a_live_reference(G):
    """One triple per ratio: all 2 * bpc + 1 windows of the blob against gfc.blackfilt of the unmodified reference after its first call."""
    res = run_js_check("tools/check_fracresample_tables.js")
    assert res["ratios"] == G["ratios"] and res["mismatches"] == 0 and res["rows"] >= 3 * G["ratios"]


def test_unchanged_oracle_reproduces_every_golden_call_sequence(G):
    """Blob + generator without a GPU: the oracle (its fill_buffer_resample works for any ratio from the blob) fed the new blobs and the golden
    call sequences.  Its flush is not called for these configurations (it aborts at the first fractional position by design)."""
    import lamejs_amd
    from oracle_py import OracleStream
    for case in G["cases"]:
        L, R = load_case_pcm(case)
        p, good, got = 0, 0, []
        with OracleStream(lamejs_amd.tables_blob(case["channels"], case["samplerate"], case["kbps"], fractional_resample=True)) as o:
            for c, n in enumerate(case["call_lens"]):
                l, r = L[p:p + n], None if R is None else R[p:p + n]
                p += n
                if c == case.get("bad_call", -1):
                    continue
                got.append(o.encode(l, r))
                assert len(got[-1]) == case["call_bytes"][good], (case["channels"], case["samplerate"], case["kbps"], case["kind"], c, len(got[-1]))
                good += 1
        assert hashlib.md5(b"".join(got)).hexdigest() == case["enc_md5"], (case["channels"], case["samplerate"], case["kbps"], case["kind"])


def test_hostsim_every_golden_case_and_the_host_arithmetic(sim, G):
    """The kernel logic (one lane) and, for every golden case, the host arithmetic alone: the predicted k and frame count per call, the flush
    frame count, lengths and clean flags equal the reference's; the calls the reference does not consume whole are refused with -4, the limit
    named, the stream untouched."""
    for case in G["cases"]:
        fc.run_case(sim, case)


def test_wavesim_subset(wavesim, G):
    """The wave programs (64 lanes as fibers), one-frame launches: one case per ratio of every kind."""
    seen, n = set(), 0
    for case in G["cases"]:
        key = (case["kind"], case["samplerate"], case["out_samplerate"])
        if key in seen:
            continue
        seen.add(key)
        fc.run_case(wavesim, case, host_arithmetic=False)
        n += 1
    assert n >= 2 * G["ratios"]


def test_hostsim_batch_over_all_49_configurations(sim, G):
    """lhip_encode_batch over one stream of every configuration at once (12 rounds of 576 samples) == the streams one by one."""
    fc.batch_all_configurations(sim, G)


def test_refused_entries_and_option_combinations(sim):
    import lamejs_amd
    enc = lamejs_amd.Mp3Encoder(2, 44100, 96, lib=sim, fractional_resample=True)
    assert enc.call_limit() == 1585
    for f in (enc.state_get, lambda: enc.state_set(b"\0" * 64)):
        with pytest.raises(lamejs_amd.LhipError, match=r"\(-4\).*fractionalResample"):
            f()
    with pytest.raises(lamejs_amd.LhipError, match=r"\(-4\)"):
        enc.seek(2304, np.zeros(enc.seek_tail_samples(), np.int16), np.zeros(enc.seek_tail_samples(), np.int16))
    enc.flush()
    with pytest.raises(lamejs_amd.LhipError, match="flushed"):
        enc.encodeBuffer(np.zeros(576, np.int16), np.zeros(576, np.int16))
    enc.close()
    with pytest.raises(lamejs_amd.LhipError, match="cannot be combined"):
        lamejs_amd.tables_blob(2, 44100, 96, reservoir=True, fractional_resample=True)
    plain = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=sim, fractional_resample=True)      # the option changes nothing where no such ratio occurs
    assert plain.call_limit() == 0
    plain.close()


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_js_beside_the_live_reference_hostsim(sim):
    """lamejs_amd/js with { fractionalResample: true } (kernel logic: the one-lane simulation) beside the live unmodified reference:
    tests/js_fracresample_check.js, fixed seed."""
    res = run_js_check("js_fracresample_check.js", 20251, lib=HOSTSIM_SO)
    assert res["calls"] == 160 and res["mismatches"] == 0 and res["refused_long_calls"] == 8 and res["clean_flush_frames"] >= 1
