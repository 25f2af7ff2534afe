"""Every quantization launch path on every configuration family (tests/path_matrix_cases.py), CPU tier: the case list, the oracle's
expectations, the side-information reader and the path bookkeeping are proven on the two simulations before any GPU time is spent.

* the scalar simulation runs the full shapes; it has no two-waves-per-frame program, so LAMEJS_HIP_PAIR_MAX_FRAMES cannot change what it
  runs: its children are the default environment and the one with both switches;
* the wave simulation runs the shapes capped at 17 frames, in the default environment (pair program up to 12 frame slots) and with
  LAMEJS_HIP_PAIR_MAX_FRAMES=0 (the persistent workgroup with its tail help at every shape);
* both run the list once more with LAMEJS_HIP_NO_FAST_QUANT=1: the quality-7 cases through the general kernel bodies.  LAMEJS_HIP_QUANT_GRID_MAX
  does not exist in the simulations: the wave simulation's g_quant_fast and g_quant are one workgroup already, and its launch records must say so.

Children's wall time measured here (the worker's own clock): the scalar simulation's 52 cases and 12 506 frames took 18.4 s (default), 17.5 s (both)
and 18.3 s (nofast) -- 17 s with the 37 quality-3 cases alone; the wave simulation's 46 cases and 1 452 frames took 72 s (default), 85 s (pair0) and 68 s
(nofast) beside other work on the machine.  The limits, 600 s and 1800 s, are more than twenty times that and only end a child that hangs."""
import numpy as np
import pytest

import path_matrix_cases as pm
import sideinfo
from libs import build_sims, sim_library


@pytest.fixture(scope="module")
def sims():
    build_sims()
    import oracle_py
    oracle_py._make_current()


def test_case_list_is_the_one_asked_for():
    cs = pm.cases()
    by = lambda kind: [c for c in cs if c["kind"] == kind]
    assert {(c["family"], c["sr"], c["kb"]) for c in by("stereo")} == {(f, sr, kb) for f, cfgs in pm.TWO_CHANNEL.items() for sr, kb in cfgs} and len(by("stereo")) == 14
    assert len(by("mono")) == 3 and all(len(by(k)) == 2 for k in ("joint", "protect", "f32gain", "downmix"))
    assert all(len(by(k)) == 4 for k in ("resv_mono", "resv_stereo", "resv_joint"))
    for fam in pm.TWO_CHANNEL:          # every family reaches every shape through its two-channel configurations
        assert {f for c in by("stereo") if c["family"] == fam for f in c["seq"]} >= set(pm.SHAPES) | {0}, fam
    for c in cs:
        if not c["resv"]:               # a sequence crosses paths: a one-frame call, a remainder and batches on both sides of eight waves
            assert 1 in c["seq"] and 0 in c["seq"] and min(f for f in c["seq"] if f > 1) <= 9 < max(c["seq"]), c["name"]
    assert len({c["name"] for c in cs}) == len(cs) == 37 + 15
    assert [c["seed"] for c in cs] == list(range(pm.SEED, pm.SEED + len(cs))) and not any(pm.is_fast(c) for c in cs[:37]) and all(pm.is_fast(c) and c["family"] == "fast" for c in cs[37:])
    # quality 7, behind the 37: kinds of their own, sequences of SEQS, the two-output cases reach every shape
    assert [(c["sr"], c["kb"]) for c in by("fast_stereo")] == pm.FAST_STEREO == [(44100, 128), (44100, 320), (32000, 160), (22050, 64), (44100, 48)]
    assert [(c["sr"], c["kb"]) for c in by("fast_mono")] == pm.FAST_MONO and pm.FAST_MONO[:3] == [(44100, 128), (22050, 64), (44100, 32)] and all(c["ch"] == 1 for c in by("fast_mono"))
    assert [(c["sr"], c["kb"]) for c in by("fast_joint")] == [(44100, 128), (22050, 64)]
    for kind in ("fast_protect", "fast_f32gain", "fast_downmix", "fast_resv_stereo"):
        assert [(c["ch"], c["sr"], c["kb"]) for c in by(kind)] == [(2, 44100, 128)], kind
    assert by("fast_protect")[0]["opts"] == dict(pm.FLAGS, quality=7) and by("fast_resv_stereo")[0]["resv"] == "helpers" and tuple(by("fast_resv_stereo")[0]["seq"]) == pm.RESV_SHAPES["helpers"][1]
    assert all(tuple(c["seq"]) in map(tuple, pm.SEQS) for c in cs[37:] if not c["resv"])
    assert {f for c in cs if c["kind"] in pm.FAST_TWO_OUT for f in c["seq"]} == set(pm.SHAPES) | {0}
    assert set(pm.ENVS) == {"default", "pair0", "noframe", "both", "nofast", "grid1"} and len(pm.SWITCHES) == 4 and all(set(e) <= set(pm.SWITCHES) for e in pm.ENVS.values())
    assert pm.ENVS["nofast"] == {"LAMEJS_HIP_NO_FAST_QUANT": "1"} and pm.ENVS["grid1"] == {"LAMEJS_HIP_QUANT_GRID_MAX": "1", "LAMEJS_HIP_PAIR_MAX_FRAMES": "0"}
    assert [c["name"] for c in pm.select(cs, "grid1") if not pm.is_fast(c)] == [c["name"] for c in cs if c["family"] == "mpeg1" and c["kind"] in ("stereo", "mono")]
    assert all(max(c["seq"]) <= 17 for c in pm.for_wavesim(cs))


def test_fast_cases_reach_every_form_of_the_fast_kernel(sims):
    """(PAIR, SKIP) of g_quant_fast by the rule of lhip_tables.h (TableSet::skip_tail) on each case's own blob.  g_quant_fast<0, 0> is reachable, and by
    common configurations: a one-channel stream's lowpass lies higher than a two-channel one's, so one channel at 44100/128, 22050/64 and 32000/96 -- and the
    downmix -- keeps the polyphase bands 28..31.  48000/320 does NOT: every one-channel 48 kHz blob has skip_tail true.  Two channels keep them at 44100/320,
    32000/160 and 22050/64.  The case list must launch all four forms, each in a 150-frame call."""
    import lamejs_amd
    cs = pm.cases()
    form = {(c["kind"], c["sr"], c["kb"]): pm.fast_form(c) for c in cs if pm.is_fast(c) and not c["resv"]}
    assert form == {("fast_stereo", 44100, 128): (1, 1), ("fast_stereo", 44100, 320): (1, 0), ("fast_stereo", 32000, 160): (1, 0), ("fast_stereo", 22050, 64): (1, 0),
                    ("fast_stereo", 44100, 48): (1, 1), ("fast_mono", 44100, 128): (0, 0), ("fast_mono", 22050, 64): (0, 0), ("fast_mono", 44100, 32): (0, 1),
                    ("fast_mono", 32000, 96): (0, 0), ("fast_joint", 44100, 128): (1, 1), ("fast_joint", 22050, 64): (1, 0), ("fast_protect", 44100, 128): (1, 1),
                    ("fast_f32gain", 44100, 128): (1, 1), ("fast_downmix", 44100, 128): (0, 0)}
    assert {pm.fast_form(c) for c in cs if pm.is_fast(c) and not c["resv"] and 150 in c["seq"]} == {(1, 1), (1, 0), (0, 1), (0, 0)}
    for kb in (128, 256, 320):
        af = pm.blob_array(lamejs_amd.tables_blob(1, 48000, kb, quality=7), "amp_filter", "f")
        assert all(float(af[b]) < 1e-12 for b in (28, 29, 30, 31)), kb


def test_oracle_blob_keeps_the_quality(sims):
    """Where the oracle's blob is not the encoder's (Float32 with gains, the downmix) it is still a quality-7 blob: the six switches of the fast mode."""
    import lamejs_amd
    from protection_cases import cfg_entry
    from quality_cases import SWITCHES
    for c in pm.cases():
        ob, eb = pm.oracle_blob(c), lamejs_amd.tables_blob(c["ch"], c["sr"], c["kb"], **c["opts"])
        assert [cfg_entry(ob, k)[1] for k in SWITCHES] == [cfg_entry(eb, k)[1] for k in SWITCHES], c["name"]
        assert (cfg_entry(ob, "noise_shaping")[1] == 0 and cfg_entry(ob, "use_best_huffman")[1] == 0) == pm.is_fast(c), c["name"]


def test_oracle_reproduces_the_reference_at_quality_7(sims):
    """The fast cases take their expectations from the unchanged oracle on a quality-7 blob.  That is a reference only because it writes the unmodified
    reference's bytes (tests/golden/golden_quality.json): two channels, one channel, joint stereo, protected frames, 22050 Hz, integer resampling."""
    import quality_cases as qc
    G = {c["name"]: c for c in qc.goldens()}
    for name in ("q7_stereo_44100_128", "q7_mono_44100_64", "q7_joint_mixed_128", "q7_protect_128", "q7_stereo_22050_48", "q7_stereo_48000_320", "q7_stereo_44100_48_resample_int"):
        assert G[name]["quality"] == 7 and qc.oracle_takes(G[name]) and qc.oracle_reproduces(G[name]), name


def test_plan_calls_completes_the_frames_it_plans(sims):
    """The planner against the library's own prediction (lhip_encode_output_bytes is exact without the reservoir): one frame's bytes per
    planned frame, on a resampling LSF stream and an MPEG-1 one."""
    import lamejs_amd
    lib = sim_library("hostsim")
    for c in (pm.cases()[10], pm.cases()[0]):
        C, frame, ratio = pm.cfg_of(c)
        assert (c["family"] == "resample") == (ratio > 1)
        lens = pm.plan_calls(c["seq"], frame, ratio, np.random.default_rng(5))
        enc = lamejs_amd.Mp3Encoder(c["ch"], c["sr"], c["kb"], lib=lib)
        z = np.zeros(max(lens), dtype=np.int16)
        for F, n in zip(c["seq"], lens):
            got = enc.encodeBuffer(z[:n], z[:n])
            assert len(sideinfo.parse(got)) == F == enc.last_batch_stats()["frames"], (c["name"], F, n)
        enc.close()


@pytest.mark.parametrize("cfg", [(2, 44100, 128, True), (2, 22050, 64, False), (1, 16000, 32, False), (2, 48000, 256, False)])
def test_sideinfo_reader_equals_the_device_side_records(sims, cfg):
    """tests/sideinfo.py against the GrSide records the host simulation keeps for the same stream (lhip_debug_read(4)), field by field and
    exact: an MPEG-1 stream (joint stereo, so mode_ext varies), LSF streams with one and two channels.  The formatter's own mappings are
    the only ones applied: part2_3_length is written with the scalefactor bits, big_values in pairs, table 14 as 16."""
    import stage_taps
    from fuzz_gpu import material
    ch, sr, kb, joint = cfg
    L, R = material(np.random.default_rng(77), 1152 * 30, ch)
    st, mp3 = stage_taps.device_stages(sim_library("hostsim"), ch, sr, kb, L, R, joint=joint)
    frames = sideinfo.parse(mp3)
    assert len(frames) == st["nframes"] >= 29
    t16 = lambda t: 16 if t == 14 else int(t)
    seen = set()
    for k, fr in enumerate(frames):
        assert fr["main_data_begin"] == 0 and fr["channels"] == ch and fr["samplerate"] == sr and fr["kbps"] == kb and not fr["protected"]
        assert fr["mode_ext"] == (int(st["side"][k, 0, 0]["mode_ext"]) if joint else 0), k
        for c in range(ch):
            assert fr["scfsi"][c] == [(int(st["side"][k, 1, c]["scfsi"]) >> b) & 1 if st["GR"] == 2 else 0 for b in range(4)], (k, c)
        for gr in range(st["GR"]):
            for c in range(ch):
                s, g = st["side"][k, gr, c], fr["gr"][gr][c]
                want = {"part2_3_length": int(s["part2_3_length"] + s["part2_length"]), "big_values": int(s["big_values"]) // 2, "global_gain": int(s["global_gain"]),
                        "scalefac_compress": int(s["scalefac_compress"]), "block_type": int(s["block_type"]),
                        "table_select": [t16(s[f"table_select{i}"]) for i in range(2 if s["block_type"] else 3)],
                        "subblock_gain": [int(s[f"subblock_gain{i}"]) if s["block_type"] else 0 for i in range(3)],
                        "region0_count": None if s["block_type"] else int(s["region0_count"]), "region1_count": None if s["block_type"] else int(s["region1_count"]),
                        "preflag": int(s["preflag"]) if st["GR"] == 2 else None, "scalefac_scale": int(s["scalefac_scale"]), "count1table_select": int(s["count1table_select"])}
                got = {f: g[f] for f in want}
                assert got == want, (k, gr, c, got, want)
                seen.add(int(s["block_type"]))
    assert len(seen) >= 2


def test_oracle_writes_protected_frames_as_the_reference_does(sims):
    """The matrix takes its CRC-protected expectations from the oracle: its protected frames are the unmodified reference's, bit for bit
    (tests/golden/golden_protection.json), on every protected golden it can encode (no downmix: it has no input mixing)."""
    import hashlib
    import lamejs_amd
    import protection_cases as pc
    n = 0
    for g in pc.goldens():
        if not g.get("protect") or g.get("downmix"):
            continue
        L, R = pc.case_pcm(g)
        blob = lamejs_amd.tables_blob(g["channels"], g["samplerate"], g["kbps"], **pc.case_opts(g))
        mp3 = pm.oracle_stream(blob, np.ascontiguousarray(L, dtype=np.int16), None if R is None else np.ascontiguousarray(R, dtype=np.int16))
        k = len(mp3) - g["flush_len"]
        assert hashlib.md5(mp3[:k]).hexdigest() == g["enc_md5"] and hashlib.md5(mp3[k:]).hexdigest() == g["flush_md5"], g["name"]
        assert pc.check_crc(mp3, True) == g["frames"]
        n += 1
    assert n >= 8


def test_material_is_not_trivial(sims):
    """The census of the ORACLE's bytes over each two-channel family (and the joint cases): all four block types, both count1 tables, ESC
    tables, scalefac_scale, subblock_gain, empty granules, for MPEG-1 preflag and scfsi, both mode_ext values -- every count at least 2,
    so that one changed granule does not flip a condition the GPU tier relies on."""
    cs = pm.cases()
    joint = sideinfo.census([st[4] for c in cs if c["kind"] == "joint" for st in pm.case_streams(c)])
    for fam in pm.TWO_CHANNEL:
        cen = sideinfo.census([st[4] for c in cs if c["kind"] == "stereo" and c["family"] == fam for st in pm.case_streams(c)])
        print(fam, {k: v for k, v in cen.items() if k != "tables"}, "tables", sorted(cen["tables"]))
        assert pm.census_ok(fam, cen, joint if fam == "mpeg1" else None, at_least=2) == [], fam
    print("joint", joint["mode_ext"])


def _run(backend, env_name, limit, cs):
    status, recs, text, _ = pm.run_child(env_name, backend, limit)
    assert status == 0, (status, text)
    print(backend, env_name, recs[-1])
    bad = pm.check_records(cs, recs, env_name, backend, 256)
    assert bad == [], "\n".join(bad[:40])
    return recs


def _fast_batches(recs):
    return [r for r in recs if r.get("kind", "").startswith("fast_") and "SEPARATE" in r.get("paths", ()) and not r["kind"].startswith("fast_resv")]


@pytest.mark.parametrize("env_name", ["default", "both", "nofast"])
def test_hostsim_matrix(sims, env_name):
    """Full shapes on the scalar simulation (the limit only ends a child that hangs)."""
    recs = _run("hostsim", env_name, 600, pm.cases())
    assert not any("QUANT_PAIR" in r.get("paths", ()) for r in recs)
    fast = _fast_batches(recs)
    assert fast and all(("QUANT_FAST" in r["paths"]) == (env_name != "nofast") for r in fast)
    assert {r["frames"] for r in fast if r["kind"] in pm.FAST_TWO_OUT} >= set(pm.SHAPES) - {1}


@pytest.mark.parametrize("env_name", ["default", "pair0", "nofast"])
def test_wavesim_matrix(sims, env_name):
    """Shapes capped at 17 frames on the wave simulation: both wave programs of the two-channel quantization, and g_quant_fast's workgroup of
    pairs / of single waves -- one workgroup, as LAMEJS_HIP_QUANT_GRID_MAX=1 makes the device's."""
    recs = _run("wavesim", env_name, 1800, pm.for_wavesim(pm.cases()))
    two = [r for r in recs if r.get("kind") in pm.TWO_OUT and r.get("frames", 0) >= 2]
    if env_name == "pair0":
        assert two and all("QUANT_PERSISTENT" in r["paths"] for r in two)
    else:
        assert {"QUANT_PAIR", "QUANT_PERSISTENT"} <= {p for r in two for p in r["paths"]}
    fast = _fast_batches(recs)
    if env_name == "nofast":
        assert fast and {"QUANT_PAIR", "QUANT_PERSISTENT"} <= {p for r in fast for p in r["paths"]} and not any("QUANT_FAST" in r["paths"] for r in fast)
    else:
        assert fast and all("QUANT_FAST" in r["paths"] and r["launch"]["wg"] == 1 and r["launch"]["waves"] == 8 for r in fast)
        need = pm.check_one_workgroup(recs, env_name, max_shape=17)
        assert [b for b in need if env_name == "pair0" or "g_quant calls" not in b] == [], need
