"""Every quantization launch path on every configuration family (tests/path_matrix_cases.py), CPU tier: the case list, the oracle's
expectations, the side-information reader and the path bookkeeping are proven on the two simulations before any GPU time is spent.

* the scalar simulation runs the full shapes; it has no two-waves-per-frame program, so LAMEJS_HIP_PAIR_MAX_FRAMES cannot change what it
  runs: its children are the default environment and the one with both switches;
* the wave simulation runs the shapes capped at 17 frames, in the default environment (pair program up to 12 frame slots) and with
  LAMEJS_HIP_PAIR_MAX_FRAMES=0 (the persistent workgroup with its tail help at every shape)."""
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
    assert len({c["name"] for c in cs}) == len(cs) == 37
    assert all(max(c["seq"]) <= 17 for c in pm.for_wavesim(cs))


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
    bad = pm.check_records(cs, recs, env_name, backend, 256)
    assert bad == [], "\n".join(bad[:40])
    return recs


@pytest.mark.parametrize("env_name", ["default", "both"])
def test_hostsim_matrix(sims, env_name):
    """Full shapes on the scalar simulation (about 10 000 frames, 17 s here; the limit only ends a child that hangs)."""
    recs = _run("hostsim", env_name, 600, pm.cases())
    assert not any("QUANT_PAIR" in r.get("paths", ()) for r in recs)


@pytest.mark.parametrize("env_name", ["default", "pair0"])
def test_wavesim_matrix(sims, env_name):
    """Shapes capped at 17 frames on the wave simulation: both wave programs of the two-channel quantization."""
    recs = _run("wavesim", env_name, 1200, pm.for_wavesim(pm.cases()))
    two = [r for r in recs if r.get("kind") in pm.TWO_OUT and r.get("frames", 0) >= 2]
    if env_name == "pair0":
        assert two and all("QUANT_PERSISTENT" in r["paths"] for r in two)
    else:
        assert {"QUANT_PAIR", "QUANT_PERSISTENT"} <= {p for r in two for p in r["paths"]}
