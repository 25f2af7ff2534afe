"""The bitstream formatter, CPU tier: the bodies behind lhip_debug_bits_probe -- kb_bits (form 0) and kb_bits_mw (form 1) of k_bits.h -- in the one-lane and in
the 64-lane simulation over the record sets of tests/bits_probe_cases.py, byte for byte against the oracle's lo_bits_probe, with byte count and output offset.
The oracle's probe path is tied to its encoder's (lo_bits_probe of harvested record k = frame k of the same lo_encode run), and the decoder of tests/maindata.py,
which goes from bits back to values, returns every record's lines and scalefactors from the oracle's bytes and consumes exactly the announced bits."""
import ctypes
import re

import numpy as np
import pytest

import bits_probe_cases as bp
import maindata
from libs import sim_library

KINDS = ("hostsim", "wavesim")


def test_bits_probe_census():
    c = bp.census()
    print("census:", {k: v for k, v in c.items() if k != "missing"})
    assert c["missing"] == [], "\n".join(c["missing"][:40])


def test_bits_probe_oracle_is_the_encoders_path():
    """lo_bits_probe(record k) of a harvested material = frame k of the lo_encode run the record was taken from."""
    for name in bp.CONFIGS:
        for (label, recs, frames), want in zip(bp.harvested(name), bp.oracle_outputs(name)):
            assert len(want) == len(frames) == bp.FRAMES
            off = 0
            for k, f in enumerate(frames):
                assert int(want[k]["status"]) == 0 and bytes(want[k]["bytes"][:int(want[k]["nbytes"])]) == f, (name, label, k)
                assert int(want[k]["offset"]) == off, (name, label, k)
                off += len(f)


@pytest.mark.parametrize("form", (0, 1))
@pytest.mark.parametrize("kind", KINDS)
def test_bits_probe_whole_set(kind, form):
    lib = sim_library(kind)
    for name in bp.CONFIGS:
        cfg = bp.cfg_of(name)
        for (group, labels, recs), want in zip(bp.groups(name), bp.oracle_outputs(name)):
            got = bp.run_probe(lib, name, recs, form=form)
            bad = bp.compare(cfg, labels, recs, got, want)
            assert bad == [], f"{kind} form {form} {name} {group}:\n" + "\n".join(bad)


def test_bits_probe_decoder_returns_the_records():
    """The third leg: the oracle's bytes decoded back to lines and scalefactors."""
    from replaygain_cases import blob_cfg
    for name in bp.CONFIGS:
        cfg = bp.cfg_of(name)
        _, e = blob_cfg(cfg.blob)
        T = maindata.Tables(e)
        for t in bp.SELECTABLE:                                    # every table is prefix-free, no duplicate code (asserted while the look-up is built)
            T.big(t)
        T.quad(0), T.quad(1)
        for (group, labels, recs), want in zip(bp.groups(name), bp.oracle_outputs(name)):
            for r, rec in enumerate(recs):
                d = maindata.decode_frame(want[r]["bytes"][:int(want[r]["nbytes"])].tobytes(), T)
                where = f"{name} {group} record {r} ({labels[r]})"
                assert len(d["gc"]) == cfg.NGC, where
                for gc, g in enumerate(d["gc"]):
                    s = rec["side"][gc]
                    gr = gc // cfg.C
                    assert g["bits"] == int(s["part2_length"]) + int(s["part2_3_length"]), (where, gc, g["bits"])
                    assert g["part2_bits"] == int(s["part2_length"]), (where, gc)
                    assert g["lines"] == rec["l3"][gc].tolist(), (where, gc, int(np.nonzero(np.array(g["lines"]) != rec["l3"][gc])[0][0]))
                    sf = [int(v) for v in s["scalefac"][:len(g["scalefac"])]]
                    if cfg.GR == 2:
                        want_sf = [None if (v == -1 and gr == 1) else v for v in sf]
                    else:
                        want_sf = [max(v, 0) for v in sf]
                    assert g["scalefac"] == want_sf, (where, gc)
                assert d["ancillary"] == maindata.expected_ancillary(d["ancillary_bits"], e["version_bytes"]), (where, d["ancillary_bits"])


def _fitting(cfg, recs):
    """The records that fit an unpadded frame: they can stand at any place of a call."""
    return np.array([bp.frame_used_bits(cfg, r) <= 8 * cfg.base for r in recs])


@pytest.mark.parametrize("kind", KINDS)
def test_bits_probe_reversed_through_one_workgroup(kind):
    """One workgroup takes record after record through one LDS image: after the 1440-byte frame filled to its last bit, the empty frame must find nothing of it
    in L.w, L.q or L.side; and every set in reversed order."""
    lib = sim_library(kind)
    name = "32000/320/stereo"
    cfg = bp.cfg_of(name)
    full, empty = bp.filled_frame(cfg, 8 * cfg.base - 8 * cfg.sideinfo_len), bp.frame_record(cfg, [])
    assert cfg.base == 1440 and bp.frame_used_bits(cfg, full) == 8 * 1440
    pair = np.array([full, empty, full, empty], dtype=cfg.rec_in)
    want = bp.oracle_probe(name, pair)
    assert bytes(want[1]["bytes"][36:40]) == b"LAME" and not want[1]["bytes"][36 + 4 + cfg.n_version:1440].any()
    for form in (0, 1):
        got = bp.run_probe(lib, name, pair, form=form, max_workgroups=1)
        bad = bp.compare(cfg, ["full", "empty", "full", "empty"], pair, got, want)
        assert bad == [], f"{kind} form {form}:\n" + "\n".join(bad)
    for name in bp.CONFIGS:
        cfg = bp.cfg_of(name)
        for group, labels, recs in bp.groups(name):
            keep = _fitting(cfg, recs)
            rv, lv = recs[keep][::-1], [l for l, k in zip(labels, keep) if k][::-1]
            want = bp.oracle_probe(name, rv)
            for form in (0, 1):
                got = bp.run_probe(lib, name, rv, form=form, max_workgroups=1)
                bad = bp.compare(cfg, lv, rv, got, want)
                assert bad == [], f"{kind} form {form} {name} {group} reversed:\n" + "\n".join(bad)


@pytest.mark.parametrize("n", (1, 2, 65))
@pytest.mark.parametrize("kind", KINDS)
def test_bits_probe_record_counts(kind, n):
    lib = sim_library(kind)
    for name in (bp.SYNTH_FULL, "22050/64/stereo"):
        cfg = bp.cfg_of(name)
        _, labels, recs = bp.groups(name)[-1]
        idx = np.nonzero(_fitting(cfg, recs))[0]
        pick = idx[np.linspace(0, len(idx) - 1, n).astype(int)]
        want = bp.oracle_probe(name, recs[pick])
        for form in (0, 1):
            for mw in (0, 1, 2):
                got = bp.run_probe(lib, name, recs[pick], form=form, max_workgroups=mw)
                bad = bp.compare(cfg, [labels[i] for i in pick], recs[pick], got, want)
                assert bad == [], f"{kind} form {form} n {n} max_workgroups {mw}:\n" + "\n".join(bad)


def _one(cfg, gc=0, l3=None, **side):
    """A valid one-record array whose granule-channel `gc` carries a few values; then fields are overwritten (lengths NOT recomputed)."""
    base_l3 = np.zeros(576, dtype=np.int16)
    base_l3[:12] = (1, -1, 0, 1, 1, 0, -1, -1, 0, 1, 0, 0)
    body = ({"big_values": 4, "count1": 12, "table_select": (1, 1, 1), "global_gain": 120}, base_l3)
    rec = bp.frame_record(cfg, [None] * gc + [body])
    for k, v in side.items():
        rec["side"][gc][k] = v
    if l3 is not None:
        for i, v in l3.items():
            rec["l3"][gc][i] = v
    return np.array([rec], dtype=cfg.rec_in)


def test_bits_probe_refusals():
    """A malformed record never reaches a kernel: every class is refused, naming the record and the field; the one-lane simulation only."""
    import lamejs_amd
    lib = sim_library("hostsim")
    name = bp.SYNTH_FULL
    cfg = bp.cfg_of(name)
    good = _one(cfg)
    enc = lamejs_amd.Mp3Encoder(cfg.ch, cfg.sr, cfg.kbps, lib=lib)
    try:
        bp.run_probe(lib, name, good, stream=enc)
        cases = [
            ("big_values", dict(big_values=5)), ("big_values", dict(big_values=578)), ("count1", dict(count1=2)), ("count1", dict(count1=580)), ("count1", dict(count1=14)),
            ("table_select", dict(table_select0=4)), ("table_select", dict(table_select1=32)), ("table_select", dict(table_select0=-1)),
            ("l3", dict(l3={0: 2})), ("l3", dict(table_select0=23, l3={0: 8207})), ("l3", dict(table_select0=16, l3={0: 17})), ("l3", dict(table_select0=0)),
            ("at or above count1", dict(l3={12: 1})), ("count1 region", dict(l3={5: 2})),
            ("region", dict(region0_count=16)), ("region", dict(region1_count=8)), ("region", dict(region0_count=15, region1_count=6)), ("region", dict(region0_count=-1)),
            ("sfbmax", dict(sfbmax=40)), ("scalefac_compress", dict(scalefac_compress=16)), ("sfbdivide", dict(sfbdivide=22)), ("scfsi", dict(scfsi=16)),
            ("block_type", dict(block_type=4)), ("global_gain", dict(global_gain=256)), ("subblock_gain", dict(subblock_gain1=8)), ("mode_ext", dict(mode_ext=4)),
            ("slen", dict(scalefac_compress=0, scalefac=np.r_[1, np.zeros(38, dtype=np.int32)])), ("slen", dict(scalefac=np.r_[-2, np.zeros(38, dtype=np.int32)])),
            ("part2_length + part2_3_length", dict(part2_3_length=int(good[0]["side"][0]["part2_3_length"]) + 1)),
            ("part2_length + part2_3_length", dict(part2_length=1)),
            ("part2_length + part2_3_length", dict(part2_3_length=4096)),
        ]
        for word, change in cases:
            for gc in (0, 3):
                bad = np.concatenate([good, good, _one(cfg, gc=gc, **change)])
                with pytest.raises(lamejs_amd.LhipError, match=rf"lhip_debug_bits_probe: record 2 granule-channel {gc}: .*{re.escape(word)}") as ei:
                    bp.run_probe(lib, name, bad, stream=enc)
                assert word in str(ei.value), (word, change, str(ei.value))
        with pytest.raises(lamejs_amd.LhipError, match="record 0 granule-channel 0: .*slen"):      # -1, a band shared through scfsi, outside granule 1
            bp.run_probe(lib, name, _one(cfg, scalefac=np.r_[-1, np.zeros(38, dtype=np.int32)]), stream=enc)
        # a frame whose parts exceed its bits: four granule-channels that each fit the 12-bit field
        big = bp.frame_record(cfg, [bp.exact_gc(cfg, 4000)] * 4)
        with pytest.raises(lamejs_amd.LhipError, match="record 1: the frame's parts exceed the frame's bits"):
            bp.run_probe(lib, name, np.array([good[0], big], dtype=cfg.rec_in), stream=enc)
        # and the oracle reports the same records instead of aborting
        assert int(bp.oracle_probe(name, np.array([big], dtype=cfg.rec_in))[0]["status"]) == -1
        assert int(bp.oracle_probe(name, _one(cfg, part2_3_length=int(good[0]["side"][0]["part2_3_length"]) + 1))[0]["status"]) == -1
        fn, vp = lib.lhip_debug_bits_probe, ctypes.c_void_p
        out = np.zeros(1, dtype=bp.REC_OUT)
        for args in ((None, 1, out.ctypes.data_as(vp), 0, 0), (good.ctypes.data_as(vp), 0, out.ctypes.data_as(vp), 0, 0), (good.ctypes.data_as(vp), 1, None, 0, 0),
                     (good.ctypes.data_as(vp), 1, out.ctypes.data_as(vp), 2, 0), (good.ctypes.data_as(vp), 1, out.ctypes.data_as(vp), 0, -1),
                     (good.ctypes.data_as(vp), 8193, out.ctypes.data_as(vp), 0, 0)):
            assert fn(enc._h, *args) < 0 and b"lhip_debug_bits_probe" in lib.lhip_last_error()
    finally:
        enc.close()
    # LSF ranges, and -1 outside granule 1
    name = "22050/64/stereo"
    cfg = bp.cfg_of(name)
    for word, change in (("scalefac_compress", dict(scalefac_compress=400)), ("scalefac_compress", dict(scalefac_compress=512)), ("scalefac_compress", dict(scalefac_compress=500)),
                         ("scalefac_compress", dict(scalefac_compress=3, preflag=1)), ("slen", dict(scalefac=np.r_[1, np.zeros(38, dtype=np.int32)]))):
        with pytest.raises(lamejs_amd.LhipError, match=word):
            bp.run_probe(lib, name, _one(cfg, **change))
    resv = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, reservoir=True)
    try:
        with pytest.raises(lamejs_amd.LhipError, match="bit reservoir"):
            bp.run_probe(lib, "44100/128/stereo", _one(bp.cfg_of("44100/128/stereo")), stream=resv)
    finally:
        resv.close()


@pytest.mark.parametrize("kind", KINDS)
def test_bits_probe_leaves_the_stream_alone(kind):
    """The probe uses a stream's tables and nothing of its state: the stream's bytes are the same with and without probe calls between its calls."""
    import lamejs_amd
    import pcm
    lib = sim_library(kind)
    name = "44100/128/stereo"
    cfg = bp.cfg_of(name)
    _, _, recs = bp.groups(name)[0]
    L, R = pcm.CORPORA["bursts"](1152 * 9, 2)
    cuts = (0, 1152 * 2 + 300, 1152 * 5, len(L))

    def encode(probe):
        enc = lamejs_amd.Mp3Encoder(cfg.ch, cfg.sr, cfg.kbps, lib=lib)
        out = []
        try:
            for a, b in zip(cuts, cuts[1:]):
                if probe:
                    bp.run_probe(lib, name, recs, form=len(out) % 2, max_workgroups=len(out) % 2, stream=enc)
                out.append(enc.encodeBuffer(L[a:b], R[a:b]))
            if probe:
                bp.run_probe(lib, name, recs[:20], form=1, stream=enc)
            out.append(enc.flush())
        finally:
            enc.close()
        return out

    plain, probed = encode(False), encode(True)
    assert sum(map(len, plain)) > 3000 and plain == probed
