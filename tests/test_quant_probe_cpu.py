"""The quantization search's pure functions, CPU tier: the kernel body behind lhip_debug_quant_probe in the one-lane and in the 64-lane simulation over the
record set of tests/quant_probe_cases.py, every output field bit for bit against the oracle's lo_quant_probe -- calc_xmin's thresholds, the analog-silence
rule, one quantization and Huffman count at a gain with the full and with the short round count, and calc_noise's distort / over_count / over_SSD /
max_noise without a cache, filling one, wholly cached, and with fresh and cached bands mixed (the 3-line body and the table set's 7- or 9-line body).
For the final state of every harvested granule-channel the thresholds and the perceptual entropy also equal what the oracle's encoder recorded in its tap
(lo_tap.l3_xmin, lo_tap.pe)."""
import ctypes

import numpy as np
import pytest

import quant_probe_cases as qp
from libs import sim_library
from noise_lines_cases import line_counts

KINDS = ("hostsim", "wavesim")


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def test_quant_probe_census():
    n = qp.census()
    print("census:", n)
    assert n["records"] >= 2000


@pytest.mark.parametrize("kind", KINDS)
def test_quant_probe_whole_set(kind):
    lib = sim_library(kind)
    for cfg in qp.CONFIGS:
        recs, names, checks = qp.record_set(cfg)
        got = qp.run_probe(lib, cfg, recs)
        bad = qp.compare(cfg, got, qp.oracle_outputs(cfg), names, kind)
        assert bad == [], "\n".join(bad)
        # the encoder's own thresholds and entropies (the oracle's tap), for the final state of every harvested granule-channel
        nx = npe = 0
        for i, chk in enumerate(checks):
            if chk is None:
                continue
            xmin, pe = chk
            n = qp.psymax_of(int(recs[i]["block_type"]))
            assert np.array_equal(_u(got[i]["xmin"][:n]), _u(xmin[:n])), (kind, names[i], "xmin against lo_tap.l3_xmin", got[i]["xmin"][:n], xmin[:n])
            nx += 1
            if pe is not None:
                assert _u(np.float64(got[i]["pe"]))[()] == _u(np.float64(pe))[()], (kind, names[i], "pe against lo_tap.pe", got[i]["pe"], pe)
                npe += 1
        assert nx >= 50 and npe >= nx // 2, (qp.config_name(cfg), nx, npe)


@pytest.mark.parametrize("kind", KINDS)
def test_quant_probe_reversed_through_one_wave(kind):
    """Every record through ONE wave's LDS record, in reversed order: what a record leaves there -- the working spectrum's words 256..287, the noise cache,
    the band tables of the other block kind -- must not reach the next one."""
    lib = sim_library(kind)
    for cfg in qp.CONFIGS:
        recs, names, _ = qp.record_set(cfg)
        got = qp.run_probe(lib, cfg, recs[::-1], max_workgroups=1)[::-1]
        bad = qp.compare(cfg, got, qp.oracle_outputs(cfg), names, kind + " reversed, one wave")
        assert bad == [], "\n".join(bad)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (1, 2, 65))
def test_quant_probe_record_counts(kind, n):
    lib = sim_library(kind)
    cfg = qp.CONFIGS[0]
    recs, names, _ = qp.record_set(cfg)
    pick = np.linspace(0, len(recs) - 1, n).astype(int)
    for mw in (0, 1, 2):
        got = qp.run_probe(lib, cfg, recs[pick], max_workgroups=mw)
        bad = qp.compare(cfg, got, qp.oracle_outputs(cfg)[pick], [names[i] for i in pick], f"{kind} n={n} max_workgroups={mw}")
        assert bad == [], "\n".join(bad)


def test_quant_probe_refusals():
    import lamejs_amd
    lib = sim_library("hostsim")
    cfg = qp.CONFIGS[0]
    recs, names, _ = qp.record_set(cfg)
    good = recs[:1].copy()
    out = np.zeros(1, dtype=qp.REC_OUT)
    enc = lamejs_amd.Mp3Encoder(cfg[2], cfg[0], cfg[1], lib=lib)
    fn, vp = lib.lhip_debug_quant_probe, ctypes.c_void_p
    try:
        assert fn(None, good.ctypes.data_as(vp), 1, out.ctypes.data_as(vp), 0) < 0
        for args in ((None, 1, out.ctypes.data_as(vp), 0), (good.ctypes.data_as(vp), 1, None, 0), (good.ctypes.data_as(vp), 0, out.ctypes.data_as(vp), 0),
                     (good.ctypes.data_as(vp), 1, out.ctypes.data_as(vp), -1)):
            assert fn(enc._h, *args) < 0 and b"lhip_debug_quant_probe" in lib.lhip_last_error()
        assert fn(enc._h, good.ctypes.data_as(vp), 1, out.ctypes.data_as(vp), 0) == 0

        def refused(why, **fields):
            r = good.copy()
            for k, v in fields.items():
                r[0][k] = v
            with pytest.raises(lamejs_amd.LhipError, match=why):
                qp.run_probe(lib, cfg, np.concatenate([good, r]), stream=enc)

        refused("record 1: block_type", block_type=4)
        refused("record 1: block_type", block_type=-1)
        refused("record 1: global_gain", global_gain=256)
        short = dict(block_type=2, global_gain=0, scalefac_scale=1, preflag=0, subblock_gain=7)
        sf = np.full(qp.SFBMAX, 15, dtype=np.int32)
        qp.run_probe(lib, cfg, np.concatenate([good, _with(good, scalefac=sf, **short)]), stream=enc)        # -116: the table's first entry
        sf[4] = 17
        refused("record 1: a band's step outside the pow20 table", scalefac=sf, **short)
        refused("record 1: preflag on a short block", block_type=2, preflag=1)
        ix = np.zeros(576, dtype=np.int16)
        ix[575] = qp.IXMAX_VAL + 1
        refused("record 1: ix_in", flags=1, ix_in=ix)
        ix[575] = -1
        refused("record 1: ix_in", flags=1, ix_in=ix)
        refused("record 1: unknown flag", flags=2)
        xr = good[0]["xr"].copy()
        xr[17] = np.nan
        refused("record 1: xr not finite", xr=xr)
        refused("record 1: ath_adjust", ath_adjust=0.0)
    finally:
        enc.close()
    q7 = lamejs_amd.Mp3Encoder(cfg[2], cfg[0], cfg[1], lib=lib, quality=7)
    try:
        with pytest.raises(lamejs_amd.LhipError, match="quality 7"):
            qp.run_probe(lib, cfg, good, stream=q7)
    finally:
        q7.close()


def _with(good, **fields):
    r = good.copy()
    for k, v in fields.items():
        r[0][k] = v
    return r


@pytest.mark.parametrize("kind", KINDS)
def test_quant_probe_leaves_the_stream_alone(kind):
    """The probe uses a stream's tables and nothing of its state: the stream's bytes are the same with and without probe calls between its calls."""
    import lamejs_amd
    import pcm
    lib = sim_library(kind)
    cfg = qp.CONFIGS[0]
    recs, _, _ = qp.record_set(cfg)
    L, R = pcm.CORPORA["bursts"](1152 * 9, 2)
    cuts = (0, 1152 * 2 + 300, 1152 * 5, len(L))

    def encode(probe):
        enc = lamejs_amd.Mp3Encoder(cfg[2], cfg[0], cfg[1], lib=lib)
        out = []
        try:
            for a, b in zip(cuts, cuts[1:]):
                if probe:
                    qp.run_probe(lib, cfg, recs[:40], max_workgroups=len(out) % 2, stream=enc)
                out.append(enc.encodeBuffer(L[a:b], R[a:b]))
            if probe:
                qp.run_probe(lib, cfg, recs[40:60], stream=enc)
            out.append(enc.flush())
        finally:
            enc.close()
        return out

    plain, probed = encode(False), encode(True)
    assert sum(map(len, plain)) > 3000 and plain == probed


def test_quant_probe_noise_bodies():
    """Which body of calc_noise's line pass a call takes (the 64-lane simulation counts them: lhip_debug_read(12)): calls e and g -- band 0 alone is fresh,
    the highest band that ends at or below line 192 alone is -- the 3-line body; every other call, h -- the band above that one alone -- among them, the
    table set's 7- or 9-line body, as the rule of lhip_tables.h says on the configuration's own blob."""
    lib = sim_library("wavesim")
    for cfg in qp.CONFIGS:
        recs, _, _ = qp.record_set(cfg)
        want = qp.oracle_outputs(cfg)
        ran = want["nz"]["ran"].sum(axis=0)
        before = line_counts(lib)
        qp.run_probe(lib, cfg, recs)
        n7, n9, n3 = (b - a for a, b in zip(before, line_counts(lib)))
        full = int(ran[[0, 1, 2, 3, 5, 7]].sum())
        assert ran[4] > 0 and ran[6] > 0 and ran[7] == ran[6] and n3 == ran[4] + ran[6], (qp.config_name(cfg), n3, ran)
        assert (n7, n9) == ((full, 0) if qp.expected_nln(cfg) == 7 else (0, full)), (qp.config_name(cfg), n7, n9, full)
