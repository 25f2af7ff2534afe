"""The quantization search's pure functions on the device: the kernel g_quant_probe (lhip_debug_quant_probe) over the record set of
tests/quant_probe_cases.py, every output field bit for bit against the oracle's lo_quant_probe (the CPU tier, tests/test_quant_probe_cpu.py, holds the two
simulations of the same body to the same outputs and shows which body of calc_noise each call takes).  Forward with the default grid; in reversed order
through one workgroup -- one wave, whose LDS record then serves every record in turn; and 1 and 65 records.  About 4500 records of 6 KB and one short
kernel per configuration: a test is a second or two.  No child processes; after a call that reported an error no further call is made."""
import numpy as np
import pytest

import quant_probe_cases as qp
from libs import lib  # noqa: F401

pytestmark = pytest.mark.gpu

_failed = []


def _probe(lib, cfg, recs, **kw):
    assert not _failed, f"not started: an earlier probe call failed ({_failed[0]})"
    try:
        return qp.run_probe(lib, cfg, recs, **kw)
    except Exception as e:
        _failed.append(f"{qp.config_name(cfg)}: {e}")
        raise


def test_gpu_quant_probe_whole_set(lib):
    for cfg in qp.CONFIGS:
        recs, names, checks = qp.record_set(cfg)
        got = _probe(lib, cfg, recs)
        bad = qp.compare(cfg, got, qp.oracle_outputs(cfg), names, "device")
        assert bad == [], "\n".join(bad)
        for i, chk in enumerate(checks):                 # the encoder's own thresholds (lo_tap.l3_xmin) and entropies (lo_tap.pe)
            if chk is None:
                continue
            xmin, pe = chk
            n = qp.psymax_of(int(recs[i]["block_type"]))
            assert np.array_equal(got[i]["xmin"][:n].view(np.uint32), xmin[:n].view(np.uint32)), (names[i], "xmin against lo_tap.l3_xmin")
            if pe is not None:
                assert np.float64(got[i]["pe"]).view(np.uint64) == np.float64(pe).view(np.uint64), (names[i], "pe against lo_tap.pe", got[i]["pe"], pe)


def test_gpu_quant_probe_reversed_through_one_workgroup(lib):
    for cfg in qp.CONFIGS:
        recs, names, _ = qp.record_set(cfg)
        got = _probe(lib, cfg, recs[::-1], max_workgroups=1)[::-1]
        bad = qp.compare(cfg, got, qp.oracle_outputs(cfg), names, "device reversed, one workgroup")
        assert bad == [], "\n".join(bad)


@pytest.mark.parametrize("n", (1, 65))
def test_gpu_quant_probe_record_counts(lib, n):
    cfg = qp.CONFIGS[0]
    recs, names, _ = qp.record_set(cfg)
    pick = np.linspace(0, len(recs) - 1, n).astype(int)
    got = _probe(lib, cfg, recs[pick])
    bad = qp.compare(cfg, got, qp.oracle_outputs(cfg)[pick], [names[i] for i in pick], f"device n={n}")
    assert bad == [], "\n".join(bad)
