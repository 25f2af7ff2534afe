"""The bitstream formatter on the device: the kernel g_bits_probe (lhip_debug_bits_probe) -- kb_bits on one wave per workgroup (form 0), kb_bits_mw on GR * C
waves that pack into one shared LDS image and meet on two LDS counters (form 1) -- over the record sets of tests/bits_probe_cases.py, byte for byte against the
oracle's lo_bits_probe with byte count and output offset (the CPU tier, tests/test_bits_probe_cpu.py, holds the two simulations of the same bodies to the same
outputs, ties the oracle's probe to its encoder and decodes the oracle's bytes back to the records).  Forward in both forms; in reversed order through one
workgroup, whose LDS image then serves every record in turn; 1 and 65 records.  One short kernel per call over at most a few hundred 6 KB records: a test is a
second or two.  No refusal cases, no child processes; after a call that reported an error no further call is made."""
import numpy as np
import pytest

import bits_probe_cases as bp
from libs import lib  # noqa: F401

pytestmark = pytest.mark.gpu

_failed = []


def _probe(lib, name, recs, **kw):
    assert not _failed, f"not started: an earlier probe call failed ({_failed[0]})"
    try:
        return bp.run_probe(lib, name, recs, **kw)
    except Exception as e:
        _failed.append(f"{name}: {e}")
        raise


def _fitting(cfg, recs):
    """The records that fit an unpadded frame: they can stand at any place of a call."""
    return np.array([bp.frame_used_bits(cfg, r) <= 8 * cfg.base for r in recs])


@pytest.mark.parametrize("form", (0, 1))
def test_gpu_bits_probe_whole_set(lib, form):
    for name in bp.CONFIGS:
        cfg = bp.cfg_of(name)
        for (group, labels, recs), want in zip(bp.groups(name), bp.oracle_outputs(name)):
            got = _probe(lib, name, recs, form=form)
            bad = bp.compare(cfg, labels, recs, got, want)
            assert bad == [], f"device form {form} {name} {group}:\n" + "\n".join(bad)


def test_gpu_bits_probe_reversed_through_one_workgroup(lib):
    name = "32000/320/stereo"
    cfg = bp.cfg_of(name)
    full, empty = bp.filled_frame(cfg, 8 * cfg.base - 8 * cfg.sideinfo_len), bp.frame_record(cfg, [])
    pair = np.array([full, empty, full, empty], dtype=cfg.rec_in)
    got = _probe(lib, name, pair, form=0, max_workgroups=1)
    bad = bp.compare(cfg, ["full", "empty", "full", "empty"], pair, got, bp.oracle_probe(name, pair))
    assert bad == [], "device, the 1440-byte frame then the empty one:\n" + "\n".join(bad)
    for name in bp.CONFIGS:
        cfg = bp.cfg_of(name)
        for group, labels, recs in bp.groups(name):
            keep = _fitting(cfg, recs)
            rv, lv = recs[keep][::-1], [l for l, k in zip(labels, keep) if k][::-1]
            got = _probe(lib, name, rv, form=0, max_workgroups=1)
            bad = bp.compare(cfg, lv, rv, got, bp.oracle_probe(name, rv))
            assert bad == [], f"device reversed, one workgroup, {name} {group}:\n" + "\n".join(bad)


@pytest.mark.parametrize("n", (1, 65))
def test_gpu_bits_probe_record_counts(lib, n):
    name = bp.SYNTH_FULL
    cfg = bp.cfg_of(name)
    _, labels, recs = bp.groups(name)[-1]
    idx = np.nonzero(_fitting(cfg, recs))[0]
    pick = idx[np.linspace(0, len(idx) - 1, n).astype(int)]
    want = bp.oracle_probe(name, recs[pick])
    for form in (0, 1):
        got = _probe(lib, name, recs[pick], form=form)
        bad = bp.compare(cfg, [labels[i] for i in pick], recs[pick], got, want)
        assert bad == [], f"device form {form} n {n}:\n" + "\n".join(bad)
