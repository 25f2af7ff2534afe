"""Every quantization launch path on every configuration family, on the device (tests/path_matrix_cases.py; the CPU tier proves the cases,
the oracle's expectations, the reader and the bookkeeping first: tests/test_path_matrix_cpu.py).  One test per environment; each starts
tests/tools/path_matrix_worker.py as a fresh child process (the switches are read once per process) under `timeout -k 10`, and asserts

1. zero mismatches against the oracle;
2. every call's path set is the one the expectation table gives for the CU count read at run time, every required (family, path, shape)
   cell was observed and none that the environment makes impossible;
3. (default environment) the material is not trivial: the census of the oracle's bytes (quality 3 only: the fast mode has no scalefac_scale /
   subblock_gain to find);
4. every call's launch record (lhip_debug_read(11): workgroups, waves per workgroup, frame slots, kernel, template form) is the one its path set, its
   shape and the device's grid rule give, and over the quality-7 cases all four forms of g_quant_fast -- (PAIR, SKIP) = (1, 1), (1, 0), (0, 1), (0, 0) --
   were launched (path_matrix_cases.check_launch).

The quality-7 cases ride in every environment.  Two environments are theirs: `nofast` (LAMEJS_HIP_NO_FAST_QUANT=1: the same streams through
g_quant_pair / g_quant, g_quant_fast never launched) and `grid1` (LAMEJS_HIP_QUANT_GRID_MAX=1 with LAMEJS_HIP_PAIR_MAX_FRAMES=0: g_quant_fast and
g_quant as ONE workgroup, so that its four pairs / eight waves take frame after frame -- 37 rounds and more per pair in a 150-frame call: the slot
handshake, the parity of the bits words, the growing done words, the seeds of a wave's previous frame and the repair they cause behind it --
and the quality-3 two-channel cases run g_quant's tail help inside one workgroup).  grid1 runs last.

After a child that ended by a signal or a time limit, or whose output holds a HIP error, no further child is started: the later tests fail
at once.  Reads nothing outside the repository tree and oracle/_ref/.

Time limits, from the children's own wall time measured on an MI355X (52 cases, 12 506 frames each): the worker's encode loop took 2.50 s
(default), 2.44 s (pair0), 2.47 s (noframe), 2.47 s (both), 2.43 s (nofast) and 2.53 s (grid1: one workgroup costs nothing measurable at these
shapes, so grid1 runs the whole case list); with interpreter start, library load and the oracle's side the tests took 3.9 - 4.2 s (default) and 2.9 -
3.8 s (the others) in two runs.  Before the quality-7 cases (37 cases, 10 223 frames) the same four loops took 2.12 / 2.00 / 2.00 / 2.02 s on the
same machine.  The limits are 90 s -- more than twenty times the slowest whole test, which bounds its child from above, for a loaded machine -- and
120 s for the default environment, which runs first and on a fresh checkout also generates the table blobs and builds the oracle (5.1 s measured
with the oracle rebuilt)."""
import pytest

import path_matrix_cases as pm
import sideinfo

pytestmark = pytest.mark.gpu

LIMITS = {"default": 120, "pair0": 90, "noframe": 90, "both": 90, "nofast": 90, "grid1": 90}
GRID1_CASES = "all"
_fatal = []


@pytest.fixture(scope="module")
def num_cus():
    import torch
    assert torch.cuda.is_available()
    n = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert n >= 1
    return n


def _run(env_name, num_cus, which="all"):
    assert not _fatal, f"not started: an earlier child faulted, hung or reported a HIP error ({_fatal[0]})"
    cs = pm.select(pm.cases(), which)
    status, recs, text, fatal = pm.run_child(env_name, "gpu", LIMITS[env_name], args=[num_cus, f"--cases={which}"])
    if fatal:
        _fatal.append(f"{env_name}: status {status}")
    assert status == 0 and not fatal, (status, text)
    print(env_name, recs[-1])
    bad = pm.check_records(cs, recs, env_name, "gpu", num_cus)
    assert bad == [], "\n".join(bad[:40])
    return recs


def test_gpu_matrix_default(num_cus):
    recs = _run("default", num_cus)
    seen = {p for r in recs for p in r.get("paths", ())}
    assert {"FRAME", "FRAME_RESV", "SEPARATE", "PREP", "PSY4", "QUANT_PAIR", "QUANT_PERSISTENT", "QUANT_FAST", "RESV_STREAM_HELPERS", "FIXUP_SINGLE", "FIXUP_COOP", "SMALL_CALL"} <= seen
    assert ("RESV_STREAM_NOHELPERS" in seen) == (pm.RESV_SHAPES["nohelpers"][0] > num_cus)
    # the material (the oracle's bytes alone)
    cs = pm.cases()
    joint = sideinfo.census([st[4] for c in cs if c["kind"] == "joint" for st in pm.case_streams(c)])
    for fam in pm.TWO_CHANNEL:
        cen = sideinfo.census([st[4] for c in cs if c["kind"] == "stereo" and c["family"] == fam for st in pm.case_streams(c)])
        assert pm.census_ok(fam, cen, joint if fam == "mpeg1" else None) == [], fam


def test_gpu_matrix_persistent_forced(num_cus):
    """LAMEJS_HIP_PAIR_MAX_FRAMES=0: every two-channel batch through g_quant and tail_help -- every two-channel configuration, joint,
    protect, Float32 interleaved with gains, at every shape >= 2."""
    recs = _run("pair0", num_cus)
    two = [r for r in recs if r.get("kind") in pm.TWO_OUT and "paths" in r]
    assert two and all("QUANT_PERSISTENT" in r["paths"] for r in two if "SEPARATE" in r["paths"])
    assert {r["frames"] for r in two if "QUANT_PERSISTENT" in r["paths"]} >= set(pm.SHAPES) - {1}


def test_gpu_matrix_separate_forced(num_cus):
    recs = _run("noframe", num_cus)
    assert not any({"FRAME", "FRAME_RESV"} & set(r.get("paths", ())) for r in recs)


def test_gpu_matrix_both_forced(num_cus):
    recs = _run("both", num_cus)
    assert not any({"FRAME", "FRAME_RESV", "QUANT_PAIR"} & set(r.get("paths", ())) for r in recs)


def _fast_batches(recs):
    return [r for r in recs if r.get("kind", "").startswith("fast_") and "SEPARATE" in r.get("paths", ()) and not r["kind"].startswith("fast_resv")]


def test_gpu_matrix_fast_forced_off(num_cus):
    """LAMEJS_HIP_NO_FAST_QUANT=1: the quality-7 cases at every shape through the general kernels, which read the same switches -- the same bytes."""
    recs = _run("nofast", num_cus)
    fast = _fast_batches(recs)
    assert fast and not any("QUANT_FAST" in r.get("paths", ()) for r in recs) and all(set(r["paths"]) & {"QUANT_PAIR", "QUANT_PERSISTENT"} for r in fast)
    assert {r["frames"] for r in fast if r["kind"] in pm.FAST_TWO_OUT} >= set(pm.SHAPES) - {1}


def test_gpu_matrix_one_workgroup(num_cus):
    """LAMEJS_HIP_QUANT_GRID_MAX=1, LAMEJS_HIP_PAIR_MAX_FRAMES=0 (the last child): one workgroup per g_quant_fast / g_quant launch, with more frames than
    pairs and than waves in it (path_matrix_cases.check_one_workgroup, part of the records' check), every form of g_quant_fast, zero mismatches."""
    recs = _run("grid1", num_cus, GRID1_CASES)
    one = [r["launch"] for r in recs if r.get("launch") and r["launch"]["kernel"] in ("fast", "persistent")]
    assert one and all(l["wg"] == 1 and l["waves"] == 8 for l in one) and not any(r["launch"]["kernel"] == "pair" for r in recs if r.get("launch"))
    assert {(l["pair"], l["skip"]) for l in one if l["kernel"] == "fast"} == {(1, 1), (1, 0), (0, 1), (0, 0)}
    assert max(l["nfs"] for l in one if l["kernel"] == "fast" and l["pair"]) == 151 and {l["skip"] for l in one if l["kernel"] == "persistent"} == {0, 1}
