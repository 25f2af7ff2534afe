"""{ fractionalResample } (extension) on the GPU: every golden case of the unmodified reference through the C ABI of the HIP library, the
batch over all 49 configurations, the refused calls, and lamejs_amd/js beside the live reference under Node.  Reads tests/golden/ and
oracle/_ref/ only."""
import json
import os
import shutil
import subprocess

import pytest

import fracresample_cases as fc
from conftest import ROOT

NODE = shutil.which("node")
ADDON = ROOT / "lamejs_amd" / "js" / "addon" / "lhip_napi.node"


@pytest.fixture(scope="module")
def lib():
    import lamejs_amd
    lib = lamejs_amd.load_library()
    assert lib.lhip_device_count() > 0 and b"HOST SIMULATION" not in lib.lhip_version()
    return lib


@pytest.mark.gpu
def test_gpu_every_golden_case(lib):
    """Each encodeBuffer() byte-equal; flush frame count, each frame's length and header equal; every flush frame the reference made of
    finite samples md5-equal, every other one with all-zero main data; the calls the reference does not consume whole return -4 with the
    limit in the text and leave the stream untouched (the later calls give the bytes of a reference run without them).  No case is skipped."""
    G = fc.golden_frac()
    ran = {}
    for case in G["cases"]:
        fc.run_case(lib, case)
        ran[case["kind"]] = ran.get(case["kind"], 0) + 1
    assert ran == {"calls576": 49, "calls1152": 23, "odd": 12, "badcall": G["ratios"]}


@pytest.mark.gpu
def test_gpu_batch_over_all_49_configurations(lib):
    """lhip_encode_batch over one stream of each of the 49 configurations at once, 12 rounds of 576 samples == the per-stream results."""
    assert fc.batch_all_configurations(lib, fc.golden_frac()) >= 1


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_gpu_js_beside_the_live_reference():
    """lamejs_amd/js with { fractionalResample: true } beside the live unmodified reference on fresh pseudo-random PCM: 8 triples x 20 calls of
    576 samples, encodeBuffer() bytes equal call by call, the flush by the clean / not-clean rule (flags from the live reference)."""
    r = subprocess.run([NODE, str(ROOT / "tests" / "js_fracresample_check.js")], capture_output=True, text=True, env=dict(os.environ))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["triples"] == 8 and res["calls"] == 8 * 20 and res["mismatches"] == 0 and res["clean_flush_frames"] >= 1 and res["refused_long_calls"] == 8
