"""{ fractionalResample } (extension) on the GPU: every golden case of the unmodified reference through the C ABI of the HIP library, the
batch over all 49 configurations, the refused calls, and lamejs_amd/js beside the live reference under Node.  Reads tests/golden/ and
oracle/_ref/ only."""
import pytest

import fracresample_cases as fc
from libs import ADDON, NODE, lib, run_js_check  # noqa: F401


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
    res = run_js_check("js_fracresample_check.js")
    assert res["triples"] == 8 and res["calls"] == 8 * 20 and res["mismatches"] == 0 and res["clean_flush_frames"] >= 1 and res["refused_long_calls"] == 8
