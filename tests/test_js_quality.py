"""{ quality } through the JavaScript drop-in on the GPU: the goldens of the unmodified reference, encodeBatch over encoders of both qualities,
{ pendingFrames }, the RangeErrors (tests/js_quality_check.js; the host-simulation run of the same check is in tests/test_quality_cpu.py)."""
import pytest

from libs import ADDON, NODE, run_js_check


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_gpu_js_quality_against_the_goldens():
    res = run_js_check("js_quality_check.js", 90421, timeout=300)
    assert res["mismatches"] == 0 and res["goldens"] == 25 and res["range_errors"] == 6
    assert set(res["families"]) >= {"goldens", "batch_mixed", "quality8", "pending", "refusals"}
