"""{ protect, copyright, original, privateBit, emphasis } through the JavaScript drop-in on the GPU, beside the live unmodified reference
(tests/js_protection_check.js; the host-simulation run of the same check is in tests/test_protection_cpu.py)."""
import pytest

from libs import ADDON, NODE, run_js_check


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_gpu_js_protection_beside_the_live_reference():
    res = run_js_check("js_protection_check.js", 90419, timeout=300)
    assert res["mismatches"] == 0 and res["crc_bad"] == 0 and res["crc_frames"] > 100 and res["range_errors"] == 3
    assert set(res["families"]) >= {"protect", "flags", "everything", "batch_mixed", "pending"}
