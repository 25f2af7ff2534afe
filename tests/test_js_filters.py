"""{ outSampleRate, lowpass, lowpassWidth, highpass, highpassWidth } through the JavaScript drop-in on the GPU: the goldens of the unmodified reference,
encodeBatch over encoders of different option sets, the RangeErrors and, where the reference's sources are present, three streams beside the live
reference (tests/js_filters_check.js; the host-simulation run of the same check is in tests/test_filters_cpu.py)."""
import pytest

import filters_cases as fc
from libs import ADDON, NODE, run_js_check


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_gpu_js_filters_against_the_goldens():
    fc.check_js_result(run_js_check("js_filters_check.js", 90431, timeout=300), fc.goldens())
