"""{ replayGain } of the JavaScript drop-in (tests/js_replaygain_check.js) against tests/golden/golden_replaygain.json: on the host simulation, and -- marked
gpu -- on the GPU."""
import pytest

from libs import ADDON, HOSTSIM_SO, NODE, run_js_check

NEEDS = pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")


def check(res):
    assert res["mismatches"] == 0 and res["cases"] == 6 and res["exact_tenth"] >= 4, res
    assert res["cut_same"] == 3 and res["batch_same"] == 1 and res["pending_same"] == 1 and res["tag_fields"] == 2 and res["refused"] == 3, res


@NEEDS
def test_js_replaygain_hostsim():
    check(run_js_check("js_replaygain_check.js", lib=HOSTSIM_SO, timeout=300))


@pytest.mark.gpu
@NEEDS
def test_gpu_js_replaygain():
    check(run_js_check("js_replaygain_check.js", timeout=300))
