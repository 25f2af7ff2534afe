"""{ infoTag } through the JavaScript drop-in beside the live unmodified reference's nMusicCRC, frame count, delay and padding, and a file
assembled as the documentation says and parsed (tests/js_infotag_check.js): on the host simulation, and -- marked gpu -- on the GPU."""
import pytest

from conftest import ROOT
from libs import ADDON, HOSTSIM_SO, NODE, run_js_check

NEEDS = pytest.mark.skipif(NODE is None or not ADDON.exists() or not (ROOT / "oracle" / "_ref" / "lame.all.js").exists(), reason="node / addon / reference bundle not available")
FAMILIES = {"plain", "joint", "reservoir", "batch_mixed", "pending"}


def check(res):
    assert res["mismatches"] == 0 and res["file_bad"] == 0 and res["files"] == 11 and res["refused"] == 3, res
    assert set(res["families"]) >= FAMILIES and res["calls"] > 80, res


@NEEDS
def test_js_infotag_beside_the_live_reference_hostsim():
    check(run_js_check("js_infotag_check.js", 20293, lib=HOSTSIM_SO, timeout=300))


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_gpu_js_infotag_beside_the_live_reference():
    check(run_js_check("js_infotag_check.js", 90420, timeout=300))
