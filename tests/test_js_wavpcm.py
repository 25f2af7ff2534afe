"""encodePcm, encodeBatch(..., { format }) and WavHeader.readFormat of the JavaScript drop-in beside the live unmodified reference fed
Float32Array.from(mapped values) (tests/js_wavpcm_check.js): on the host simulation, and -- marked gpu -- on the GPU."""
import pytest

from conftest import ROOT
from libs import ADDON, HOSTSIM_SO, NODE, run_js_check

NEEDS = pytest.mark.skipif(NODE is None or not ADDON.exists() or not (ROOT / "oracle" / "_ref" / "lame.all.js").exists(), reason="node / addon / reference bundle not available")


def check(res):
    assert res["mismatches"] == 0 and res["range_errors"] == 4 and res["type_errors"] == 1, res
    assert res["headers_ok"] == 18 and res["headers_refused"] == 8 and res["clamped"] == 1 and res["pending_range_errors"] == 2 and res["read_header_same"] == 1, res
    assert set(res["families"]) >= {"u8", "s16", "s24", "s32", "f32", "f64", "s24_resample", "pending", "batch", "refused_sample"}
    assert all(res["families"][f]["calls"] == 27 for f in ("u8", "s16", "s24", "s32", "f32", "f64")) and res["families"]["batch"]["calls"] == 18, res


@NEEDS
def test_js_wavpcm_beside_the_live_reference_hostsim():
    check(run_js_check("js_wavpcm_check.js", 20301, lib=HOSTSIM_SO, timeout=300))


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_gpu_js_wavpcm_beside_the_live_reference():
    check(run_js_check("js_wavpcm_check.js", 90431, timeout=300))
