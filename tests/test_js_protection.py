"""{ protect, copyright, original, privateBit, emphasis } through the JavaScript drop-in on the GPU, beside the live unmodified reference
(tests/js_protection_check.js; the host-simulation run of the same check is in tests/test_protection_cpu.py)."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
ADDON = ROOT / "lamejs_amd" / "js" / "addon" / "lhip_napi.node"


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_gpu_js_protection_beside_the_live_reference():
    r = subprocess.run([NODE, str(ROOT / "tests" / "js_protection_check.js"), "90419"], capture_output=True, text=True, env=dict(os.environ), timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mismatches"] == 0 and res["crc_bad"] == 0 and res["crc_frames"] > 100 and res["range_errors"] == 3
    assert set(res["families"]) >= {"protect", "flags", "everything", "batch_mixed", "pending"}
