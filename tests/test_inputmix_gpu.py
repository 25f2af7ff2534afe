"""Input gains (scale, scale_left, scale_right) and the stereo-to-mono downmix on the GPU: the goldens of the unmodified reference, the
one-frame program against the batch kernels, a batch of unequal streams, the device-pointer entry, a random family against the oracle and
the JavaScript wrapper beside the live reference.  Streams of at most 12 frames.  Reads tests/golden/ and oracle/_ref/ only."""
import sys

import numpy as np
import pytest

import inputmix_cases as mc
import pcmformats_cases as pc
from conftest import ROOT
from libs import ADDON, NODE, lib, run_check, run_js_check  # noqa: F401
from pcmformats_cases import F32, INTER, S16


@pytest.mark.gpu
def test_gpu_every_golden(lib):
    """Every call and the flush of every golden, planar and interleaved alternating from call to call (both phases)."""
    G = mc.goldens()
    assert len(G) == 28
    for i, c in enumerate(G):
        mc.run_golden_case(lib, c, fmt_of_call=(lambda k: INTER if (k + i) % 2 else 0))
        mc.run_golden_case(lib, c, fmt_of_call=(lambda k: 0 if (k + i) % 2 else INTER))


@pytest.mark.gpu
def test_gpu_one_frame_program_equals_the_batch_kernels(lib):
    """The same stream in 1152-sample calls (g_frame) and in one whole call (g_psyA / g_poly / g_quant ...): downmix, gains, a resampling downmix,
    in all four formats."""
    G = {c["name"]: c for c in mc.goldens()}
    for name in ("downmix_f32", "gains_f32", "downmix_flip_left_double_right", "downmix_44100_32_resample_int"):
        c = G[name]
        L, R = mc.case_pcm(c)
        n = 10 * 1152
        for fmt in mc.FORMATS:
            l, r = (L[:n], R[:n]) if (fmt & F32 or c["kind"] != "f32") else (np.rint(L[:n]), np.rint(R[:n]))
            a, b = mc.make_encoder(lib, c), mc.make_encoder(lib, c)
            calls = b"".join(pc.encode_fmt(lib, a, fmt, l[1152 * k:1152 * (k + 1)], r[1152 * k:1152 * (k + 1)]) for k in range(10)) + a.flush()
            whole = pc.encode_fmt(lib, b, fmt, l, r) + b.flush()
            assert calls == whole and len(whole) > 1000, (name, fmt)       # (the smallest: 12 frames at 32 kbps, 22050 Hz)
            a.close()
            b.close()


@pytest.mark.gpu
def test_gpu_batch_of_three_unequal_streams(lib):
    """lhip_encode_batch_pcm over three downmix streams of unequal lengths == the streams one by one, in all four formats."""
    c = next(x for x in mc.goldens() if x["name"] == "downmix_f32")
    L, R = mc.case_pcm(c)
    cuts = [(0, 5 * 1152 + 7), (1000, 1000 + 1152), (2000, 2000 + 9 * 1152 - 1)]
    for fmt in mc.FORMATS:
        l, r = (L, R) if fmt & F32 else (np.rint(L), np.rint(R))
        encs, solo = [mc.make_encoder(lib, c) for _ in cuts], [mc.make_encoder(lib, c) for _ in cuts]
        got, _ = pc.batch_pcm(lib, encs, fmt, [l[a:b] for a, b in cuts], [r[a:b] for a, b in cuts])
        want = [pc.encode_fmt(lib, e, fmt, l[a:b], r[a:b]) for e, (a, b) in zip(solo, cuts)]
        assert got == want and [e.flush() for e in encs] == [e.flush() for e in solo], fmt
        for e in encs + solo:
            e.close()


@pytest.mark.gpu
def test_gpu_device_entry_zeroes_and_counts_both_source_channels():
    """In a process of its own (torch initialises the GPU before the library is loaded): inputmix_cases.device_downmix_check."""
    assert run_check([sys.executable, ROOT / "tests" / "inputmix_cases.py", "--device-downmix"], timeout=300)["device_downmix_formats"] == 4


@pytest.mark.gpu
def test_gpu_random_family_equals_the_oracle(lib):
    assert mc.family_check(lib, mc.family(20273, 10)) == 10


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node / addon not available")
def test_gpu_js_beside_the_live_reference():
    res = run_js_check("js_inputmix_check.js", 90418, timeout=300)
    assert res["calls"] == 137 and res["mismatches"] == 0 and res["type_errors"] == 2
