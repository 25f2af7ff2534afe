"""The sample types a WAV file stores (LHIP_PCM_U8 .. LHIP_PCM_F64) on the GPU: the kernel g_ingest.  The same bodies the CPU tier runs on the
simulations (tests/wavpcm_cases.py): reference bytes, exact conversion, the shapes where the kernel can go wrong, the launch paths, refusals.
Checks that hold torch tensors run in a process of their own (torch initialises the GPU first, then the library is loaded)."""
import ctypes
import sys

import numpy as np
import pytest

import pcmformats_cases as pc
import wavpcm_cases as wc
from conftest import ROOT
from libs import lib, run_check  # noqa: F401
from wavpcm_cases import F32N, F64, F64N, S24, S32, U8

CASES = ROOT / "tests" / "wavpcm_cases.py"


# ---- 1. reference bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("typ", wc.FRAC_TYPES, ids=lambda t: wc.NAMES[t])
def test_gpu_frac_goldens_device_entry(typ):
    """All 11 `frac` cases interleaved and the first five planar, every call a device-pointer call over torch.uint8 tensors: g_ingest in front of
    g_frame, the separate kernels, both resamplers, the reservoir."""
    assert run_check([sys.executable, CASES, "--goldens-device", "frac", wc.NAMES[typ]], timeout=300)["runs"] == 16


@pytest.mark.gpu
@pytest.mark.parametrize("typ", wc.HOT_TYPES, ids=lambda t: wc.NAMES[t])
def test_gpu_hot_goldens_device_entry(typ):
    assert run_check([sys.executable, CASES, "--goldens-device", "hot", wc.NAMES[typ]], timeout=300)["runs"] == 16


@pytest.mark.gpu
def test_gpu_goldens_host_entry(lib):
    """The host entry (these calls are small calls: the host converts while it fills the pinned block): every case of both kinds in every type."""
    G = pc.golden_floatpcm()
    for typ in wc.FRAC_TYPES:
        assert wc.run_goldens(lib, G, "frac", typ, entries=("host",)) == (11, 16)
    for typ in wc.HOT_TYPES:
        assert wc.run_goldens(lib, G, "hot", typ, entries=("host",)) == (11, 16)


@pytest.mark.gpu
def test_gpu_u8_every_family_configuration(lib):
    assert wc.u8_family_check(lib, 801, entries=("host",)) == 14
    assert run_check([sys.executable, CASES, "--u8-device"], timeout=300)["configs"] == 14


# ---- 2. exact conversion, 3. shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_exact_conversion(lib):
    assert wc.exact_conversion_check(lib) == 9


@pytest.mark.gpu
def test_gpu_shapes(lib):
    assert wc.shapes_check(lib) == 16 * 9 * 3 + 4 * 3 * 3


@pytest.mark.gpu
def test_gpu_six_streams_one_batch():
    """Six streams of {0, 1, 1152, 1153, 2305, 777} samples in one device batch, S24, each starting where the one before it ended in one
    torch.uint8 tensor; then the same over downmix streams."""
    assert run_check([sys.executable, CASES, "--six-streams"], timeout=300)["runs"] == 2


# ---- 4. paths ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_device_paths():
    assert run_check([sys.executable, CASES, "--device-paths"], timeout=300)["batches"] == 12


@pytest.mark.gpu
@pytest.mark.parametrize("env,expect", [({}, [0, 0, 0, 0, 0]), ({"LAMEJS_HIP_NO_SMALL_CALLS": "1"}, [1, 1, 1, 0, 1]), ({"LAMEJS_HIP_HOST_CHUNK_FRAMES": "4", "LAMEJS_HIP_TRACE_CHUNKS": "1", "WAVPCM_EXPECT_UNITS": "5"}, [1, 0, 1, 0, 1])],
                         ids=["small", "no_small_calls", "chunked"])
def test_gpu_host_paths(env, expect, monkeypatch):
    monkeypatch.setenv("WAVPCM_EXPECT_INGEST", str(expect))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert run_check([sys.executable, CASES, "--host-paths"], timeout=300)["calls"] == 5


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_refusals(lib):
    """An undefined type; a float host call with a bad sample consumes nothing and the good call behind it gives a fresh stream's first bytes.
    (The misaligned device pointer: tests/wavpcm_cases.py device_paths_check, beside the tensors it needs.)"""
    G = pc.golden_floatpcm()
    case = next(c for c in G if c["kind"] == "frac" and c["name"] == "m1_128_stereo")
    enc = pc.make_encoder(lib, case)
    a, out = np.zeros(4 * 1152, np.uint8), np.empty(8192, np.uint8)
    for fmt in (5, 7, 9, 13, 28, 32, -1):
        assert lib.lhip_encode_pcm(enc._h, fmt, a.ctypes.data, a.ctypes.data, 100, out.ctypes.data, len(out)) == -4 and b"unknown sample format" in lib.lhip_last_error()
    enc.close()
    for typ in (F32N, F64N, F64):
        l, r = wc.case_elements(case, typ)
        for inter in (True, False):
            enc, fresh = pc.make_encoder(lib, case), pc.make_encoder(lib, case)
            bl, br = l[:2304].copy(), r[:2304].copy()
            bl[77] = np.inf
            assert wc.encode_raw(lib, enc, typ, bl, br, inter, strict=False) == -4
            msg = lib.lhip_last_error().decode()
            assert "stream 0" in msg and "channel 0" in msg and "index 77" in msg and "inf" in msg.lower(), msg
            assert wc.encode_raw(lib, enc, typ, l[:2304], r[:2304], inter) == wc.encode_raw(lib, fresh, typ, l[:2304], r[:2304], inter) != b""
            enc.close()
            fresh.close()
