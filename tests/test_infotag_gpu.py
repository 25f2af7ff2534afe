"""The Info/LAME tag frame on the GPU: the CRC kernel against a bitwise CRC, the goldens of the unmodified reference, batches whose bytes stay
in HBM (tagged beside untagged streams; the bit reservoir, whose byte counts only the device knows; a long stream over several workgroups; a
device-pointer call), the host path of small calls, and the one-frame batch without the frame kernel.  Yardsticks: tests/infotag_cases.py.
Reads tests/golden/ only; the children get time limits."""
import ctypes
import sys

import numpy as np
import pytest

import infotag_cases as ic
import pcm
from conftest import ROOT
from libs import lib, run_check  # noqa: F401

WORKER = ROOT / "tests" / "tools" / "infotag_worker.py"


@pytest.fixture(scope="module")
def G():
    G = ic.goldens()
    assert len(G) == 22
    return G


@pytest.mark.gpu
def test_gpu_crc_kernel_against_the_bitwise_crc(lib):
    """g_out_crc + g_out_crc_fold over seeded random buffers: every length of the table at every misalignment."""
    assert ic.check_crc_table(lib, 20292) == 12 * 16


@pytest.mark.gpu
def test_gpu_goldens_one_encoder_each(lib, G):
    import lamejs_amd
    seen = set()
    for c in G:
        ic.run_golden_case(lib, c)
        seen |= set(lamejs_amd.last_batch_paths(lib))
    assert "SMALL_CALL" in seen and "OUT_CRC" not in seen          # calls this small: the host's CRC over the pinned mirror, no launch gained


@pytest.mark.gpu
def test_gpu_mixed_batch_host_path(lib):
    assert "OUT_CRC" not in ic.mixed_batch_check(lib)


@pytest.mark.gpu
def test_gpu_mixed_batch_device_path(monkeypatch):
    """The same batch with the small-call path switched off: the streams' bytes stay in HBM, at odd addresses and with unequal lengths."""
    monkeypatch.setenv("LAMEJS_HIP_NO_SMALL_CALLS", "1")
    res = run_check([sys.executable, WORKER, "batch"], timeout=120)
    assert "OUT_CRC" in res["paths"] and "SMALL_CALL" not in res["paths"], res


@pytest.mark.gpu
def test_gpu_reservoir_batch_device_path(monkeypatch):
    monkeypatch.setenv("LAMEJS_HIP_NO_SMALL_CALLS", "1")
    res = run_check([sys.executable, WORKER, "resv_batch"], timeout=120)
    assert "OUT_CRC" in res["paths"] and "RESV_STREAM_HELPERS" in res["paths"], res


@pytest.mark.gpu
def test_gpu_reservoir_batch_host_path(lib):
    assert "OUT_CRC" not in ic.resv_batch_check(lib)


@pytest.mark.gpu
def test_gpu_long_stream_in_one_call_and_in_frame_sized_calls(lib):
    one_call, small_calls = ic.long_stream_check(lib, 2000)
    assert "OUT_CRC" in one_call and "SMALL_CALL" not in one_call, one_call
    assert "OUT_CRC" not in small_calls and "SMALL_CALL" in small_calls and "FRAME" in small_calls, small_calls


@pytest.mark.gpu
def test_gpu_device_pointer_call(lib):
    """lhip_encode_batch_device on a tagged stream (sync = 0): the placeholder arrives in front of the audio in the caller's device buffer, the call
    fetches the CRC -- so it has synchronised when it returns -- and the totals are those of the bytes."""
    import lamejs_amd
    from protection_cases import frames as walk_frames
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    n = 50 * 1152 + 3
    L, R = pcm.bursts(n, 2, seed=321)
    enc = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, info_tag=True, device=0)
    cap = int(lib.lhip_max_output_bytes(enc._h, n))
    bufs = []
    try:
        for size in (2 * n, 2 * n, cap):
            p = ctypes.c_void_p()
            assert hip.hipMalloc(ctypes.byref(p), size) == 0
            bufs.append(p)
        dl, dr, do = bufs
        assert hip.hipMemcpy(dl, L.ctypes.data, 2 * n, 1) == 0 and hip.hipMemcpy(dr, R.ctypes.data, 2 * n, 1) == 0
        H, a_l, a_r, a_o = (ctypes.c_void_p * 1)(enc._h), (ctypes.c_void_p * 1)(dl.value), (ctypes.c_void_p * 1)(dr.value), (ctypes.c_void_p * 1)(do.value)
        a_n, a_c, wr = (ctypes.c_size_t * 1)(n), (ctypes.c_size_t * 1)(cap), (ctypes.c_int64 * 1)()
        assert lib.lhip_encode_batch_device(H, 1, a_l, a_r, a_n, a_o, a_c, wr, 0) == 0, lib.lhip_last_error()
        assert "OUT_CRC" in lamejs_amd.last_batch_paths(lib)
        si = enc.stream_info()                                   # (valid without another synchronisation: the call fetched the CRC)
        host = np.empty(int(wr[0]), dtype=np.uint8)
        assert hip.hipMemcpy(host.ctypes.data, do, int(wr[0]), 2) == 0
        body = host.tobytes()
        nt = si["tag_bytes"]
        lone = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib)
        want = lone.encodeBuffer(L, R)
        lone.close()
        assert body[nt:] == want and si["audio_bytes"] == len(want) and si["music_crc"] == ic.crc16(want) and si["frames"] == len(walk_frames(want)) == 49
        assert ic.header_fields(int.from_bytes(body[:4], "big"))["frame_bytes"] == nt and body[4:nt] == bytes(nt - 4)
    finally:
        enc.close()
        for p in bufs:
            hip.hipFree(p)


@pytest.mark.gpu
def test_gpu_one_frame_batches_without_the_frame_kernel(monkeypatch):
    """LAMEJS_HIP_NO_FRAME_KERNEL=1: the goldens' frame-sized calls through the separate kernels (g_bits, with the reservoir g_resv_stream)."""
    monkeypatch.setenv("LAMEJS_HIP_NO_FRAME_KERNEL", "1")
    res = run_check([sys.executable, WORKER, "goldens", "stereo_44100_128", "resv_stereo_128", "protect_joint_resv_128", "mono_8000_24_mpeg25"], timeout=120)
    assert res["cases"] == 4 and "FRAME" not in res["paths"] and "FRAME_RESV" not in res["paths"] and "SEPARATE" in res["paths"], res
