"""The sample types a WAV file stores (LHIP_PCM_U8 .. LHIP_PCM_F64) -- CPU tier: the kernel body of g_ingest in both simulations.  Reference
bytes (the unmodified reference's goldens for Float32Array input, reached exactly from 24-bit, 32-bit and normalised input; the oracle for
8-bit input), the conversions bit for bit against numpy, the shapes where the kernel can go wrong, refusals, and the bounds of every load and
store under AddressSanitizer in a stand-alone program."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pcmformats_cases as pc
import wavpcm_cases as wc
from conftest import ROOT
from libs import HOSTSIM_SO, run_check, sim, wavesim  # noqa: F401
from wavpcm_cases import F32N, F64, F64N, INTER, S24, S32, U8


@pytest.fixture(scope="module")
def G():
    return pc.golden_floatpcm()


# ---- 1. reference bytes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", wc.FRAC_TYPES, ids=lambda t: wc.NAMES[t])
def test_hostsim_frac_goldens(sim, G, typ):
    """All 11 `frac` cases, each with its own call pattern, interleaved; the first five planar as well; through the host entry (calls this small are
    converted by the host) and through the simulation's device entry (the kernel body)."""
    assert wc.run_goldens(sim, G, "frac", typ) == (11, 32)


@pytest.mark.parametrize("typ", wc.HOT_TYPES, ids=lambda t: wc.NAMES[t])
def test_hostsim_hot_goldens(sim, G, typ):
    assert wc.run_goldens(sim, G, "hot", typ) == (11, 32)


@pytest.mark.parametrize("typ", wc.FRAC_TYPES, ids=lambda t: wc.NAMES[t])
def test_wavesim_frac_goldens(wavesim, G, typ):
    assert wc.run_goldens(wavesim, G, "frac", typ, entries=("device",)) == (11, 16)


@pytest.mark.parametrize("typ", wc.HOT_TYPES, ids=lambda t: wc.NAMES[t])
def test_wavesim_hot_goldens(wavesim, G, typ):
    assert wc.run_goldens(wavesim, G, "hot", typ, entries=("device",)) == (11, 16)


def test_u8_every_family_configuration(sim, wavesim):
    assert wc.u8_family_check(sim, 801) == len(pc.FAMILY_CONFIGS) == 14
    assert wc.u8_family_check(wavesim, 802, max_frames=3) == 14


# ---- 2. exact conversion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("libname", ["sim", "wavesim"])
def test_exact_conversion(libname, request):
    assert wc.exact_conversion_check(request.getfixturevalue(libname)) == 9


# ---- 3. shapes ----------------------------------------------------------------------------------------------------------------------------
def test_shapes_wavesim(wavesim):
    assert wc.shapes_check(wavesim) == 16 * 9 * 3 + 4 * 3 * 3


def test_shapes_hostsim(sim):
    assert wc.shapes_check(sim) == 16 * 9 * 3 + 4 * 3 * 3


@pytest.mark.parametrize("libname", ["sim", "wavesim"])
def test_six_streams_one_batch(libname, request):
    lib = request.getfixturevalue(libname)
    assert wc.six_streams_batch(lib) == 2
    assert wc.six_streams_batch(lib, downmix=True) == 2


# ---- 4. paths (the host side's decisions are the simulations' too) ---------------------------------------------------------------------------
@pytest.mark.parametrize("env,expect", [({}, [0, 0, 0, 0, 0]), ({"LAMEJS_HIP_NO_SMALL_CALLS": "1"}, [1, 1, 1, 0, 1]), ({"LAMEJS_HIP_HOST_CHUNK_FRAMES": "4", "LAMEJS_HIP_TRACE_CHUNKS": "1", "WAVPCM_EXPECT_UNITS": "5"}, [1, 0, 1, 0, 1])],
                         ids=["small", "no_small_calls", "chunked"])
def test_host_paths_hostsim(env, expect, monkeypatch):
    """A 20-frame host call: converted by the host where it is a small call, by g_ingest on the general path and, cut into units, on the chunked path; a
    one-frame call stays small; an Int16 call never shows the bit; the type changes from call to call."""
    monkeypatch.setenv("WAVPCM_EXPECT_INGEST", str(expect))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert run_check([sys.executable, ROOT / "tests" / "wavpcm_cases.py", "--host-paths"], lib=HOSTSIM_SO)["calls"] == 5


def test_path_bit_and_constants_are_mirrored():
    import re
    import lamejs_amd
    hdr = (ROOT / "include" / "lamejs_hip.h").read_text()
    assert re.search(r"#define LHIP_PATH_INGEST \(1u << 14\)", hdr)
    assert lamejs_amd.PATH_BITS == lamejs_amd.PATH_NAMES + ("OUT_CRC", "INGEST") and lamejs_amd.PATH_BITS.index("INGEST") == 14
    for name, val in (("U8", 4), ("S24", 8), ("S32", 12), ("F32N", 16), ("F64N", 20), ("F64", 24)):
        assert re.search(rf"#define LHIP_PCM_{name}\s+{val}\b", hdr) and getattr(lamejs_amd, f"PCM_{name}") == val


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("libname", ["sim", "wavesim"])
def test_refusals(libname, request, G):
    lib = request.getfixturevalue(libname)
    case = next(c for c in G if c["kind"] == "frac" and c["name"] == "m1_128_stereo")
    enc = pc.make_encoder(lib, case)
    a = np.zeros(4 * 1152, np.uint8)
    out = np.empty(8192, np.uint8)
    for fmt in (5, 7, 9, 11, 13, 28, 30, 32, 64, -1, 1 << 20):          # (a type that is not defined; until now `format & 1` read such a call as Int16)
        assert lib.lhip_encode_pcm(enc._h, fmt, a.ctypes.data, a.ctypes.data, 100, out.ctypes.data, len(out)) == -4, fmt
        assert b"unknown sample format" in lib.lhip_last_error()
    # the device entry: a misaligned pointer of a 4- or 8-byte type
    H, op, cp, wr = (ctypes.c_void_p * 1)(enc._h), (ctypes.c_void_p * 1)(out.ctypes.data), (ctypes.c_size_t * 1)(len(out)), (ctypes.c_int64 * 1)()
    ns = (ctypes.c_size_t * 1)(100)
    base = a.ctypes.data + (-a.ctypes.data) % 8
    for typ, off in ((S32, 2), (F32N, 1), (F64, 4), (F64N, 4)):
        for lp, rp in ((base + off, base), (base, base + off)):
            state = enc.state_get()
            rc = lib.lhip_encode_batch_device_pcm(H, 1, typ, (ctypes.c_void_p * 1)(lp), (ctypes.c_void_p * 1)(rp), ns, op, cp, wr, 1)
            assert rc == -4 and wr[0] == -4 and b"not a multiple" in lib.lhip_last_error(), (typ, off)
            assert enc.state_get() == state
    assert lib.lhip_encode_batch_device_pcm(H, 1, S24, (ctypes.c_void_p * 1)(base + 1), (ctypes.c_void_p * 1)(base + 2), ns, op, cp, wr, 1) == 0          # S24 lies anywhere
    enc.close()
    # a float host call with a bad sample: -4, the text names stream, channel, index and value, nothing is consumed -- the good call that follows gives a fresh stream's first bytes
    L, R = wc.case_elements(case, F64N)
    for typ, (l, r) in ((F64N, (L, R)), (F32N, wc.case_elements(case, F32N)), (F64, wc.case_elements(case, F64))):
        for inter in (True, False):
            enc, fresh = pc.make_encoder(lib, case), pc.make_encoder(lib, case)
            bl, br = l[:2304].copy(), r[:2304].copy()
            br[1234] = np.nan if typ != F64N else 4.0000001
            assert wc.encode_raw(lib, enc, typ, bl, br, inter, strict=False) == -4
            msg = lib.lhip_last_error().decode()
            assert "stream 0" in msg and "channel 1" in msg and "index 1234" in msg and ("nan" in msg.lower() or "4" in msg), msg
            assert wc.encode_raw(lib, enc, typ, l[:2304], r[:2304], inter) == wc.encode_raw(lib, fresh, typ, l[:2304], r[:2304], inter) != b""
            enc.close()
            fresh.close()


def test_python_mirror(sim, G):
    import lamejs_amd
    case = next(c for c in G if c["kind"] == "frac" and c["name"] == "m1_128_stereo")
    L, R = wc.case_elements(case, S24)
    enc = pc.make_encoder(sim, case)
    parts = [enc.encode_pcm(wc.pack(S24, wc.interleave(L[p:p + 1152], R[p:p + 1152])), lamejs_amd.PCM_S24) for p in range(0, len(L), 1152)]
    from golden_cases import check_stream
    check_stream(case, parts, enc.flush())
    enc.close()
    enc = pc.make_encoder(sim, case)
    parts = [enc.encode_pcm(np.frombuffer(wc.pack(S24, L[p:p + 1152]) + wc.pack(S24, R[p:p + 1152]), np.uint8), lamejs_amd.PCM_S24, interleaved=False) for p in range(0, len(L), 1152)]
    check_stream(case, parts, enc.flush())
    enc.close()
    a, b = pc.make_encoder(sim, case), pc.make_encoder(sim, case)
    res = lamejs_amd.encode_streams([a, b], [wc.pack(S24, wc.interleave(L, R)), wc.pack(S24, wc.interleave(L[:5000], R[:5000]))], interleaved=True, fmt=lamejs_amd.PCM_S24)
    c = pc.make_encoder(sim, case)
    res2 = lamejs_amd.encode_streams([c], [wc.pack(S24, L[:5000])], [wc.pack(S24, R[:5000])], fmt=lamejs_amd.PCM_S24)
    assert len(res[0]) == sum(case["call_bytes"]) + case["flush_len"] and res[1] == res2[0]
    with pytest.raises(lamejs_amd.LhipError, match="index 2"):
        c.encode_pcm(wc.pack(F64N, [0.0, 0.0, 0.0, 0.0, 0.0, np.inf]), lamejs_amd.PCM_F64N)
    with pytest.raises(ValueError):
        c.encode_pcm(b"\0" * 7, lamejs_amd.PCM_S24)
    with pytest.raises(ValueError):          # raw PCM is bytes: an array of another dtype is refused, not cast value by value
        lamejs_amd.encode_streams([c], [np.zeros(1152, np.int16)], interleaved=True, fmt=lamejs_amd.PCM_S16)
    with pytest.raises(ValueError):
        c.encode_pcm(np.zeros(12, np.int16), lamejs_amd.PCM_S24)
    for e in (a, b, c):
        e.close()


# ---- 6. bounds: a stand-alone program under AddressSanitizer, both simulations ------------------------------------------------------------------
@pytest.mark.parametrize("wave", [False, True], ids=["one_lane", "wave"])
def test_bounds_under_asan(tmp_path, wave):
    """tests/tools/wavpcm_bounds.c with lhip_api.cpp, -fsanitize=address, the flags of tests/hostsim/Makefile: lhip_debug_ingest and lhip_encode_pcm
    on heap buffers that end with the input and are poisoned in front of it, for the shapes of test 3.  Nothing goes through Python, nothing is preloaded."""
    mk = (ROOT / "tests" / "hostsim" / "Makefile").read_text()
    import re
    flags = re.search(r"^CXXFLAGS = (.*)$", mk, flags=re.M).group(1).split()
    flags = [f for f in flags if f not in ("-shared", "-fPIC", "-O2")]
    exe = tmp_path / "wavpcm_bounds"
    blob = tmp_path / "t.bin"
    import lamejs_amd
    blob.write_bytes(lamejs_amd.tables_blob(2, 44100, 128))
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-fsanitize=address", "-static-libasan", *flags] + (["-DLHIP_WAVESIM"] if wave else []) + \
          ["-I", str(ROOT / "include"), "-x", "c++", str(ROOT / "tests" / "tools" / "wavpcm_bounds.c"), str(ROOT / "lamejs_amd" / "csrc" / "lhip_api.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=900)          # (the sanitizer's runtime is linked statically: the environment is the inherited one)
    assert r.returncode == 0 and "wavpcm_bounds OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
