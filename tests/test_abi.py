"""The C-ABI library must load without a GPU and export every symbol include/lamejs_hip.h declares."""
import ctypes
import re

import pytest

from conftest import ROOT


def test_hip_library_exports_declared_symbols():
    import lamejs_amd
    lib = lamejs_amd.load_library()
    hdr = (ROOT / "include" / "lamejs_hip.h").read_text()
    names = set(re.findall(r"\b(lhip_[a-z_0-9]+)\s*\(", hdr))
    assert len(names) >= 12
    for n in names:
        assert hasattr(lib, n), f"missing export {n}"
    assert b"HIP gfx950" in lib.lhip_version()


def test_signature_table_matches_the_header():
    """lamejs_amd.ABI, the one ctypes declaration of the C ABI, against the prototypes of include/lamejs_hip.h: the same entries, the same
    parameter counts, and no pointer, size_t or 64-bit parameter or result declared as a C int (ctypes would truncate it)."""
    import lamejs_amd
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lamejs_hip.h").read_text(), flags=re.S)
    protos = {name: (ret, [] if args.strip() == "void" else args.split(","))
              for ret, name, args in re.findall(r"^([\w \*]+?)\b(lhip_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)}
    assert len(protos) >= 30 and set(lamejs_amd.ABI) == set(protos)
    wide = re.compile(r"\*|\b(size_t|u?int64_t)\b")
    narrow = (ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, None)
    for name, (ret, params) in protos.items():
        restype, argtypes = lamejs_amd.ABI[name]
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        assert not (wide.search(ret) and restype in narrow), (name, ret)
        for text, t in zip(params, argtypes):
            assert not (wide.search(text) and t in narrow), (name, text.strip())
            assert wide.search(text) or t is ctypes.c_int, (name, text.strip())


def test_debug_last_paths_is_exported_and_mirrored():
    """lhip_debug_last_paths: declared, exported, refuses a null pointer, reports no path before any batch; the mirror's names are the
    header's LHIP_PATH_* bits in order."""
    import lamejs_amd
    lib = lamejs_amd.load_library()
    hdr = (ROOT / "include" / "lamejs_hip.h").read_text()
    assert re.search(r"\bint\s+lhip_debug_last_paths\s*\(\s*uint32_t\s*\*", hdr) and hasattr(lib, "lhip_debug_last_paths")
    bits = re.findall(r"#define LHIP_PATH_([A-Z0-9_]+) (0x[0-9a-f]+)u", hdr)
    assert [n for n, _ in bits] == list(lamejs_amd.PATH_NAMES) and [int(v, 16) for _, v in bits] == [1 << i for i in range(len(bits))] and len(bits) == 13
    assert lib.lhip_debug_last_paths(None) < 0 and b"lhip_debug_last_paths" in lib.lhip_last_error()
    assert lamejs_amd.last_batch_paths(lib) == frozenset()


def test_no_cpu_fallback_without_device():
    """On a box without a HIP device creation must fail loudly (never silently fall back)."""
    import lamejs_amd
    lib = lamejs_amd.load_library()
    if lib.lhip_device_count() > 0:
        return
    try:
        lamejs_amd.Mp3Encoder(1, 44100, 128)
    except lamejs_amd.LhipError as e:
        assert "no HIP device" in str(e) or "failed" in str(e)
    else:
        raise AssertionError("encoder creation succeeded without a HIP device")


def test_product_does_not_reference_oracle():
    for p in list((ROOT / "lamejs_amd").rglob("*.h")) + list((ROOT / "lamejs_amd").rglob("*.cpp")) + list((ROOT / "lamejs_amd").rglob("*.py")) + list((ROOT / "lamejs_amd").rglob("*.js")):
        txt = p.read_text(errors="ignore")
        assert "oracle/" not in txt and "lame_oracle" not in txt and "oracle_py" not in txt, p


def test_configs_outside_the_envelope_fail_loudly(golden):
    """Configurations the reference would resample to an MPEG-2 rate are refused (no silent fallback)."""
    import lamejs_amd
    outside = [c for c in golden if c.get("outside_envelope")]
    assert len(outside) >= 3
    for c in outside:
        with pytest.raises(lamejs_amd.LhipError, match="resampl"):
            lamejs_amd.tables_blob(c["channels"], c.get("samplerate", 44100), c["kbps"])


def test_set_devices_argument_handling():
    """lhip_set_devices without a GPU: fails loudly (no device to allow); with one: rejects masks naming absent devices."""
    import lamejs_amd
    lib = lamejs_amd.load_library()
    n = lib.lhip_device_count()
    if n <= 0:
        assert lib.lhip_set_devices(1) < 0 and b"no HIP device" in lib.lhip_last_error()
    else:
        assert lib.lhip_set_devices(1 << 63) < 0
        assert lib.lhip_set_devices(0) == n


def test_device_code_resources(tmp_path):
    """The resource usage the design rests on, read from the shipped library's own gfx950 code object (no GPU needed): the persistent
    quantization kernel spills nothing to scratch memory, stays within 128 registers (4 waves per SIMD) and two of its workgroups fit the
    160 KB of LDS of a CU; the batch kernels of the steady-state path use no scratch either; the one-frame and the
    per-stream reservoir kernel run two waves per SIMD, fit a CU's LDS, and the one-frame kernel stays far below the scratch size that slows its launch (4.6)."""
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    objdump, readelf = f"{llvm}/llvm-objdump", f"{llvm}/llvm-readelf"
    so = ROOT / "lamejs_amd" / "lib" / "liblamejs_hip.so"
    if not (shutil.which(objdump) and shutil.which(readelf) and so.exists()):
        pytest.skip("llvm tools or the built library not present")
    shutil.copy(so, tmp_path / "l.so")
    subprocess.run([objdump, "--offloading", "l.so"], cwd=tmp_path, capture_output=True, check=True)
    co = [p for p in tmp_path.iterdir() if "amdgcn" in p.name]
    assert len(co) == 1 and "gfx950" in co[0].name, [p.name for p in tmp_path.iterdir()]
    notes = subprocess.run([readelf, "--notes", str(co[0])], capture_output=True, text=True, check=True).stdout
    kern = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        f = {k: v for k, v in re.findall(r"\.(name|private_segment_fixed_size|vgpr_count|group_segment_fixed_size):\s+(\S+)", blk)}
        kern[f["name"]] = {k: int(v) for k, v in f.items() if k != "name"}
    q = next(v for k, v in kern.items() if k.startswith("_Z7g_quantILi0"))
    assert q["private_segment_fixed_size"] == 0, q
    assert q["vgpr_count"] <= 128 and 2 * q["group_segment_fixed_size"] <= 160 * 1024, q
    fx = next(v for k, v in kern.items() if k.startswith("_Z7g_fixup"))          # the repair kernel: two workgroups per CU as well (it may spill a little)
    assert fx["vgpr_count"] <= 128 and 2 * fx["group_segment_fixed_size"] <= 160 * 1024, fx
    for name in ("g_psyA", "g_psyB", "g_poly", "g_mdct", "g_bits", "g_validate_fast", "g_scan_ath", "g_quant_pair", "g_load", "g_save"):
        ks = [v for k, v in kern.items() if re.match(rf"_Z\d+{name}(I|N|5|E)", k)]
        assert ks, name
        assert all(v["private_segment_fixed_size"] == 0 for v in ks), (name, ks)
    # the latency kernels: eight waves per workgroup on four SIMDs (g_resv_stream: two workgroups of four) are two waves per SIMD -- 256 registers; a
    # workgroup's LDS must fit a CU; past ~0.5 KB of scratch per lane a one-frame launch itself gets slower (the comment above g_frame's stage loop)
    fr = {k: v for k, v in kern.items() if k.startswith("_Z7g_frameILi0") or k.startswith("_Z7g_frameILi1")}
    assert len(fr) == 2, sorted(kern)
    rs = {k: v for k, v in kern.items() if k.startswith("_Z13g_resv_stream")}
    assert len(rs) == 1, sorted(kern)
    for k, v in {**fr, **rs}.items():
        assert v["vgpr_count"] <= 256 and v["group_segment_fixed_size"] <= 160 * 1024, (k, v)
    for k, v in fr.items():
        assert v["private_segment_fixed_size"] < 512, (k, v)
