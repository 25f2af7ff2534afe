"""TEST INFRASTRUCTURE: ctypes binding of the CPU oracle (oracle/_ref/liblame_oracle.so)."""
import ctypes
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
_SO = ROOT / "oracle" / "_ref" / "liblame_oracle.so"
_lib = None


def _sources_hash() -> str:
    import hashlib
    h = hashlib.sha256()
    for f in sorted((ROOT / "oracle").glob("*.[ch]")) + [ROOT / "oracle" / "Makefile"]:
        h.update(f.name.encode() + b"\0" + f.read_bytes())
    return h.hexdigest()


def _make_current():
    """The library in oracle/_ref/ is the build of the sources that are here now -- decided by CONTENT (a hash of oracle/*.c, *.h and the
    Makefile kept beside the build), not by file times: oracle/_ref/ is untracked and can outlive the sources it was built from, with any
    time stamp.  A build of other sources is made again from scratch; otherwise `make` only confirms it."""
    stamp = _SO.parent / "sources.sha256"
    want = _sources_hash()
    fresh = _SO.exists() and stamp.exists() and stamp.read_text().strip() == want
    subprocess.run(["make", "-C", str(ROOT / "oracle")] + ([] if fresh else ["-B"]) + ["all"], check=True, capture_output=True)
    if not fresh:
        stamp.write_text(want + "\n")


def _load():
    global _lib
    if _lib is None:
        _make_current()          # before the first load: the process keeps the handle it loads
        lib = ctypes.CDLL(str(_SO))
        lib.lo_create.restype = ctypes.c_void_p
        lib.lo_create.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        lib.lo_destroy.argtypes = [ctypes.c_void_p]
        lib.lo_encode.restype = ctypes.c_long
        lib.lo_encode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        lib.lo_flush.restype = ctypes.c_long
        lib.lo_flush.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        _lib = lib
    return _lib


def oracle_encode(channels, samplerate, kbps, left, right=None, chunk=None, flush=True, joint=False, reservoir=False) -> bytes:
    sys.path.insert(0, str(ROOT))
    from lamejs_amd import tables_blob

    lib = _load()
    blob = tables_blob(channels, samplerate, kbps, joint, reservoir)
    buf = ctypes.create_string_buffer(blob, len(blob))
    h = lib.lo_create(buf, len(blob))
    if not h:
        raise RuntimeError("lo_create failed")
    L = np.ascontiguousarray(left, dtype=np.int16)
    R = L if (channels == 1 or right is None) else np.ascontiguousarray(right, dtype=np.int16)
    n = len(L)
    chunk = chunk or max(n, 1)
    cap = (n // 1152 + 8) * 1500 + 16384
    out = np.empty(cap, dtype=np.uint8)
    off = 0
    try:
        for p in range(0, n, chunk):
            m = min(chunk, n - p)
            w = lib.lo_encode(h, L[p:].ctypes.data, R[p:].ctypes.data, m, out[off:].ctypes.data, cap - off)
            if w < 0:
                raise RuntimeError(f"lo_encode {w}")
            off += w
        if flush:
            w = lib.lo_flush(h, out[off:].ctypes.data, cap - off)
            if w < 0:
                raise RuntimeError(f"lo_flush {w}")
            off += w
    finally:
        lib.lo_destroy(h)
    return out[:off].tobytes()
