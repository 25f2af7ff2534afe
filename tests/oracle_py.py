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
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        for name, restype, argtypes in (("lo_create", vp, [vp, sz]), ("lo_destroy", None, [vp]), ("lo_encode", ctypes.c_long, [vp, vp, vp, sz, vp, sz]),
                                        ("lo_flush", ctypes.c_long, [vp, vp, sz]), ("lo_enable_tap", None, [vp]), ("lo_get_tap", vp, [vp]),
                                        ("lo_tap_size", sz, []), ("lo_math", None, [ctypes.c_int, vp, vp, sz]), ("lo_quant_probe", None, [vp, vp, sz, vp]),
                                        ("lo_bits_probe", ctypes.c_int, [vp, vp, sz, vp])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
    return _lib


class OracleStream:
    """One oracle encoder on a table blob -- the only driver of lo_create / lo_encode / lo_flush / lo_destroy.  Samples are converted to Int16
    here; ``right=None`` (always, for a one-channel blob) hands the left plane over twice; every call gets an output buffer of
    ``(n // 1152 + 8) * 1500 + 16384`` bytes (no frame of any configuration exceeds 1441 bytes per 1152 samples); a negative return
    raises, naming the call.  ``tap=True``: the stage taps of oracle/lo_common.h are recorded, ``tap()`` returns the last frame's."""

    def __init__(self, blob, tap=False):
        self._lib = _load()
        buf = ctypes.create_string_buffer(blob, len(blob))
        self._h = self._lib.lo_create(buf, len(blob))
        if not self._h:
            raise RuntimeError("lo_create failed")
        self._calls = 0
        if tap:
            self._lib.lo_enable_tap(self._h)

    def _out(self, what, n, call):
        out = np.empty((n // 1152 + 8) * 1500 + 16384, dtype=np.uint8)
        w = call(out.ctypes.data, len(out))
        if w < 0:
            raise RuntimeError(f"{what} (call {self._calls}): {w}")
        self._calls += 1
        return out[:w].tobytes()

    def encode(self, left, right=None) -> bytes:
        L = np.ascontiguousarray(left, dtype=np.int16)
        R = L if right is None else np.ascontiguousarray(right, dtype=np.int16)
        assert len(R) == len(L)
        return self._out("lo_encode", len(L), lambda out, cap: self._lib.lo_encode(self._h, L.ctypes.data, R.ctypes.data, len(L), out, cap))

    def flush(self) -> bytes:
        return self._out("lo_flush", 0, lambda out, cap: self._lib.lo_flush(self._h, out, cap))

    def tap(self) -> bytes:
        """The lo_tap record of the frame the last call completed (tests/stage_taps.py: TAP)."""
        return ctypes.string_at(self._lib.lo_get_tap(self._h), self._lib.lo_tap_size())

    def quant_probe(self, records, out_dtype):
        """lo_quant_probe over an array of probe records (tests/quant_probe_cases.py: REC_IN) -> array of ``out_dtype`` (REC_OUT)."""
        rec = np.ascontiguousarray(records)
        out = np.zeros(len(rec), dtype=out_dtype)
        self._lib.lo_quant_probe(self._h, rec.ctypes.data, len(rec), out.ctypes.data)
        return out

    def bits_probe(self, records, out_dtype):
        """lo_bits_probe over an array of frame records (tests/bits_probe_cases.py: rec_in) -> array of ``out_dtype`` (REC_OUT)."""
        rec = np.ascontiguousarray(records)
        out = np.zeros(len(rec), dtype=out_dtype)
        if self._lib.lo_bits_probe(self._h, rec.ctypes.data, len(rec), out.ctypes.data) != 0:
            raise RuntimeError("lo_bits_probe refused the configuration")
        return out

    def close(self):
        if self._h:
            self._lib.lo_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def oracle_calls(blob, L, R, lens, flush=True):
    """The stream cut into calls of ``lens`` samples -> (bytes per call, flush bytes; b"" without a flush)."""
    with OracleStream(blob) as o:
        parts, p = [], 0
        for n in lens:
            parts.append(o.encode(L[p:p + n], None if R is None else R[p:p + n]))
            p += n
        return parts, (o.flush() if flush else b"")


def oracle_encode(channels, samplerate, kbps, left, right=None, chunk=None, flush=True, joint=False, reservoir=False) -> bytes:
    sys.path.insert(0, str(ROOT))
    from lamejs_amd import tables_blob

    n = len(left)
    chunk = chunk or max(n, 1)
    parts, tail = oracle_calls(tables_blob(channels, samplerate, kbps, joint, reservoir), left, None if channels == 1 else right,
                               [min(chunk, n - p) for p in range(0, n, chunk)], flush)
    return b"".join(parts) + tail
