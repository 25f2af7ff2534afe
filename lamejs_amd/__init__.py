"""lamejs_amd -- MI355X-native MP3 frame-encode path behind the lamejs ``Mp3Encoder`` API.

Python mirror of the reference's operator interface for this path (``src/js/index.js:66-136``):
``Mp3Encoder(channels, samplerate, kbps).encodeBuffer(left[, right]) -> bytes`` and ``.flush()``.
It is a thin ctypes binding over the C ABI of ``include/lamejs_hip.h`` (``lib/liblamejs_hip.so``,
hand-written HIP for gfx950).  There is no CPU fallback: if the shared library is missing or no
HIP device is visible, construction raises.

The production host is JavaScript (``lamejs_amd/js/index.js`` + N-API addon); this mirror exists
so that the pytest suite and ``bench.py`` can drive exactly the same C ABI.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
_LIB_PATH = _PKG / "lib" / "liblamejs_hip.so"
_TABLE_DIR = _PKG / "tables"

__all__ = ["Mp3Encoder", "load_library", "tables_blob", "LhipError", "encode_streams", "PCM_S16", "PCM_F32", "PCM_INTERLEAVED", "PATH_NAMES", "PATH_NAMES_ALL", "PATH_BITS", "PATH_BITS_ALL", "PATH_BITS_QUALITY", "last_batch_paths", "StreamInfo",
           "PCM_U8", "PCM_S24", "PCM_S32", "PCM_F32N", "PCM_F64N", "PCM_F64", "PCM_BYTES"]

# launch paths of a batch (include/lamejs_hip.h: LHIP_PATH_*), in bit order
PATH_NAMES = ("FRAME", "FRAME_RESV", "SEPARATE", "PREP", "PSY4", "QUANT_PAIR", "QUANT_PERSISTENT", "RESV_STREAM_HELPERS", "RESV_STREAM_NOHELPERS",
              "RESV_FLUSH", "FIXUP_SINGLE", "FIXUP_COOP", "SMALL_CALL")
# every bit in bit order: the ones above, then those the header states as shifts -- OUT_CRC (the music CRC of ``info_tag`` streams came from the kernel
# g_out_crc, not from the host) and INGEST (samples of a WAV sample type were turned into Float32 planes by the kernel g_ingest, not by the host)
PATH_BITS = PATH_NAMES + ("OUT_CRC", "INGEST")
PATH_NAMES_ALL = PATH_BITS[:14]      # (the names up to OUT_CRC, kept for callers that index it)
# ... and GAIN: the batch held ``replay_gain`` streams and the kernels g_gain_stage / g_gain ran behind it.  (A tuple of its own: PATH_BITS is held at its
# fifteen names by the suite, as PATH_NAMES is at thirteen.)
PATH_BITS_ALL = PATH_BITS + ("GAIN",)
# ... and QUANT_FAST: the batch's quantization was the bin-search-only kernel g_quant_fast of ``quality=7`` streams.  (Again a tuple of its own: the suite holds
# PATH_BITS_ALL at its sixteen names.)  This is the tuple ``last_batch_paths`` decodes with.
PATH_BITS_QUALITY = PATH_BITS_ALL + ("QUANT_FAST",)


def last_batch_paths(lib=None) -> frozenset:
    """Names of the launch paths the most recent batch on this thread took (``lhip_debug_last_paths``; a debug/test hook)."""
    lib = lib or load_library()
    m = ctypes.c_uint32()
    rc = lib.lhip_debug_last_paths(ctypes.byref(m))
    if rc != 0:
        raise LhipError(f"lhip_debug_last_paths failed ({rc}): {lib.lhip_last_error().decode()}")
    if m.value >> len(PATH_BITS_QUALITY):
        raise LhipError(f"lhip_debug_last_paths: unknown bits in {m.value:#x}")
    return frozenset(n for i, n in enumerate(PATH_BITS_QUALITY) if m.value >> i & 1)


# sample formats of the *_pcm entries (include/lamejs_hip.h: LHIP_PCM_*): a sample type, optionally or-ed with PCM_INTERLEAVED
PCM_S16, PCM_F32, PCM_INTERLEAVED = 0, 1, 2
# ... and the sample types a WAV file stores: 8-bit unsigned, packed 24-bit, 32-bit integers, float / double in [-1, 1], double used as given
PCM_U8, PCM_S24, PCM_S32, PCM_F32N, PCM_F64N, PCM_F64 = 4, 8, 12, 16, 20, 24
# bytes per sample of a sample type
PCM_BYTES = {PCM_S16: 2, PCM_F32: 4, PCM_U8: 1, PCM_S24: 3, PCM_S32: 4, PCM_F32N: 4, PCM_F64N: 8, PCM_F64: 8}


class LhipError(RuntimeError):
    pass


class _Config(ctypes.Structure):
    _fields_ = [("channels", ctypes.c_int32), ("samplerate", ctypes.c_int32), ("kbps", ctypes.c_int32),
                ("device", ctypes.c_int32)]


class StreamInfo(ctypes.Structure):
    """``lhip_stream_info_t``: what an ``info_tag`` stream has put out so far."""
    _fields_ = [("frames", ctypes.c_int64), ("audio_bytes", ctypes.c_int64), ("music_crc", ctypes.c_uint32), ("delay", ctypes.c_int32),
                ("padding", ctypes.c_int32), ("tag_bytes", ctypes.c_int32)]


# The C ABI of include/lamejs_hip.h, entry -> (restype, argtypes): the one place that states it.  load_library() applies it to every library it
# loads, so no caller declares a signature (an undeclared entry would pass Python integers as 32-bit C int: a truncation for size_t, int64_t
# and pointers).  tests/test_abi.py holds it against the header's prototypes.
_int, _i64, _size, _ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p
_pi32, _pi64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
ABI = {
    "lhip_device_count": (_int, []),
    "lhip_set_devices": (_int, [ctypes.c_uint64]),
    "lhip_stream_device": (_int, [_ptr]),
    "lhip_device_identity": (_int, [_int, ctypes.c_char_p, ctypes.c_char_p, _size]),
    "lhip_state_bytes": (_size, [_ptr]),
    "lhip_state_get": (_int, [_ptr, _ptr, _size]),
    "lhip_state_set": (_int, [_ptr, _ptr, _size]),
    "lhip_seek_tail_samples": (_size, [_ptr]),
    "lhip_seek": (_int, [_ptr, _i64, _ptr, _ptr]),
    "lhip_create": (_int, [ctypes.POINTER(_Config), _ptr, _size, ctypes.POINTER(_ptr)]),
    "lhip_encode": (_i64, [_ptr, _ptr, _ptr, _size, _ptr, _size]),
    "lhip_encode_pcm": (_i64, [_ptr, _int, _ptr, _ptr, _size, _ptr, _size]),
    "lhip_flush": (_i64, [_ptr, _ptr, _size]),
    "lhip_destroy": (None, [_ptr]),
    "lhip_max_output_bytes": (_size, [_ptr, _size]),
    "lhip_encode_output_bytes": (_i64, [_ptr, _size]),
    "lhip_output_bytes_is_exact": (_int, [_ptr]),
    "lhip_encode_batch": (_int, [_ptr, _size] + [_ptr] * 6),
    "lhip_encode_batch_pcm": (_int, [_ptr, _size, _int] + [_ptr] * 6),
    "lhip_flush_batch": (_int, [_ptr, _size] + [_ptr] * 3),
    "lhip_encode_batch_device": (_int, [_ptr, _size] + [_ptr] * 6 + [_int]),
    "lhip_encode_batch_device_pcm": (_int, [_ptr, _size, _int] + [_ptr] * 6 + [_int]),
    "lhip_last_batch_rejected_samples": (_i64, []),
    "lhip_set_hip_stream": (_int, [_int, _ptr]),
    "lhip_last_batch_stats": (None, [_pi64] * 3),
    "lhip_debug_last_paths": (_int, [ctypes.POINTER(ctypes.c_uint32)]),
    "lhip_debug_read": (_i64, [_int, _ptr, _size]),
    "lhip_kernel_timing": (_int, [_int]),
    "lhip_kernel_times": (_int, [_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double), _pi64]),
    "lhip_debug_math": (_int, [_int, _ptr, _ptr, _size]),
    "lhip_debug_set_spec_seed": (_int, [_int, _int]),
    "lhip_debug_release_context": (_int, [_int]),
    "lhip_frac_call_limit": (_i64, [_ptr]),
    "lhip_debug_frac_call": (_int, [_ptr, _size, _pi32, _pi32]),
    "lhip_debug_frac_flush": (_int, [_ptr, _pi32, _pi32, _int]),
    "lhip_stream_info": (_int, [_ptr, ctypes.POINTER(StreamInfo)]),
    "lhip_info_tag": (_i64, [_ptr, _ptr, _size]),
    "lhip_debug_crc_span": (_size, []),
    "lhip_debug_crc16": (_int, [_ptr, _size, _size, ctypes.POINTER(ctypes.c_uint32)]),
    "lhip_debug_info_toc": (_int, [_ptr, _size, _int, _ptr]),
    "lhip_debug_ingest": (_int, [_int, _int, _ptr, _size, _size, _ptr, _ptr, _pi64]),
    "lhip_replay_gain": (_int, [_ptr, _pi32, _pi64, _pi64]),
    "lhip_debug_gain_histogram": (_int, [_ptr, _ptr]),
    "lhip_debug_gain_windows": (_int, [_int, _int, _ptr, _ptr, _size, _ptr, _ptr]),
    "lhip_debug_quant_probe": (_int, [_ptr, _ptr, _size, _ptr, _int]),
    "lhip_debug_bits_probe": (_int, [_ptr, _ptr, _size, _ptr, _int, _int]),
    "lhip_last_error": (ctypes.c_char_p, []),
    "lhip_version": (ctypes.c_char_p, []),
}

TEST_HOOKS_OPTIONAL_IN_NAMED_LIBRARIES = frozenset({"lhip_debug_quant_probe", "lhip_debug_bits_probe"})      # see load_library

_lib = None


def load_library(path: os.PathLike | None = None) -> ctypes.CDLL:
    """Load the HIP shared library (built by ``__graft_entry__.build()``); raises if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else Path(os.environ.get("LAMEJS_HIP_LIB", _LIB_PATH))
    if not p.exists():
        raise LhipError(f"{p} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
                        "lamejs_amd has no CPU fallback.")
    lib = ctypes.CDLL(str(p))
    for name, (restype, argtypes) in ABI.items():      # a library without one of these entries is not this package's library
        # ... but for a test hook in a library named by the caller (a simulation, a variant build): one built from a tree that did not have the hook yet
        # still serves every caller that does not use it, and a use of the hook fails loudly (AttributeError).  The product library has them all.
        if path is not None and name in TEST_HOOKS_OPTIONAL_IN_NAMED_LIBRARIES and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if path is None:
        _lib = lib
    return lib


_src_hash = None


def generator_hash() -> bytes:
    """First 8 bytes of sha256(js/tables.js ++ js/constants.json): what tables.js writes into every blob as entry ``src_sha256_64``."""
    global _src_hash
    if _src_hash is None:
        import hashlib
        _src_hash = hashlib.sha256((_PKG / "js" / "tables.js").read_bytes() + (_PKG / "js" / "constants.json").read_bytes()).digest()[:8]
    return _src_hash


def blob_is_current(blob: bytes) -> bool:
    """Was this LHTB blob generated by the tables.js / constants.json that are here now?  Decided by CONTENT (the hash the generator embeds), not
    by file times -- those are arbitrary after a checkout, so a changed generator could silently meet an old blob."""
    import struct
    if len(blob) < 16 or blob[:4] != b"LHTB":
        return False
    n = struct.unpack_from("<I", blob, 8)[0]
    for k in range(n):
        e = 16 + 48 * k
        if blob[e:e + 32].split(b"\0", 1)[0] == b"src_sha256_64":
            count, off = struct.unpack_from("<II", blob, e + 36)
            return count == 2 and blob[off:off + 8] == generator_hash()
    return False


def _gain_text(g) -> str:
    """A gain as tables.js reads it back exactly (``Number(repr)``); also the blob cache's file-name part."""
    return repr(float(g))


def tables_blob(channels: int, samplerate: int, kbps: int, joint: bool = False, reservoir: bool = False, fractional_resample: bool = False,
                downmix: bool = False, scale=None, scale_left=None, scale_right=None, protect: bool = False, copyright: bool = False, original: bool = True,
                private_bit: bool = False, emphasis: int = 0, info_tag: bool = False, replay_gain: bool = False, quality: int = 3,
                out_samplerate=None, lowpass=None, lowpass_width=None, highpass=None, highpass_width=None) -> bytes:
    """The LHTB table blob for a configuration.

    Built by the host-side JavaScript ``lamejs_amd/js/tables.js`` (so every transcendental comes
    from the same engine the reference uses).  Blobs for the BASELINE configurations are generated
    at build time into ``lamejs_amd/tables/``; other configurations are generated on demand when
    ``node`` is available.  ``joint``: the reference's joint-stereo mode (an extension: its own
    ``Mp3Encoder`` never selects it, index.js:105); only meaningful for two channels.
    ``fractional_resample``: accept the configurations that resample by a non-integer ratio (extension, call-sequence-exact:
    ``{ fractionalResample: true }`` of tables.js); for every other configuration the blob is the same with and without it.
    ``downmix`` (two channels in, mono out), ``scale``, ``scale_left``, ``scale_right``: the reference's input gains and downmix
    (``{ downmix, scale, scaleLeft, scaleRight }`` of tables.js); without them the blob is the bytes it always was.
    ``protect`` (CRC-protected frames), ``copyright``, ``original``, ``private_bit``, ``emphasis`` (0, 1 or 3): the frame header's settings
    (``{ protect, copyright, original, privateBit, emphasis }`` of tables.js); at their defaults the blob is the bytes it always was.
    ``info_tag``: the stream starts with the placeholder of an Info/LAME tag frame and keeps the totals the tag reports (``{ infoTag }`` of
    tables.js: the tag's constants as named entries that exist only with the option); without it the blob is the bytes it always was.
    ``replay_gain``: the stream analyses the samples it encodes for its ReplayGain track gain (``{ replayGain }`` of tables.js: one named entry that
    exists only with the option); without it the blob is the bytes it always was.
    ``quality``: 3 (the reference wrapper's setting) or 7, LAME's ``-f`` (``{ quality }`` of tables.js: the psychoacoustic model still decides block
    switching and mid/side, the quantization is the bin search alone); 8 is encoded as 7, as the reference's core does.  At 3 the blob is the bytes
    it always was.
    ``out_samplerate``, ``lowpass``, ``lowpass_width``, ``highpass``, ``highpass_width`` (``{ outSampleRate, lowpass, lowpassWidth, highpass, highpassWidth }`` of
    tables.js): the reference core's ``gfp.out_samplerate``, ``lowpassfreq``, ``lowpasswidth``, ``highpassfreq`` and ``highpasswidth`` -- LAME's ``--resample``,
    ``--lowpass``, ``--lowpass-width``, ``--highpass``, ``--highpass-width`` -- as whole numbers of Hz.  ``out_samplerate``: one of the nine MPEG rates, the input
    rate or the input rate divided by a whole number; ``lowpass``: at least 1, or -1 for no lowpass (without ``out_samplerate`` it also chooses the output
    rate, as the core does); the widths: at least 0, a cosine transition instead of the hard edge; ``highpass``: at least 1 and not below the stream's minimum
    (tables.js names it).  A value of another type raises ``ValueError``, as does whatever tables.js refuses with a ``RangeError``.  No blob entry is
    added: without the five options the blob is the bytes it always was.
    """
    filt = []
    for word, name, v, lo, minus_one in (("outrate", "out_samplerate", out_samplerate, 1, False), ("lowpass", "lowpass", lowpass, 1, True), ("lowpasswidth", "lowpass_width", lowpass_width, 0, False),
                                         ("highpass", "highpass", highpass, 1, False), ("highpasswidth", "highpass_width", highpass_width, 0, False)):
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not (v >= lo or (minus_one and v == -1)):
            raise ValueError(f"{name} must be a whole number of Hz >= {lo}" + (", or -1" if minus_one else ""))
        filt.append(f"{word}={int(v)}")
    if highpass_width is not None and highpass is None:
        raise ValueError("highpass_width needs highpass")
    if isinstance(quality, bool) or quality not in (3, 7, 8):
        raise ValueError("quality must be 3, 7 or 8 (8 is encoded as 7)")
    quality = 7 if quality == 8 else int(quality)
    for name, v in (("protect", protect), ("copyright", copyright), ("original", original), ("private_bit", private_bit), ("info_tag", info_tag), ("replay_gain", replay_gain)):
        if v not in (True, False, 0, 1):
            raise ValueError(f"{name} must be True or False")
    if isinstance(emphasis, bool) or emphasis not in (0, 1, 3):
        raise ValueError("emphasis must be 0 (none), 1 (50/15 us) or 3 (CCITT J.17); 2 is reserved")
    if downmix and channels != 2:
        raise TypeError("downmix needs two input channels")
    if downmix and joint:
        raise TypeError("downmix and joint cannot be combined")
    joint = bool(joint) and channels == 2
    frac = bool(fractional_resample)
    mix = (["downmix"] if downmix else []) + [f"{k}={_gain_text(v)}" for k, v in (("scale", scale), ("scaleLeft", scale_left), ("scaleRight", scale_right)) if v is not None]
    mix += (["protect"] if protect else []) + (["copyright"] if copyright else []) + ([] if original else ["original=0"]) + (["privateBit"] if private_bit else []) + ([f"emphasis={int(emphasis)}"] if emphasis else [])
    mix += ["infoTag"] if info_tag else []
    mix += ["replayGain"] if replay_gain else []
    mix += [f"quality={quality}"] if quality != 3 else []
    mix += filt
    f = _TABLE_DIR / f"t_{channels}_{samplerate}_{kbps}{'_joint' if joint else ''}{'_resv' if reservoir else ''}{'_frac' if frac else ''}{''.join('_' + m.replace('=', '') for m in mix)}.bin"
    if not f.exists() or not blob_is_current(f.read_bytes()):      # a cached blob made by another version of its generator is stale
        _TABLE_DIR.mkdir(exist_ok=True)
        try:
            subprocess.run(["node", str(_PKG / "js" / "tables.js"), str(channels), str(samplerate), str(kbps), str(f)] + (["joint"] if joint else []) + (["reservoir"] if reservoir else []) + (["fracresample"] if frac else []) + mix,
                           check=True, capture_output=True, text=True)
        except (OSError, subprocess.CalledProcessError) as e:  # pragma: no cover
            msg = getattr(e, "stderr", "") or str(e)
            if filt and "RangeError" in msg:           # a filter setting tables.js refuses: the caller's value, not a missing blob
                raise ValueError(next((ln for ln in msg.splitlines() if "RangeError" in ln), msg).strip())
            if isinstance(e, OSError) and f.exists():      # no node on this machine: use the blob that was shipped
                return f.read_bytes()
            raise LhipError(f"no table blob for ({channels},{samplerate},{kbps}{',joint' if joint else ''}) and node could not build it: {msg}")
    return f.read_bytes()


def _as_i16(a) -> np.ndarray:
    arr = np.ascontiguousarray(a, dtype=np.int16)
    if arr.ndim != 1:
        raise ValueError("PCM must be a 1-D Int16 array")
    return arr


def _as_pcm(a):
    """(array, sample type) of one PCM argument: integer dtypes go in as Int16 as they always did, floating dtypes as Float32 --
    which is what the reference's encodeBuffer makes of any numbers it is given (Lame.js:1506-1510)."""
    arr = np.asarray(a)
    if arr.dtype.kind == "f":
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        if arr.ndim != 1:
            raise ValueError("PCM must be a 1-D array")
        return arr, PCM_F32
    return _as_i16(arr), PCM_S16


def _as_raw(data) -> np.ndarray:
    """``bytes`` or a 1-D ``uint8`` array, as a contiguous ``uint8`` array; anything else is refused (no cast: an Int16 array is not raw bytes)."""
    a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise ValueError("raw PCM must be bytes or a 1-D uint8 array")
    return np.ascontiguousarray(a)


def _same_type(arrs):
    """Arrays of one call share one sample type: Float32 if any of them is floating (Int16 values are exact in Float32)."""
    pairs = [_as_pcm(a) for a in arrs]
    if all(t == PCM_S16 for _, t in pairs):
        return [a for a, _ in pairs], PCM_S16
    return [np.ascontiguousarray(a, dtype=np.float32) for a, _ in pairs], PCM_F32


class Mp3Encoder:
    """Mirror of the reference's ``Mp3Encoder`` (index.js:66-136)."""

    def __init__(self, channels: int = 1, samplerate: int = 44100, kbps: int = 128, device: int = -1, lib=None, joint: bool = False, reservoir: bool = False,
                 fractional_resample: bool = False, downmix: bool = False, scale=None, scale_left=None, scale_right=None, protect: bool = False,
                 copyright: bool = False, original: bool = True, private_bit: bool = False, emphasis: int = 0, info_tag: bool = False, replay_gain: bool = False, quality: int = 3,
                 out_samplerate=None, lowpass=None, lowpass_width=None, highpass=None, highpass_width=None):
        """``joint`` (extension, not in the reference's wrapper): encode two channels in the reference's joint-stereo mode --
        per frame mid/side or left/right, as its encoder core decides when asked for MPEGMode.JOINT_STEREO.
        ``reservoir`` (extension): encode with the bit reservoir in use (the reference's wrapper disables it, index.js:108); the frames
        of a stream then form a serial chain, so only batches of many streams use the GPU well.
        ``fractional_resample`` (extension): accept the configurations the reference resamples by a non-integer ratio, as call-sequence
        streams -- each ``encodeBuffer`` gives the reference's bytes for the same sequence of call lengths, a call longer than the
        reference consumes whole raises (``call_limit()`` samples are always accepted), each call completes at most one frame, and the
        stream ends with ``flush()`` (include/lamejs_hip.h).
        ``downmix`` (extension, two channels): the reference's MPEGMode.MONO for two input channels -- ``encodeBuffer(l, r)`` and
        ``encode_interleaved`` take both channels, the stream is a mono stream of ``0.5 * (l + r)`` mixed where the samples are read.
        ``scale``, ``scale_left``, ``scale_right`` (extension): the reference's ``gfp.scale`` (replaces the preset's) and per-channel
        gains, applied in its order and with its roundings (include/lamejs_hip.h, "Input gains and downmix").
        ``protect`` (extension): CRC-protected frames, the reference core's ``gfp.error_protection`` (LAME's ``-p``) -- the same frame sizes,
        two more bytes of side information and so 16 bits less main data per frame.  ``copyright``, ``original``, ``private_bit``,
        ``emphasis`` (0, 1 or 3; 2 is reserved): the header bits of those names.  A value outside these raises ``ValueError``.
        ``info_tag`` (extension): the stream is a file -- its first call returns the placeholder of an Info/LAME tag frame in front of the audio
        (which is byte for byte the stream without the option), ``stream_info()`` reports the totals, and after ``flush()``
        ``info_tag_frame()`` returns the finished frame to be written over the placeholder at offset 0 (include/lamejs_hip.h, "Info tag").
        ``replay_gain`` (extension): the samples the encoder consumes (behind gains, downmix and resampler) are analysed on the device as the reference
        core's ReplayGain analysis does; ``replay_gain()`` reports the track gain, and with ``info_tag`` the tag's radio field carries it.
        ``quality`` (extension): 3, the reference wrapper's setting, or 7 -- LAME's ``-f``, the reference core's fast mode: block switching and mid/side as
        always, quantization by the bin search alone (a batch of such streams is quantized by the kernel g_quant_fast).  8 is encoded as 7; any other
        value raises ``ValueError``.
        ``out_samplerate``, ``lowpass``, ``lowpass_width``, ``highpass``, ``highpass_width`` (extension): the reference core's output sample rate and polyphase
        filter settings in whole Hz (``tables_blob``) -- ``Mp3Encoder(2, 44100, 96, out_samplerate=44100)`` is a stream without resampling.  A value that is no
        whole number, a highpass below the stream's minimum or not below the lowpass, upsampling and a non-integer ratio raise ``ValueError``."""
        self._lib = lib or load_library()
        self.channels, self.samplerate, self.kbps = int(channels), int(samplerate), int(kbps)
        self._resv = bool(reservoir)
        blob = tables_blob(self.channels, self.samplerate, self.kbps, joint, reservoir, fractional_resample, downmix, scale, scale_left, scale_right,
                           protect, copyright, original, private_bit, emphasis, info_tag, replay_gain, quality,
                           out_samplerate, lowpass, lowpass_width, highpass, highpass_width)
        cfg = _Config(self.channels, self.samplerate, self.kbps, device)
        h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(blob, len(blob))
        rc = self._lib.lhip_create(ctypes.byref(cfg), buf, len(blob), ctypes.byref(h))
        if rc != 0:
            raise LhipError(f"lhip_create failed ({rc}): {self._lib.lhip_last_error().decode()}")
        self._h = h

    def stream_info(self) -> dict:
        """``info_tag`` streams: frames, audio bytes, music CRC, delay, padding (-1 before ``flush()``) and the tag frame's size."""
        si = StreamInfo()
        rc = self._lib.lhip_stream_info(self._h, ctypes.byref(si))
        if rc != 0:
            raise LhipError(f"lhip_stream_info failed ({rc}): {self._lib.lhip_last_error().decode()}")
        return {"frames": si.frames, "audio_bytes": si.audio_bytes, "music_crc": si.music_crc, "delay": si.delay, "padding": si.padding, "tag_bytes": si.tag_bytes}

    def info_tag_frame(self) -> bytes:
        """``info_tag`` streams, after ``flush()``: the finished Info/LAME tag frame -- write it over the placeholder at offset 0 of the file."""
        out = np.empty(2880, dtype=np.uint8)
        n = self._lib.lhip_info_tag(self._h, out.ctypes.data, len(out))
        if n < 0:
            raise LhipError(f"lhip_info_tag failed ({n}): {self._lib.lhip_last_error().decode()}")
        return out[:n].tobytes()

    def replay_gain(self):
        """``replay_gain`` streams: ``(tenth_db, windows, samples)`` -- the track gain in tenths of a dB (``None`` while no window of
        ``ceil(out_samplerate / 20)`` samples is complete), the complete windows and the samples analysed so far.  Waits for the stream's device."""
        t, w, n = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
        rc = self._lib.lhip_replay_gain(self._h, ctypes.byref(t), ctypes.byref(w), ctypes.byref(n))
        if rc < 0:
            raise LhipError(f"lhip_replay_gain failed ({rc}): {self._lib.lhip_last_error().decode()}")
        return (t.value if rc == 0 else None), w.value, n.value

    def call_limit(self) -> int:
        """``fractional_resample`` streams: the ``encodeBuffer`` length that is accepted whatever calls came before (0: any length goes)."""
        return int(self._lib.lhip_frac_call_limit(self._h))

    # ---- frame-range sharding of one stream (extension; include/lamejs_hip.h: lhip_seek / lhip_state_get / lhip_state_set) ----
    def seek_tail_samples(self) -> int:
        return int(self._lib.lhip_seek_tail_samples(self._h))

    def seek(self, sample_pos: int, tail_left, tail_right=None) -> None:
        """Put this FRESH encoder at input position ``sample_pos`` (a whole number >= 2 of frames); ``tail_*``: the
        ``seek_tail_samples()`` input samples in front of that position."""
        l = _as_i16(tail_left)
        if self.channels == 2 and tail_right is None:
            raise ValueError("seek: a two-channel stream needs both tails")
        r = l if self.channels == 1 else _as_i16(tail_right)
        assert len(l) == self.seek_tail_samples() == len(r)
        rc = self._lib.lhip_seek(self._h, int(sample_pos), l.ctypes.data, r.ctypes.data)
        if rc != 0:
            raise LhipError(f"lhip_seek failed ({rc}): {self._lib.lhip_last_error().decode()}")

    def state_get(self) -> bytes:
        """The complete carried state of the stream (host counters + device record): equal blobs = equal futures."""
        n = int(self._lib.lhip_state_bytes(self._h))
        buf = ctypes.create_string_buffer(n)
        rc = self._lib.lhip_state_get(self._h, buf, n)
        if rc != 0:
            raise LhipError(f"lhip_state_get failed ({rc}): {self._lib.lhip_last_error().decode()}")
        return buf.raw

    def state_set(self, blob: bytes) -> None:
        buf = ctypes.create_string_buffer(blob, len(blob))
        rc = self._lib.lhip_state_set(self._h, buf, len(blob))
        if rc != 0:
            raise LhipError(f"lhip_state_set failed ({rc}): {self._lib.lhip_last_error().decode()}")

    def encodeBuffer(self, left, right=None) -> bytes:
        """Integer arrays are encoded as Int16 (lhip_encode, as always); floating arrays as the Float32 values they are (lhip_encode_pcm),
        fractional parts and values beyond 16 bits included -- the reference's bytes for the same numbers.  A floating sample that is not
        finite or lies beyond +-131072 raises and consumes nothing."""
        if self.channels == 1 or right is None:
            (l,), fmt = _same_type([left])
            r = l
        else:
            (l, r), fmt = _same_type([left, right])
        if len(l) != len(r):
            raise ValueError("left/right length mismatch")
        return self._encode(fmt, l, r, len(l))

    def encode_interleaved(self, samples) -> bytes:
        """Extension: ``channels * n`` samples as they lie in a WAV file (L R L R ...), Int16 or floating; the bytes of ``encodeBuffer`` on the
        de-interleaved samples."""
        (a,), fmt = _same_type([samples])
        if len(a) % self.channels:
            raise ValueError("interleaved PCM: the length is not a multiple of the channel count")
        return self._encode(fmt | PCM_INTERLEAVED, a, a, len(a) // self.channels)

    def encode_pcm(self, data, fmt, interleaved=True) -> bytes:
        """Extension: PCM as a WAV file stores it.  ``data``: a ``bytes`` object or a ``uint8`` array holding samples of the type ``fmt`` (``PCM_U8``,
        ``PCM_S16``, ``PCM_S24``, ``PCM_S32``, ``PCM_F32N``, ``PCM_F64N``; also ``PCM_F32`` / ``PCM_F64``: values used as given) -- interleaved
        (L R L R ..., as in the file), or with ``interleaved=False`` the left plane followed by the right one.  The bytes travel as they are and
        the kernel g_ingest converts them; only a call small enough for one pinned block (a few frames) is converted by the host while it fills
        that block.  Integer types are never looked at on the host; a call of a float type is scanned first, and a sample outside the contract
        raises and consumes nothing."""
        fmt = int(fmt)
        if fmt not in PCM_BYTES:
            raise ValueError(f"unknown sample type {fmt}")
        a = _as_raw(data)
        unit = PCM_BYTES[fmt] * self.channels
        if len(a) % unit:
            raise ValueError("encode_pcm: the length is not a whole number of sample frames")
        n = len(a) // unit
        if interleaved or self.channels == 1:
            return self._encode(fmt | (PCM_INTERLEAVED if self.channels == 2 else 0), a, a, n)
        return self._encode(fmt, a, a[n * PCM_BYTES[fmt]:], n)

    def _encode(self, fmt, l, r, nsamples) -> bytes:
        if nsamples == 0:
            return b""
        # the N-API binding's protocol: the result array is allocated at lhip_encode_output_bytes() and written in place
        cap = self._lib.lhip_encode_output_bytes(self._h, nsamples)
        if cap < 0:
            raise LhipError(f"lhip_encode_output_bytes failed ({cap}): {self._lib.lhip_last_error().decode()}")
        out = np.empty(cap, dtype=np.uint8)
        entry = "lhip_encode" if fmt == PCM_S16 else "lhip_encode_pcm"
        if fmt == PCM_S16:
            n = self._lib.lhip_encode(self._h, l.ctypes.data, r.ctypes.data, nsamples, out.ctypes.data, cap)
        else:
            n = self._lib.lhip_encode_pcm(self._h, fmt, l.ctypes.data, r.ctypes.data, nsamples, out.ctypes.data, cap)
        if n < 0:
            raise LhipError(f"{entry} failed ({n}): {self._lib.lhip_last_error().decode()}")
        if self._lib.lhip_output_bytes_is_exact(self._h) == 1 and n != cap:      # exact without the bit reservoir: that is what lets a binding skip the copy
            raise LhipError(f"lhip_encode returned {n} bytes, lhip_encode_output_bytes promised {cap}")
        return out[:n].tobytes()

    def flush(self) -> bytes:
        cap = self._lib.lhip_max_output_bytes(self._h, 4 * 1152)
        out = np.empty(cap, dtype=np.uint8)
        n = self._lib.lhip_flush(self._h, out.ctypes.data, cap)
        if n < 0:
            raise LhipError(f"lhip_flush failed ({n}): {self._lib.lhip_last_error().decode()}")
        return out[:n].tobytes()

    def last_batch_stats(self):
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._lib.lhip_last_batch_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return {"frames": a.value, "repaired_frames": b.value, "repair_iterations": c.value}

    def last_batch_paths(self) -> frozenset:
        """Which launch paths the most recent batch on this thread took, as a set of names (``PATH_NAMES``; include/lamejs_hip.h)."""
        return last_batch_paths(self._lib)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lhip_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def encode_streams(encoders, lefts, rights=None, flush=True, interleaved=False, fmt=None):
    """Batch extension (BASELINE config 5): one launch for many independent streams.

    encoders: list of Mp3Encoder with identical configuration (``fractional_resample`` streams may mix configurations); lefts/rights: per-stream arrays.
    Int16 if every array is of an integer dtype, otherwise the whole batch as Float32 -- still one launch.  ``interleaved``: ``lefts[i]``
    holds ``channels * n`` samples (L R L R ...), ``rights`` is ignored.
    ``fmt``: a sample type (``PCM_U8`` ... ``PCM_F64``; ``PCM_BYTES``): the arrays are ``bytes`` / ``uint8`` arrays of samples of that type, as
    ``Mp3Encoder.encode_pcm`` takes them (planar: ``lefts[i]`` and ``rights[i]`` one plane each).
    Returns a list of bytes objects (encode [+ flush] output per stream)."""
    lib = encoders[0]._lib
    n = len(encoders)
    if fmt is not None:
        fmt = int(fmt)
        if fmt not in PCM_BYTES:
            raise ValueError(f"unknown sample type {fmt}")
        L = [_as_raw(a) for a in lefts]
        R = L if rights is None or interleaved else [_as_raw(a) for a in rights]
        unit = [PCM_BYTES[fmt] * (e.channels if interleaved else 1) for e in encoders]
        if any(len(a) % u for a, u in zip(L, unit)) or any(len(a) != len(b) for a, b in zip(L, R)):
            raise ValueError("encode_streams: an array is not a whole number of sample frames, or left / right differ in length")
        counts = [len(a) // u for a, u in zip(L, unit)]
    else:
        arrs, fmt = _same_type(list(lefts) + ([] if rights is None or interleaved else list(rights)))
        L = arrs[:n]
        R = L if len(arrs) == n else arrs[n:]
        counts = [len(a) // e.channels if interleaved else len(a) for e, a in zip(encoders, L)]
    if interleaved:
        fmt |= PCM_INTERLEAVED
    H = (ctypes.c_void_p * n)(*[e._h for e in encoders])
    lp = (ctypes.c_void_p * n)(*[a.ctypes.data for a in L])
    rp = (ctypes.c_void_p * n)(*[a.ctypes.data for a in R])
    ns = (ctypes.c_size_t * n)(*counts)
    caps = [lib.lhip_max_output_bytes(e._h, c) for e, c in zip(encoders, counts)]
    outs = [np.empty(c, dtype=np.uint8) for c in caps]
    op = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    cp = (ctypes.c_size_t * n)(*caps)
    wr = (ctypes.c_int64 * n)()
    if fmt == PCM_S16:
        rc = lib.lhip_encode_batch(H, n, lp, rp, ns, op, cp, wr)
    else:
        rc = lib.lhip_encode_batch_pcm(H, n, fmt, lp, rp, ns, op, cp, wr)
    if rc != 0:
        raise LhipError(f"{'lhip_encode_batch' if fmt == PCM_S16 else 'lhip_encode_batch_pcm'} failed ({rc}): {lib.lhip_last_error().decode()}")
    res = [outs[i][: wr[i]].tobytes() for i in range(n)]
    if flush:
        caps2 = [lib.lhip_max_output_bytes(e._h, 4 * 1152) for e in encoders]
        outs2 = [np.empty(c, dtype=np.uint8) for c in caps2]
        op2 = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs2])
        cp2 = (ctypes.c_size_t * n)(*caps2)
        rc = lib.lhip_flush_batch(H, n, op2, cp2, wr)
        if rc != 0:
            raise LhipError(f"lhip_flush_batch failed ({rc}): {lib.lhip_last_error().decode()}")
        res = [res[i] + outs2[i][: wr[i]].tobytes() for i in range(n)]
    return res
