"""TEST INFRASTRUCTURE shared by tests/test_protection_cpu.py and tests/test_protection_gpu.py: CRC frame protection and the header's flag
bits.  Two independent yardsticks: the unmodified reference's bytes (tests/golden/golden_protection.json, tests/tools/gen_golden_protection.js)
and the CRC-16 of ISO 11172-3 computed here bit by bit (``iso_crc``) over every frame the code under test produced.  The flag bits alone are
also checked against the unchanged oracle, which reads them from the blob."""
import ctypes
import struct

import numpy as np

import pcm
from golden_cases import check_stream, feed_calls, load, pinned

BR1 = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320]
BR2 = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160]
SR = {3: [44100, 48000, 32000], 2: [22050, 24000, 16000], 0: [11025, 12000, 8000]}


def goldens():
    return load("golden_protection")["cases"]


def case_opts(c):
    return {"joint": bool(c.get("jointStereo")), "reservoir": bool(c.get("reservoir")), "downmix": bool(c.get("downmix")), "protect": bool(c.get("protect")),
            "copyright": bool(c.get("copyright")), "original": bool(c.get("original", 1)), "private_bit": bool(c.get("privateBit")), "emphasis": c.get("emphasis", 0)}


def case_pcm(c):
    return pinned(pcm.CORPORA[c["corpus"]](c["nsamples"], c["channels"]), c["pcm_md5"])


def make_encoder(lib, c, **kw):
    import lamejs_amd
    return lamejs_amd.Mp3Encoder(c["channels"], c["samplerate"], c["kbps"], lib=lib, **dict(case_opts(c), **kw))


# ---- the second yardstick: ISO 11172-3, 2.4.3.1 -- CRC-16, polynomial x^16 + x^15 + x^2 + 1, register preset to all ones, MSB first ----
def iso_crc(data):
    crc = 0xFFFF
    for b in data:
        for i in range(7, -1, -1):
            top = ((crc >> 15) & 1) ^ ((b >> i) & 1)
            crc = (crc << 1) & 0xFFFF
            if top:
                crc ^= 0x8005
    return crc


def frames(mp3):
    """(position, size, header word) of every frame of a whole stream; the stream must end on a frame boundary."""
    out, pos = [], 0
    while pos + 4 <= len(mp3):
        h = struct.unpack_from(">I", mp3, pos)[0]
        assert (h >> 21) == 0x7FF, f"lost sync at {pos}"
        ver, bri, sri, pad = (h >> 19) & 3, (h >> 12) & 15, (h >> 10) & 3, (h >> 9) & 1
        size = (144000 if ver == 3 else 72000) * (BR1 if ver == 3 else BR2)[bri] // SR[ver][sri] + pad
        out.append((pos, size, h))
        pos += size
    assert pos == len(mp3), "stream does not end on a frame boundary"
    return out


def sideinfo_len_of(h):
    """Header + side information bytes of a frame with this header word (Lame.js:1103-1110)."""
    mpeg1, mono, prot = ((h >> 19) & 3) == 3, ((h >> 6) & 3) == 3, not ((h >> 16) & 1)
    return 4 + ((17 if mono else 32) if mpeg1 else (9 if mono else 17)) + (2 if prot else 0)


def check_crc(mp3, protect):
    """Every frame of the stream carries the protection bit as asked and, if protected, the ISO CRC over header bytes 2, 3 and the side
    information (in a reservoir stream too: header and side information sit together at the fixed frame starts).  Returns the frame count."""
    fr = frames(mp3)
    for pos, size, h in fr:
        assert (not ((h >> 16) & 1)) == bool(protect), f"protection bit of the frame at {pos}"
        if protect:
            sl = sideinfo_len_of(h)
            stored = (mp3[pos + 4] << 8) | mp3[pos + 5]
            want = iso_crc(mp3[pos + 2:pos + 4] + mp3[pos + 6:pos + sl])
            assert stored == want, f"frame at {pos}: stored CRC {stored:04x}, ISO CRC {want:04x}"
    return len(fr)


def check_flags(mp3, c):
    """The header's flag bits of every frame are what the case asks for."""
    for pos, size, h in frames(mp3):
        got = {"privateBit": (h >> 8) & 1, "copyright": (h >> 3) & 1, "original": (h >> 2) & 1, "emphasis": h & 3}
        want = {"privateBit": c.get("privateBit", 0), "copyright": c.get("copyright", 0), "original": c.get("original", 1), "emphasis": c.get("emphasis", 0)}
        assert got == want, (c["name"], pos, got)


def check_against_golden(c, parts, flush, calls=True):
    """parts: the bytes of the encode calls (any chunking of the case's samples gives the same stream); calls: they were the case's own calls."""
    check_stream(c, parts, flush, call_bytes=calls)
    whole = b"".join(parts) + flush
    assert check_crc(whole, c.get("protect")) == c["frames"], c["name"]
    check_flags(whole, c)
    return whole


def run_golden_case(lib, c, lens=None):
    """The case through encodeBuffer in calls of `lens` samples (default: the case's own calls), then flush."""
    L, R = case_pcm(c)
    enc = make_encoder(lib, c)
    try:
        assert sum(lens or c["call_lens"]) == c["nsamples"]
        parts = feed_calls(lens or c["call_lens"], L, R, lambda i, l, r: enc.encodeBuffer(l, r))
        return check_against_golden(c, parts, enc.flush(), calls=lens is None)
    finally:
        enc.close()


# ---- blobs ----
def cfg_entry(blob, key):
    """(byte offset of cfg_i[key], its value) in an LHTB blob."""
    n = struct.unpack_from("<I", blob, 8)[0]
    ent = {}
    for k in range(n):
        e = 16 + 48 * k
        ent[blob[e:e + 32].split(b"\0", 1)[0].decode()] = struct.unpack_from("<II", blob, e + 36)
    cnt, off = ent["cfg_i_names"]
    names = "".join(chr(x) for x in struct.unpack_from(f"<{cnt}i", blob, off) if x).split(",")
    at = ent["cfg_i"][1] + 4 * names.index(key)
    return at, struct.unpack_from("<i", blob, at)[0]


def patched(blob, **values):
    b = bytearray(blob)
    for k, v in values.items():
        struct.pack_into("<i", b, cfg_entry(blob, k)[0], v)
    return bytes(b)


def create_rc(lib, channels, samplerate, kbps, blob):
    """(return code, message) of lhip_create on this blob; a created stream is destroyed."""
    from lamejs_amd import _Config
    h = ctypes.c_void_p()
    buf = ctypes.create_string_buffer(blob, len(blob))
    rc = lib.lhip_create(ctypes.byref(_Config(channels, samplerate, kbps, -1)), buf, len(blob), ctypes.byref(h))
    msg = lib.lhip_last_error().decode() if rc != 0 else ""
    if rc == 0:
        lib.lhip_destroy(h)
    return rc, msg


# ---- the flag bits alone, against the unchanged oracle (it reads copyright / original / extension / emphasis from the blob) ----
FLAG_CONFIGS = [(2, 44100, 128, False), (1, 44100, 64, False), (2, 48000, 320, False), (1, 22050, 32, False), (2, 16000, 32, False), (1, 8000, 8, False), (2, 44100, 128, True)]


def flag_family(seed, count, max_frames=5):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        ch, sr, kb, joint = FLAG_CONFIGS[i % len(FLAG_CONFIGS)]
        flags = {"copyright": bool(rng.randint(0, 2)), "original": bool(rng.randint(0, 2)), "private_bit": bool(rng.randint(0, 2)), "emphasis": int(rng.choice([0, 1, 3]))}
        if i < 4:                                            # each flag alone at least once
            flags = {"copyright": i == 0, "original": i != 1, "private_bit": i == 2, "emphasis": 3 if i == 3 else 0}
        n = int(rng.randint(600, max_frames * 1152))
        out.append({"cfg": (ch, sr, kb, joint), "flags": flags, "corpus": ["sine", "bursts"][int(rng.randint(0, 2))], "seed": int(rng.randint(1, 1 << 30)), "n": n,
                    "chunk": int(rng.choice([1152, 777, 2305, n]))})
    return out


def flag_family_check(lib, cases):
    import lamejs_amd
    from oracle_py import oracle_calls
    for fc in cases:
        ch, sr, kb, joint = fc["cfg"]
        L, R = pcm.CORPORA[("centre_" if joint else "") + fc["corpus"]](fc["n"], ch, fc["seed"])
        parts, tail = oracle_calls(lamejs_amd.tables_blob(ch, sr, kb, joint=joint, **fc["flags"]), L, R,
                                   [min(fc["chunk"], fc["n"] - p) for p in range(0, fc["n"], fc["chunk"])])
        want = b"".join(parts) + tail
        enc = lamejs_amd.Mp3Encoder(ch, sr, kb, lib=lib, joint=joint, **fc["flags"])
        got = b"".join(enc.encodeBuffer(L[p:p + fc["chunk"]], None if R is None else R[p:p + fc["chunk"]]) for p in range(0, fc["n"], fc["chunk"])) + enc.flush()
        enc.close()
        assert got == want, (fc["cfg"], fc["flags"], fc["chunk"])
        f = fc["flags"]
        check_flags(got, {"name": str(fc["cfg"]), "copyright": int(f["copyright"]), "original": int(f["original"]), "privateBit": int(f["private_bit"]), "emphasis": f["emphasis"]})
        check_crc(got, False)
    return len(cases)
