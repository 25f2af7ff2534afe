"""TEST INFRASTRUCTURE shared by tests/test_infotag_cpu.py and tests/test_infotag_gpu.py: the Info/LAME tag frame ({ infoTag }).  Yardsticks, all
independent of the code under test: what the unmodified reference computes while it runs (tests/golden/golden_infotag.json,
tests/tools/gen_golden_infotag.js: music CRC, delay, padding, frame count, bytes, the settings the tag reports), a bitwise CRC-16 written here
(``crc16``), a parser of the tag frame written here from the public Xing / LAME tag format (``parse_tag``), and LAME's seek-table bookkeeping
walked frame by frame (``toc_by_frames``)."""
import ctypes
import hashlib
import math
import struct

import numpy as np

import pcm
from golden_cases import feed_calls, load, pinned

BR1 = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320]
BR2 = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160]
SR = {3: [44100, 48000, 32000], 2: [22050, 24000, 16000], 0: [11025, 12000, 8000]}


def goldens():
    return load("golden_infotag")["cases"]


def crc16(data, crc=0):
    """CRC-16, reflected polynomial 0xA001, initial value 0, no final XOR -- bit by bit."""
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0xA001 if crc & 1 else crc >> 1
    return crc


def iso_crc(data):
    """ISO 11172-3 CRC-16 (polynomial 0x8005, preset 0xffff, MSB first), bit by bit."""
    crc = 0xFFFF
    for b in data:
        for i in range(7, -1, -1):
            top = ((crc >> 15) & 1) ^ ((b >> i) & 1)
            crc = (crc << 1) & 0xFFFF
            if top:
                crc ^= 0x8005
    return crc


def lib_crc16(lib, data, misalign=0):
    """lhip_debug_crc16: the kernel (or its simulation body) over ``data`` placed ``misalign`` bytes past a 16-byte boundary."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    r = ctypes.c_uint32(0xFFFFFFFF)
    rc = lib.lhip_debug_crc16(buf.ctypes.data, len(data), misalign, ctypes.byref(r))
    assert rc == 0, (rc, lib.lhip_last_error())
    return r.value


def crc_table_lengths(lib):
    """The lengths the issue names; the workgroup span comes from the library."""
    span = int(lib.lhip_debug_crc_span())
    assert span >= 1024 and span % 16 == 0
    return [0, 1, 15, 16, 17, 1023, 1024, 1025, span - 1, span, span + 1, 3 * span + 5]


def check_crc_table(lib, seed):
    """Seeded random buffers of every length of the table at every misalignment 0 .. 15, and a buffer of zeros with one set bit at each end,
    against the bitwise CRC.  Returns the number of (length, misalignment) pairs checked."""
    rng = np.random.RandomState(seed)
    n_checked = 0
    for n in crc_table_lengths(lib):
        data = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        want = crc16(data)
        for mis in range(16):
            got = lib_crc16(lib, data, mis)
            assert got == want, (n, mis, hex(got), hex(want))
            n_checked += 1
        if n >= 2:
            z = bytearray(n)
            z[0] |= 0x80
            z[-1] |= 0x01
            want = crc16(z)
            for mis in (0, 1, 15):
                assert lib_crc16(lib, z, mis) == want, ("zeros with a bit at each end", n, mis)
    return n_checked


# ---- the golden cases ----
def case_opts(c):
    kw = {"joint": bool(c.get("jointStereo")), "reservoir": bool(c.get("reservoir")), "downmix": bool(c.get("downmix")), "protect": bool(c.get("protect"))}
    if "scaleLeft" in c:
        kw["scale_left"] = c["scaleLeft"]
    if "scaleRight" in c:
        kw["scale_right"] = c["scaleRight"]
    return kw


def case_pcm(c):
    return pinned(pcm.CORPORA[c["corpus"]](c["nsamples"], c["channels"]), c["pcm_md5"])


def make_encoder(lib, c, tagged=True, **kw):
    import lamejs_amd
    return lamejs_amd.Mp3Encoder(c["channels"], c["samplerate"], c["kbps"], lib=lib, info_tag=tagged, **dict(case_opts(c), **kw))


# ---- the tag frame, from the format ----
def header_fields(h):
    ver, layer, prot = (h >> 19) & 3, (h >> 17) & 3, not ((h >> 16) & 1)
    assert (h >> 21) == 0x7FF and layer == 1 and ver != 1
    f = {"mpeg1": ver == 3, "protected": prot, "bitrate_index": (h >> 12) & 15, "samplerate_index": (h >> 10) & 3, "padding": (h >> 9) & 1, "private": (h >> 8) & 1,
         "mode": (h >> 6) & 3, "mode_ext": (h >> 4) & 3, "copyright": (h >> 3) & 1, "original": (h >> 2) & 1, "emphasis": h & 3}
    f["kbps"] = (BR1 if ver == 3 else BR2)[f["bitrate_index"]]
    f["samplerate"] = SR[ver][f["samplerate_index"]]
    f["frame_bytes"] = (144000 if ver == 3 else 72000) * f["kbps"] // f["samplerate"] + f["padding"]
    f["sideinfo_len"] = 4 + ((17 if f["mode"] == 3 else 32) if ver == 3 else (9 if f["mode"] == 3 else 17)) + (2 if prot else 0)
    return f


def parse_tag(frame):
    """The Xing / LAME tag of a frame.  The tag starts behind an UNPROTECTED frame's side information whether or not the frame is protected
    (in a protected frame that is two bytes before the end of its side information)."""
    h = struct.unpack_from(">I", frame, 0)[0]
    f = header_fields(h)
    off = f["sideinfo_len"] - (2 if f["protected"] else 0)
    t = dict(f, offset=off, magic=bytes(frame[off:off + 4]))
    t["flags"], t["frames"], t["bytes"] = struct.unpack_from(">III", frame, off + 4)
    t["toc"] = list(frame[off + 16:off + 116])
    p = off + 116
    t["quality"] = struct.unpack_from(">I", frame, p)[0]
    t["version"] = bytes(frame[p + 4:p + 13])
    t["method"], t["lowpass"] = frame[p + 13], frame[p + 14]
    t["peak"], t["radio_gain"], t["audiophile_gain"] = struct.unpack_from(">IHH", frame, p + 15)
    t["lame_flags"], t["bitrate"] = frame[p + 23], frame[p + 24]
    d = (frame[p + 25] << 16) | (frame[p + 26] << 8) | frame[p + 27]
    t["delay"], t["end_padding"] = d >> 12, d & 0xFFF
    t["misc"], t["unused"] = frame[p + 28], frame[p + 29]
    t["preset"], t["music_length"], t["music_crc"], t["tag_crc"] = struct.unpack_from(">HIHH", frame, p + 30)
    t["tag_crc_offset"] = p + 38
    t["rest"] = bytes(frame[p + 40:])
    return t


def toc_by_frames(frames, kbps):
    """LAME's seek-table bookkeeping (VBRTag.c AddVbr / Xing_seek_table), one frame at a time."""
    summ = seen = pos = 0
    want, size, bag = 1, 400, [0] * 400
    for _ in range(frames):
        summ += kbps
        seen += 1
        if seen < want:
            continue
        if pos < size:
            bag[pos] = summ
            pos += 1
            seen = 0
        if pos == size:
            for i in range(1, size, 2):
                bag[i // 2] = bag[i]
            want *= 2
            pos //= 2
    toc = [0] * 100
    if pos > 0:
        for i in range(1, 100):
            toc[i] = min(255, 256 * bag[min(pos - 1, i * pos // 100)] // summ)
    return toc, pos


def expected_misc(c):
    """VBRTag.js:686-732 from the case's options."""
    mode = 0 if (c["channels"] == 1 or c.get("downmix")) else (3 if c.get("jointStereo") else 1)
    sr = c["samplerate"]
    source = 0 if sr <= 32000 else 2 if sr == 48000 else 3 if sr > 48000 else 1
    non_optimal = int(c.get("scaleLeft", 0) != c.get("scaleRight", 0) or (not c.get("reservoir") and c["ref_brate"] < 320) or c["ATHtype"] == 0 or sr <= 32000)
    return c["noise_shaping"] + (mode << 2) + (non_optimal << 5) + (source << 6)


def check_tag_frame(c, frame, audio):
    """``frame`` against the format, the case's recorded values and ``audio`` (all audio bytes of the stream)."""
    who = c["name"]
    t = parse_tag(frame)
    assert t["frame_bytes"] == len(frame) and t["padding"] == 0 and t["mode_ext"] == 0, who
    assert t["samplerate"] == c["out_samplerate"] and t["kbps"] == c["ref_brate"] and t["protected"] == bool(c.get("protect")), who
    assert t["mode"] == (3 if c["ref_channels_out"] == 1 else 1 if c.get("jointStereo") else 0), who
    assert t["sideinfo_len"] == c["ref_sideinfo_len"], who
    assert frame[4:t["offset"]] == bytes(t["offset"] - 4) or t["protected"], who            # nothing but the header in front of the tag
    assert t["magic"] == b"Info" and t["flags"] == 0xF, who
    assert t["frames"] == c["frameNum"] and t["bytes"] == c["total_bytes"] + len(frame) == t["music_length"], who
    toc, _ = toc_by_frames(c["frameNum"], c["ref_brate"])
    assert t["toc"] == toc and t["toc"][0] == 0 and all(a <= b for a, b in zip(t["toc"], t["toc"][1:])), who
    assert t["quality"] == 100 - 10 * c["VBR_q"] - c["quality"], who
    assert t["version"] == c["version_string"].encode() and len(t["version"]) == 9, who
    assert t["method"] == 1 and t["lowpass"] == min(255, int(math.floor(c["lowpassfreq"] / 100.0 + .5))), who
    assert (t["peak"], t["radio_gain"], t["audiophile_gain"], t["unused"]) == (0, 0, 0, 0), who
    assert t["lame_flags"] == c["ATHtype"] + (c["exp_nspsytune"] << 4) and t["bitrate"] == min(255, c["ref_brate"]), who
    assert t["delay"] == c["encoder_delay"] and t["end_padding"] == int(math.floor(c["encoder_padding"])), who
    assert t["misc"] == expected_misc(c) and t["preset"] == c["preset"], who
    assert t["music_crc"] == crc16(audio) == c["nMusicCRC"], who
    # the tag's own CRC covers every byte in front of it: the first 190 bytes in the layout the format's description has in mind
    assert t["tag_crc"] == crc16(frame[:t["tag_crc_offset"]]), who
    if t["sideinfo_len"] == 36:
        assert t["tag_crc_offset"] == 190, who
    assert t["rest"] == bytes(len(t["rest"])), who
    if t["protected"]:
        assert (frame[4] << 8 | frame[5]) == iso_crc(frame[2:4] + frame[6:t["sideinfo_len"]]), who
    return t


def check_placeholder(c, ph):
    f = header_fields(struct.unpack_from(">I", ph, 0)[0])
    assert f["frame_bytes"] == len(ph) and f["padding"] == 0 and f["samplerate"] == c["out_samplerate"] and f["kbps"] == c["ref_brate"], c["name"]
    body = bytearray(ph[4:])
    if f["protected"]:
        assert (ph[4] << 8 | ph[5]) == iso_crc(ph[2:4] + ph[6:f["sideinfo_len"]]), c["name"]
        body[0:2] = b"\0\0"
    assert bytes(body) == bytes(len(body)), c["name"]


def run_golden_case(lib, c, lens=None, check_info=None):
    """The case through a tagged and an untagged encoder in calls of ``lens`` samples (default: the case's own), then flush: the tagged stream
    is the placeholder and then, call by call, the untagged stream's bytes; those are the reference's; stream_info() is what the reference
    recorded; the tag frame parses to it.  Returns the file as the documentation assembles it: the stream written, then offset 0 overwritten."""
    import lamejs_amd
    who = c["name"]
    L, R = case_pcm(c)
    lens = lens or c["call_lens"]
    assert sum(lens) == c["nsamples"]
    tag, plain = make_encoder(lib, c), make_encoder(lib, c, tagged=False)
    try:
        si0 = tag.stream_info()
        nt = si0["tag_bytes"]
        assert (si0["frames"], si0["audio_bytes"], si0["music_crc"], si0["padding"], si0["delay"]) == (0, 0, 0, -1, c["encoder_delay"]), who
        with __import__("pytest").raises(lamejs_amd.LhipError, match="not been flushed"):
            tag.info_tag_frame()
        a = feed_calls(lens, L, R, lambda i, l, r: tag.encodeBuffer(l, r))
        b = feed_calls(lens, L, R, lambda i, l, r: plain.encodeBuffer(l, r))
        fa, fb = tag.flush(), plain.flush()
        check_placeholder(c, a[0][:nt])
        assert a[0][nt:] == b[0] and a[1:] == b[1:] and fa == fb, who
        audio = b"".join(b) + fb
        assert len(audio) == c["total_bytes"] and hashlib.md5(audio).hexdigest() == c["all_md5"], who
        if not c.get("reservoir") and lens == c["call_lens"]:
            assert [len(x) for x in b] == c["call_bytes"], who
        si = tag.stream_info()
        assert si == {"frames": c["frameNum"], "audio_bytes": c["total_bytes"], "music_crc": c["nMusicCRC"], "delay": c["encoder_delay"],
                      "padding": int(math.floor(c["encoder_padding"])), "tag_bytes": nt}, (who, si)
        frame = tag.info_tag_frame()
        assert len(frame) == nt
        check_tag_frame(c, frame, audio)
        assert tag.flush() == b"" and tag.stream_info() == si and tag.info_tag_frame() == frame, who
        return frame + audio
    finally:
        tag.close()
        plain.close()


# ---- batches and paths (CPU simulations and the GPU alike) ----
def end_padding(nsamples, frame=1152):
    """Lame.js:1393-1412 for a stream fed ``nsamples`` samples without resampling (mf_samples_to_encode starts at 576 + 1152)."""
    pad = frame - (nsamples + 576) % frame
    return pad if pad >= 576 else pad + frame


def mixed_batch_check(lib):
    """encode_streams over three streams of 1, 2 and 37 frames, tagged and untagged mixed (odd start addresses, unequal lengths): every stream
    is the stream a lone untagged encoder gives, the tagged ones with the placeholder in front and their own totals.  Returns the paths seen."""
    import lamejs_amd
    from protection_cases import frames as walk_frames
    lens = [1152, 2 * 1152 + 3, 37 * 1152 + 11]
    pcms = [pcm.bursts(n, 2, seed=900 + i) for i, n in enumerate(lens)]
    tagged = [False, True, True]         # (blobs are launched in order of first appearance: the tagged streams' group is the one launched last)
    encs = [lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, info_tag=t) for t in tagged]
    got = lamejs_amd.encode_streams(encs, [p[0] for p in pcms], [p[1] for p in pcms], flush=False)
    paths = set(lamejs_amd.last_batch_paths(lib))            # (of the group launched last)
    tails = lamejs_amd.encode_streams(encs, [p[0][:0] for p in pcms], [p[1][:0] for p in pcms], flush=True)
    for i, (e, t) in enumerate(zip(encs, tagged)):
        lone = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib)
        want = lone.encodeBuffer(*pcms[i]) + lone.flush()
        lone.close()
        whole = got[i] + tails[i]
        if not t:
            assert whole == want, i
            continue
        si = e.stream_info()
        assert whole[si["tag_bytes"]:] == want and si["audio_bytes"] == len(want) and si["music_crc"] == crc16(want) and si["padding"] == end_padding(lens[i]), (i, si)
        tg = parse_tag(e.info_tag_frame())
        assert tg["frames"] == si["frames"] == len(walk_frames(want)) and tg["music_crc"] == si["music_crc"] and tg["end_padding"] == si["padding"], i
    for e in encs:
        e.close()
    return paths


def resv_batch_check(lib, frames=(1, 5, 12)):
    """One batch of tagged bit-reservoir streams of unequal lengths -- how many bytes each put out is known on the device only -- and their
    flush: per stream the bytes of a lone untagged encoder, the CRC of exactly those.  Returns the paths the encode batch took."""
    import lamejs_amd
    pcms = [pcm.bursts(n * 1152 + 7 * i, 2, seed=700 + i) for i, n in enumerate(frames)]
    encs = [lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, reservoir=True, info_tag=True) for _ in frames]
    got = lamejs_amd.encode_streams(encs, [p[0] for p in pcms], [p[1] for p in pcms], flush=False)
    paths = set(lamejs_amd.last_batch_paths(lib))
    tails = lamejs_amd.encode_streams(encs, [p[0][:0] for p in pcms], [p[1][:0] for p in pcms], flush=True)
    for i, e in enumerate(encs):
        lone = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, reservoir=True)
        want = lone.encodeBuffer(*pcms[i]) + lone.flush()
        lone.close()
        si = e.stream_info()
        assert (got[i] + tails[i])[si["tag_bytes"]:] == want and si["audio_bytes"] == len(want) and si["music_crc"] == crc16(want), (i, si)
        assert parse_tag(e.info_tag_frame())["music_crc"] == si["music_crc"]
        e.close()
    return paths


def long_stream_check(lib, frames):
    """One stream of ``frames`` frames of 44.1 kHz / 128 kbps in ONE call -- its bytes stay in HBM until they are copied back, several workgroups
    of the CRC kernel cover them and the fold stage runs -- and the same stream in calls of 1152 samples, where the host computes the CRC over
    the pinned mirror: the same bytes, the same totals, the same tag frame, and the CRC of a bitwise pass over the bytes."""
    import lamejs_amd
    L, R = pcm.sine(frames * 1152 + 5, 2)
    a, b = (lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, info_tag=True) for _ in range(2))
    x = a.encodeBuffer(L, R)
    pa = set(a.last_batch_paths())
    x += a.flush()
    nt = a.stream_info()["tag_bytes"]
    assert len(x) - nt > 3 * int(lib.lhip_debug_crc_span()), "the stream must span several workgroups of the CRC kernel"
    pb, parts = set(), []
    for p in range(0, len(L), 1152):
        parts.append(b.encodeBuffer(L[p:p + 1152], R[p:p + 1152]))
        pb |= set(b.last_batch_paths())
    y = b"".join(parts) + b.flush()
    sa, sb = a.stream_info(), b.stream_info()
    assert x == y and sa == sb and sa["music_crc"] == crc16(x[nt:]) and sa["frames"] == frames + 2 and a.info_tag_frame() == b.info_tag_frame()
    t = parse_tag(a.info_tag_frame())
    assert t["toc"] == toc_by_frames(sa["frames"], 128)[0] and t["bytes"] == len(x)
    a.close()
    b.close()
    return pa, pb
