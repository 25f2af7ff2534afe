"""TEST INFRASTRUCTURE: a reader of the side information of an MP3 byte string (ISO 11172-3 2.4.1.7 for MPEG-1, ISO 13818-3 2.4.1.7 for the
low-sampling-frequency layout that MPEG-2 and MPEG-2.5 share), with and without CRC, one or two channels.  It reads headers and side
information only: they sit together at the fixed frame starts, in a bit-reservoir stream too, so main data is never decoded.

Used to take a census of test material (which Huffman tables, block types, scalefactor modes a set of streams really contains).  It is itself
checked, field by field, against the side records the host simulation hands out (tests/test_path_matrix_cpu.py)."""
import struct

BR1 = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320]
BR2 = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160]
SR = {3: [44100, 48000, 32000], 2: [22050, 24000, 16000], 0: [11025, 12000, 8000]}


class _Bits:
    def __init__(self, data, pos):
        self.d, self.p = data, pos * 8

    def get(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.d[self.p >> 3] >> (7 - (self.p & 7))) & 1)
            self.p += 1
        return v


def _granule(b, mpeg1):
    g = {"part2_3_length": b.get(12), "big_values": b.get(9), "global_gain": b.get(8), "scalefac_compress": b.get(4 if mpeg1 else 9)}
    if b.get(1):                                  # window_switching_flag
        g["block_type"], g["mixed_block_flag"] = b.get(2), b.get(1)
        g["table_select"] = [b.get(5), b.get(5)]
        g["subblock_gain"] = [b.get(3), b.get(3), b.get(3)]
        g["region0_count"] = g["region1_count"] = None      # implied by the block type, not transmitted
        assert g["block_type"] != 0, "window switching with block type 0 is forbidden"
    else:
        g["block_type"], g["mixed_block_flag"] = 0, 0
        g["table_select"] = [b.get(5), b.get(5), b.get(5)]
        g["subblock_gain"] = [0, 0, 0]
        g["region0_count"], g["region1_count"] = b.get(4), b.get(3)
    g["preflag"] = b.get(1) if mpeg1 else None   # (the LSF layout carries it inside scalefac_compress)
    g["scalefac_scale"], g["count1table_select"] = b.get(1), b.get(1)
    return g


def parse(mp3):
    """One dict per frame: the header's fields, ``main_data_begin``, ``mode_ext``, ``scfsi`` ([channel][band], MPEG-1 only) and
    ``gr`` ([granule][channel] dicts with the fields of the granule's side information).  The stream must end on a frame boundary."""
    out, pos = [], 0
    while pos + 4 <= len(mp3):
        h = struct.unpack_from(">I", mp3, pos)[0]
        assert (h >> 21) == 0x7FF, f"lost sync at {pos}"
        ver, layer, noprot = (h >> 19) & 3, (h >> 17) & 3, (h >> 16) & 1
        bri, sri, pad = (h >> 12) & 15, (h >> 10) & 3, (h >> 9) & 1
        mode, mode_ext = (h >> 6) & 3, (h >> 4) & 3
        assert ver in SR and layer == 1 and 0 < bri < 15 and sri < 3, f"frame at {pos}: not an MPEG layer III header ({h:08x})"
        mpeg1, nch = ver == 3, 1 if mode == 3 else 2
        size = (144000 if mpeg1 else 72000) * (BR1 if mpeg1 else BR2)[bri] // SR[ver][sri] + pad
        b = _Bits(mp3, pos + 4 + (0 if noprot else 2))
        fr = {"pos": pos, "size": size, "version": {3: "1", 2: "2", 0: "2.5"}[ver], "samplerate": SR[ver][sri], "kbps": (BR1 if mpeg1 else BR2)[bri],
              "protected": not noprot, "padding": pad, "channels": nch, "mode": mode, "mode_ext": mode_ext}
        if mpeg1:
            fr["main_data_begin"] = b.get(9)
            b.get(5 if nch == 1 else 3)
            fr["scfsi"] = [[b.get(1) for _ in range(4)] for _ in range(nch)]
            fr["gr"] = [[_granule(b, True) for _ in range(nch)] for _ in range(2)]
        else:
            fr["main_data_begin"] = b.get(8)
            b.get(nch)
            fr["scfsi"] = [[0, 0, 0, 0] for _ in range(nch)]
            fr["gr"] = [[_granule(b, False) for _ in range(nch)]]
        used = b.p // 8 - pos
        assert b.p % 8 == 0 and used == 4 + (0 if noprot else 2) + ((17 if nch == 1 else 32) if mpeg1 else (9 if nch == 1 else 17)), (pos, used)
        out.append(fr)
        pos += size
    assert pos == len(mp3), "stream does not end on a frame boundary"
    return out


def granules(frames):
    """Every (frame, granule-channel dict) of parsed frames, flat."""
    for fr in frames:
        for gr in fr["gr"]:
            for g in gr:
                yield fr, g


def census(streams):
    """What a set of MP3 byte strings contains, as counts of granule-channels (frames for scfsi and mode_ext): the conditions a test sets on
    its material are read off this."""
    c = {"granules": 0, "frames": 0, "block_type": {0: 0, 1: 0, 2: 0, 3: 0}, "count1table": {0: 0, 1: 0}, "tables": {}, "esc_table": 0, "scalefac_scale": 0,
         "subblock_gain": 0, "empty": 0, "preflag": 0, "scfsi": 0, "mode_ext": {}}
    for mp3 in streams:
        frames = parse(mp3)
        for fr in frames:
            c["frames"] += 1
            c["scfsi"] += any(any(s) for s in fr["scfsi"])
            c["mode_ext"][fr["mode_ext"]] = c["mode_ext"].get(fr["mode_ext"], 0) + 1
        for fr, g in granules(frames):
            c["granules"] += 1
            c["block_type"][g["block_type"]] += 1
            c["count1table"][g["count1table_select"]] += g["part2_3_length"] > 0
            if g["big_values"] > 0:
                for t in g["table_select"]:
                    c["tables"][t] = c["tables"].get(t, 0) + 1
                c["esc_table"] += any(t >= 16 for t in g["table_select"])
            c["scalefac_scale"] += g["scalefac_scale"]
            c["subblock_gain"] += any(g["subblock_gain"])
            c["empty"] += g["part2_3_length"] == 0
            c["preflag"] += bool(g["preflag"])
    return c
