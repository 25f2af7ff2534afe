"""TEST INFRASTRUCTURE: a decoder of the main data of self-contained MP3 frames (no bit reservoir: main_data_begin = 0), next to tests/sideinfo.py, whose
``parse`` reads the headers and the side information.  ISO 11172-3 2.4.2.7 / 2.4.3.4 for MPEG-1, ISO 13818-3 2.4.3.2 for the scalefactors of the
low-sampling-frequency layout (without intensity stereo).  It goes from bits to values: scalefactors (slen1 / slen2 with scfsi reuse; the four LSF partitions,
both scalefac_compress ranges), the big-value regions through look-up tables built from the configuration's own table blob -- building them asserts that
every table is prefix-free and has no duplicate code --, linbits, sign bits, the count1 quadruples of both tables, and the ancillary bytes up to the frame end.

It is a third, independent leg beside the library's packer and the oracle's writer, which are line-by-line siblings: nothing here goes from values to bits.
Never compared for speed."""
import numpy as np

import sideinfo

SCFSI_BANDS = (0, 6, 11, 16, 21)


class Tables:
    """Decoding tables of a configuration, from the arrays of its table blob (tests/replaygain_cases.blob_entries)."""

    def __init__(self, e):
        self.xlen, self.off = [int(v) for v in e["ht_xlen"]], [int(v) for v in e["ht_off"]]
        self.hlen, self.code = [int(v) for v in e["ht_hlen"]], [int(v) for v in e["ht_code"]]
        self.sfb_l, self.sfb_s = [int(v) for v in e["sfb_l"]], [int(v) for v in e["sfb_s"]]
        self.slen1, self.slen2 = [int(v) for v in e["slen1_tab"]], [int(v) for v in e["slen2_tab"]]
        self._big, self._quad = {}, {}

    @staticmethod
    def _lookup(entries):
        """entries: (code length, code, symbol).  -> (longest length, array indexed by the next `longest` bits -> entry number).  Every code claims the indices
        it is a prefix of; an index claimed twice is a duplicate code or a code that is a prefix of another."""
        longest = max(n for n, _, _ in entries)
        lut = np.full(1 << longest, -1, dtype=np.int32)
        for k, (n, c, _) in enumerate(entries):
            assert 0 < n and 0 <= c < (1 << n), (n, c)
            lo, hi = c << (longest - n), (c + 1) << (longest - n)
            assert (lut[lo:hi] == -1).all(), f"code {c:0{n}b} collides with code {entries[int(lut[lo:hi].max())][1]:b}: not prefix-free"
            lut[lo:hi] = k
        return longest, lut.tolist()

    def big(self, t):
        """Table t of the big-value regions: (longest, lut, [(length, x, y)]), linbits."""
        if t not in self._big:
            assert 0 < t < 32 and t not in (4, 14) and self.off[t] >= 0, f"table {t} does not exist"
            n = 16 if t > 15 else self.xlen[t]
            ent = []
            for x in range(n):
                for y in range(n):
                    h = self.hlen[self.off[t] + x * n + y] - (x != 0) - (y != 0)      # the blob's lengths count the sign bits
                    ent.append((h, self.code[self.off[t] + x * n + y], (x, y)))
            longest, lut = self._lookup(ent)
            self._big[t] = (longest, lut, [(h, s[0], s[1]) for h, _, s in ent], self.xlen[t] if t > 15 else 0)
        return self._big[t]

    def quad(self, sel):
        if sel not in self._quad:
            o = self.off[32 + sel]
            ent = []
            for p in range(16):
                ns = bin(p).count("1")
                ent.append((self.hlen[o + p] - ns, self.code[o + p] >> ns, p))          # the blob's codes leave room for the sign bits
            longest, lut = self._lookup(ent)
            self._quad[sel] = (longest, lut, [(h, p) for h, _, p in ent])
        return self._quad[sel]


class _Reader:
    def __init__(self, data):
        self.n = 8 * len(data) + 64
        self.v = int.from_bytes(bytes(data) + b"\0" * 8, "big")
        self.p = 0

    def get(self, n):
        if n == 0:
            return 0
        v = (self.v >> (self.n - self.p - n)) & ((1 << n) - 1)
        self.p += n
        return v

    def peek(self, n):
        return (self.v >> (self.n - self.p - n)) & ((1 << n) - 1)


def _scalefactors(b, T, fr, g, gr, ch, prev):
    """-> list of scalefactors in transmission order (None: not transmitted, shared with granule 0 through scfsi)."""
    short = g["block_type"] == 2
    assert not g["mixed_block_flag"], "mixed blocks are outside the envelope"
    if fr["version"] == "1":
        s1, s2 = T.slen1[g["scalefac_compress"]], T.slen2[g["scalefac_compress"]]
        if short:
            return [b.get(s1) for _ in range(18)] + [b.get(s2) for _ in range(18)]
        out = []
        for k in range(4):
            for sfb in range(SCFSI_BANDS[k], SCFSI_BANDS[k + 1]):
                shared = gr == 1 and fr["scfsi"][ch][k]
                out.append(None if shared else b.get(s1 if sfb < 11 else s2))
        return out
    sc = g["scalefac_compress"]
    assert not (fr["mode"] == 1 and (fr["mode_ext"] & 1) and ch == 1), "intensity stereo is outside the envelope"
    if sc < 400:
        widths, counts = [(sc >> 4) // 5, (sc >> 4) % 5, (sc % 16) >> 2, sc % 4], ([9, 9, 9, 9] if short else [6, 5, 5, 5])
    elif sc < 500:
        sc -= 400
        widths, counts = [(sc >> 2) // 5, (sc >> 2) % 5, sc % 4, 0], ([9, 9, 12, 6] if short else [6, 5, 7, 3])
    else:
        sc -= 500
        widths, counts = [sc // 3, sc % 3, 0, 0], ([18, 18, 0, 0] if short else [11, 10, 0, 0])
    return [b.get(w) for w, c in zip(widths, counts) for _ in range(c)]


def _linbits_sign(b, v, linbits):
    if v == 15 and linbits:
        v += b.get(linbits)
    if v and b.get(1):
        v = -v
    return v


def decode_frame(frame, T):
    """One self-contained frame -> {"header": sideinfo's dict, "gc": [per granule-channel {"lines": 576 signed ints, "scalefac": list, "part2_bits": n,
    "bits": bits consumed}], "ancillary_bits": the bits behind the main data up to the frame end, "ancillary": their value}."""
    fr = sideinfo.parse(bytes(frame))[0]
    assert fr["main_data_begin"] == 0
    nch = fr["channels"]
    b = _Reader(frame)
    b.p = 8 * (4 + (2 if fr["protected"] else 0) + ((17 if nch == 1 else 32) if fr["version"] == "1" else (9 if nch == 1 else 17)))
    out = []
    for gr, granule in enumerate(fr["gr"]):
        for ch, g in enumerate(granule):
            start = b.p
            end = start + g["part2_3_length"]
            sf = _scalefactors(b, T, fr, g, gr, ch, out)
            p2 = b.p - start
            lines = [0] * 576
            bv = 2 * g["big_values"]
            assert bv <= 576
            if g["block_type"] == 2:
                bounds = [min(3 * T.sfb_s[3], bv), bv, bv]
            elif g["block_type"] != 0:
                bounds = [min(T.sfb_l[8], bv), bv, bv]
            else:
                bounds = [min(T.sfb_l[g["region0_count"] + 1], bv), min(T.sfb_l[g["region0_count"] + g["region1_count"] + 2], bv), bv]
            i = 0
            for region, hi in enumerate(bounds):
                if i >= hi:
                    continue
                t = g["table_select"][region]
                if t == 0:
                    i = hi
                    continue
                longest, lut, ent, linbits = T.big(t)
                while i < hi:
                    k = lut[b.peek(longest)]
                    assert k >= 0, f"gr {gr} ch {ch}: no code of table {t} at bit {b.p}"
                    n, x, y = ent[k]
                    b.p += n
                    lines[i] = _linbits_sign(b, x, linbits)
                    lines[i + 1] = _linbits_sign(b, y, linbits)
                    i += 2
            longest, lut, ent = T.quad(g["count1table_select"])
            while b.p < end and i <= 572:
                k = lut[b.peek(longest)]
                assert k >= 0, f"gr {gr} ch {ch}: no count1 code at bit {b.p}"
                n, p = ent[k]
                b.p += n
                for j in range(4):
                    if (p >> (3 - j)) & 1:
                        lines[i + j] = -1 if b.get(1) else 1
                i += 4
            out.append({"lines": lines, "scalefac": sf, "part2_bits": p2, "bits": b.p - start, "count1_end": i})
    nanc = 8 * len(frame) - b.p
    assert nanc >= 0, "main data runs past the frame end"
    end_bit = b.p
    return {"header": fr, "gc": out, "main_data_end_bit": end_bit, "ancillary_bits": nanc, "ancillary": b.get(nanc)}


def expected_ancillary(nbits, version_bytes):
    """What an encoder without the bit reservoir puts behind the main data (BitStream.js drain_into_ancillary), as (value, bits): "LAME" byte by byte while 8
    bits remain, the version characters if 32 bits remain after that (each while 8 remain), zero bits."""
    v, left = 0, nbits
    for c in b"LAME":
        if left >= 8:
            v, left = (v << 8) | c, left - 8
    if left >= 32:
        for c in version_bytes:
            if left >= 8:
                v, left = (v << 8) | int(c), left - 8
    return v << left
