"""CRC frame protection and the header's flag bits on the GPU: the goldens of the unmodified reference through the three paths that format
frames -- the batch kernels (g_bits), the one-frame program (g_frame) and the reservoir walk (g_resv_stream) --, a flush, a batch that mixes
protected and unprotected encoders of two configurations, seek and state transplant; a bitwise ISO 11172-3 CRC-16 over every frame produced.
Streams of 12 frames (24 for the cut stream).  Reads tests/golden/ only."""
import pytest

import pcm
import protection_cases as pc
from libs import lib  # noqa: F401


@pytest.fixture(scope="module")
def G():
    G = pc.goldens()
    assert len(G) == 20
    return G


@pytest.mark.gpu
def test_gpu_goldens_through_the_batch_path(lib, G):
    """One call with all twelve frames' samples: g_psyA ... g_quant, g_bits (reservoir streams: g_resv_stream over one stream)."""
    for c in G:
        pc.run_golden_case(lib, c, lens=[c["nsamples"]])


@pytest.mark.gpu
def test_gpu_goldens_through_the_one_frame_path(lib, G):
    """The goldens' own calls: twelve of 1152 samples (g_frame; with the reservoir g_frame<1>), and the uneven ones."""
    for c in G:
        pc.run_golden_case(lib, c)


@pytest.mark.gpu
def test_gpu_reservoir_path_batch_of_eight_streams(lib, G):
    """encode_streams over 8 reservoir streams of 12 frames, flush included: the even streams carry a golden's samples (the reference's bytes),
    the odd ones the same corpus under another seed (each equal to its own stream encoded alone)."""
    import lamejs_amd
    n = 0
    for c in G:
        if not (c.get("reservoir") and c.get("protect")):
            continue
        n += 1
        L, R = pc.case_pcm(c)
        streams = [(L, R) if i % 2 == 0 else pcm.CORPORA[c["corpus"]](c["nsamples"], c["channels"], 1000 + i) for i in range(8)]
        encs = [pc.make_encoder(lib, c) for _ in streams]
        got = lamejs_amd.encode_streams(encs, [s[0] for s in streams], None if c["channels"] == 1 else [s[1] for s in streams], flush=True)
        for i, (s, g) in enumerate(zip(streams, got)):
            assert pc.check_crc(g, True) == c["frames"], (c["name"], i)
            if i % 2 == 0:
                import hashlib
                assert len(g) == sum(c["call_bytes"]) + c["flush_len"] and hashlib.md5(g[len(g) - c["flush_len"]:]).hexdigest() == c["flush_md5"] and \
                    hashlib.md5(g[:len(g) - c["flush_len"]]).hexdigest() == c["enc_md5"], (c["name"], i)
            elif i == 1:
                solo = pc.make_encoder(lib, c)
                assert solo.encodeBuffer(s[0], s[1]) + solo.flush() == g, (c["name"], i)
                solo.close()
        for e in encs:
            e.close()
    assert n >= 5


@pytest.mark.gpu
def test_gpu_flush_of_a_protected_stream(lib):
    """A flush right behind a call that completes no frame, one behind 2.6 frames, and lhip_flush_batch: the same bytes as the stream in one
    encode_streams call, every frame with its CRC."""
    import lamejs_amd
    for ch, sr, kb, kw in ((2, 44100, 128, {}), (1, 22050, 32, {}), (2, 44100, 128, {"reservoir": True})):
        L, R = pcm.bursts(3000, ch)
        for n in (700, 3000):
            a, b = (lamejs_amd.Mp3Encoder(ch, sr, kb, lib=lib, protect=True, **kw) for _ in range(2))
            one = a.encodeBuffer(L[:n], None if R is None else R[:n]) + a.flush()
            two = lamejs_amd.encode_streams([b], [L[:n]], None if R is None else [R[:n]], flush=True)[0]
            assert one == two and pc.check_crc(one, True) >= 2, (ch, sr, kb, kw, n)
            a.close()
            b.close()


@pytest.mark.gpu
def test_gpu_mixed_batch_of_protected_and_unprotected_encoders(lib, G):
    """One lhip_encode_batch over protected and unprotected encoders of two configurations (44.1 kHz / 128 and 22.05 kHz / 48): every stream
    gets the bytes it gets alone -- the reference's for the streams that carry a golden's samples."""
    import lamejs_amd
    by = {c["name"]: c for c in G}
    cases = [by["protect_stereo_44100_128"], by["flag_copyright"], by["protect_stereo_22050_48"], by["flag_private"], by["protect_stereo_44100_128"]]
    pcms = [pc.case_pcm(c) for c in cases]
    encs = [pc.make_encoder(lib, c) for c in cases]
    got = lamejs_amd.encode_streams(encs, [p[0] for p in pcms], [p[1] for p in pcms], flush=True)
    for c, g in zip(cases, got):
        k = len(g) - c["flush_len"]
        pc.check_against_golden(c, [g[:k]], g[k:], calls=False)
    for e in encs:
        e.close()


@pytest.mark.gpu
def test_gpu_seek_and_state_transplant_on_a_protected_stream(lib):
    """A protected 24-frame stream cut in two: lhip_seek + warm-up reaches the state of the unbroken stream at the cut, a transplanted state
    continues it byte for byte (with the reservoir too: its record holds the queued headers, CRC included)."""
    import lamejs_amd
    L, R = pcm.sine(24 * 1152, 2)          # (steady material: the speculated state of a seek hits; on bursts the loudness adaptation has a longer memory than a test's warm-up)
    cutpos, warm = 12 * 1152, 3 * 1152
    for kw in ({}, {"reservoir": True}):
        mk = lambda: lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib, protect=True, **kw)
        whole, graft = mk(), mk()
        head = whole.encodeBuffer(L[:cutpos], R[:cutpos])
        state_at_cut = whole.state_get()
        rest = whole.encodeBuffer(L[cutpos:], R[cutpos:]) + whole.flush()
        assert pc.check_crc(head + rest, True) == 25
        graft.state_set(state_at_cut)
        assert graft.encodeBuffer(L[cutpos:], R[cutpos:]) + graft.flush() == rest
        if not kw:                                         # (seek is not for reservoir streams)
            cut = mk()
            nt, p0 = cut.seek_tail_samples(), cutpos - warm
            cut.seek(p0, L[p0 - nt:p0], R[p0 - nt:p0])
            cut.encodeBuffer(L[p0:cutpos], R[p0:cutpos])
            assert cut.state_get() == state_at_cut
            assert cut.encodeBuffer(L[cutpos:], R[cutpos:]) + cut.flush() == rest
            cut.close()
        whole.close()
        graft.close()


@pytest.mark.gpu
def test_gpu_flag_bits_against_the_oracle(lib):
    assert pc.flag_family_check(lib, pc.flag_family(20283, 10)) == 10
