"""TEST INFRASTRUCTURE: the golden files of the families (tests/golden/<name>.json: bytes of the unmodified reference, recorded per call) and
the one way a stream is held against a case of them.  What a family does NOT check is said where it calls ``check_stream``."""
import hashlib
import json

from conftest import ROOT


def load(name):
    return json.loads((ROOT / "tests" / "golden" / f"{name}.json").read_text())


def pinned(arrays, md5):
    """The PCM a case is fed is the PCM its generator hashed (planes in order, None left out); returns ``arrays``."""
    h = hashlib.md5()
    for a in arrays:
        if a is not None:
            h.update(a.tobytes())
    assert h.hexdigest() == md5, "PCM drifted from the golden generator's"
    return arrays


def feed_calls(lens, L, R, encode_call):
    """The stream cut into calls of ``lens`` samples: [encode_call(i, left, right or None)]."""
    parts, p = [], 0
    for i, n in enumerate(lens):
        parts.append(encode_call(i, L[p:p + n], None if R is None else R[p:p + n]))
        p += n
    return parts


def check_stream(case, parts, flush, *, call_bytes=True, enc_md5=True, flush_md5=True, all_md5=False):
    """``parts`` (the bytes of the encode calls) and ``flush`` against the case: the total length, every call's byte count, the md5 of the
    calls' bytes, the flush's length and md5.  ``all_md5``: the md5 of everything instead of the flush's own length -- for a stream whose
    split into calls and flush is not the reference's (the bit reservoir)."""
    who = (case.get("kind"), case["name"])
    enc = b"".join(parts)
    assert len(enc) + len(flush) == sum(case["call_bytes"]) + case["flush_len"], who
    if call_bytes:
        assert [len(p) for p in parts] == case["call_bytes"], (who, [len(p) for p in parts], case["call_bytes"])
    if enc_md5:
        assert hashlib.md5(enc).hexdigest() == case["enc_md5"], who
    if all_md5:
        assert hashlib.md5(enc + flush).hexdigest() == case["all_md5"], who
    else:
        assert len(flush) == case["flush_len"], who
    if flush_md5:
        assert hashlib.md5(flush).hexdigest() == case["flush_md5"], who
