"""TEST INFRASTRUCTURE shared by tests/test_psy_lazy_cpu.py and tests/test_psy_lazy_gpu.py: the short-block psychoacoustics computed only where
somebody reads them (a "lazy" batch: lhip_batch.h plan_batch, k_psy_a.h psy_need_s / psy_need_f).

The psy call in granule slot g leaves its thresholds in W.E[g] (lhip_debug_read(2): 122 entries per psy channel -- en.l 22, en.s 39, thm.l 22,
thm.s 39); the quantization of slot g + 1 reads them, the short ones only when that granule is a short block.  By definition, per call:

    needS(g) = g is its stream's last slot in the batch, or a channel of slot g + 1 has block type 2 (lhip_debug_read(1))
    needF(g) = needS(g) or needS(g + 1)            (the short spectra: the short limiting looks back two sub-blocks)

A lazy batch writes zeros into the short entries of a call without needS; everything else -- the bytes, the stream state, every long entry, the
short entries with needS -- is what an eager batch computes.  LAMEJS_PSY_LAZY_MIN_FRAMES (read per batch) selects: 0 always lazy, NEVER eager.

Cases: 40 frames' worth of samples (46080) of pcm.CORPORA material with its default seed; `expect` = (psy calls, needS, needF) of the one-call
encode, counted in the parent's host simulation."""
import contextlib
import ctypes
import functools
import os

import numpy as np

HOOK = "LAMEJS_PSY_LAZY_MIN_FRAMES"
LAZY, NEVER = "0", "2000000000"
NSAMPLES = 1152 * 40
LONG = np.r_[0:22, 61:83]
SHORT = np.r_[22:61, 83:122]
SHORT_TYPE = 2

CASES = [
    dict(name="stereo128/bursts", ch=2, sr=44100, kb=128, joint=False, material="bursts", expect=(78, 10, 19)),
    dict(name="mono128/bursts", ch=1, sr=44100, kb=128, joint=False, material="bursts", expect=(78, 6, 11)),
    dict(name="mono22k64/bursts", ch=1, sr=22050, kb=64, joint=False, material="bursts", expect=(79, 6, 11)),
    dict(name="stereo128/sine", ch=2, sr=44100, kb=128, joint=False, material="sine", expect=(78, 2, 3)),
    dict(name="joint128/centre_bursts", ch=2, sr=44100, kb=128, joint=True, material="centre_bursts", expect=None),
    dict(name="joint128/bursts", ch=2, sr=44100, kb=128, joint=True, material="bursts", expect=None),
]
GPU_CASES = ("stereo128/bursts", "stereo128/sine", "joint128/centre_bursts", "joint128/bursts")


def case(name):
    return next(c for c in CASES if c["name"] == name)


@contextlib.contextmanager
def hook(value):
    """LAMEJS_PSY_LAZY_MIN_FRAMES for the batches inside (None: unset, the default threshold); the library reads it where it plans a batch."""
    old = os.environ.get(HOOK)
    if value is None:
        os.environ.pop(HOOK, None)
    else:
        os.environ[HOOK] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(HOOK, None)
        else:
            os.environ[HOOK] = old


@functools.lru_cache(maxsize=None)
def material(name, nsamples=NSAMPLES):
    """(left, right or None, the oracle's bytes with the flush) of a case: computed once per process, shared and read-only."""
    import pcm
    from oracle_py import oracle_encode
    c = case(name)
    L, R = pcm.CORPORA[c["material"]](nsamples, c["ch"])
    L = np.asarray(L, dtype=np.int16)
    R = None if (R is None or c["ch"] == 1) else np.asarray(R, dtype=np.int16)
    want = oracle_encode(c["ch"], c["sr"], c["kb"], L, R, joint=c["joint"])
    for a in (L, R):
        if a is not None:
            a.setflags(write=False)
    return L, R, want


def _geometry(c):
    return c["ch"], (4 if c["joint"] else c["ch"]), (2 if c["sr"] >= 32000 else 1)


def read_taps(lib, c, nframes, nstreams=1):
    """(block types [slot, channel], thresholds [slot, psy channel, 122]) of the last batch."""
    C, Cp, GR = _geometry(c)
    ngs = GR * nframes + nstreams
    bt = np.empty(ngs * C, dtype="<i4")
    E = np.empty(ngs * Cp * 122, dtype="<f4")
    for what, a in ((1, bt), (2, E)):
        assert lib.lhip_debug_read(what, a.ctypes.data_as(ctypes.c_void_p), a.nbytes) == a.nbytes, what
    return bt.reshape(ngs, C), E.reshape(ngs, Cp, 122)


def need_flags(bt, starts):
    """needS, needF per granule slot by the definition above (False in the carry slots); `starts`: every stream's carry slot, ascending."""
    ngs = len(bt)
    needS, needF = np.zeros(ngs, dtype=bool), np.zeros(ngs, dtype=bool)
    for s0, s1 in zip(starts, list(starts[1:]) + [ngs]):
        for g in range(s0 + 1, s1):
            needS[g] = g == s1 - 1 or bool((bt[g + 1] == SHORT_TYPE).any())
        for g in range(s0 + 1, s1):
            needF[g] = needS[g] or (g + 1 < s1 and needS[g + 1])
    return needS, needF


def encode_calls(lib, c, L, R, lens, mode):
    """One stream through `lib` in calls of `lens` samples with the hook at `mode`, then its flush: {"bytes", "calls": [{frames, state, paths, bt, E}]}."""
    import lamejs_amd
    with hook(mode):
        enc = lamejs_amd.Mp3Encoder(c["ch"], c["sr"], c["kb"], lib=lib, joint=c["joint"])
        out, calls, p = b"", [], 0
        for n in lens:
            out += enc.encodeBuffer(L[p:p + n], None if R is None else R[p:p + n])
            p += n
            nfr = enc.last_batch_stats()["frames"]
            bt, E = read_taps(enc._lib, c, nfr)
            calls.append(dict(frames=nfr, state=enc.state_get(), paths=enc.last_batch_paths(), bt=bt, E=E))
        assert p == len(L)
        out += enc.flush()
        state = enc.state_get()
        enc.close()
    return dict(bytes=out, calls=calls, final_state=state)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_taps(eager, lazy, starts, C, label):
    """Tap 2 of a lazy batch against the eager one's, tap 1 deciding: returns (calls whose short entries are zero, calls whose short entries were computed)."""
    assert np.array_equal(eager["bt"], lazy["bt"]), label
    bt, Ee, El = eager["bt"], eager["E"], lazy["E"]
    needS, needF = need_flags(bt, starts)
    zeroed = computed = 0
    for g in range(len(bt)):
        if g in starts:                          # the carry slot: the state's thresholds, as loaded
            assert np.array_equal(u32(Ee[g]), u32(El[g])), (label, g)
            continue
        assert np.array_equal(u32(Ee[g][:, LONG]), u32(El[g][:, LONG])), (label, "long entries", g)
        # (so that a zero can only mean a skip: the material leaves no all-zero short block in L / R)
        assert all(u32(Ee[g][ch, SHORT]).any() for ch in range(C)), (label, "the eager run has an all-zero short block", g)
        if needS[g]:
            assert np.array_equal(u32(Ee[g][:, SHORT]), u32(El[g][:, SHORT])), (label, "short entries of a call that is read", g)
            computed += 1
        else:
            assert not u32(El[g][:, SHORT]).any(), (label, "short entries of a call nobody reads", g)
            zeroed += 1
    return zeroed, computed, int(needS.sum()), int(needF.sum())


def check_case(lib, name, lens=None):
    """A case in one call (or in calls of `lens`), lazy against eager against the oracle; the taps of every batch of two frames or more (a smaller one is the
    one-frame program, which is never lazy).  Returns the counts of the first checked batch."""
    c = case(name)
    L, R, want = material(name)
    lens = [len(L)] if lens is None else lens
    eager = encode_calls(lib, c, L, R, lens, NEVER)
    lazy = encode_calls(lib, c, L, R, lens, LAZY)
    assert eager["bytes"] == want, name
    assert lazy["bytes"] == want, name
    counts = []
    for k, (a, b) in enumerate(zip(eager["calls"], lazy["calls"])):
        assert a["state"] == b["state"], (name, "stream state after call", k)
        assert a["frames"] == b["frames"] and a["paths"] == b["paths"], (name, k)
        if a["frames"] >= 2:
            assert "SEPARATE" in b["paths"], (name, k, sorted(b["paths"]))
            counts.append(check_taps(a, b, [0], c["ch"], f"{name} call {k}"))
    assert eager["final_state"] == lazy["final_state"], name
    return counts, eager


def check_three_streams(lib, frames=(20, 27, 34)):
    """One batch of three `bursts` stereo streams of different lengths: every stream's last call keeps its short side, bytes and states per stream."""
    import lamejs_amd
    import pcm
    from oracle_py import oracle_encode
    c = case("stereo128/bursts")
    pcms = [pcm.bursts(1152 * f, 2, seed=777 + i) for i, f in enumerate(frames)]
    res = {}
    for mode in (NEVER, LAZY):
        with hook(mode):
            encs = [lamejs_amd.Mp3Encoder(2, 44100, 128, lib=lib) for _ in frames]
            got = lamejs_amd.encode_streams(encs, [p[0] for p in pcms], [p[1] for p in pcms], flush=False)
            nfr = encs[0].last_batch_stats()["frames"]
            bt, E = read_taps(encs[0]._lib, c, nfr, len(frames))
            states = [e.state_get() for e in encs]
            got = [g + e.flush() for g, e in zip(got, encs)]
            for e in encs:
                e.close()
        res[mode] = dict(bytes=got, states=states, bt=bt, E=E)
    for i, (l, r) in enumerate(pcms):
        want = oracle_encode(2, 44100, 128, l, r)
        assert res[NEVER]["bytes"][i] == want and res[LAZY]["bytes"][i] == want, i
    assert res[NEVER]["states"] == res[LAZY]["states"]
    bt = res[NEVER]["bt"]
    starts = [int(g) for g in np.nonzero(bt[:, 0] < 0)[0]]          # a fresh stream's carry slot holds block type -1
    assert len(starts) == len(frames) and starts[0] == 0, starts
    z, n, ns, nf = check_taps(res[NEVER], res[LAZY], starts, 2, "three streams")
    needS, _ = need_flags(bt, starts)
    assert all(needS[s - 1] for s in starts[1:]) and needS[-1]      # the last call of every stream
    return z, n


def first_short_granule(bt):
    """Index (slot - 1) of the first granule with a short block in a one-stream batch."""
    g = np.nonzero((bt[1:] == SHORT_TYPE).any(axis=1))[0]
    assert len(g), "the material has no short block"
    return int(g[0])
