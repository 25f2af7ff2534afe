"""TEST TOOL: the flush frames of the { fractionalResample } goldens, counted -- how many the reference makes of finite samples (encoded byte for byte),
how many of its own NaN samples (replaced by silent frames), and how many of the latter happen to be byte-equal to the stand-in.  The stand-in frames are
made on the host, so the one-lane simulation gives the numbers of the HIP library.   usage: python tests/tools/frac_flush_stats.py > profiles/r07_fractional_resample_flush.txt"""
import hashlib
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import fracresample_cases as fc   # noqa: E402
import lamejs_amd                  # noqa: E402
import libs                        # noqa: E402

lib = libs.sim_library("hostsim")
G = fc.golden_frac()
print("# kind ch in_rate kbps -> out_rate | calls | flush frames | clean (byte-exact) | NaN frames of the reference | of those byte-equal to the silent stand-in")
tot = [0, 0, 0, 0]
for c in G["cases"]:
    L, R = fc.load_case_pcm(c)
    enc = lamejs_amd.Mp3Encoder(c["channels"], c["samplerate"], c["kbps"], lib=lib, fractional_resample=True)
    p = 0
    for i, n in enumerate(c["call_lens"]):
        if i != c.get("bad_call", -1):
            enc.encodeBuffer(L[p:p + n], None if R is None else R[p:p + n])
        p += n
    fl = enc.flush()
    enc.close()
    frames = fc.frames_of(fl, [f["bytes"] for f in c["flush"]])
    clean = sum(1 for f in c["flush"] if not f["nan_in_window"])
    assert all(hashlib.md5(g).hexdigest() == f["md5"] for f, g in zip(c["flush"], frames) if not f["nan_in_window"])
    same = sum(1 for f, g in zip(c["flush"], frames) if f["nan_in_window"] and hashlib.md5(g).hexdigest() == f["md5"])
    n = len(frames)
    tot = [tot[0] + n, tot[1] + clean, tot[2] + n - clean, tot[3] + same]
    print(f'{c["kind"]:9s} {c["channels"]} {c["samplerate"]:5d} {c["kbps"]:3d} -> {c["out_samplerate"]:5d} | {len(c["call_lens"]):2d} | {n} | {clean} | {n - clean} | {same}')
print(f"# {len(G['cases'])} cases: {tot[0]} flush frames, {tot[1]} clean and byte-exact, {tot[2]} made of NaN samples by the reference, of which {tot[3]} are byte-equal to the silent stand-in")
print("# characterisation: the first flush frame is clean in every case (a condition of the golden generator, which picks the smallest number of calls >= 12 for which")
print("# it holds); 48000 -> 32000 and the other ratio-1.5 pairs flush two clean frames (their bunches of zeros have whole lengths until a pass ends on a whole frame);")
print("# a later flush frame carries NaN because an earlier pass used a fractional number of input samples (the carried 32-sample tail is then read at fractional")
print("# positions) or because a tap reads beyond the reference's persistent input buffer, which is only as long as the largest call so far.")
