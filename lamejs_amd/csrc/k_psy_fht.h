// k_psy_fht.h -- the radix-4 FHT passes over points held in LDS (FFT.js:45-112) and the bank-padded layout of a transform buffer (fzp / fzo).
#pragma once
#include "lhip_defs.h"
namespace lhip {
// ---------------------------------------------------------------------------------------------
// FHT butterflies, one radix-4 pass over n points held in LDS (FFT.js:45-112).
// Work item t in [0, n/8): block m = t / kx, index i = t % kx inside the block.
// ---------------------------------------------------------------------------------------------
// The i == 0 butterfly of block m (no twiddles) and the i >= 1 butterflies are separate work lists, so that a
// wave never executes both code paths for one batch of items.
// LDS layout of a transform buffer while the passes run: one pad word after every 32 (index a lives at a + a / 32).  The butterflies of the
// first passes touch, lane after lane, addresses 16 (k1 = 4) or 64 (k1 = 16) words apart: in a plain array that is 2 resp. 7 of the 32 LDS
// banks for a whole wave -- 72 % of g_psyA's LDS cycles were bank conflicts (profiles/r03_pmc_lds_config3.json) -- with the pad the 64 lanes
// of the k1 = 4 pass spread over all 32 banks.  Everything that reads or writes transform DATA goes through fzp(): the windowing's outputs,
// the passes, the energies' operands, the joint-stereo copies; the other phases use the same memory as plain scratch, and every transition
// between the two views already goes through registers and a wave_sync.
LHIP_DEV int fzp(int a) { return a + (a >> 5); }
// offsets inside an item: index + c lands at fzp(index) + c + c / 32 because (index & 31) + (c & 31) < 32 for every operand of every pass
// (k1 = 4: a 16-aligned group; k1 = 16: i < 16 and c & 31 is 0 or 16; k1 >= 64: c is a multiple of 32)
LHIP_DEV int fzo(int c) { return c + (c >> 5); }
LHIP_DEV void fht_item0(float* fz, int base, int k1, int kx, int m) {
    const int k2 = k1 << 1, k3 = k2 + k1, k4 = k2 << 1;
    const int K1 = fzo(k1), K2 = fzo(k2), K3 = fzo(k3);
    float* fi = fz + fzp(base + m * k4);
    float* gi = fz + fzp(base + m * k4 + kx);
    double f0, f1, f2, f3;
    f1 = (double)fi[0] - (double)fi[K1];
    f0 = (double)fi[0] + (double)fi[K1];
    f3 = (double)fi[K2] - (double)fi[K3];
    f2 = (double)fi[K2] + (double)fi[K3];
    fi[K2] = (float)(f0 - f2);
    fi[0] = (float)(f0 + f2);
    fi[K3] = (float)(f1 - f3);
    fi[K1] = (float)(f1 + f3);
    f1 = (double)gi[0] - (double)gi[K1];
    f0 = (double)gi[0] + (double)gi[K1];
    f3 = LHIP_SQRT2 * (double)gi[K3];
    f2 = LHIP_SQRT2 * (double)gi[K2];
    gi[K2] = (float)(f0 - f2);
    gi[0] = (float)(f0 + f2);
    gi[K3] = (float)(f1 - f3);
    gi[K1] = (float)(f1 + f3);
}
LHIP_DEV void fht_item1(float* fz, int base, int k1, int kx, int m, int i, const double* tw) {
    const int k2 = k1 << 1, k3 = k2 + k1, k4 = k2 << 1;
    const int K1 = fzo(k1), K2 = fzo(k2), K3 = fzo(k3);
    (void)kx;
    float* fi = fz + fzp(base + m * k4 + i);
    float* gi = fz + fzp(base + m * k4 + k1 - i);
    const double c1 = tw[4 * (i - 1) + 0], s1 = tw[4 * (i - 1) + 1], c2 = tw[4 * (i - 1) + 2], s2 = tw[4 * (i - 1) + 3];
    double a, b, g0, f0, f1, g1, f2, g2, f3, g3;
    b = s2 * (double)fi[K1] - c2 * (double)gi[K1];
    a = c2 * (double)fi[K1] + s2 * (double)gi[K1];
    f1 = (double)fi[0] - a;
    f0 = (double)fi[0] + a;
    g1 = (double)gi[0] - b;
    g0 = (double)gi[0] + b;
    b = s2 * (double)fi[K3] - c2 * (double)gi[K3];
    a = c2 * (double)fi[K3] + s2 * (double)gi[K3];
    f3 = (double)fi[K2] - a;
    f2 = (double)fi[K2] + a;
    g3 = (double)gi[K2] - b;
    g2 = (double)gi[K2] + b;
    b = s1 * f2 - c1 * g3;
    a = c1 * f2 + s1 * g3;
    fi[K2] = (float)(f0 - a);
    fi[0] = (float)(f0 + a);
    gi[K3] = (float)(g1 - b);
    gi[K1] = (float)(g1 + b);
    b = c1 * g2 - s1 * f3;
    a = s1 * g2 + c1 * f3;
    gi[K2] = (float)(g0 - a);
    gi[0] = (float)(g0 + a);
    fi[K3] = (float)(f1 - b);
    fi[K1] = (float)(f1 + b);
}
// one radix-4 pass over n points: the n/8 work items are the n/(8 kx) twiddle-free ones and the rest
LHIP_DEV void fht_pass(float* fz, int n, int k1, int kx, int lane, int nl, int base, const double* tw) {
    const int items = n / 8, nz = items / kx, kx1 = kx - 1;
    for (int t = lane - base; t < nz; t += nl) if (t >= 0) fht_item0(fz, 0, k1, kx, t);
    for (int t = lane - base; t < items - nz; t += nl) if (t >= 0) { const int m = t / kx1; fht_item1(fz, 0, k1, kx, m, 1 + t - m * kx1, tw); }
}

// the same pass over `nb` equally long transforms stored back to back (ONE padded buffer), as ONE work list: three 256-point transforms have
// 32 items each per pass -- one list of 96 fills the lanes where three lists of 32 leave half of them idle
LHIP_DEV void fht_pass_blocks(float* fz, int nb, int n, int k1, int kx, int lane, int nl, const double* tw) {
    const int items = n / 8, nz = items / kx, kx1 = kx - 1, n1 = items - nz;
    for (int t = lane; t < nb * nz; t += nl) { const int b = t / nz; fht_item0(fz, b * n, k1, kx, t - b * nz); }
    for (int t = lane; t < nb * n1; t += nl) {
        const int b = t / n1, r = t - b * n1, m = r / kx1;
        fht_item1(fz, b * n, k1, kx, m, 1 + r - m * kx1, tw);
    }
}
}  // namespace lhip
