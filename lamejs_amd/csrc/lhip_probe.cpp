// The kernels of the test hooks lhip_debug_quant_probe and lhip_debug_bits_probe, compiled apart from the product's kernels into a code object of its own (lib/lhip_quant_probe.co, device
// code only; lhip_api.cpp loads it on first use).  Inside lhip_api.cpp's module the added kernel changed how the backend scheduled a neighbour (three
// instructions of g_quant_pair); apart, every shipped kernel stays instruction for instruction what it was
// (profiles/quant_probe_code_object_diff_parent_vs_result.txt), while the probe calls the same device functions from the same headers.
// HIP builds only; the simulations run the body (k_quant_probe.h) from lhip_api.cpp.
#include "lhip_defs.h"
#include "lhip_wave.h"
#include "lhip_math.h"
#include "lhip_layout.h"
#include "k_quant.h"
#define LHIP_PROBE_BODY 1
#include "k_quant_probe.h"
#include "k_bits_probe.h"

using namespace lhip;

// One wave per workgroup; a wave takes record after record in a loop, as g_quant's waves take frames, so its LDS record serves one record after the other.
// Nothing of a stream is read or written.
extern "C" __global__ __launch_bounds__(64) void g_quant_probe(ProbeArgs a_unused) {
    __shared__ QuantTabs Q;
    __shared__ QuantLds L;
    const ProbeArgs* A = (const ProbeArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    q_copy_tabs(A->T, Q, threadIdx.x, 64);
    __syncthreads();
    for (int r = blockIdx.x; r < A->n; r += A->grid) kb_quant_probe(A->T, A->pb, A->in, A->out, r, threadIdx.x & 63, L, Q);
}

// The kernel of the test hook lhip_debug_bits_probe (k_bits_probe.h): the bit packer over the caller's frames, in the two forms the library launches it in.
// form 0: kb_bits, one wave per workgroup (64 threads), a wave takes frame after frame through its one LDS image, as g_bits's wave takes its frame.
// form 1: kb_bits_mw on GR * C waves (64 GR C threads) that pack into wave 0's image and meet on two LDS counters, as g_frame's FS_BITS_SAVE phase calls it.
extern "C" __global__ __launch_bounds__(256) void g_bits_probe(BitsProbeArgs a_unused) {
    __shared__ BitsLds L[4];
    __shared__ int meet[2];
    const BitsProbeArgs* A = (const BitsProbeArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (A->form == 0) {
        for (int r = blockIdx.x; r < A->n; r += A->grid) { kb_bits(A->T, A->W, A->SD, r, lane, L[0]); wave_sync(); }
        return;
    }
    const int nparts = A->T.mode_gr * A->T.channels_out;       // == blockDim.x / 64 (the host launches it so)
    for (int r = blockIdx.x; r < A->n; r += A->grid) {
        if (threadIdx.x < 2) meet[threadIdx.x] = 0;
        __syncthreads();
        kb_bits_mw(A->T, A->W, A->SD, r, lane, L[wv], L[0].w, wv, nparts, meet);
        __syncthreads();
    }
}
