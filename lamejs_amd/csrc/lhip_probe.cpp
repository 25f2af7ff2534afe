// The kernel of the test hook lhip_debug_quant_probe, compiled apart from the product's kernels into a code object of its own (lib/lhip_quant_probe.co, device
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
