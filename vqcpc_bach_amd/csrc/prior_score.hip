// Scoring GIVEN codes under the prior (priors/scoring.py, `PriorRelative.score_codes(method='windows')`; the five outputs are stated
// once, in numpy float64, in tests/prior_score_reference.py, and in include/vqcpc.h).  The codes of a piece are known, so nothing is
// sequential: the host runs every model window of a piece as one row of a teacher-forced forward, passes the scored positions'
// hidden rows through the head, and ONE launch per stage of
//   * vqcpc_prior_score: R independent rows of up to 4096 logits.  A row's target code is read from the sequence at the row's
//     (piece, column) and every result is written at the same place of a (pieces, ld) array: gather and scatter are fused.
// turns them into log-probability, entropy, rank, arg-max and the arg-max's log-probability.
// The row statistics RESTATE prior_sample_kernel<true>'s log-probability block (prior_kernels.h, behind `if (logp && ...)`): thread t
// owns codes 16t .. 16t + 15, the same ascending serial sum, the same block_max / block_sum, the same expression, and this file is
// compiled with prior.hip's flags (the contraction flag reaches into the expansion of expf / logf).  logp therefore has the bits
// the samplers write; tests/test_prior_score_kernel_gpu.py holds the two files together.
// Two forms of one body.  BLOCK: a workgroup of 256 threads per row, prior_kernels.h's reductions.  WAVE (V <= 1024): a wavefront
// per row, four rows per workgroup, no LDS and no barrier.  With V <= 1024 the codes of waves 1 - 3 of the BLOCK form lie past V:
// their maxima are -inf and their sums +0.0f, so (r0 + 0) + (0 + 0) and max(max(r0, -inf), -inf) are wave 0's values bit for bit.
// The row is read ONCE, 16 values per thread in registers (the sampler re-reads it).  Plain C++: vector loads and stores only.
#include "prior_kernels.h"

namespace vq {
namespace prior {

constexpr int kScoreWaveVocab = 64 * kPer;                   // 1024: the largest V one wavefront holds

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

template <bool WAVE>
__global__ __launch_bounds__(kThreads) void prior_score_kernel(
    const float* __restrict__ logits, int64_t ldl, int V, int ncb, int stage, int64_t R, const int32_t* __restrict__ row_b,
    const int32_t* __restrict__ row_col, const int64_t* __restrict__ seq, int64_t ldseq, int64_t B, int64_t cols,
    float* __restrict__ logp, int64_t ldlogp, int64_t ld, float* __restrict__ entropy, int32_t* __restrict__ rank,
    int64_t* __restrict__ best, float* __restrict__ best_logp) {
    __shared__ float redf[kWaves];
    __shared__ int redi[kWaves];
    const int t = WAVE ? (threadIdx.x & 63) : threadIdx.x;   // the owner of codes 16t .. 16t + 15
    const int64_t r = WAVE ? (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    if (r >= R) return;                                       // WAVE: wave-uniform, and that form has no barrier
    const int64_t b = row_b[r], col = row_col[r];
    if (col < 0 || col >= cols || b < 0 || b >= B) return;    // a skipped row (uniform over the row's threads): nothing is read or written
    const float ninf = -INFINITY;
    auto gmax = [&](float v) { if constexpr (WAVE) return wave_max(v); else return block_max(v, redf); };
    auto gsum = [&](float v) { if constexpr (WAVE) return wave_sum(v); else return block_sum(v, redf); };
    auto gsum_int = [&](int v) { if constexpr (WAVE) return wave_sum_int(v); else return block_sum_int(v, redi); };
    auto gmin_int = [&](int v) { if constexpr (WAVE) return wave_min_int(v); else return block_min_int(v, redi); };
    // the target: the forced code clamped to the V^ncb codes, and its digit `stage` (prior_sample_kernel's rule; ncb = 1: the code)
    int64_t vtot = 1;
    for (int i = 0; i < ncb; ++i) vtot *= V;
    uint32_t q = (uint32_t)min(max(seq[b * ldseq + col], (int64_t)0), vtot - 1);
    for (int i = 0; i < stage; ++i) q /= (uint32_t)V;
    const int tok = (int)(q % (uint32_t)V);
    const float* row = logits + r * ldl;
    const int i0 = t * kPer;
    float raw[kPer];
    if (i0 + kPer <= V && (reinterpret_cast<uintptr_t>(row + i0) & 15u) == 0) {
#pragma unroll
        for (int k = 0; k < kPer / 4; ++k) {
            const float4 v = reinterpret_cast<const float4*>(row + i0)[k];
            raw[4 * k] = v.x, raw[4 * k + 1] = v.y, raw[4 * k + 2] = v.z, raw[4 * k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kPer; ++k) raw[k] = i0 + k < V ? row[i0 + k] : ninf;
    }
    // ---- prior_sample_kernel<true>'s row statistics --------------------------------------------------------------------------
    float rmx = ninf;
#pragma unroll
    for (int k = 0; k < kPer; ++k) rmx = fmaxf(rmx, raw[k]);
    rmx = gmax(rmx);
    float rs = 0.0f;
#pragma unroll
    for (int k = 0; k < kPer; ++k) rs += raw[k] > ninf ? expf(raw[k] - rmx) : 0.0f;
    rs = gsum(rs);
    const float rt = row[tok];
    if (logp && t == 0) {                                     // stage 0 stores, later stages add in ascending stage order
        const float lp = (rt - rmx) - logf(rs);
        float* o = logp + b * ldlogp + col;
        *o = stage == 0 ? lp : *o + lp;
    }
    // ---- what the samplers do not form ---------------------------------------------------------------------------------------
    const int64_t o = b * ld + col * ncb + stage;
    if (entropy) {                                            // H = log s + (sum_i e_i (m - x_i)) / s: every term is >= 0
        float es = 0.0f;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const float d = rmx - raw[k];                     // +inf past V and for a -inf logit: e == 0 there, the term is 0
            const float e = raw[k] > ninf ? expf(raw[k] - rmx) : 0.0f;
            es += e > 0.0f ? e * d : 0.0f;
        }
        es = gsum(es);
        if (t == 0) entropy[o] = logf(rs) + es / rs;
    }
    if (rank) {                                               // codes the model puts before the target: exact
        int n = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int i = i0 + k;
            n += (i < V) & ((raw[k] > rt) | ((raw[k] == rt) & (i < tok)));
        }
        n = gsum_int(n);
        if (t == 0) rank[o] = n;
    }
    if (best || best_logp) {                                  // the arg-max, the lowest index among equals
        int first = 1 << 30;
#pragma unroll
        for (int k = kPer - 1; k >= 0; --k)
            if (i0 + k < V && raw[k] == rmx) first = i0 + k;
        first = gmin_int(first);
        const int bt = first < (1 << 30) ? first : 0;         // no code holds the maximum (a NaN row): code 0
        if (t == 0) {
            if (best) best[o] = bt;
            if (best_logp) best_logp[o] = (row[bt] - rmx) - logf(rs);
        }
    }
}

}  // namespace prior
}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_prior_score(const float* logits, int64_t ldl, int V, int ncb, int stage, int64_t R, const int32_t* row_b,
                      const int32_t* row_col, const int64_t* seq, int64_t ldseq, int64_t B, int64_t cols, float* logp,
                      int64_t ldlogp, int64_t ld, float* entropy, int32_t* rank, int64_t* best, float* best_logp, void* stream) {
    VQ_REQUIRE(logits && row_b && row_col && seq, "prior_score: null pointer (logits, row_b, row_col, seq)");
    VQ_REQUIRE(V >= 1 && V <= prior::kMaxVocab, "prior_score: %d codes (1 <= V <= 4096)", V);
    VQ_REQUIRE(ncb >= 1 && ncb <= 4 && stage >= 0 && stage < ncb, "prior_score: stage %d of %d (1 <= ncb <= 4, 0 <= stage < ncb)", stage, ncb);
    int64_t vtot = 1;
    for (int j = 0; j < ncb; ++j) vtot *= V;
    VQ_REQUIRE(vtot < (int64_t)1 << 31, "prior_score: V^ncb < 2^31 expected");
    VQ_REQUIRE(R >= 1 && R <= (int64_t)1 << 30 && B >= 1 && cols >= 1, "prior_score: bad arguments (R >= 1, B >= 1, cols >= 1)");
    // the rows' (piece, column) pairs live on the device: the kernel skips a pair outside [0, B) x [0, cols), and every array
    // that is read or written at a pair must hold cols columns (cols * ncb for the per-stage outputs)
    VQ_REQUIRE(ldl >= V && ldseq >= cols && (!logp || ldlogp >= cols) && (!(entropy || rank || best || best_logp) || ld >= cols * ncb),
               "prior_score: bad leading dimensions (ldl >= V; ldseq, ldlogp >= cols; ld >= cols * ncb)");
    if (V <= prior::kScoreWaveVocab)
        hipLaunchKernelGGL(prior::prior_score_kernel<true>, dim3((unsigned)ceil_div(R, prior::kWaves)), dim3(prior::kThreads), 0,
                           (hipStream_t)stream, logits, ldl, V, ncb, stage, R, row_b, row_col, seq, ldseq, B, cols, logp, ldlogp, ld,
                           entropy, rank, best, best_logp);
    else
        hipLaunchKernelGGL(prior::prior_score_kernel<false>, dim3((unsigned)R), dim3(prior::kThreads), 0, (hipStream_t)stream, logits,
                           ldl, V, ncb, stage, R, row_b, row_col, seq, ldseq, B, cols, logp, ldlogp, ld, entropy, rank, best,
                           best_logp);
    VQ_CHECK_LAUNCH("prior_score");
    return VQCPC_OK;
}

}  // extern "C"
