// Scoring GIVEN tokens under the decoder (decoders/scoring.py, `Decoder.score_tokens`; the six outputs are stated once, in numpy
// float64, in tests/score_reference.py, and in include/vqcpc.h).  The tokens of a piece are known, so nothing is sequential: the host
// runs every model window of a piece as one row of a teacher-forced forward, passes the scored positions' hidden rows through the
// concatenated head, and ONE launch of
//   * vqcpc_decode_score: a wavefront per row of logits, kScoreWaves rows per workgroup, no LDS, no barrier.  Lane l holds tokens
//     4l .. 4l + 3 of the row's voice, as decode_sample_kernel does.  The row's target token is read from the chorale at the row's
//     (piece, column) and every result is written at the same place of a (pieces, ld) array: gather and scatter are fused.
// turns them into log-probability, allowed mass, entropy, rank, arg-max and the arg-max's log-probability.
// The row statistics below RESTATE decode_sample_kernel's lines (csrc/decode.hip, the `if constexpr (MASK)` block behind the draw):
// the same expressions on the same lane layout with the same wave_max / wave_sum, and this file is compiled with decode.hip's flags
// (the default contraction: the flag reaches into the expansion of logf, see the head of beam.hip).  logp and logmass therefore
// have the bits the samplers write; tests/test_decode_score_kernel_gpu.py holds the two files together.
#include "common.h"

namespace vq {

constexpr int kScoreWaves = 4;
constexpr int kScoreMaxVoices = 16;
constexpr int kScoreMaxVocab = 256;

struct ScoreVoiceOffsets {
    int off[kScoreMaxVoices + 1];
};

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float pick4(const float (&v)[4], int t) { return t == 0 ? v[0] : t == 1 ? v[1] : t == 2 ? v[2] : v[3]; }

__global__ __launch_bounds__(64 * kScoreWaves) void decode_score_kernel(
    const float* __restrict__ logits, int64_t ldl, ScoreVoiceOffsets vo, int nc, int64_t R, const int32_t* __restrict__ row_b,
    const int32_t* __restrict__ row_col, const int64_t* __restrict__ chorale, int64_t ldch, const uint32_t* __restrict__ allowed,
    int64_t ldallow, int64_t B, int64_t cols, int64_t ld, float* __restrict__ logp, float* __restrict__ logmass,
    float* __restrict__ entropy, int32_t* __restrict__ rank, int64_t* __restrict__ best, float* __restrict__ best_logp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * kScoreWaves + wave;
    if (r >= R) return;                                       // wave-uniform; the kernel has no barrier
    const int64_t b = row_b[r], col = row_col[r];
    if (col < 0 || col >= cols || b < 0 || b >= B) return;    // a skipped row (uniform): nothing is read or written
    const int c = (int)(col % nc);
    const int V = vo.off[c + 1] - vo.off[c];
    const float ninf = -INFINITY;
    uint32_t ok = 0xFu;                                       // bit t = token 4 * lane + t is in the position's set
    if (allowed) {                                            // uniform over the wave: the ballot runs in every lane
        const uint32_t word = allowed[(b * ldallow + col) * 8 + (lane >> 3)];
        const int mine = V - 4 * lane;                        // this lane's tokens below V
        const uint32_t bits = (word >> ((lane & 7) * 4)) & (mine >= 4 ? 0xFu : mine > 0 ? (1u << mine) - 1u : 0u);
        if (__ballot(bits != 0u) != 0ull) ok = bits;          // an empty set restricts nothing
    }
    float raw[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i = 4 * lane + t;
        raw[t] = i < V ? logits[r * ldl + vo.off[c] + i] : ninf;
    }
    // the target, clamped as the sampler clamps a forced token (the host refuses one outside [0, V) before the launch)
    int tok = (int)min(max(chorale[b * ldch + col], (int64_t)0), (int64_t)kScoreMaxVocab);
    tok = min(max(tok, 0), V - 1);
    // ---- decode_sample_kernel's row statistics: the maximum, the exp-sum (lane-serial sum of four, then wave_sum) --------------
    const float rmx = wave_max(fmaxf(fmaxf(raw[0], raw[1]), fmaxf(raw[2], raw[3])));
    float rs = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) rs += raw[t] > ninf ? expf(raw[t] - rmx) : 0.0f;
    rs = wave_sum(rs);
    const float rt = __shfl(pick4(raw, tok & 3), tok >> 2, 64);
    const int64_t o = b * ld + col;
    if (logp && lane == 0) logp[o] = (rt - rmx) - logf(rs);
    if (logmass) {                                            // uniform
        float ar[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) ar[t] = (ok >> t) & 1u ? raw[t] : ninf;
        const float amx = wave_max(fmaxf(fmaxf(ar[0], ar[1]), fmaxf(ar[2], ar[3])));
        float as = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) as += ar[t] > ninf ? expf(ar[t] - amx) : 0.0f;
        as = wave_sum(as);
        if (lane == 0) logmass[o] = (amx - rmx) + logf(as) - logf(rs);
    }
    // ---- what the samplers do not form -----------------------------------------------------------------------------------------
    if (entropy) {                                            // H = log s + (sum_i e_i |d_i|) / s: every term is >= 0
        float es = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float d = rmx - raw[t];                     // +inf past V and for a -inf logit: e == 0 there, the term is 0
            const float e = raw[t] > ninf ? expf(raw[t] - rmx) : 0.0f;
            es += e > 0.0f ? e * d : 0.0f;
        }
        es = wave_sum(es);
        if (lane == 0) entropy[o] = logf(rs) + es / rs;
    }
    if (rank) {                                               // tokens the model puts before the target: exact
        int n = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = 4 * lane + t;
            n += (i < V) & ((raw[t] > rt) | ((raw[t] == rt) & (i < tok)));
        }
        n = wave_sum_int(n);
        if (lane == 0) rank[o] = n;
    }
    if (best || best_logp) {                                  // the arg-max, the lowest index among equals: the lowest lane that
        const bool has = raw[0] == rmx || raw[1] == rmx || raw[2] == rmx || raw[3] == rmx;     // holds the maximum, its first slot
        const int first = __ffsll((long long)__ballot(has)) - 1;
        const int t0 = raw[0] == rmx ? 0 : raw[1] == rmx ? 1 : raw[2] == rmx ? 2 : 3;
        const int bt = first >= 0 ? 4 * first + __shfl(t0, max(first, 0), 64) : 0;             // no lane (a NaN row): token 0
        const float rb = __shfl(pick4(raw, bt & 3), bt >> 2, 64);
        if (lane == 0) {
            if (best) best[o] = bt;
            if (best_logp) best_logp[o] = (rb - rmx) - logf(rs);
        }
    }
}

}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_decode_score(const float* logits, int64_t ldl, const int32_t* voice_offsets, int nc, int64_t R, const int32_t* row_b,
                       const int32_t* row_col, const int64_t* chorale, int64_t ldch, const uint32_t* allowed, int64_t ldallow,
                       int64_t B, int64_t cols, int64_t ld, float* logp, float* logmass, float* entropy, int32_t* rank, int64_t* best,
                       float* best_logp, void* stream) {
    VQ_REQUIRE(logits && voice_offsets && row_b && row_col && chorale && nc >= 1 && nc <= kScoreMaxVoices && R >= 1 &&
               R <= (int64_t)1 << 30 && B >= 1 && cols >= 1,
               "decode_score: bad arguments (logits, voice_offsets, row_b, row_col, chorale, 1 <= nc <= 16, R >= 1, B >= 1, cols >= 1)");
    ScoreVoiceOffsets vo;
    vo.off[0] = voice_offsets[0];
    VQ_REQUIRE(vo.off[0] >= 0, "decode_score: negative voice offset");
    for (int c = 0; c < nc; ++c) {
        const int V = voice_offsets[c + 1] - voice_offsets[c];
        VQ_REQUIRE(V >= 1 && V <= kScoreMaxVocab, "decode_score: voice %d has %d tokens (1 <= V_c <= 256)", c, V);
        vo.off[c + 1] = voice_offsets[c + 1];
    }
    for (int c = nc + 1; c <= kScoreMaxVoices; ++c) vo.off[c] = vo.off[nc];
    // the rows' (piece, column) pairs live on the device: the kernel skips a pair outside [0, B) x [0, cols), and every array
    // that is read or written at a pair must hold cols columns
    VQ_REQUIRE(ldl >= vo.off[nc] && ldch >= cols && ld >= cols && (!allowed || ldallow >= cols),
               "decode_score: bad leading dimensions (ldl >= the voices' widths; ldch, ld, ldallow >= cols)");
    hipLaunchKernelGGL(decode_score_kernel, dim3((unsigned)ceil_div(R, kScoreWaves)), dim3(64 * kScoreWaves), 0, (hipStream_t)stream,
                       logits, ldl, vo, nc, R, row_b, row_col, chorale, ldch, allowed, ldallow, B, cols, ld, logp, logmass, entropy,
                       rank, best, best_logp);
    VQ_CHECK_LAUNCH("decode_score");
    return VQCPC_OK;
}

}  // extern "C"
