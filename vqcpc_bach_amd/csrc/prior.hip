// Autoregressive sampling of code sequences from the prior (reference: VQCPCB/priors/prior_relative.py:308-353, one full
// forward per code and np.random.choice on the host).  The prior is one causal stack over the codes of a model window, so
// its incremental step is the decoder's without the cross-attention and reuses vqcpc_decode_linear / vqcpc_decode_attn /
// vqcpc_decode_prefill_attn (csrc/decode.hip).  New here, because the decoder's sampler stops at 256 tokens per voice and
// the prior's vocabulary is codebook_size ** num_codebooks:
//   * vqcpc_prior_sample: the step's tail for V <= 4096.  ONE WORKGROUP PER ROW (256 threads, thread t owns the 16
//     consecutive tokens 16t .. 16t + 15), so the order of every reduction is a function of V alone and a row's codes do
//     not depend on which rows share the call.  logits * temperature (the reference's sense, :346), top-k by a bitwise
//     radix select of the k-th largest logit, top-p by a bitonic sort of (logit, index) keys in LDS and a scan in sorted
//     order, softmax, one counter-based draw.  The position counter is shared by every kernel of the step: the last
//     workgroup to finish (a ticket in device memory) advances it.
//   * vqcpc_prior_sample_constrained: the same kernel body under a compile-time flag.  Per (row, sequence column) a code to
//     emit or < 0 for the draw, and the emitted code's log-probability under the row as the model gave it.
//   * vqcpc_prior_sample_masked: one more compile-time flag on top of that.  Per (row, sequence column) a set of the codes that
//     may be drawn, and the log of the probability the unmodified row gives to the set.
//   * vqcpc_prior_window: ONE workgroup.  Commits the live window's codes into the sequence, loads the next window, the
//     prefix's table-row indices, the input row of position P, the window's seeds and `pos`.
// The kernels themselves are in prior_kernels.h, which csrc/product_codes.hip instantiates for product codes.
#include "prior_kernels.h"

using namespace vq;

extern "C" {

int vqcpc_prior_sample(const float* logits, int64_t ldl, int V, int64_t M, float temperature, int top_k, float top_p,
                       const int64_t* seeds, const int64_t* teacher, int64_t ldteach, int64_t* codes, int64_t ldc, int N,
                       const float* table, int64_t table_rows, int d, float* next_in, int64_t ldn, float* probs, int64_t ldp,
                       int32_t* pos, int32_t* ticket, void* stream) {
    VQ_REQUIRE(V >= 1 && V <= prior::kMaxVocab, "prior_sample: %d codes (1 <= V <= 4096)", V);
    VQ_REQUIRE(M >= 1 && M <= prior::kMaxRows, "prior_sample: %lld rows (1 <= M <= 64)", (long long)M);
    VQ_REQUIRE(logits && codes && table && next_in && pos && ticket, "prior_sample: null pointer");
    VQ_REQUIRE(N >= 1 && N <= prior::kMaxWindow && d >= 1 && d <= prior::kMaxDim,
               "prior_sample: bad arguments (1 <= N <= 1024, 1 <= d <= 4096)");
    VQ_REQUIRE(temperature > 0.0f && top_k >= 0 && top_p == top_p, "prior_sample: temperature > 0, top_k >= 0");
    VQ_REQUIRE(teacher || seeds, "prior_sample: seeds are needed unless the codes are teacher-forced");
    VQ_REQUIRE(ldl >= V && ldc >= N && ldn >= d && (!teacher || ldteach >= N) && (!probs || ldp >= V) && table_rows >= V,
               "prior_sample: bad leading dimensions, or a table of fewer than V rows");
    hipLaunchKernelGGL(prior::prior_sample_kernel<false>, dim3((unsigned)M), dim3(prior::kThreads), 0, (hipStream_t)stream,
                       logits, ldl, V, temperature, top_k, top_p, seeds, teacher, ldteach, codes, ldc, N, table, d, next_in, ldn,
                       probs, ldp, pos, ticket, (float*)nullptr, (int64_t)0, (const int32_t*)nullptr, prior::NoStage{});
    VQ_CHECK_LAUNCH("prior_sample");
    return VQCPC_OK;
}

int vqcpc_prior_sample_constrained(const float* logits, int64_t ldl, int V, int64_t M, float temperature, int top_k, float top_p,
                                   const int64_t* seeds, const int64_t* constraint, int64_t ldcons, float* logp, int64_t ldlogp,
                                   const int32_t* win, int64_t* codes, int64_t ldc, int N, const float* table,
                                   int64_t table_rows, int d, float* next_in, int64_t ldn, float* probs, int64_t ldp,
                                   int32_t* pos, int32_t* ticket, void* stream) {
    VQ_REQUIRE(V >= 1 && V <= prior::kMaxVocab, "prior_sample_constrained: %d codes (1 <= V <= 4096)", V);
    VQ_REQUIRE(M >= 1 && M <= prior::kMaxRows, "prior_sample_constrained: %lld rows (1 <= M <= 64)", (long long)M);
    VQ_REQUIRE(logits && codes && table && next_in && pos && ticket, "prior_sample_constrained: null pointer");
    VQ_REQUIRE(seeds, "prior_sample_constrained: seeds are needed (a position the constraint leaves free is drawn)");
    VQ_REQUIRE(N >= 1 && N <= prior::kMaxWindow && d >= 1 && d <= prior::kMaxDim,
               "prior_sample_constrained: bad arguments (1 <= N <= 1024, 1 <= d <= 4096)");
    VQ_REQUIRE(temperature > 0.0f && top_k >= 0 && top_p == top_p, "prior_sample_constrained: temperature > 0, top_k >= 0");
    VQ_REQUIRE(ldl >= V && ldc >= N && ldn >= d && (!constraint || ldcons >= N) && (!logp || ldlogp >= N) &&
               (!probs || ldp >= V) && table_rows >= V,
               "prior_sample_constrained: bad leading dimensions (ldcons, ldlogp >= N), or a table of fewer than V rows");
    hipLaunchKernelGGL(prior::prior_sample_kernel<true>, dim3((unsigned)M), dim3(prior::kThreads), 0, (hipStream_t)stream,
                       logits, ldl, V, temperature, top_k, top_p, seeds, constraint, ldcons, codes, ldc, N, table, d, next_in,
                       ldn, probs, ldp, pos, ticket, logp, ldlogp, win, prior::NoStage{});
    VQ_CHECK_LAUNCH("prior_sample_constrained");
    return VQCPC_OK;
}

int vqcpc_prior_sample_masked(const float* logits, int64_t ldl, int V, int64_t M, float temperature, int top_k, float top_p,
                              const int64_t* seeds, const int64_t* constraint, int64_t ldcons, float* logp, int64_t ldlogp,
                              const int32_t* win, const uint32_t* allowed, int64_t ldallow, float* logmass, int64_t ldmass,
                              int64_t* codes, int64_t ldc, int N, const float* table, int64_t table_rows, int d, float* next_in,
                              int64_t ldn, float* probs, int64_t ldp, int32_t* pos, int32_t* ticket, void* stream) {
    VQ_REQUIRE(V >= 1 && V <= prior::kMaxVocab, "prior_sample_masked: %d codes (1 <= V <= 4096)", V);
    VQ_REQUIRE(M >= 1 && M <= prior::kMaxRows, "prior_sample_masked: %lld rows (1 <= M <= 64)", (long long)M);
    VQ_REQUIRE(logits && codes && table && next_in && pos && ticket, "prior_sample_masked: null pointer");
    VQ_REQUIRE(seeds, "prior_sample_masked: seeds are needed (a position the constraint leaves free is drawn)");
    VQ_REQUIRE(N >= 1 && N <= prior::kMaxWindow && d >= 1 && d <= prior::kMaxDim,
               "prior_sample_masked: bad arguments (1 <= N <= 1024, 1 <= d <= 4096)");
    VQ_REQUIRE(temperature > 0.0f && top_k >= 0 && top_p == top_p, "prior_sample_masked: temperature > 0, top_k >= 0");
    VQ_REQUIRE(ldl >= V && ldc >= N && ldn >= d && (!constraint || ldcons >= N) && (!logp || ldlogp >= N) &&
               (!probs || ldp >= V) && table_rows >= V,
               "prior_sample_masked: bad leading dimensions (ldcons, ldlogp >= N), or a table of fewer than V rows");
    VQ_REQUIRE((!allowed || ldallow >= N) && (!logmass || ldmass >= N), "prior_sample_masked: bad leading dimensions (ldallow, ldmass >= N)");
    const prior::MaskedNoStage ps{{}, {allowed, ldallow, logmass, ldmass, nullptr}};
    hipLaunchKernelGGL((prior::prior_sample_kernel<true, false, true>), dim3((unsigned)M), dim3(prior::kThreads), 0,
                       (hipStream_t)stream, logits, ldl, V, temperature, top_k, top_p, seeds, constraint, ldcons, codes, ldc, N,
                       table, d, next_in, ldn, probs, ldp, pos, ticket, logp, ldlogp, win, ps);
    VQ_CHECK_LAUNCH("prior_sample_masked");
    return VQCPC_OK;
}

int vqcpc_prior_window(int64_t* seq, int64_t ldseq, int64_t num_tokens, int32_t* win, int advance, int64_t* codes_win, int N,
                       int P, int64_t* prefix_rows, const float* table, int64_t table_rows, int d, float* x, int64_t ldx,
                       const int64_t* seeds_in, int64_t* seeds_out, int32_t* pos, int64_t M, void* stream) {
    VQ_REQUIRE(M >= 1 && M <= prior::kMaxRows, "prior_window: %lld rows (1 <= M <= 64)", (long long)M);
    VQ_REQUIRE(seq && win && codes_win && table && x && seeds_in && seeds_out && pos, "prior_window: null pointer");
    VQ_REQUIRE(N >= 1 && N <= prior::kMaxWindow && num_tokens >= N && ldseq >= num_tokens && P >= 0 && P < N &&
               (P == 0 || prefix_rows) && d >= 1 && d <= prior::kMaxDim && ldx >= d && table_rows >= 2 && advance >= 0,
               "prior_window: 1 <= N <= 1024, num_tokens >= N, ldseq >= num_tokens, 0 <= P < N, 1 <= d <= 4096");
    hipLaunchKernelGGL(prior::prior_window_kernel<false>, dim3(1), dim3(1024), 0, (hipStream_t)stream, seq, ldseq, num_tokens, win,
                       advance, codes_win, N, P, prefix_rows, table, table_rows, d, x, ldx, seeds_in, seeds_out, pos, (int)M,
                       (const float*)nullptr, 0, 0);
    VQ_CHECK_LAUNCH("prior_window");
    return VQCPC_OK;
}

}  // extern "C"
