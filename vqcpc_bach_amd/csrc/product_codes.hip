// Product codes downstream of the encoder (include/vqcpc.h, the "Product codes" section; ops.ProductEmbeddingFn is the caller).
// A merged code is ncb digits of K values, digit j = (code / K^j) % K (Encoder.merge_codes), and its embedding the sum of one
// row per codebook: no table of K^ncb rows exists anywhere.
//   * product_gather: one thread per float4 of an output row, as block_table_gather.  The digits come from 32-bit divisions by K
//     (V + n_extra < 2^31); the rows are added left to right, every add a separately rounded fp32 add (no multiply is near them, so
//     nothing can be contracted), starting at the residual when there is one and at the first table row otherwise.
//   * product_gather_bwd: the scheme of embedding_bwd (embed_ln.hip) over the (row, codebook) pairs.  The caller sorts the keys
//     j * K + digit_j (ncb * K + e for start-of-sentence row e) with ONE stable sort; the workgroup at the first position of a run
//     sums the run's rows of g in that order, i.e. in ascending m -- deterministic, no atomics; rows nobody refers to keep the zero
//     fill.
//   * prior_sample_product / prior_window_product: the prior's sampler and window kernels (prior_kernels.h) instantiated with their
//     PROD flag -- one stage (digit) of a step's tail per launch, and the window move with the product row rule.  One codebook is
//     the merged kernels bit for bit.
// Plain C++: vector loads and stores only.
#include <algorithm>

#include "prior_kernels.h"

namespace vq {

constexpr int kProductMaxBooks = 4;
constexpr int kProductMaxK = 4096;

__global__ __launch_bounds__(256) void product_gather_kernel(const float* __restrict__ tables, const int64_t* __restrict__ idx,
                                                             const float* __restrict__ res, int64_t ldr4,
                                                             const float* __restrict__ extra, float* __restrict__ out,
                                                             int64_t ldo4, int64_t M, int nj, int K, int64_t V, int C4) {
    const int64_t total = M * C4;
    const float4* t4 = reinterpret_cast<const float4*>(tables);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / C4;
        const int c = (int)(e - r * C4);
        const int64_t id = idx[r];
        float4 acc;
        if (id >= V) {                                                    // start-of-sentence rows follow the V codes
            acc = reinterpret_cast<const float4*>(extra)[(id - V) * C4 + c];
        } else {
            uint32_t q = (uint32_t)id;
            acc = t4[(int64_t)(q % (uint32_t)K) * C4 + c];
            if (res) {
                const float4 h = reinterpret_cast<const float4*>(res)[r * ldr4 + c];
                acc = make_float4(h.x + acc.x, h.y + acc.y, h.z + acc.z, h.w + acc.w);
            }
            for (int j = 1; j < nj; ++j) {
                q /= (uint32_t)K;
                const float4 t = t4[((int64_t)j * K + q % (uint32_t)K) * C4 + c];
                acc = make_float4(acc.x + t.x, acc.y + t.y, acc.z + t.z, acc.w + t.w);
            }
        }
        reinterpret_cast<float4*>(out)[r * ldo4 + c] = acc;
    }
}

// One workgroup per sorted (row, codebook) pair; all but the first of a run of equal keys leave at once.  perm[s] % M is the row
// of g the pair stands for (the caller sorts the flattened [nj][M] key array).  Keys >= n_rows belong to nobody: the digits
// j >= 1 of a start-of-sentence row.
__global__ __launch_bounds__(256) void product_gather_bwd_kernel(const float* __restrict__ g, int64_t ldg,
                                                                 const int64_t* __restrict__ sorted_keys,
                                                                 const int64_t* __restrict__ perm, float* __restrict__ d_tables,
                                                                 float* __restrict__ d_extra, int64_t M, int64_t S,
                                                                 int64_t n_table_rows, int64_t n_rows, int C) {
    constexpr int U = 8;                                              // rows in flight per lane; added in ascending order
    const int64_t s = blockIdx.x;
    const int64_t v = sorted_keys[s];
    if (v < 0 || v >= n_rows || (s > 0 && sorted_keys[s - 1] == v)) return;
    int64_t lo = s, hi = S;                                           // end of the run: first position whose key differs
    while (lo + 1 < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sorted_keys[mid] == v) lo = mid; else hi = mid;
    }
    const int64_t end = hi;
    float* dst = v < n_table_rows ? d_tables + v * C : d_extra + (v - n_table_rows) * C;
    for (int col = threadIdx.x; col < C; col += 256) {
        float acc = 0.0f;
        for (int64_t ss = s; ss < end; ss += U) {
            float x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = ss + u < end ? g[(perm[ss + u] % M) * ldg + col] : 0.0f;
#pragma unroll
            for (int u = 0; u < U; ++u) acc += x[u];
        }
        dst[col] = acc;
    }
}

static bool product_shape_ok(int ncb, int K, int n_extra) {
    if (ncb < 1 || ncb > kProductMaxBooks || K < 1 || K > kProductMaxK || n_extra < 0) return false;
    int64_t V = 1;
    for (int j = 0; j < ncb; ++j) V *= K;                            // <= 2^48
    return V + n_extra < (int64_t)1 << 31;
}

}  // namespace vq

using namespace vq;

int vqcpc_product_gather(const float* tables, const int64_t* idx, const float* res, int64_t ldr, const float* extra, int n_extra,
                         float* out, int64_t ldo, int64_t M, int ncb, int K, int nj, int C, void* stream) {
    VQ_REQUIRE(product_shape_ok(ncb, K, n_extra), "product_gather: need 1 <= ncb <= 4, 1 <= K <= 4096, K^ncb + n_extra < 2^31");
    VQ_REQUIRE(nj >= 1 && nj <= ncb && M >= 0 && C >= 4 && C % 4 == 0 && ldo >= C && ldo % 4 == 0, "product_gather: bad shape");
    VQ_REQUIRE(!res || (ldr >= C && ldr % 4 == 0), "product_gather: bad residual stride");
    VQ_REQUIRE(!(res && extra) && (extra != nullptr) == (n_extra > 0), "product_gather: res and extra exclude each other, extra goes with n_extra > 0");
    if (M == 0) return VQCPC_OK;
    VQ_REQUIRE(tables && idx && out, "product_gather: null pointer");
    VQ_REQUIRE(aligned16(tables) && aligned16(out) && aligned16(res) && aligned16(extra), "product_gather: buffers must be 16-byte aligned");
    int64_t V = 1;
    for (int j = 0; j < ncb; ++j) V *= K;
    const int blocks = (int)std::min<int64_t>(ceil_div(M * (C / 4), 256), 16384);
    hipLaunchKernelGGL(product_gather_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, tables, idx, res, ldr / 4, extra, out,
                       ldo / 4, M, nj, K, V, C / 4);
    VQ_CHECK_LAUNCH("product_gather");
    return VQCPC_OK;
}

int vqcpc_product_gather_bwd(const float* g, int64_t ldg, const int64_t* sorted_keys, const int64_t* perm, float* d_tables,
                             float* d_extra, int64_t M, int64_t S, int ncb, int K, int n_extra, int C, void* stream) {
    VQ_REQUIRE(product_shape_ok(ncb, K, n_extra), "product_gather_bwd: need 1 <= ncb <= 4, 1 <= K <= 4096, K^ncb + n_extra < 2^31");
    VQ_REQUIRE(d_tables && C >= 1 && M >= 0 && S >= 0 && (d_extra != nullptr) == (n_extra > 0), "product_gather_bwd: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_tables, 0, (size_t)ncb * K * C * sizeof(float), s) != hipSuccess ||
        (d_extra && hipMemsetAsync(d_extra, 0, (size_t)n_extra * C * sizeof(float), s) != hipSuccess)) {
        set_error("product_gather_bwd: memset failed");
        return VQCPC_ELAUNCH;
    }
    if (M == 0 || S == 0) return VQCPC_OK;
    VQ_REQUIRE(g && sorted_keys && perm && ldg >= C && S < (int64_t)1 << 31, "product_gather_bwd: bad arguments");
    hipLaunchKernelGGL(product_gather_bwd_kernel, dim3((unsigned)S), dim3(256), 0, s, g, ldg, sorted_keys, perm, d_tables, d_extra, M,
                       S, (int64_t)ncb * K, (int64_t)ncb * K + n_extra, C);
    VQ_CHECK_LAUNCH("product_gather_bwd");
    return VQCPC_OK;
}

// the checks the two product samplers share; `name` is the entry point's
static int product_stage_check(const char* name, const float* logits, int64_t ldl, int K, int ncb, int stage, int64_t M,
                               float temperature, int top_k, float top_p, const int64_t* seeds, const int64_t* teacher,
                               int64_t ldteach, const int64_t* constraint, int64_t ldcons, float* logp, int64_t ldlogp,
                               int32_t* digits, float* logp_acc, const float* h, int64_t ldh, const float* dtab, float* h_next,
                               int64_t ldhn, int64_t* codes, int64_t ldc, int N, const float* tables, int d, float* next_in,
                               int64_t ldn, float* probs, int64_t ldp, int32_t* pos, int32_t* ticket) {
    VQ_REQUIRE(product_shape_ok(ncb, K, 1), "%s: need 1 <= ncb <= 4, 1 <= K <= 4096, K^ncb + 1 < 2^31", name);
    VQ_REQUIRE(stage >= 0 && stage < ncb, "%s: stage %d of %d", name, stage, ncb);
    VQ_REQUIRE(M >= 1 && M <= prior::kMaxRows, "%s: %lld rows (1 <= M <= 64)", name, (long long)M);
    VQ_REQUIRE(logits && seeds && pos && ticket, "%s: null pointer", name);
    VQ_REQUIRE(N >= 1 && N <= prior::kMaxWindow && d >= 1 && d <= prior::kMaxDim,
               "%s: bad arguments (1 <= N <= 1024, 1 <= d <= 4096)", name);
    VQ_REQUIRE(temperature > 0.0f && top_k >= 0 && top_p == top_p, "%s: temperature > 0, top_k >= 0", name);
    VQ_REQUIRE(!(teacher && (constraint || logp)), "%s: teacher excludes constraint and logp", name);
    VQ_REQUIRE(ldl >= K && (!teacher || ldteach >= N) && (!constraint || ldcons >= N) && (!logp || ldlogp >= N) && (!probs || ldp >= K),
               "%s: bad leading dimensions (ldl, ldp >= K; ldteach, ldcons, ldlogp >= N)", name);
    VQ_REQUIRE(ncb == 1 || (digits && (!logp || logp_acc)), "%s: the digit and log-probability scratch is needed", name);
    if (stage < ncb - 1)
        VQ_REQUIRE(h && dtab && h_next && ldh >= d && ldhn >= d, "%s: an earlier stage needs h, dtab, h_next", name);
    else
        VQ_REQUIRE(codes && tables && next_in && ldc >= N && ldn >= d, "%s: the last stage needs codes, tables, next_in", name);
    return VQCPC_OK;
}

int vqcpc_prior_sample_product(const float* logits, int64_t ldl, int K, int ncb, int stage, int64_t M, float temperature, int top_k,
                               float top_p, const int64_t* seeds, const int64_t* teacher, int64_t ldteach,
                               const int64_t* constraint, int64_t ldcons, float* logp, int64_t ldlogp, const int32_t* win,
                               int32_t* digits, float* logp_acc, const float* h, int64_t ldh, const float* dtab, float* h_next,
                               int64_t ldhn, int64_t* codes, int64_t ldc, int N, const float* tables, int d, float* next_in,
                               int64_t ldn, float* probs, int64_t ldp, int32_t* pos, int32_t* ticket, void* stream) {
    const int rc = product_stage_check("prior_sample_product", logits, ldl, K, ncb, stage, M, temperature, top_k, top_p, seeds, teacher,
                                       ldteach, constraint, ldcons, logp, ldlogp, digits, logp_acc, h, ldh, dtab, h_next, ldhn, codes,
                                       ldc, N, tables, d, next_in, ldn, probs, ldp, pos, ticket);
    if (rc != VQCPC_OK) return rc;
    const prior::ProductStage ps{stage, ncb, teacher, ldteach, digits, logp_acc, h, ldh, dtab, h_next, ldhn};
    hipLaunchKernelGGL((prior::prior_sample_kernel<true, true>), dim3((unsigned)M), dim3(prior::kThreads), 0, (hipStream_t)stream,
                       logits, ldl, K, temperature, top_k, top_p, seeds, constraint, ldcons, codes, ldc, N, tables, d, next_in, ldn,
                       probs, ldp, pos, ticket, logp, ldlogp, win, ps);
    VQ_CHECK_LAUNCH("prior_sample_product");
    return VQCPC_OK;
}

int vqcpc_prior_sample_product_masked(const float* logits, int64_t ldl, int K, int ncb, int stage, int64_t M, float temperature,
                                      int top_k, float top_p, const int64_t* seeds, const int64_t* teacher, int64_t ldteach,
                                      const int64_t* constraint, int64_t ldcons, float* logp, int64_t ldlogp, const int32_t* win,
                                      const uint32_t* allowed, int64_t ldallow, float* logmass, int64_t ldmass, int32_t* digits,
                                      float* logp_acc, float* mass_acc, const float* h, int64_t ldh, const float* dtab,
                                      float* h_next, int64_t ldhn, int64_t* codes, int64_t ldc, int N, const float* tables, int d,
                                      float* next_in, int64_t ldn, float* probs, int64_t ldp, int32_t* pos, int32_t* ticket,
                                      void* stream) {
    const int rc = product_stage_check("prior_sample_product_masked", logits, ldl, K, ncb, stage, M, temperature, top_k, top_p, seeds,
                                       teacher, ldteach, constraint, ldcons, logp, ldlogp, digits, logp_acc, h, ldh, dtab, h_next,
                                       ldhn, codes, ldc, N, tables, d, next_in, ldn, probs, ldp, pos, ticket);
    if (rc != VQCPC_OK) return rc;
    VQ_REQUIRE(!(teacher && (allowed || logmass)), "prior_sample_product_masked: teacher excludes allowed and logmass");
    VQ_REQUIRE((!allowed || ldallow >= N) && (!logmass || ldmass >= N),
               "prior_sample_product_masked: bad leading dimensions (ldallow, ldmass >= N)");
    VQ_REQUIRE(ncb == 1 || !logmass || mass_acc, "prior_sample_product_masked: the log-mass scratch is needed");
    const prior::MaskedProductStage ps{{stage, ncb, teacher, ldteach, digits, logp_acc, h, ldh, dtab, h_next, ldhn},
                                       {allowed, ldallow, logmass, ldmass, mass_acc}};
    hipLaunchKernelGGL((prior::prior_sample_kernel<true, true, true>), dim3((unsigned)M), dim3(prior::kThreads), 0,
                       (hipStream_t)stream, logits, ldl, K, temperature, top_k, top_p, seeds, constraint, ldcons, codes, ldc, N,
                       tables, d, next_in, ldn, probs, ldp, pos, ticket, logp, ldlogp, win, ps);
    VQ_CHECK_LAUNCH("prior_sample_product_masked");
    return VQCPC_OK;
}

int vqcpc_prior_window_product(int64_t* seq, int64_t ldseq, int64_t num_tokens, int32_t* win, int advance, int64_t* codes_win,
                               int N, int P, int64_t* prefix_rows, const float* tables, int ncb, int K, const float* sos, int d,
                               float* x, int64_t ldx, const int64_t* seeds_in, int64_t* seeds_out, int32_t* pos, int64_t M,
                               void* stream) {
    VQ_REQUIRE(product_shape_ok(ncb, K, 1), "prior_window_product: need 1 <= ncb <= 4, 1 <= K <= 4096, K^ncb + 1 < 2^31");
    VQ_REQUIRE(M >= 1 && M <= prior::kMaxRows, "prior_window_product: %lld rows (1 <= M <= 64)", (long long)M);
    VQ_REQUIRE(seq && win && codes_win && tables && sos && x && seeds_in && seeds_out && pos, "prior_window_product: null pointer");
    VQ_REQUIRE(N >= 1 && N <= prior::kMaxWindow && num_tokens >= N && ldseq >= num_tokens && P >= 0 && P < N &&
               (P == 0 || prefix_rows) && d >= 1 && d <= prior::kMaxDim && ldx >= d && advance >= 0,
               "prior_window_product: 1 <= N <= 1024, num_tokens >= N, ldseq >= num_tokens, 0 <= P < N, 1 <= d <= 4096");
    int64_t V = 1;
    for (int j = 0; j < ncb; ++j) V *= K;
    hipLaunchKernelGGL(prior::prior_window_kernel<true>, dim3(1), dim3(1024), 0, (hipStream_t)stream, seq, ldseq, num_tokens, win,
                       advance, codes_win, N, P, prefix_rows, tables, V + 1, d, x, ldx, seeds_in, seeds_out, pos, (int)M, sos, K, ncb);
    VQ_CHECK_LAUNCH("prior_window_product");
    return VQCPC_OK;
}
