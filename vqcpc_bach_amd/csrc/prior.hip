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
//   * vqcpc_prior_window: ONE workgroup.  Commits the live window's codes into the sequence, loads the next window, the
//     prefix's table-row indices, the input row of position P, the window's seeds and `pos`.
#include "common.h"

namespace vq {
namespace prior {

constexpr int kMaxRows = 64;
constexpr int kMaxDim = 4096;
constexpr int kMaxVocab = 4096;
constexpr int kMaxWindow = 1024;
constexpr int kThreads = 256;
constexpr int kPer = kMaxVocab / kThreads;               // 16 tokens per thread
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// order-preserving map float -> uint32 (a < b  <=>  key(a) < key(b); -inf is the smallest key of a non-NaN value).  -0.0 takes
// the key of +0.0: the two compare equal as floats (the reference's `logits < kth`, utils.py:113, keeps a -0.0 next to a k-th
// largest +0.0), and their bit patterns would order them strictly
__device__ __forceinline__ uint32_t float_key(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// block reductions over 4 wavefronts in a fixed order; `red` holds kWaves entries
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ int block_sum_int(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ int block_min_int(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return min(min(red[0], red[1]), min(red[2], red[3]));
}
__device__ __forceinline__ int block_max_int(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return max(max(red[0], red[1]), max(red[2], red[3]));
}
// sum over the block: wave butterfly, then the four waves' totals pairwise
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// exclusive prefix of the threads' totals in thread order (wave scan, then the previous waves' totals in wave order);
// `total` receives the sum over the block
__device__ __forceinline__ float block_excl_scan(float v, float* red, float& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    __syncthreads();
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    float base = 0.0f, all = 0.0f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) base += red[w];
        all += red[w];
    }
    total = all;
    return base + incl - v;
}

// CONS (vqcpc_prior_sample_constrained): `teacher` is the constraint -- per (row, column) a code to emit, or < 0 for a draw --
// and the emitted code's log-probability under the UNFILTERED row (temperature 1) goes to logp.  Both are addressed at the
// sequence column col = pos (win == NULL) or win[1] + pos, the live window's first code plus the position: one captured step
// and one captured move serve every window.  A column outside [0, ldteach) / [0, ldlogp) is free / not written.  The
// log-sum-exp re-reads the row from global memory: thread t sums its 16 codes in ascending order, then `block_sum` -- an order
// that depends on V only.  Without CONS the kernel is what it was before the flag: none of the added code is instantiated.
template <bool CONS>
__global__ __launch_bounds__(kThreads) void prior_sample_kernel(
    const float* __restrict__ logits, int64_t ldl, int V, float temperature, int top_k, float top_p,
    const int64_t* __restrict__ seeds, const int64_t* __restrict__ teacher, int64_t ldteach, int64_t* __restrict__ codes,
    int64_t ldc, int N, const float* __restrict__ table, int d, float* __restrict__ next_in, int64_t ldn,
    float* __restrict__ probs, int64_t ldp, int32_t* __restrict__ posp, int32_t* __restrict__ ticket,
    float* __restrict__ logp, int64_t ldlogp, const int32_t* __restrict__ win) {
    __shared__ float sl[kMaxVocab];                           // the row's (filtered) logits
    __shared__ uint64_t keys[kMaxVocab];                      // top-p: (descending logit, index) sort keys
    __shared__ float redf[kWaves];
    __shared__ int redi[kWaves];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int M = gridDim.x;
    const int pos = *posp;
    if (pos < 0 || pos >= N) return;                         // past the end: nothing happens (uniform over the grid)
    const float ninf = -INFINITY;
    int64_t col = -1;                                         // CONS: the column of constraint / logp, < 0 = no live window
    if constexpr (CONS) {
        const int w0 = win ? win[1] : 0;
        if (w0 >= 0) col = (int64_t)w0 + pos;
    }
    for (int i = tid; i < kMaxVocab; i += kThreads) sl[i] = i < V ? logits[b * ldl + i] * temperature : ninf;
    __syncthreads();
    const int i0 = tid * kPer;
    float l[kPer];
#pragma unroll
    for (int t = 0; t < kPer; ++t) l[t] = sl[i0 + t];
    // top-k (utils.py:111-114): drop logits < the k-th largest.  Its key is the largest T with #{key >= T} >= k, found bit
    // by bit from the top (integer counts: no order dependence)
    if (top_k > 0 && top_k < V) {
        uint32_t k32[kPer];
#pragma unroll
        for (int t = 0; t < kPer; ++t) k32[t] = float_key(l[t]);
        uint32_t thr = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = thr | (1u << bit);
            int cnt = 0;
#pragma unroll
            for (int t = 0; t < kPer; ++t) cnt += (i0 + t < V) & (k32[t] >= cand);
            if (block_sum_int(cnt, redi) >= top_k) thr = cand;
        }
#pragma unroll
        for (int t = 0; t < kPer; ++t)
            if (k32[t] < thr) l[t] = ninf;
    }
    // top-p (utils.py:116-126): softmax over the sorted survivors, drop entries whose cumulative probability BEFORE them
    // exceeds top_p (the shift by one), the first is always kept
    if (top_p > 0.0f && top_p < 1.0f) {
        int n2 = 64;
        while (n2 < V) n2 <<= 1;                             // <= 4096
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kPer; ++t) {
            const int i = i0 + t;
            sl[i] = l[t];
            // ascending sort of (~key, index): descending logits, equal logits by ascending index; the padding sorts last
            keys[i] = i < V ? ((uint64_t)(~float_key(l[t])) << 32) | (uint32_t)i : ~0ull;
        }
        __syncthreads();
        for (int k = 2; k <= n2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < n2; i += kThreads) {
                    const int p = i ^ j;
                    if (p > i) {
                        const uint64_t a = keys[i], c = keys[p];
                        const bool up = (i & k) == 0;
                        if ((a > c) == up) {
                            keys[i] = c;
                            keys[p] = a;
                        }
                    }
                }
                __syncthreads();
            }
        }
        float mx = ninf;
#pragma unroll
        for (int t = 0; t < kPer; ++t) mx = fmaxf(mx, l[t]);
        mx = block_max(mx, redf);
        // thread t owns the sorted positions 16t .. 16t + 15
        float e[kPer], run = 0.0f;
        int idx[kPer];
#pragma unroll
        for (int t = 0; t < kPer; ++t) {
            const uint64_t kk = keys[i0 + t];
            idx[t] = (i0 + t < V) ? (int)(uint32_t)kk : -1;
            const float v = idx[t] >= 0 ? sl[idx[t]] : ninf;
            e[t] = v > ninf ? expf(v - mx) : 0.0f;
            run += e[t];
        }
        float total;
        float before = block_excl_scan(run, redf, total);   // sum of the weights sorted before this thread's first
        const float lim = top_p * total;                     // cum / total > top_p
        __syncthreads();                                     // every thread has read sl through its sorted indices
#pragma unroll
        for (int t = 0; t < kPer; ++t) {
            if (idx[t] >= 0 && i0 + t >= 1 && before > lim) sl[idx[t]] = ninf;
            before += e[t];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kPer; ++t) l[t] = sl[i0 + t];
    }
    // softmax of the filtered row and one draw: the first token whose inclusive cumulative weight exceeds u * total
    float mx = ninf;
#pragma unroll
    for (int t = 0; t < kPer; ++t) mx = fmaxf(mx, l[t]);
    mx = block_max(mx, redf);
    float e[kPer], cum[kPer], run = 0.0f;
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        e[t] = l[t] > ninf ? expf(l[t] - mx) : 0.0f;
        run += e[t];
        cum[t] = run;
    }
    float total;
    const float base = block_excl_scan(run, redf, total);
    if (probs) {
        const float inv = 1.0f / total;
#pragma unroll
        for (int t = 0; t < kPer; ++t)
            if (i0 + t < V) probs[b * ldp + i0 + t] = e[t] * inv;
    }
    int tok;
    int64_t forced = -1;
    if constexpr (CONS) {
        if (teacher && col >= 0 && col < ldteach) forced = teacher[b * ldteach + col];
    }
    if (CONS ? forced >= 0 : teacher != nullptr) {           // uniform over the workgroup
        tok = CONS ? (int)min(forced, (int64_t)kMaxVocab) : (int)teacher[b * ldteach + pos];
    } else {
        const uint64_t sd = (uint64_t)seeds[b];
        const uint32_t r = rng_u24_from_x0(rng_x0(sd, (uint32_t)pos), (uint32_t)(sd >> 32));
        const float target = ((float)r + 0.5f) * (1.0f / 16777216.0f) * total;
        int first = 1 << 30, last = -1;
#pragma unroll
        for (int t = 0; t < kPer; ++t) {
            if (e[t] > 0.0f) {
                if (first == (1 << 30) && base + cum[t] > target) first = i0 + t;
                last = i0 + t;
            }
        }
        first = block_min_int(first, redi);
        last = block_max_int(last, redi);
        tok = first < (1 << 30) ? first : last;              // u * total rounded up to total: the last token of weight
    }
    tok = min(max(tok, 0), V - 1);
    if (tid == 0) codes[b * ldc + pos] = tok;
    for (int k = tid; k < d; k += kThreads) next_in[b * ldn + k] = table[(int64_t)tok * d + k];   // input of position pos + 1
    if constexpr (CONS) {
        if (logp && col >= 0 && col < ldlogp) {              // uniform: every thread reaches the barriers below or none does
            float raw[kPer], rmx = ninf;
#pragma unroll
            for (int t = 0; t < kPer; ++t) {
                raw[t] = i0 + t < V ? logits[b * ldl + i0 + t] : ninf;     // the row as the model gave it
                rmx = fmaxf(rmx, raw[t]);
            }
            rmx = block_max(rmx, redf);
            float rs = 0.0f;
#pragma unroll
            for (int t = 0; t < kPer; ++t) rs += raw[t] > ninf ? expf(raw[t] - rmx) : 0.0f;
            rs = block_sum(rs, redf);
            if (tid == 0) logp[b * ldlogp + col] = (logits[b * ldl + tok] - rmx) - logf(rs);
        }
    }
    // the last workgroup to get here advances the position: every workgroup read it before it took its ticket
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        const int done = atomicAdd(ticket, 1);
        if (done == M - 1) {
            *ticket = 0;
            *posp = pos + 1;
        }
    }
}

__global__ __launch_bounds__(1024) void prior_window_kernel(int64_t* __restrict__ seq, int64_t ldseq, int64_t nt,
                                                            int32_t* __restrict__ win, int advance,
                                                            int64_t* __restrict__ codes_win, int N, int P,
                                                            int64_t* __restrict__ prefix_rows, const float* __restrict__ table,
                                                            int64_t table_rows, int d, float* __restrict__ x, int64_t ldx,
                                                            const int64_t* __restrict__ seeds_in,
                                                            int64_t* __restrict__ seeds_out, int32_t* __restrict__ posp, int M) {
    const int tid = threadIdx.x;
    const int next = win[0], live = win[1], cur = min(max(*posp, 0), N);
    __syncthreads();                                         // every thread has read win and pos
    if (live >= 0 && (int64_t)live + N <= nt) {              // commit: the live window's codes [0, pos) into the sequence
        for (int e = tid; e < M * cur; e += 1024) {
            const int m = e / cur, j = e % cur;
            seq[(int64_t)m * ldseq + live + j] = codes_win[(int64_t)m * N + j];
        }
    }
    __threadfence_block();
    __syncthreads();                                         // the load below reads what the commit wrote
    if (next < 0 || (int64_t)next + N > nt) return;          // commit only (uniform)
    const int64_t sos = table_rows - 1;
    for (int e = tid; e < M * N; e += 1024) {
        const int m = e / N, j = e % N;
        const int64_t code = seq[(int64_t)m * ldseq + next + j];
        codes_win[e] = code;
        if (j + 1 < P) prefix_rows[(int64_t)m * P + j + 1] = min(max(code, (int64_t)0), sos - 1);   // input of position j + 1
    }
    for (int m = tid; m < M; m += 1024) {
        if (P > 0) prefix_rows[(int64_t)m * P] = sos;
        const uint64_t sd = (uint64_t)seeds_in[m];
        // window 0 keeps the row's seed (the head regime); the rule of vqcpc_decode_window
        seeds_out[m] = (int64_t)(next == 0 ? sd : splitmix64(sd ^ ((uint64_t)next * 0xD1B54A32D192ED03ull)));
    }
    for (int e = tid; e < M * d; e += 1024) {                // the input row of position P
        const int m = e / d, c = e % d;
        int64_t row = sos;
        if (P > 0) row = min(max(seq[(int64_t)m * ldseq + next + P - 1], (int64_t)0), sos - 1);
        x[(int64_t)m * ldx + c] = table[row * d + c];
    }
    if (tid == 0) {
        *posp = P;
        win[0] = next + advance;
        win[1] = next;
    }
}

}  // namespace prior
}  // namespace vq

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
                       probs, ldp, pos, ticket, (float*)nullptr, (int64_t)0, (const int32_t*)nullptr);
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
                       ldn, probs, ldp, pos, ticket, logp, ldlogp, win);
    VQ_CHECK_LAUNCH("prior_sample_constrained");
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
    hipLaunchKernelGGL(prior::prior_window_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, seq, ldseq, num_tokens, win,
                       advance, codes_win, N, P, prefix_rows, table, table_rows, d, x, ldx, seeds_in, seeds_out, pos, (int)M);
    VQ_CHECK_LAUNCH("prior_window");
    return VQCPC_OK;
}

}  // extern "C"
