// The prior's sampling and window kernels, shared by csrc/prior.hip (the merged code as one symbol: vqcpc_prior_sample,
// vqcpc_prior_sample_constrained, vqcpc_prior_window -- that file's header describes them) and csrc/product_codes.hip (the merged
// code digit by digit: vqcpc_prior_sample_product, vqcpc_prior_window_product).  ONE kernel body each; the product forms are
// compile-time flags (PROD), so that a product code of ONE codebook is the merged code's kernel instruction for instruction, and
// without PROD the kernels are what they were before the flag: none of the added code is instantiated.  The masked forms
// (vqcpc_prior_sample_masked, vqcpc_prior_sample_product_masked) are one more flag of the sampler, MASK, under the same rule.
#pragma once

#include <type_traits>

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

// PROD: what one stage of a product code's step needs on top of the merged sampler's arguments (include/vqcpc.h,
// vqcpc_prior_sample_product).  The kernel's `V` is then K, its `logits` the stage's, its `table` the input tables [ncb][K][d].
struct ProductStage {
    int stage, ncb;
    const int64_t* teacher;        // (M, ldteach) merged codes to force at the window position, or NULL
    int64_t ldteach;
    int32_t* digits;               // [M][ncb] scratch: the digits the earlier stages of this position emitted
    float* logp_acc;               // [M] scratch: the sum of the earlier stages' log-probabilities
    const float* h;                // (M, ldh) what this stage's head read
    int64_t ldh;
    const float* dtab;             // [ncb - 1][K][d] digit-conditioning rows
    float* h_next;                 // (M, ldhn) what the next stage's head reads
    int64_t ldhn;
};
struct NoStage {};

// MASK: what vqcpc_prior_sample_masked / vqcpc_prior_sample_product_masked add (include/vqcpc.h).  The arguments ride behind the
// stage's in the kernel's LAST parameter, so the three instantiations without MASK keep their argument layout.
struct MaskArgs {
    const uint32_t* allowed;       // [M][ldallow][words] (PROD: [M][ldallow][ncb][words]), words = ceil(V / 32), or NULL
    int64_t ldallow;
    float* logmass;                // (M, ldmass), or NULL
    int64_t ldmass;
    float* mass_acc;               // PROD: [M] scratch, the sum of the earlier stages' log-masses
};
struct MaskedNoStage : NoStage {
    MaskArgs mk;
};
struct MaskedProductStage : ProductStage {
    MaskArgs mk;
};
template <bool PROD, bool MASK>
using SampleExtra = std::conditional_t<MASK, std::conditional_t<PROD, MaskedProductStage, MaskedNoStage>,
                                       std::conditional_t<PROD, ProductStage, NoStage>>;

// the draw key of stage j: stage 0 draws with the row's seed, as the merged sampler; a later stage with a seed derived from it
// and j alone (the constant differs from the window rule's, so no (window, stage) pair shares a key with another)
__device__ __forceinline__ uint64_t stage_seed(uint64_t sd, int stage) {
    return stage == 0 ? sd : splitmix64(sd ^ ((uint64_t)stage * 0xA0761D6478BD642Full));
}

// CONS (vqcpc_prior_sample_constrained): `teacher` is the constraint -- per (row, column) a code to emit, or < 0 for a draw --
// and the emitted code's log-probability under the UNFILTERED row (temperature 1) goes to logp.  Both are addressed at the
// sequence column col = pos (win == NULL) or win[1] + pos, the live window's first code plus the position: one captured step
// and one captured move serve every window.  A column outside [0, ldteach) / [0, ldlogp) is free / not written.  The
// log-sum-exp re-reads the row from global memory: thread t sums its 16 codes in ascending order, then `block_sum` -- an order
// that depends on V only.  Without CONS the kernel is what it was before the flag: none of the added code is instantiated.
// PROD (with CONS; vqcpc_prior_sample_product): ONE STAGE of a product code's step.  The row is the stage's K logits and `tok` its
// digit: drawn as above with the stage's key, or digit `stage` of the forced code (teacher, else constraint) clamped to the K^ncb
// codes.  The stage's log-probability is stored (stage 0) or added (later stages) in ps.logp_acc.  A stage before the last
// stores its digit and writes h_next = h + dtab[stage][digit], and leaves codes, next_in, logp, pos and the ticket alone; the last
// forms the merged code from the stored digits and its own, writes next_in as the left-to-right sum of the digits' input-table
// rows (the chain of vqcpc_product_gather), logp from the accumulator, and advances pos.  With ncb = 1 every added statement
// reduces to the CONS kernel's: the same instructions on the same values.
// MASK (with CONS; vqcpc_prior_sample_masked, and with PROD vqcpc_prior_sample_product_masked): at the column `col` the row has a
// set of the codes (PROD: of the stage's digits) that may be drawn.  A thread's 16 codes are half a word of the set, so the set
// costs one global word per thread and no LDS: a code outside it becomes -inf as the thread takes its codes from LDS, before top-k
// and top-p.  Only bits [0, V) count and a set without any is no restriction (one block-wide count, uniform); a forced code
// ignores it.  logmass gets, at logp's column rule, (m_a - m) + log(s_a) - log(s): maximum and exp-sum of the row (the logp
// code's) and of its allowed codes, summed in the same order -- the full set gives exactly 0.  PROD: stage 0 stores the stage's
// log-mass in mk.mass_acc, later stages add theirs, the last writes the sum.  Without MASK none of this is instantiated.
template <bool CONS, bool PROD = false, bool MASK = false>
__global__ __launch_bounds__(kThreads) void prior_sample_kernel(
    const float* __restrict__ logits, int64_t ldl, int V, float temperature, int top_k, float top_p,
    const int64_t* __restrict__ seeds, const int64_t* __restrict__ teacher, int64_t ldteach, int64_t* __restrict__ codes,
    int64_t ldc, int N, const float* __restrict__ table, int d, float* __restrict__ next_in, int64_t ldn,
    float* __restrict__ probs, int64_t ldp, int32_t* __restrict__ posp, int32_t* __restrict__ ticket,
    float* __restrict__ logp, int64_t ldlogp, const int32_t* __restrict__ win,
    SampleExtra<PROD, MASK> ps) {
    static_assert(CONS || !PROD, "the product stage builds on the constrained kernel");
    static_assert(CONS || !MASK, "the mask is addressed at the constraint's column");
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
    uint32_t ok = 0xFFFFu;                                    // MASK: bit t = code i0 + t may be drawn
    if constexpr (MASK) {
        if (ps.mk.allowed && col >= 0 && col < ps.mk.ldallow) {       // uniform: the count below has barriers
            const int words = (V + 31) >> 5;
            int64_t set = b * ps.mk.ldallow + col;
            if constexpr (PROD) set = set * ps.ncb + ps.stage;
            const int w = tid >> 1;
            const uint32_t word = w < words ? ps.mk.allowed[set * words + w] : 0u;
            const int nv = min(max(V - i0, 0), kPer);                 // the thread's codes inside the vocabulary
            const uint32_t mine = (word >> ((tid & 1) * kPer)) & ((1u << nv) - 1u);
            if (block_sum_int(mine != 0u, redi) > 0) {                // a set without a code of the vocabulary restricts nothing
                ok = mine;
#pragma unroll
                for (int t = 0; t < kPer; ++t)
                    if (!((ok >> t) & 1u)) l[t] = ninf;
            }
        }
    }
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
    if constexpr (PROD) {
        if (ps.teacher) forced = max(ps.teacher[b * ps.ldteach + pos], (int64_t)0);
        if (forced >= 0) {                                   // this stage's digit of the forced code, clamped to the K^ncb codes
            int64_t vtot = 1;
            for (int i = 0; i < ps.ncb; ++i) vtot *= V;
            uint32_t q = (uint32_t)min(forced, vtot - 1);
            for (int i = 0; i < ps.stage; ++i) q /= (uint32_t)V;
            forced = q % (uint32_t)V;
        }
    }
    if (CONS ? forced >= 0 : teacher != nullptr) {           // uniform over the workgroup
        tok = CONS ? (int)min(forced, (int64_t)kMaxVocab) : (int)teacher[b * ldteach + pos];
    } else {
        uint64_t sd = (uint64_t)seeds[b];
        if constexpr (PROD) sd = stage_seed(sd, ps.stage);
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
    bool last = true;
    if constexpr (PROD) last = ps.stage == ps.ncb - 1;
    if constexpr (PROD) {
        if (!last) {                                          // an earlier stage: its digit, and the next stage's head input
            if (tid == 0) ps.digits[b * ps.ncb + ps.stage] = tok;
            const float* drow = ps.dtab + ((int64_t)ps.stage * V + tok) * d;
            for (int k = tid; k < d; k += kThreads) ps.h_next[b * ps.ldhn + k] = ps.h[b * ps.ldh + k] + drow[k];
        } else {                                              // the last stage: the merged code, the input of position pos + 1
            int dg[4] = {tok, 0, 0, 0};
            int64_t code = 0, mul = 1;
            for (int i = 0; i < ps.stage; ++i) {
                dg[i] = ps.digits[b * ps.ncb + i];
                code += dg[i] * mul;
                mul *= V;
            }
            dg[ps.stage] = tok;
            code += tok * mul;
            if (tid == 0) codes[b * ldc + pos] = code;
            for (int k = tid; k < d; k += kThreads) {
                float acc = table[(int64_t)dg[0] * d + k];
                for (int i = 1; i < ps.ncb; ++i) acc += table[((int64_t)i * V + dg[i]) * d + k];
                next_in[b * ldn + k] = acc;
            }
        }
    } else {
        if (tid == 0) codes[b * ldc + pos] = tok;
        for (int k = tid; k < d; k += kThreads) next_in[b * ldn + k] = table[(int64_t)tok * d + k];   // input of position pos + 1
    }
    if constexpr (CONS) {
        const bool wl = logp && col >= 0 && col < ldlogp;
        bool wm = false;
        if constexpr (MASK) wm = ps.mk.logmass && col >= 0 && col < ps.mk.ldmass;
        if (wl || wm) {                                      // uniform: every thread reaches the barriers below or none does
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
            if (wl) {
                if constexpr (PROD) {                        // stage 0 stores, later stages add in ascending stage order
                    if (tid == 0) {
                        const float lp = (logits[b * ldl + tok] - rmx) - logf(rs);
                        const float acc = ps.stage == 0 ? lp : ps.logp_acc[b] + lp;
                        if (last) logp[b * ldlogp + col] = acc; else ps.logp_acc[b] = acc;
                    }
                } else {
                    if (tid == 0) logp[b * ldlogp + col] = (logits[b * ldl + tok] - rmx) - logf(rs);
                }
            }
            if constexpr (MASK) {
                if (wm) {                                    // uniform: the same over the allowed codes, in the same order
                    float amx = ninf;
#pragma unroll
                    for (int t = 0; t < kPer; ++t) {
                        if (!((ok >> t) & 1u)) raw[t] = ninf;
                        amx = fmaxf(amx, raw[t]);
                    }
                    amx = block_max(amx, redf);
                    float as = 0.0f;
#pragma unroll
                    for (int t = 0; t < kPer; ++t) as += raw[t] > ninf ? expf(raw[t] - amx) : 0.0f;
                    as = block_sum(as, redf);
                    if (tid == 0) {
                        const float lm = amx > ninf ? (amx - rmx) + logf(as) - logf(rs) : ninf;
                        if constexpr (PROD) {
                            const float acc = ps.stage == 0 ? lm : ps.mk.mass_acc[b] + lm;
                            if (last) ps.mk.logmass[b * ps.mk.ldmass + col] = acc; else ps.mk.mass_acc[b] = acc;
                        } else {
                            ps.mk.logmass[b * ps.mk.ldmass + col] = lm;
                        }
                    }
                }
            }
        }
    }
    if constexpr (PROD) {
        if (!last) return;                                   // earlier stages never touch pos (uniform over the grid)
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

// PROD (vqcpc_prior_window_product): `table` is the input tables [ncb][K][d], table_rows = K^ncb + 1, so that the
// start-of-sentence index is V = K^ncb as in the merged form; the input row of a code is the left-to-right sum of its digits' rows
// (the chain of vqcpc_product_gather), that of the start of sentence is `sosrow`.  Everything else is the merged kernel's.
template <bool PROD = false>
__global__ __launch_bounds__(1024) void prior_window_kernel(int64_t* __restrict__ seq, int64_t ldseq, int64_t nt,
                                                            int32_t* __restrict__ win, int advance,
                                                            int64_t* __restrict__ codes_win, int N, int P,
                                                            int64_t* __restrict__ prefix_rows, const float* __restrict__ table,
                                                            int64_t table_rows, int d, float* __restrict__ x, int64_t ldx,
                                                            const int64_t* __restrict__ seeds_in,
                                                            int64_t* __restrict__ seeds_out, int32_t* __restrict__ posp, int M,
                                                            const float* __restrict__ sosrow = nullptr, int K = 0, int ncb = 0) {
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
        if constexpr (PROD) {
            float acc;
            if (row == sos) {
                acc = sosrow[c];
            } else {
                uint32_t q = (uint32_t)row;
                acc = table[(int64_t)(q % (uint32_t)K) * d + c];
                for (int j = 1; j < ncb; ++j) {
                    q /= (uint32_t)K;
                    acc += table[((int64_t)j * K + q % (uint32_t)K) * d + c];
                }
            }
            x[(int64_t)m * ldx + c] = acc;
        } else {
            x[(int64_t)m * ldx + c] = table[row * d + c];
        }
    }
    if (tid == 0) {
        *posp = P;
        win[0] = next + advance;
        win[1] = next;
    }
}

}  // namespace prior
}  // namespace vq
