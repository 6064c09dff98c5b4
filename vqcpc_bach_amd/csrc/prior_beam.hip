// Beam search over the prior's code plans (priors/generation.py `beam=W`; the rule is stated once, in numpy, in
// tests/prior_beam_reference.py, and in include/vqcpc.h).  The M <= 64 rows of an incremental stack are G = M / W groups of W
// consecutive rows, the hypotheses of one user row.  The decoder's vqcpc_decode_beam_select (csrc/beam.hip) is one workgroup with a
// wavefront per row of at most 256 tokens; a prior row has up to 4 096 merged codes, so the step's tail is TWO launches here:
//   * vqcpc_prior_beam_expand: ONE WORKGROUP PER ROW, 256 threads, thread t owns codes 16t .. 16t + 15 -- prior_sample_kernel's
//     layout.  It forms the row's log-probabilities and the log-mass of its set exactly as prior_sample_kernel<true, false, true>
//     forms logp and logmass (the raw row re-read from global, thread-ascending sums of expf, `block_max` / `block_sum` of
//     prior_kernels.h), adds the row's score and leaves the row's min(W, live) best candidates in a global scratch, ordered by
//     cand descending, then code ascending.  A row can contribute at most W candidates to its group.  The W best are found with
//     what the sampler already has, not by W rounds of a block arg-max (64 rounds x two barriers): the top-k filter's bitwise
//     radix select gives the W-th largest cand, a scan compacts the codes above it and the lowest codes equal to it, and a
//     bitonic sort orders those <= 64 (order-preserving bits of cand descending, code ascending) keys in LDS.
//   * vqcpc_prior_beam_select: ONE workgroup, a wavefront per group.  Stage 2 of beam_select_kernel: it stages the rows' lists in
//     LDS (as that kernel holds them) and merges the W sorted lists by rounds of a wave max plus a ballot (the lowest lane is the lowest row, whose list head is its lowest code among equal
//     scores) and writes everything of the live column in slot order, the next input rows and the counters.
// The moves that follow (row k <- row ancestors[k]) are vqcpc_particle_permute_*.
// A product prior emits a code as ncb digit stages, each stage's head reading what the earlier digits of the SAME hypothesis made
// of the stack's output.  vqcpc_prior_beam_expand_product / vqcpc_prior_beam_select_product are the same two kernel bodies under a
// compile-time flag (PROD), one pair PER STAGE: the search prunes to the group's W best (row, digit) pairs after every digit.
// A stage before the last moves only the stage's own small state into slot order -- the digits so far, the logp / log-mass
// accumulators (the sampler's chain: stage 0 stores, later stages add in ascending stage order), the stage score, the next
// head's input h_next[k] = h[ancestor] + dtab[stage][digit] and the ancestor composed over the stages -- and leaves codes,
// next_in, logp and pos alone; the last stage writes what the merged select writes, with the composed ancestors.  With ncb = 1
// every added statement reduces to the merged kernels'.  Without PROD none of the added code is instantiated.
// This file is compiled with the DEFAULT contraction, as prior.hip is and for beam.hip's reason: lp must have the sampler's
// bits.  The one operation that must be rounded on its own, cand = score + lp, is kept from contracting in `pbeam_add`.
#include "prior_kernels.h"

namespace vq {
namespace prior {

constexpr int kBeamWaves = 16;

__device__ __forceinline__ float pbeam_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// the inverse of float_key (no -0.0 comes back: its key is +0.0's)
__device__ __forceinline__ float key_float(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// exclusive prefix of the threads' counts in thread order; `total` receives the sum over the block
__device__ __forceinline__ int block_excl_scan_int(int v, int* red, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    __syncthreads();
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) base += red[w];
        all += red[w];
    }
    total = all;
    return base + incl - v;
}

// PROD: what a digit stage adds to the expansion.  The kernel's `V` is then K, its `logits` the stage's, its `score` the base the
// stage adds to (the hypotheses' scores at stage 0, the previous stage's scores afterwards).  Rows are in slot order from stage 1
// on, so the constraint and the sets of a row are those of the stack row it descends from, anc_in[b] (NULL at stage 0: b).
struct ExpandStage {
    int stage, ncb;
    const int32_t* anc_in;
};
struct SelectStage {
    int stage, ncb;
    int32_t* digits;               // [M][ncb], in place: the digits of the hypothesis in each slot
    float* logp_acc;               // [M], in place: the sum of the earlier stages' log-probabilities
    float* mass_acc;               // [M], in place: the sum of the earlier stages' log-masses
    float* stage_score;            // [M] out (a stage before the last): the slots' scores, the next stage's base
    int32_t* anc_total;            // [M], in place: the stack row each slot descends from, composed over the stages so far
    const float* h;                // (M, ldh) what this stage's head read
    int64_t ldh;
    const float* dtab;             // [ncb - 1][K][d] digit-conditioning rows
    float* h_next;                 // (M, ldhn) what the next stage's head reads
    int64_t ldhn;
};
struct NoBeamStage {};
template <bool PROD>
using ExpandExtra = std::conditional_t<PROD, ExpandStage, NoBeamStage>;
template <bool PROD>
using SelectExtra = std::conditional_t<PROD, SelectStage, NoBeamStage>;

template <bool PROD = false>
__global__ __launch_bounds__(kThreads) void prior_beam_expand_kernel(
    const float* __restrict__ logits, int64_t ldl, int V, int W, const int64_t* __restrict__ constraint, int64_t ldcons,
    const uint32_t* __restrict__ allowed, int64_t ldallow, const int32_t* __restrict__ win, const float* __restrict__ score, int N,
    const int32_t* __restrict__ posp, float* __restrict__ scr_cand, int32_t* __restrict__ scr_code, float* __restrict__ scr_lp,
    float* __restrict__ row_mass, int32_t* __restrict__ row_low, float* __restrict__ row_lowlp, float* __restrict__ cand_out,
    ExpandExtra<PROD> st) {
    __shared__ float slp[kMaxVocab];                          // the row's log-probabilities
    __shared__ uint64_t keys[kMaxRows];                       // the row's best candidates: (descending cand, code) sort keys
    __shared__ float redf[kWaves];
    __shared__ int redi[kWaves];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int pos = *posp;
    if (pos < 0 || pos >= N) return;                         // nothing is written (uniform over the grid)
    const float ninf = -INFINITY;
    const int w0 = win ? win[1] : 0;
    const int64_t col = w0 >= 0 ? (int64_t)w0 + pos : -1;    // < 0: no live window
    const int i0 = tid * kPer;
    int64_t ob = b;                                           // the row whose constraint and sets apply
    if constexpr (PROD) {
        if (st.anc_in) ob = min(max((int64_t)st.anc_in[b], (int64_t)0), (int64_t)gridDim.x - 1);
    }

    // ---- lp and the set's log-mass, with the masked sampler's expressions ------------------------------------------------
    uint32_t ok = 0xFFFFu;                                    // bit t = code i0 + t is in the row's set
    if (allowed && col >= 0 && col < ldallow) {               // uniform: the count below has barriers
        const int words = (V + 31) >> 5;
        int64_t set = ob * ldallow + col;
        if constexpr (PROD) set = set * st.ncb + st.stage;
        const int w = tid >> 1;
        const uint32_t word = w < words ? allowed[set * words + w] : 0u;
        const int nv = min(max(V - i0, 0), kPer);
        const uint32_t mine = (word >> ((tid & 1) * kPer)) & ((1u << nv) - 1u);
        if (block_sum_int(mine != 0u, redi) > 0) ok = mine;  // a set without a code of the vocabulary restricts nothing
    }
    float raw[kPer], rmx = ninf;
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        raw[t] = i0 + t < V ? logits[b * ldl + i0 + t] : ninf;             // the row as the model gave it
        rmx = fmaxf(rmx, raw[t]);
    }
    rmx = block_max(rmx, redf);
    float rs = 0.0f;
#pragma unroll
    for (int t = 0; t < kPer; ++t) rs += raw[t] > ninf ? expf(raw[t] - rmx) : 0.0f;
    rs = block_sum(rs, redf);
    float lp[kPer];
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        lp[t] = (raw[t] - rmx) - logf(rs);
        slp[i0 + t] = lp[t];
    }
    {
        float ar[kPer], amx = ninf;
#pragma unroll
        for (int t = 0; t < kPer; ++t) {
            ar[t] = (ok >> t) & 1u ? raw[t] : ninf;
            amx = fmaxf(amx, ar[t]);
        }
        amx = block_max(amx, redf);
        float as = 0.0f;
#pragma unroll
        for (int t = 0; t < kPer; ++t) as += ar[t] > ninf ? expf(ar[t] - amx) : 0.0f;
        as = block_sum(as, redf);
        if (tid == 0) row_mass[b] = amx > ninf ? (amx - rmx) + logf(as) - logf(rs) : ninf;
    }

    // ---- the candidates and their scores ---------------------------------------------------------------------------------
    int64_t forced = -1;
    if (constraint && col >= 0 && col < ldcons) forced = constraint[ob * ldcons + col];
    if constexpr (PROD) {
        if (forced >= 0) {                                    // this stage's digit of the forced code, clamped to the K^ncb codes
            int64_t vtot = 1;
            for (int i = 0; i < st.ncb; ++i) vtot *= V;
            uint32_t q = (uint32_t)min(forced, vtot - 1);
            for (int i = 0; i < st.stage; ++i) q /= (uint32_t)V;
            forced = q % (uint32_t)V;
        }
    }
    const int ftok = min(max((int)min(forced, (int64_t)kMaxVocab), 0), V - 1);
    const float sc = score[b];
    uint32_t k32[kPer];
    int low = 1 << 30, live = 0;
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        const int i = i0 + t;
        bool is = i < V;
        if (forced >= 0) is = is && i == ftok;
        else is = is && ((ok >> t) & 1u);
        float cand = pbeam_add(pbeam_add(sc, lp[t]), 0.0f);   // -0 becomes +0: the two tie
        if (!is || cand != cand) cand = ninf;                 // NaN counts as -inf
        k32[t] = float_key(cand);
        if (is && low == 1 << 30) low = i;
        live += cand > ninf;
        if (cand_out) cand_out[b * kMaxVocab + i] = cand;
    }
    low = block_min_int(low, redi);
    if (low == 1 << 30) low = 0;                              // no candidate at all: code 0
    if (tid == low / kPer) {                                  // slp[low] is this thread's own store
        row_low[b] = low;
        row_lowlp[b] = slp[low];
    }
    const int kk = min(W, block_sum_int(live, redi));         // the candidates this row hands to its group

    // ---- the kk best: the kk-th largest key bit by bit from the top, as the sampler's top-k ------------------------------------
    const uint32_t kninf = float_key(ninf);
    uint32_t thr = 0;
    if (kk > 0) {                                             // uniform
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t c = thr | (1u << bit);
            int cnt = 0;
#pragma unroll
            for (int t = 0; t < kPer; ++t) cnt += (k32[t] > kninf) & (k32[t] >= c);
            if (block_sum_int(cnt, redi) >= kk) thr = c;
        }
    }
    // codes above it, then the lowest codes equal to it: one scan of both counts (above < 64 in all, equal <= 4096)
    int na = 0, ne = 0;
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        const bool lv = kk > 0 && k32[t] > kninf;
        na += lv & (k32[t] > thr);
        ne += lv & (k32[t] == thr);
    }
    int total;
    const int before = block_excl_scan_int((na << 16) | ne, redi, total);
    const int above = total >> 16;
    int ia = before >> 16, ie = before & 0xFFFF;
    if (tid < kMaxRows) keys[tid] = ~0ull;                    // the padding sorts last
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        const bool lv = kk > 0 && k32[t] > kninf;
        int slot = -1;
        if (lv && k32[t] > thr) slot = ia++;
        else if (lv && k32[t] == thr) {
            if (above + ie < kk) slot = above + ie;
            ++ie;
        }
        if (slot >= 0 && slot < kMaxRows) keys[slot] = ((uint64_t)(~k32[t]) << 32) | (uint32_t)(i0 + t);
    }
    __syncthreads();
    // ascending sort of (~key, code): descending cand, equal cand by ascending code
    for (int k = 2; k <= kMaxRows; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (tid < kMaxRows) {
                const int p = tid ^ j;
                if (p > tid) {
                    const uint64_t a = keys[tid], c = keys[p];
                    const bool up = (tid & k) == 0;
                    if ((a > c) == up) {
                        keys[tid] = c;
                        keys[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid < W) {
        float cand = ninf, l = 0.0f;
        int code = 0;
        if (tid < kk) {
            const uint64_t key = keys[tid];
            code = (int)(uint32_t)key;
            cand = key_float(~(uint32_t)(key >> 32));
            l = slp[code];
        }
        scr_cand[b * W + tid] = cand;
        scr_code[b * W + tid] = code;
        scr_lp[b * W + tid] = l;
    }
}

template <bool PROD = false>
__global__ __launch_bounds__(64 * kBeamWaves) void prior_beam_select_kernel(
    const float* __restrict__ scr_cand, const int32_t* __restrict__ scr_code, const float* __restrict__ scr_lp,
    const float* __restrict__ row_mass, const int32_t* __restrict__ row_low, const float* __restrict__ row_lowlp, int V, int M,
    int W, float* __restrict__ logp, int64_t ldlogp, float* __restrict__ logmass, int64_t ldmass, const int32_t* __restrict__ win,
    int64_t* __restrict__ codes, int64_t ldc, int N, const float* __restrict__ table, int d, float* __restrict__ next_in,
    int64_t ldn, float* __restrict__ score, int32_t* __restrict__ ancestors, int32_t* __restrict__ flag,
    int32_t* __restrict__ bound, int32_t* __restrict__ hist_anc, int64_t hist_rows, int32_t* __restrict__ posp,
    SelectExtra<PROD> st) {
    __shared__ float lcand[kMaxRows * kMaxRows];              // the rows' lists: a merge round reads LDS, not global memory
    __shared__ int lcode[kMaxRows * kMaxRows];
    __shared__ float llp[kMaxRows * kMaxRows];
    __shared__ int scode[kMaxRows];                           // the codes in slot order
    __shared__ int sanc[PROD ? kMaxRows : 1];                 // PROD: the slots' ancestors of this stage, and their digits
    __shared__ int sdig[PROD ? kMaxRows * 4 : 1];
    __shared__ int moved;
    bool last = true;
    if constexpr (PROD) last = st.stage == st.ncb - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pos = *posp;
    if (pos < 0 || pos >= N) {                                // uniform: nothing happens, and the moves that follow find flag 0
        if (threadIdx.x == 0 && last) *flag = 0;
        return;
    }
    const float ninf = -INFINITY;
    const int w0 = win ? win[1] : 0;
    const int64_t col = w0 >= 0 ? (int64_t)w0 + pos : -1;
    const bool wl = logp && col >= 0 && col < ldlogp, wm = logmass && col >= 0 && col < ldmass;
    if (threadIdx.x == 0) moved = 0;
    for (int i = threadIdx.x; i < M * W; i += 64 * kBeamWaves) {
        lcand[i] = scr_cand[i];
        lcode[i] = scr_code[i];
        llp[i] = scr_lp[i];
    }
    __syncthreads();

    // ---- a wavefront per group: the W best of the W sorted lists, and the live column in slot order ----------------------
    const int G = M / W;
    for (int g = wave; g < G; g += kBeamWaves) {              // a wave's own trip count: no barrier inside
        const int base = g * W;
        const bool mem = lane < W;
        const int r = base + (mem ? lane : 0);
        int h = 0;                                            // this row's list head
        float cur = mem ? lcand[r * W] : ninf;
        int anc = r, code = 0;
        float sc = ninf, l = 0.0f;
        int n = 0;
        for (; n < W; ++n) {
            const float best = wave_max(cur);
            if (!(best > ninf)) break;                        // uniform
            const int first = __ffsll((long long)__ballot(cur == best)) - 1;  // the lowest row; its head is its lowest code
            const bool head = mem && h < W;
            const int bc = __shfl(head ? lcode[r * W + h] : 0, first, 64);
            const float bl = __shfl(head ? llp[r * W + h] : 0.0f, first, 64);
            if (lane == n) {
                anc = base + first;
                code = bc;
                sc = best;
                l = bl;
            }
            if (lane == first) {
                ++h;
                cur = h < W ? lcand[r * W + h] : ninf;
            }
        }
        if (n == 0) {                                         // no live candidate: the identity, every row's own lowest code
            if (mem) {
                code = row_low[r];
                l = row_lowlp[r];
            }
        } else {                                              // dead slots copy slot 0 (their score stays -inf)
            const int a0 = __shfl(anc, 0, 64), c0 = __shfl(code, 0, 64);
            const float l0 = __shfl(l, 0, 64);
            if (lane >= n) {
                anc = a0;
                code = c0;
                l = l0;
            }
        }
        code = min(max(code, 0), V - 1);                      // what the expansion wrote lies there already
        if constexpr (PROD) {
            // the ancestor's stage state: every lane's loads return before the first store below issues (one wavefront holds
            // the whole group), so the in-place buffers are read for every slot before any is written
            int dg[4] = {0, 0, 0, 0}, at = anc;
            float la = l, ma = mem ? row_mass[anc] : 0.0f;
            if (mem && st.stage > 0) {
                for (int i = 0; i < st.stage; ++i) dg[i] = min(max(st.digits[anc * st.ncb + i], 0), V - 1);
                la = st.logp_acc[anc] + l;                    // stage 0 stores, later stages add in ascending stage order
                ma = st.mass_acc[anc] + ma;
                at = st.anc_total[anc];
            }
            if (mem) {
                for (int i = 0; i < st.stage; ++i) sdig[r * 4 + i] = dg[i];
                sdig[r * 4 + st.stage] = code;
                sanc[r] = anc;
                if (!last) {
                    for (int i = 0; i < st.stage; ++i) st.digits[r * st.ncb + i] = dg[i];
                    st.digits[r * st.ncb + st.stage] = code;
                    st.logp_acc[r] = la;
                    st.mass_acc[r] = ma;
                    st.stage_score[r] = sc;
                    st.anc_total[r] = at;
                } else {
                    int64_t merged = 0, mul = 1;
                    for (int i = 0; i < st.stage; ++i) {
                        merged += dg[i] * mul;
                        mul *= V;
                    }
                    merged += code * mul;
                    ancestors[r] = at;
                    score[r] = sc;
                    codes[(int64_t)r * ldc + pos] = merged;
                    if (wl) logp[(int64_t)r * ldlogp + col] = la;
                    if (wm) logmass[(int64_t)r * ldmass + col] = ma;
                    if (hist_anc && col >= 0 && col < hist_rows) hist_anc[col * M + r] = at;
                    if (at != r) moved = 1;                   // benign race: every writer stores 1
                }
            }
            continue;
        }
        if (mem) {
            ancestors[r] = anc;
            score[r] = sc;
            codes[(int64_t)r * ldc + pos] = code;
            if (wl) logp[(int64_t)r * ldlogp + col] = l;
            if (wm) logmass[(int64_t)r * ldmass + col] = row_mass[anc];
            if (hist_anc && col >= 0 && col < hist_rows) hist_anc[col * M + r] = anc;
            scode[r] = code;
            if (anc != r) moved = 1;                          // benign race: every writer stores 1
        }
    }
    __syncthreads();

    if constexpr (PROD) {
        for (int b = wave; b < M; b += kBeamWaves) {
            const int* dg = sdig + b * 4;
            if (!last) {                                      // the next stage's head input, from the ancestor's
                const float* drow = st.dtab + ((int64_t)st.stage * V + dg[st.stage]) * d;
                const float* hrow = st.h + (int64_t)sanc[b] * st.ldh;
                for (int k = lane; k < d; k += 64) st.h_next[(int64_t)b * st.ldhn + k] = hrow[k] + drow[k];
            } else {                                          // the left-to-right sum of the digits' input-table rows
                for (int k = lane; k < d; k += 64) {
                    float acc = table[(int64_t)dg[0] * d + k];
                    for (int i = 1; i < st.ncb; ++i) acc += table[((int64_t)i * V + dg[i]) * d + k];
                    next_in[(int64_t)b * ldn + k] = acc;
                }
            }
        }
        if (!last) return;                                    // earlier stages never touch the counters (uniform)
        if (threadIdx.x == 0) {
            *flag = moved;
            bound[0] = pos;
            bound[1] = (int32_t)col;
            *posp = pos + 1;
        }
        return;
    }
    // ---- the next input rows (the sampler's table row), then the counters ------------------------------------------------
    for (int b = wave; b < M; b += kBeamWaves) {
        const int64_t row = scode[b];
        for (int k = lane; k < d; k += 64) next_in[(int64_t)b * ldn + k] = table[row * d + k];
    }
    if (threadIdx.x == 0) {
        *flag = moved;
        bound[0] = pos;
        bound[1] = (int32_t)col;
        *posp = pos + 1;                                      // after the barriers: every thread has read pos
    }
}

}  // namespace prior
}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_prior_beam_expand(const float* logits, int64_t ldl, int V, int64_t M, int W, const int64_t* constraint, int64_t ldcons,
                            const uint32_t* allowed, int64_t ldallow, const int32_t* win, const float* score, int N,
                            const int32_t* pos, float* scratch_cand, int32_t* scratch_code, float* scratch_lp, float* row_mass,
                            int32_t* row_low, float* row_lowlp, float* cand_out, void* stream) {
    VQ_REQUIRE(V >= 1 && V <= prior::kMaxVocab, "prior_beam_expand: %d codes (1 <= V <= 4096)", V);
    VQ_REQUIRE(M >= 1 && M <= prior::kMaxRows && W >= 1 && W <= prior::kMaxRows && M % W == 0,
               "prior_beam_expand: %lld rows in groups of %d (1 <= M <= 64, 1 <= W <= 64, M %% W == 0)", (long long)M, W);
    VQ_REQUIRE(logits && score && pos && scratch_cand && scratch_code && scratch_lp && row_mass && row_low && row_lowlp,
               "prior_beam_expand: null pointer");
    VQ_REQUIRE(N >= 1 && N <= prior::kMaxWindow && ldl >= V && (!constraint || ldcons >= N) && (!allowed || ldallow >= N),
               "prior_beam_expand: bad arguments (1 <= N <= 1024, ldl >= V, ldcons, ldallow >= N)");
    hipLaunchKernelGGL(prior::prior_beam_expand_kernel<false>, dim3((unsigned)M), dim3(prior::kThreads), 0, (hipStream_t)stream,
                       logits, ldl, V, W, constraint, ldcons, allowed, ldallow, win, score, N, pos, scratch_cand, scratch_code,
                       scratch_lp, row_mass, row_low, row_lowlp, cand_out, prior::NoBeamStage{});
    VQ_CHECK_LAUNCH("prior_beam_expand");
    return VQCPC_OK;
}

int vqcpc_prior_beam_select(const float* scratch_cand, const int32_t* scratch_code, const float* scratch_lp, const float* row_mass,
                            const int32_t* row_low, const float* row_lowlp, int V, int64_t M, int W, float* logp, int64_t ldlogp,
                            float* logmass, int64_t ldmass, const int32_t* win, int64_t* codes, int64_t ldc, int N,
                            const float* table, int64_t table_rows, int d, float* next_in, int64_t ldn, float* score,
                            int32_t* ancestors, int32_t* flag, int32_t* bound, int32_t* hist_ancestors, int64_t hist_rows,
                            int32_t* pos, void* stream) {
    VQ_REQUIRE(V >= 1 && V <= prior::kMaxVocab, "prior_beam_select: %d codes (1 <= V <= 4096)", V);
    VQ_REQUIRE(M >= 1 && M <= prior::kMaxRows && W >= 1 && W <= prior::kMaxRows && M % W == 0,
               "prior_beam_select: %lld rows in groups of %d (1 <= M <= 64, 1 <= W <= 64, M %% W == 0)", (long long)M, W);
    VQ_REQUIRE(scratch_cand && scratch_code && scratch_lp && row_mass && row_low && row_lowlp && codes && table && next_in &&
               score && ancestors && flag && bound && pos, "prior_beam_select: null pointer");
    VQ_REQUIRE(N >= 1 && N <= prior::kMaxWindow && d >= 1 && d <= prior::kMaxDim && hist_rows >= 0,
               "prior_beam_select: bad arguments (1 <= N <= 1024, 1 <= d <= 4096, hist_rows >= 0)");
    VQ_REQUIRE(ldc >= N && ldn >= d && (!logp || ldlogp >= N) && (!logmass || ldmass >= N) && table_rows >= V,
               "prior_beam_select: bad leading dimensions (ldlogp, ldmass >= N), or a table of fewer than V rows");
    hipLaunchKernelGGL(prior::prior_beam_select_kernel<false>, dim3(1), dim3(64 * prior::kBeamWaves), 0, (hipStream_t)stream,
                       scratch_cand, scratch_code, scratch_lp, row_mass, row_low, row_lowlp, V, (int)M, W, logp, ldlogp, logmass,
                       ldmass, win, codes, ldc, N, table, d, next_in, ldn, score, ancestors, flag, bound, hist_ancestors, hist_rows,
                       pos, prior::NoBeamStage{});
    VQ_CHECK_LAUNCH("prior_beam_select");
    return VQCPC_OK;
}

static bool beam_product_shape_ok(int ncb, int K) {
    if (ncb < 1 || ncb > 4 || K < 1 || K > prior::kMaxVocab) return false;
    int64_t v = 1;
    for (int j = 0; j < ncb; ++j) v *= K;
    return v + 1 < ((int64_t)1 << 31);
}

int vqcpc_prior_beam_expand_product(const float* logits, int64_t ldl, int K, int ncb, int stage, int64_t M, int W,
                                    const int64_t* constraint, int64_t ldcons, const uint32_t* allowed, int64_t ldallow,
                                    const int32_t* win, const float* base, const int32_t* anc_in, int N, const int32_t* pos,
                                    float* scratch_cand, int32_t* scratch_code, float* scratch_lp, float* row_mass,
                                    int32_t* row_low, float* row_lowlp, float* cand_out, void* stream) {
    VQ_REQUIRE(beam_product_shape_ok(ncb, K), "prior_beam_expand_product: need 1 <= ncb <= 4, 1 <= K <= 4096, K^ncb + 1 < 2^31");
    VQ_REQUIRE(stage >= 0 && stage < ncb, "prior_beam_expand_product: stage %d of %d", stage, ncb);
    VQ_REQUIRE(M >= 1 && M <= prior::kMaxRows && W >= 1 && W <= prior::kMaxRows && M % W == 0,
               "prior_beam_expand_product: %lld rows in groups of %d (1 <= M <= 64, 1 <= W <= 64, M %% W == 0)", (long long)M, W);
    VQ_REQUIRE(logits && base && pos && scratch_cand && scratch_code && scratch_lp && row_mass && row_low && row_lowlp,
               "prior_beam_expand_product: null pointer");
    VQ_REQUIRE(stage == 0 || anc_in, "prior_beam_expand_product: a stage after the first needs the composed ancestors");
    VQ_REQUIRE(N >= 1 && N <= prior::kMaxWindow && ldl >= K && (!constraint || ldcons >= N) && (!allowed || ldallow >= N),
               "prior_beam_expand_product: bad arguments (1 <= N <= 1024, ldl >= K, ldcons, ldallow >= N)");
    const prior::ExpandStage st{stage, ncb, stage == 0 ? nullptr : anc_in};
    hipLaunchKernelGGL(prior::prior_beam_expand_kernel<true>, dim3((unsigned)M), dim3(prior::kThreads), 0, (hipStream_t)stream,
                       logits, ldl, K, W, constraint, ldcons, allowed, ldallow, win, base, N, pos, scratch_cand, scratch_code,
                       scratch_lp, row_mass, row_low, row_lowlp, cand_out, st);
    VQ_CHECK_LAUNCH("prior_beam_expand_product");
    return VQCPC_OK;
}

int vqcpc_prior_beam_select_product(const float* scratch_cand, const int32_t* scratch_code, const float* scratch_lp,
                                    const float* row_mass, const int32_t* row_low, const float* row_lowlp, int K, int ncb, int stage,
                                    int64_t M, int W, int32_t* digits, float* logp_acc, float* mass_acc, float* stage_score,
                                    int32_t* anc_total, const float* h, int64_t ldh, const float* dtab, float* h_next, int64_t ldhn,
                                    float* logp, int64_t ldlogp, float* logmass, int64_t ldmass, const int32_t* win, int64_t* codes,
                                    int64_t ldc, int N, const float* tables, int d, float* next_in, int64_t ldn, float* score,
                                    int32_t* ancestors, int32_t* flag, int32_t* bound, int32_t* hist_ancestors, int64_t hist_rows,
                                    int32_t* pos, void* stream) {
    VQ_REQUIRE(beam_product_shape_ok(ncb, K), "prior_beam_select_product: need 1 <= ncb <= 4, 1 <= K <= 4096, K^ncb + 1 < 2^31");
    VQ_REQUIRE(stage >= 0 && stage < ncb, "prior_beam_select_product: stage %d of %d", stage, ncb);
    VQ_REQUIRE(M >= 1 && M <= prior::kMaxRows && W >= 1 && W <= prior::kMaxRows && M % W == 0,
               "prior_beam_select_product: %lld rows in groups of %d (1 <= M <= 64, 1 <= W <= 64, M %% W == 0)", (long long)M, W);
    VQ_REQUIRE(scratch_cand && scratch_code && scratch_lp && row_mass && row_low && row_lowlp && pos,
               "prior_beam_select_product: null pointer");
    VQ_REQUIRE(N >= 1 && N <= prior::kMaxWindow && d >= 1 && d <= prior::kMaxDim && hist_rows >= 0,
               "prior_beam_select_product: bad arguments (1 <= N <= 1024, 1 <= d <= 4096, hist_rows >= 0)");
    VQ_REQUIRE(ncb == 1 || (digits && logp_acc && mass_acc && stage_score && anc_total),
               "prior_beam_select_product: the digit, accumulator, stage score and ancestor scratch is needed");
    if (stage < ncb - 1)
        VQ_REQUIRE(h && dtab && h_next && h != h_next && ldh >= d && ldhn >= d,
                   "prior_beam_select_product: an earlier stage needs h, dtab and another buffer h_next");
    else
        VQ_REQUIRE(codes && tables && next_in && score && ancestors && flag && bound && ldc >= N && ldn >= d &&
                   (!logp || ldlogp >= N) && (!logmass || ldmass >= N),
                   "prior_beam_select_product: the last stage needs codes, tables, next_in, score, ancestors, flag, bound");
    const prior::SelectStage st{stage, ncb, digits, logp_acc, mass_acc, stage_score, anc_total, h, ldh, dtab, h_next, ldhn};
    hipLaunchKernelGGL(prior::prior_beam_select_kernel<true>, dim3(1), dim3(64 * prior::kBeamWaves), 0, (hipStream_t)stream,
                       scratch_cand, scratch_code, scratch_lp, row_mass, row_low, row_lowlp, K, (int)M, W, logp, ldlogp, logmass,
                       ldmass, win, codes, ldc, N, tables, d, next_in, ldn, score, ancestors, flag, bound, hist_ancestors, hist_rows,
                       pos, st);
    VQ_CHECK_LAUNCH("prior_beam_select_product");
    return VQCPC_OK;
}

}  // extern "C"
