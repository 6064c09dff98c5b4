// Beam search for decoder generation (decoders/generation.py `beam=W`; the rule is stated once, in numpy, in
// tests/beam_reference.py, and in include/vqcpc.h).  The M <= 64 rows of an incremental stack are G = M / W groups of W consecutive
// rows, the hypotheses of one user row.  vqcpc_decode_beam_select takes the sampler's place at the end of a step: ONE workgroup,
//   1. a wavefront per row forms the row's log-probabilities exactly as decode_sample_kernel<true> forms logp (lane l holds tokens
//      4l .. 4l + 3, the same wave_max / wave_sum), adds the row's score, and reduces its <= 256 candidates to its W best by W
//      rounds of a wave arg-max -- a row can contribute at most W candidates to its group;
//   2. a wavefront per group merges the W sorted lists by W rounds of an arg-max over the W list heads (lane j = row j) and writes
//      everything of the live column in slot order;
//   3. every wavefront copies the table rows of the chosen tokens into next_in, and one thread advances pos.
// An arg-max round is a wave_max of the candidate scores and a ballot of the lanes that hold the maximum: the lowest such lane holds
// the lowest token (stage 1: tokens ascend with the lane, and inside it) or is the lowest row (stage 2: a row's list is in token order
// among equal scores), which is the stated tie rule; -inf is "no candidate".  The moves that follow (row k <- row ancestors[k]) are
// vqcpc_particle_permute_*.
// This file is compiled with the DEFAULT contraction, as decode.hip is and unlike particles.hip: the flag reaches into the expansion
// of logf (its last multiply and add fuse), so only the sampler's own flags give the sampler's bits.  The one operation that must be
// rounded on its own, cand = score + lp, is kept from contracting in `beam_add`.
#include "common.h"

namespace vq {

constexpr int kBeamMaxRows = 64;
constexpr int kBeamMaxDim = 4096;
constexpr int kBeamMaxVoices = 16;
constexpr int kBeamMaxVocab = 256;
constexpr int kBeamWaves = 16;

struct BeamVoiceOffsets {
    int off[kBeamMaxVoices + 1];
};

__device__ __forceinline__ float beam_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// A row's log-probabilities and allowed mass with the bits decode_sample_kernel writes: the same expressions on the same lane
// layout under the same compiler flags.  raw: the lane's four logits (-inf past V); ok: its set bits.
__device__ __forceinline__ void beam_row_lp(const float (&raw)[4], uint32_t ok, bool want_mass, float (&lp)[4], float& mass) {
    const float ninf = -INFINITY;
    const float rmx = wave_max(fmaxf(fmaxf(raw[0], raw[1]), fmaxf(raw[2], raw[3])));
    float rs = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) rs += raw[t] > ninf ? expf(raw[t] - rmx) : 0.0f;
    rs = wave_sum(rs);
#pragma unroll
    for (int t = 0; t < 4; ++t) lp[t] = (raw[t] - rmx) - logf(rs);
    mass = 0.0f;
    if (want_mass) {                                          // uniform
        float ar[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) ar[t] = (ok >> t) & 1u ? raw[t] : ninf;
        const float amx = wave_max(fmaxf(fmaxf(ar[0], ar[1]), fmaxf(ar[2], ar[3])));
        float as = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) as += ar[t] > ninf ? expf(ar[t] - amx) : 0.0f;
        as = wave_sum(as);
        mass = (amx - rmx) + logf(as) - logf(rs);
    }
}

__global__ __launch_bounds__(64 * kBeamWaves) void beam_select_kernel(
    const float* __restrict__ logits, int64_t ldl, BeamVoiceOffsets vo, int nc, int M, int W, const uint32_t* __restrict__ exclude,
    const int64_t* __restrict__ constraint, int64_t ldcons, const uint32_t* __restrict__ allowed, int64_t ldallow,
    float* __restrict__ logp, int64_t ldlogp, float* __restrict__ logmass, int64_t ldmass, int32_t* __restrict__ report,
    int64_t ldrep, const int32_t* __restrict__ win, int64_t* __restrict__ tokens, int64_t ldtok, int T,
    const float* __restrict__ table, int64_t table_rows, int d, int U, float* __restrict__ next_in, int64_t ldn,
    float* __restrict__ score, int32_t* __restrict__ ancestors, int32_t* __restrict__ flag, int32_t* __restrict__ bound,
    int32_t* __restrict__ hist_anc, int64_t hist_rows, float* __restrict__ cand_out, int32_t* __restrict__ posp) {
    __shared__ float rcand[kBeamMaxRows * kBeamMaxRows];      // row b's W best scores, descending, at [b * W, (b + 1) * W); -inf: none
    __shared__ int rtok[kBeamMaxRows * kBeamMaxRows];         // their tokens
    __shared__ float rlp[kBeamMaxRows * kBeamMaxRows];        // and log-probabilities
    __shared__ float rmass[kBeamMaxRows];                     // the row's allowed mass
    __shared__ float lowlp[kBeamMaxRows];                     // the row's lowest candidate token and its log-probability
    __shared__ int lowtok[kBeamMaxRows];
    __shared__ int stok[kBeamMaxRows];                        // the tokens in slot order
    __shared__ int moved;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pos = *posp;
    if (pos < 0 || pos >= T) {                                // uniform: nothing happens, and the moves that follow find flag 0
        if (threadIdx.x == 0) *flag = 0;
        return;
    }
    const int c = pos % nc;
    const int V = vo.off[c + 1] - vo.off[c];
    const float ninf = -INFINITY;
    const int w0 = win ? win[1] : 0;
    const int64_t col = w0 >= 0 ? (int64_t)w0 * U + pos : -1;             // < 0: no live window
    const bool wl = logp && col >= 0 && col < ldlogp, wm = logmass && col >= 0 && col < ldmass;
    if (threadIdx.x == 0) moved = 0;

    // ---- 1. a wavefront per row: lp, the candidates and the row's W best -----------------------------------------------------
    for (int b = wave; b < M; b += kBeamWaves) {              // a wave's own trip count: no barrier inside
        uint32_t ok = 0xFu;                                   // bit t = token 4 * lane + t is in the row's set
        if (allowed && col >= 0 && col < ldallow) {           // uniform over the wave: the ballot runs in every lane
            const uint32_t word = allowed[((int64_t)b * ldallow + col) * 8 + (lane >> 3)];
            const int mine = V - 4 * lane;
            const uint32_t bits = (word >> ((lane & 7) * 4)) & (mine >= 4 ? 0xFu : mine > 0 ? (1u << mine) - 1u : 0u);
            if (__ballot(bits != 0u) != 0ull) ok = bits;      // an empty set restricts nothing
        }
        float raw[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = 4 * lane + t;
            raw[t] = i < V ? logits[(int64_t)b * ldl + vo.off[c] + i] : ninf;
        }
        float lp[4], mass;
        beam_row_lp(raw, ok, wm, lp, mass);
        if (wm && lane == 0) rmass[b] = mass;
        int64_t forced = -1;
        if (constraint && col >= 0 && col < ldcons) forced = constraint[(int64_t)b * ldcons + col];
        const int ftok = min(max((int)min(forced, (int64_t)kBeamMaxVocab), 0), V - 1);
        const float sc = score[b];
        float cd[4];
        int low = 1 << 30;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = 4 * lane + t;
            bool is = i < V;
            if (forced >= 0) is = is && i == ftok;
            else is = is && ((ok >> t) & 1u) && !(exclude && ((exclude[c * 8 + (i >> 5)] >> (i & 31)) & 1u));
            float cand = beam_add(beam_add(sc, lp[t]), 0.0f);               // -0 becomes +0: the two tie
            if (!is || cand != cand) cand = ninf;             // NaN counts as -inf
            cd[t] = cand;
            if (is) low = min(low, i);
            if (cand_out) cand_out[(int64_t)b * kBeamMaxVocab + i] = cand;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) low = min(low, __shfl_xor(low, o, 64));
        if (low == 1 << 30) low = 0;                          // no candidate at all: token 0
        {
            const int tt = low & 3;
            const float mine = tt == 0 ? lp[0] : tt == 1 ? lp[1] : tt == 2 ? lp[2] : lp[3];
            const float l = __shfl(mine, low >> 2, 64);
            if (lane == 0) {
                lowtok[b] = low;
                lowlp[b] = l;
            }
        }
        int k = 0;
        for (; k < W; ++k) {
            const float best = wave_max(fmaxf(fmaxf(cd[0], cd[1]), fmaxf(cd[2], cd[3])));
            if (!(best > ninf)) break;                        // uniform
            const bool has = cd[0] == best || cd[1] == best || cd[2] == best || cd[3] == best;
            if (lane == __ffsll((long long)__ballot(has)) - 1) {              // the lowest lane: the lowest token
                bool done = false;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (!done && cd[t] == best) {
                        rcand[b * W + k] = best;
                        rtok[b * W + k] = 4 * lane + t;
                        rlp[b * W + k] = lp[t];
                        cd[t] = ninf;
                        done = true;
                    }
                }
            }
        }
        for (int j = k + lane; j < W; j += 64) rcand[b * W + j] = ninf;
    }
    __syncthreads();

    // ---- 2. a wavefront per group: the W best of the W sorted lists, and the live column in slot order -----------------------
    const int G = M / W;
    for (int g = wave; g < G; g += kBeamWaves) {
        const int base = g * W;
        const bool mem = lane < W;
        const int r = base + (mem ? lane : 0);
        int h = 0;                                            // this row's list head
        float cur = mem ? rcand[r * W] : ninf;
        int anc = r, tok = 0;
        float sc = ninf, l = 0.0f;
        int n = 0;
        for (; n < W; ++n) {
            const float best = wave_max(cur);
            if (!(best > ninf)) break;                        // uniform
            const int first = __ffsll((long long)__ballot(cur == best)) - 1;  // the lowest row; its head is its lowest token
            const bool head = mem && h < W;
            const int bt = __shfl(head ? rtok[r * W + h] : 0, first, 64);
            const float bl = __shfl(head ? rlp[r * W + h] : 0.0f, first, 64);
            if (lane == n) {
                anc = base + first;
                tok = bt;
                sc = best;
                l = bl;
            }
            if (lane == first) {
                ++h;
                cur = h < W ? rcand[r * W + h] : ninf;
            }
        }
        if (n == 0) {                                         // no live candidate: the identity, every row's own lowest token
            if (mem) {
                tok = lowtok[r];
                l = lowlp[r];
            }
        } else {                                              // dead slots copy slot 0 (their score stays -inf)
            const int a0 = __shfl(anc, 0, 64), t0 = __shfl(tok, 0, 64);
            const float l0 = __shfl(l, 0, 64);
            if (lane >= n) {
                anc = a0;
                tok = t0;
                l = l0;
            }
        }
        if (mem) {
            int32_t rep = 0;
            const bool wr = report && col >= 0 && col < ldrep;
            if (wr) rep = report[(int64_t)anc * ldrep + col];     // every lane's load returns before the first store issues
            ancestors[r] = anc;
            score[r] = sc;
            tokens[(int64_t)r * ldtok + pos] = tok;
            if (wl) logp[(int64_t)r * ldlogp + col] = l;
            if (wm) logmass[(int64_t)r * ldmass + col] = rmass[anc];
            if (wr) report[(int64_t)r * ldrep + col] = rep;
            if (hist_anc && col >= 0 && col < hist_rows) hist_anc[col * M + r] = anc;
            stok[r] = tok;
            if (anc != r) moved = 1;                          // benign race: every writer stores 1
        }
    }
    __syncthreads();

    // ---- 3. the next input rows (the sampler's table row rule), then the counters ----------------------------------------------
    for (int b = wave; b < M; b += kBeamWaves) {
        const int64_t row = min((int64_t)stok[b] * U + pos % U, table_rows - 1);
        for (int k = lane; k < d; k += 64) next_in[(int64_t)b * ldn + k] = table[row * d + k];
    }
    if (threadIdx.x == 0) {
        *flag = moved;
        bound[0] = pos;
        bound[1] = (int32_t)col;
        *posp = pos + 1;                                      // after the barriers: every thread has read pos
    }
}

}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_decode_beam_select(const float* logits, int64_t ldl, const int32_t* voice_offsets, int nc, int64_t M, int W,
                             const uint32_t* exclude, const int64_t* constraint, int64_t ldcons, const uint32_t* allowed,
                             int64_t ldallow, float* logp, int64_t ldlogp, float* logmass, int64_t ldmass, int32_t* rule_report,
                             int64_t ldreport, const int32_t* win, int64_t* tokens, int64_t ldtok, int T, const float* table,
                             int64_t table_rows, int d, int U, float* next_in, int64_t ldn, float* score, int32_t* ancestors,
                             int32_t* flag, int32_t* bound, int32_t* hist_ancestors, int64_t hist_rows, float* cand_out,
                             int32_t* pos, void* stream) {
    VQ_REQUIRE(logits && voice_offsets && tokens && table && next_in && pos && score && ancestors && flag && bound && nc >= 1 &&
               nc <= kBeamMaxVoices && M >= 1 && M <= kBeamMaxRows && W >= 1 && W <= kBeamMaxRows && M % W == 0 && T >= 1 &&
               d >= 1 && d <= kBeamMaxDim && U >= 1 && table_rows >= 1 && hist_rows >= 0,
               "decode_beam_select: bad arguments (1 <= M <= 64, 1 <= W <= 64, M %% W == 0, 1 <= nc <= 16, 1 <= d <= 4096)");
    BeamVoiceOffsets vo;
    vo.off[0] = voice_offsets[0];
    VQ_REQUIRE(vo.off[0] >= 0, "decode_beam_select: negative voice offset");
    int vmax = 0;
    for (int c = 0; c < nc; ++c) {
        const int V = voice_offsets[c + 1] - voice_offsets[c];
        VQ_REQUIRE(V >= 1 && V <= kBeamMaxVocab, "decode_beam_select: voice %d has %d tokens (1 <= V_c <= 256)", c, V);
        vo.off[c + 1] = voice_offsets[c + 1];
        vmax = std::max(vmax, V);
    }
    for (int c = nc + 1; c <= kBeamMaxVoices; ++c) vo.off[c] = vo.off[nc];
    VQ_REQUIRE(ldl >= vo.off[nc] && ldtok >= T && ldn >= d, "decode_beam_select: bad leading dimensions");
    // as the samplers: with win the host can only ask for one window's columns; the kernel checks the column itself
    VQ_REQUIRE((!constraint || ldcons >= T) && (!allowed || ldallow >= T) && (!logp || ldlogp >= T) && (!logmass || ldmass >= T) &&
               (!rule_report || ldreport >= T),
               "decode_beam_select: bad leading dimensions (ldcons, ldallow, ldlogp, ldmass, ldreport >= T)");
    VQ_REQUIRE((int64_t)(vmax - 1) * U + (U - 1) < table_rows, "decode_beam_select: the table has too few rows for V_c * U");
    hipLaunchKernelGGL(beam_select_kernel, dim3(1), dim3(64 * kBeamWaves), 0, (hipStream_t)stream, logits, ldl, vo, nc, (int)M, W,
                       exclude, constraint, ldcons, allowed, ldallow, logp, ldlogp, logmass, ldmass, rule_report, ldreport, win,
                       tokens, ldtok, T, table, table_rows, d, U, next_in, ldn, score, ancestors, flag, bound, hist_ancestors,
                       hist_rows, cand_out, pos);
    VQ_CHECK_LAUNCH("decode_beam_select");
    return VQCPC_OK;
}

}  // extern "C"
