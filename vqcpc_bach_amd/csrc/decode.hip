// Autoregressive generation of the decoder (reference: VQCPCB/decoders/decoder.py:552-723, utils.py:101-128): the
// kernels of ONE incremental step, for a few rows (M <= 64 sequences) at a time.
//
// Nothing in the decoder looks ahead (causal target self-attention, a memory that does not depend on the target,
// row-wise embedding / LayerNorm / FFN), so position t's logits depend on tokens < t only and a KV-cached step computes
// the same function at one row per layer and token (vqcpc_bach_amd/decoders/generation.py):
//   * vqcpc_decode_linear: y = x W^T + b (ReLU) (+ residual) for M <= 64 rows.  Weight-streaming: a wavefront owns two
//     output columns, reads their rows of W once per 32 input rows and applies them to every row.  Plain fp32 FMA in a fixed
//     order per output element -- lane l sums k = 4l + 256i (i ascending, the four components in order), then a xor
//     butterfly over the 64 lanes -- which does not depend on M: row b of a batch is bit-identical to the row alone.
//   * vqcpc_decode_attn: one query row per (sequence, head) against the layer's K/V cache (self: the step's k / v row is
//     stored at row `pos` first; causal) or the memory's K/V (cross: the rectangular rule of vqcpc_relattn_x_fwd).
//     `pos` is read from device memory, so a captured step is position-independent.
//   * vqcpc_decode_attn_probs: the same kernel body with a compile-time flag: the normalised attention row -- the very
//     sc[j] * inv the P.V product multiplies by -- is also written out, one coalesced store of Lk floats per (sequence, head),
//     at the row of the position's CHORALE coordinate (the device window index, as the constrained sampler's column).
//   * vqcpc_decode_sample: temperature, exclusion mask, top-k, top-p, softmax and one counter-based draw per row; writes the
//     token, the next step's input row (a row of the target table) and advances `pos`.  ONE workgroup: the position
//     counter is read by every kernel of the step and written here once, after a barrier.
//   * vqcpc_decode_sample_constrained: the same kernel body with a compile-time flag: per (row, position) a token to emit or a
//     draw, and the emitted token's log-probability under the unfiltered row; both addressed in chorale coordinates through
//     the device window index.
//   * vqcpc_decode_sample_masked: one more compile-time flag on top of that: per (row, position) a 256-bit set of the tokens that
//     may be drawn, applied where the exclusion is, and the log of the probability mass the set leaves open; same addressing.
//
// Sliding-window generation (reference: decoder.py:729-854) moves the model window by one code at a time; the caches of
// the new window's prefix are rebuilt by a teacher-forced pass over its P prefix rows (GEMMs + LayerNorm of the training
// path, row-wise) whose attention is
//   * vqcpc_decode_prefill_attn: the multi-query companion of vqcpc_decode_attn.  A workgroup owns a strip of 16 query rows
//     of one (sequence, head); K / V / relative-table tiles go through LDS and are shared by the strip, key tiles the mask
//     rules out are skipped, the softmax is online in fp32.  Self mode also stores the prefix's k / v rows into the cache.
//   * vqcpc_decode_window: ONE workgroup.  Puts the live window's tokens back into the chorale, loads the next window's
//     codes and tokens (its index is read from device memory and advanced), the prefix's table-row indices, the input row
//     of position P, the window's effective sampling seeds and `pos`.
//
// A decoder on continuous latents (a NoQuantization encoder) has a linear layer where the others have an embedding table:
//   * vqcpc_decode_source_rows: src = z W^T + b on the S latents of the live window of every sequence; the window's first
//     code is read from the device memory that vqcpc_decode_window maintains.
#include <algorithm>

#include "common.h"

namespace vq {

constexpr int kDecMaxRows = 64;
constexpr int kDecMaxDim = 4096;
constexpr int kDecMaxLk = 1024;
constexpr int kDecMaxVoices = 16;
constexpr int kDecMaxVocab = 256;
constexpr int kLinCols = 2;                  // output columns per wavefront
constexpr int kLinWaves = 4;
constexpr float kDecNegBig = -1.0e30f;       // the masked score of relattn_x.hip: exp(kDecNegBig - max) == 0

// =====================================================================================================================
// decode_linear
template <int RB>
__global__ __launch_bounds__(64 * kLinWaves) void decode_linear_kernel(const float* __restrict__ x, int64_t ldx,
                                                                       const int64_t* __restrict__ gather,
                                                                       const float* __restrict__ w,
                                                                       const float* __restrict__ bias,
                                                                       const float* __restrict__ res, int64_t ldr,
                                                                       float* __restrict__ y, int64_t ldy, int M, int N,
                                                                       int K, int relu) {
    static_assert(RB * kLinCols <= 64, "one output element per lane in the epilogue");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = (blockIdx.x * kLinWaves + wave) * kLinCols;
    if (n0 >= N) return;                                     // wave-uniform; the kernel has no barrier
    const float* wr[kLinCols];
#pragma unroll
    for (int c = 0; c < kLinCols; ++c) wr[c] = w + (int64_t)min(n0 + c, N - 1) * K;
    for (int m0 = 0; m0 < M; m0 += RB) {
        const int rows = min(RB, M - m0);
        const float* xr[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int m = m0 + min(r, rows - 1);
            xr[r] = x + (gather ? gather[m] : (int64_t)m) * ldx;
        }
        float acc[kLinCols][RB];
#pragma unroll
        for (int c = 0; c < kLinCols; ++c)
#pragma unroll
            for (int r = 0; r < RB; ++r) acc[c][r] = 0.0f;
        for (int k = 4 * lane; k < K; k += 256) {
            float4 wv[kLinCols];
#pragma unroll
            for (int c = 0; c < kLinCols; ++c) wv[c] = *reinterpret_cast<const float4*>(wr[c] + k);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (r < rows) {
                    const float4 xv = *reinterpret_cast<const float4*>(xr[r] + k);
#pragma unroll
                    for (int c = 0; c < kLinCols; ++c) {
                        float a = acc[c][r];
                        a = fmaf(wv[c].x, xv.x, a);
                        a = fmaf(wv[c].y, xv.y, a);
                        a = fmaf(wv[c].z, xv.z, a);
                        a = fmaf(wv[c].w, xv.w, a);
                        acc[c][r] = a;
                    }
                }
            }
        }
        // butterfly: every lane ends with the same sums (a + b == b + a at each level), lane c * RB + r stores (r, c)
        float mine = 0.0f;
#pragma unroll
        for (int c = 0; c < kLinCols; ++c)
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (r < rows) {
                    const float s = wave_sum(acc[c][r]);
                    if (lane == c * RB + r) mine = s;
                }
            }
        const int c = lane / RB, r = lane % RB;
        if (c < kLinCols && r < rows && n0 + c < N) {
            const int m = m0 + r, n = n0 + c;
            float v = mine + (bias ? bias[n] : 0.0f);
            if (relu) v = fmaxf(v, 0.0f);
            if (res) v += res[(int64_t)m * ldr + n];
            y[(int64_t)m * ldy + n] = v;
        }
    }
}

// =====================================================================================================================
// decode_attn: one workgroup per (sequence, head); thread j walks keys j, j + 256, ...
__device__ __forceinline__ float block_max256(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// s_k = qs.k and s_e = qs.e in one pass (the loads of both rows in flight together); sequential fp32 FMA over c
template <int HD>
__device__ __forceinline__ void dot_rows(const float* __restrict__ qs, const float* __restrict__ kr, const float* __restrict__ er,
                                         float& s_k, float& s_e) {
    float a = 0.0f, e = 0.0f;
#pragma unroll 4
    for (int c = 0; c < HD; c += 4) {
        const float4 t = *reinterpret_cast<const float4*>(kr + c);
        const float4 u = *reinterpret_cast<const float4*>(er + c);
        a = fmaf(qs[c], t.x, a);
        a = fmaf(qs[c + 1], t.y, a);
        a = fmaf(qs[c + 2], t.z, a);
        a = fmaf(qs[c + 3], t.w, a);
        e = fmaf(qs[c], u.x, e);
        e = fmaf(qs[c + 1], u.y, e);
        e = fmaf(qs[c + 2], u.z, e);
        e = fmaf(qs[c + 3], u.w, e);
    }
    s_k = a;
    s_e = e;
}

// PROBS (vqcpc_decode_attn_probs): the row of probabilities goes to probs[b][h][r][0 .. Lk), r = pos (win == NULL) or
// win[1] * win_stride + pos; no live window (win[1] < 0) or r outside [0, rows): nothing is written, ctx and the cache rows are
// produced as usual.  Every thread stores the keys it owns in the score loop (j = tid, tid + 256, ...): it reads back its own
// sc[j], no barrier is needed.  Without PROBS the kernel is what it was before the flag: none of the added code is instantiated.
template <int HD, bool PROBS>
__global__ __launch_bounds__(256) void decode_attn_kernel(const float* __restrict__ q, int64_t ldq, float* __restrict__ kc,
                                                          float* __restrict__ vc, int64_t ldc,
                                                          const float* __restrict__ knew, const float* __restrict__ vnew,
                                                          int64_t ldn, const float* __restrict__ e1,
                                                          const float* __restrict__ e2, float* __restrict__ ctx, int64_t ldo,
                                                          const int32_t* __restrict__ posp, int Lk, int ratio, int H,
                                                          int mask, float scale, float* __restrict__ probs, int64_t ldp,
                                                          int64_t rows, const int32_t* __restrict__ win, int win_stride) {
    constexpr int G = 1024 / HD;                             // key groups of the P.V product
    __shared__ __attribute__((aligned(16))) float qs[HD];
    __shared__ float sc[kDecMaxLk];
    __shared__ __attribute__((aligned(16))) float part[1024];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / H;
    const int h = (int)(blockIdx.x % H);
    const int pos = *posp;
    const bool self = knew != nullptr;
    const int p = self ? pos : pos / ratio;
    if (pos < 0 || p >= Lk) return;                          // past the end: nothing to attend (uniform)
    const int64_t hoff = (int64_t)h * HD;
    if (self) {                                              // the step's k / v row joins the cache at row pos
        for (int c = tid; c < HD; c += 256) {
            kc[(b * Lk + pos) * ldc + hoff + c] = knew[b * ldn + hoff + c];
            vc[(b * Lk + pos) * ldc + hoff + c] = vnew[b * ldn + hoff + c];
        }
    }
    for (int c = tid; c < HD; c += 256) qs[c] = q[b * ldq + hoff + c] * scale;
    __syncthreads();
    // scores: qs.k_j + qs.Erel[j - p + Lk - 1] (the two sums of relattn_x_fwd_kernel, added in the same order)
    float mx = kDecNegBig;
    for (int j = tid; j < Lk; j += 256) {
        const bool keep = ((mask == 0) | ((mask == 1) & (j <= p)) | ((mask == 2) & (j >= p))) && (!self || j <= pos);
        float s = kDecNegBig;
        if (keep) {
            const float* kr = (self && j == pos) ? knew + b * ldn + hoff : kc + (b * Lk + j) * ldc + hoff;
            const int xr = j - p + Lk - 1;
            const float* er = xr < Lk ? e1 + ((int64_t)h * Lk + xr) * HD : e2 + ((int64_t)h * Lk + (xr - Lk + 1)) * HD;
            float sk, se;
            dot_rows<HD>(qs, kr, er, sk, se);
            s = sk + se;
        }
        sc[j] = s;
        mx = fmaxf(mx, s);
    }
    const float m = block_max256(mx, red);
    float sum = 0.0f;
    for (int j = tid; j < Lk; j += 256) {
        const float s = sc[j];
        const float e = s > 0.5f * kDecNegBig ? __expf(s - m) : 0.0f;
        sc[j] = e;
        sum += e;
    }
    const float inv = 1.0f / block_sum256(sum, red);
    if constexpr (PROBS) {
        const int w0 = win ? win[1] : 0;
        const int64_t r = win ? (int64_t)w0 * win_stride + pos : (int64_t)pos;
        if (w0 >= 0 && r >= 0 && r < rows) {                 // uniform
            float* pr = probs + ((b * H + h) * rows + r) * ldp;
            for (int j = tid; j < Lk; j += 256) pr[j] = sc[j] * inv;     // masked keys and (self) j > pos: 0.0f * inv == +0
        }
    }
    // ctx[c] = sum_j p_j v_j[c]: thread (g, c4) owns columns 4c4 .. 4c4 + 3 and keys j = g, g + G, ...  (eight in flight);
    // the G partial sums are added in group order
    const int c4 = tid % (HD / 4), g = tid / (HD / 4);
    const int jend = self ? pos + 1 : Lk;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j0 = g; j0 < jend; j0 += 8 * G) {
        float4 vv[8];
        float pj[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = min(j0 + u * G, jend - 1);
            const float* vr = (self && j == pos) ? vnew + b * ldn + hoff : vc + (b * Lk + j) * ldc + hoff;
            vv[u] = *reinterpret_cast<const float4*>(vr + 4 * c4);
            pj[u] = j0 + u * G < jend ? sc[j] * inv : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {                    // masked keys: p == 0 and the (unwritten) row is never used
            if (pj[u] != 0.0f) {
                o.x = fmaf(pj[u], vv[u].x, o.x);
                o.y = fmaf(pj[u], vv[u].y, o.y);
                o.z = fmaf(pj[u], vv[u].z, o.z);
                o.w = fmaf(pj[u], vv[u].w, o.w);
            }
        }
    }
    reinterpret_cast<float4*>(part)[tid] = o;
    __syncthreads();
    if (tid < HD) {
        const int cc = tid;
        float t = part[cc];
        for (int gg = 1; gg < G; ++gg) t += part[gg * HD + cc];
        ctx[b * ldo + hoff + cc] = t;
    }
}

// =====================================================================================================================
// decode_prefill_attn: grid (strips of kPfRows query rows, M * H); 256 threads.  Thread (r, l) = (tid / 16, tid % 16) owns
// keys l, l + 16 of the tile in the score phase and HD / 16 output columns of row r in the P.V phase; the 16 lanes of a row
// are consecutive lanes of one wavefront, so the row statistics are xor-shuffles of width 16.
constexpr int kPfRows = 16;

template <int HD, int KT>
__global__ __launch_bounds__(256) void decode_prefill_attn_kernel(
    const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, const float* __restrict__ v, int64_t ldk,
    float* __restrict__ kc, float* __restrict__ vc, int64_t ldc, const float* __restrict__ e1, const float* __restrict__ e2,
    float* __restrict__ ctx, int64_t ldo, int P, int Lk, int ratio, int H, int mask, float scale) {
    constexpr int QR = kPfRows, LD = HD + 4, NJ = KT / 16, CPT = HD / 16, ER = KT + QR - 1;
    __shared__ __attribute__((aligned(16))) float qs[QR * LD];
    __shared__ __attribute__((aligned(16))) float ks[KT * LD];
    __shared__ __attribute__((aligned(16))) float vs[KT * HD];
    __shared__ __attribute__((aligned(16))) float es[ER * LD];
    __shared__ float sc[QR][KT + 1];
    const int tid = threadIdx.x, r = tid >> 4, l = tid & 15;
    const int64_t b = blockIdx.y / H;
    const int h = (int)(blockIdx.y % H);
    const int64_t hoff = (int64_t)h * HD;
    const int i0 = blockIdx.x * QR;
    const int i1 = min(i0 + QR, P) - 1;                      // last live row of the strip (i0 < P by the grid)
    const bool self = kc != nullptr;
    const int64_t kvrow0 = self ? b * P : b * Lk;            // self: the prefix rows of the in_proj output; cross: the memory
    const int nkeys = self ? P : Lk;
    if (self) {                                              // the strip's own k / v rows join the cache [M][Lk][ldc]
        for (int e = tid; e < QR * (HD / 4); e += 256) {
            const int rr = e / (HD / 4), c = (e % (HD / 4)) * 4;
            if (i0 + rr <= i1) {
                const int64_t src = (kvrow0 + i0 + rr) * ldk + hoff + c, dst = (b * Lk + i0 + rr) * ldc + hoff + c;
                *reinterpret_cast<float4*>(kc + dst) = *reinterpret_cast<const float4*>(k + src);
                *reinterpret_cast<float4*>(vc + dst) = *reinterpret_cast<const float4*>(v + src);
            }
        }
        if (!ctx) return;                                    // the last layer: nothing reads its prefix outputs
    }
    for (int e = tid; e < QR * (HD / 4); e += 256) {
        const int rr = e / (HD / 4), c = (e % (HD / 4)) * 4;
        float4 t = *reinterpret_cast<const float4*>(q + (b * P + min(i0 + rr, i1)) * ldq + hoff + c);
        t.x *= scale, t.y *= scale, t.z *= scale, t.w *= scale;
        *reinterpret_cast<float4*>(qs + rr * LD + c) = t;
    }
    // key range of the strip under the mask: p = i / ratio (self: ratio 1)
    const int p_lo = i0 / ratio, p_hi = i1 / ratio;
    const int j_lo = mask == 2 ? p_lo : 0, j_hi = mask == 1 ? min(p_hi, nkeys - 1) : nkeys - 1;
    const int i = min(i0 + r, i1), p = i / ratio;
    float m_run = kDecNegBig, l_run = 0.0f, o[CPT];
#pragma unroll
    for (int t = 0; t < CPT; ++t) o[t] = 0.0f;
    for (int j0 = (j_lo / KT) * KT; j0 <= j_hi; j0 += KT) {
        __syncthreads();                                     // the previous tile's readers are done (and qs is written)
        for (int e = tid; e < KT * (HD / 4); e += 256) {
            const int jj = e / (HD / 4), c = (e % (HD / 4)) * 4;
            const int64_t src = (kvrow0 + min(j0 + jj, nkeys - 1)) * ldk + hoff + c;
            *reinterpret_cast<float4*>(ks + jj * LD + c) = *reinterpret_cast<const float4*>(k + src);
            *reinterpret_cast<float4*>(vs + jj * HD + c) = *reinterpret_cast<const float4*>(v + src);
        }
        // relative rows xr = j - p + Lk - 1 of the tile: [j0 - p_hi + Lk - 1, j0 + KT - 1 - p_lo + Lk - 1], clamped to the
        // tables' 2 Lk - 1 rows (e1 rows 0 .. Lk - 1, then e2 rows 1 .. Lk - 1, the rule of vqcpc_decode_attn)
        const int xr0 = j0 - p_hi + Lk - 1;
        for (int e = tid; e < ER * (HD / 4); e += 256) {
            const int rr = e / (HD / 4), c = (e % (HD / 4)) * 4;
            const int xr = min(max(xr0 + rr, 0), 2 * Lk - 2);
            const float* er = xr < Lk ? e1 + ((int64_t)h * Lk + xr) * HD : e2 + ((int64_t)h * Lk + (xr - Lk + 1)) * HD;
            *reinterpret_cast<float4*>(es + rr * LD + c) = *reinterpret_cast<const float4*>(er + c);
        }
        __syncthreads();
        float s[NJ], mx = kDecNegBig;
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
            const int jj = l + 16 * u, j = j0 + jj;
            const bool keep = j < nkeys && ((mask == 0) | ((mask == 1) & (j <= p)) | ((mask == 2) & (j >= p)));
            float sk = 0.0f, se = 0.0f;
            if (keep) dot_rows<HD>(qs + r * LD, ks + jj * LD, es + (j - p + Lk - 1 - xr0) * LD, sk, se);
            s[u] = keep ? sk + se : kDecNegBig;
            mx = fmaxf(mx, s[u]);
        }
#pragma unroll
        for (int w = 8; w > 0; w >>= 1) mx = fmaxf(mx, __shfl_xor(mx, w, 64));
        const float m_new = fmaxf(m_run, mx);
        float sum = 0.0f;
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
            const float e = s[u] > 0.5f * kDecNegBig ? __expf(s[u] - m_new) : 0.0f;
            sc[r][l + 16 * u] = e;
            sum += e;
        }
#pragma unroll
        for (int w = 8; w > 0; w >>= 1) sum += __shfl_xor(sum, w, 64);
        const float alpha = __expf(m_run - m_new);           // 1 while every key so far was masked (m_run == m_new)
        l_run = l_run * alpha + sum;
        m_run = m_new;
#pragma unroll
        for (int t = 0; t < CPT; ++t) o[t] *= alpha;
        __syncthreads();                                     // sc rows are read by the row's 16 lanes (one wavefront), and
                                                             // uniformly by every row: a barrier keeps it simple
        const int jn = min(KT, j_hi - j0 + 1);
        for (int jj = 0; jj < jn; ++jj) {
            const float pj = sc[r][jj];
#pragma unroll
            for (int t = 0; t < CPT; ++t) o[t] = fmaf(pj, vs[jj * HD + l * CPT + t], o[t]);
        }
    }
    if (i0 + r <= i1) {
        const float inv = 1.0f / l_run;                      // every live row keeps at least one key (host-checked masks)
#pragma unroll
        for (int t = 0; t < CPT; ++t) ctx[(b * P + i0 + r) * ldo + hoff + l * CPT + t] = o[t] * inv;
    }
}

// =====================================================================================================================
// decode_window: ONE workgroup of 1024 threads (integer plumbing of M * T tokens and one input row per sequence)
__device__ __forceinline__ uint64_t splitmix64_dev(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(1024) void decode_window_kernel(
    const int64_t* __restrict__ codes_full, int64_t nb, int64_t* __restrict__ chorale, int64_t ldch, int32_t* __restrict__ win,
    int advance, int64_t* __restrict__ codes_win, int S, int64_t* __restrict__ tokens, int T, int U, int P,
    int64_t* __restrict__ prefix_rows, const float* __restrict__ table, int64_t table_rows, int d, float* __restrict__ x,
    int64_t ldx, const int64_t* __restrict__ seeds_in, int64_t* __restrict__ seeds_out, int32_t* __restrict__ posp, int M) {
    const int tid = threadIdx.x;
    const int next = win[0], live = win[1], cur = min(max(*posp, 0), T);
    __syncthreads();                                         // every thread has read win and pos
    if (live >= 0 && (int64_t)live + S <= nb) {              // commit: the live window's tokens [0, pos) back into the chorale
        for (int e = tid; e < M * cur; e += 1024) {
            const int m = e / cur, j = e % cur;
            chorale[(int64_t)m * ldch + (int64_t)live * U + j] = tokens[(int64_t)m * T + j];
        }
    }
    __threadfence_block();
    __syncthreads();                                         // the load below reads what the commit wrote
    if (next < 0 || (int64_t)next + S > nb) return;          // commit only (uniform)
    const int64_t sos = table_rows - 1;
    for (int e = tid; e < M * S; e += 1024) {
        const int m = e / S, s = e % S;
        codes_win[e] = codes_full[(int64_t)m * nb + next + s];
    }
    for (int e = tid; e < M * T; e += 1024) {
        const int m = e / T, j = e % T;
        const int64_t tok = chorale[(int64_t)m * ldch + (int64_t)next * U + j];
        tokens[e] = tok;
        // the input row of position j + 1 (decoders/decoder.py:_target_rows): table row token * U + j % U
        if (j + 1 < P) prefix_rows[(int64_t)m * P + j + 1] = min(max(tok * U + j % U, (int64_t)0), sos - 1);
    }
    for (int m = tid; m < M; m += 1024) {
        if (P > 0) prefix_rows[(int64_t)m * P] = sos;
        const uint64_t sd = (uint64_t)seeds_in[m];
        // window 0 keeps the row's seed: a generation that never slides draws what the fixed-window generation draws
        seeds_out[m] = (int64_t)(next == 0 ? sd : splitmix64_dev(sd ^ ((uint64_t)next * 0xD1B54A32D192ED03ull)));
    }
    for (int e = tid; e < M * d; e += 1024) {                // the input row of position P
        const int m = e / d, c = e % d;
        int64_t row = sos;
        if (P > 0) {
            const int64_t tok = chorale[(int64_t)m * ldch + (int64_t)next * U + P - 1];
            row = min(max(tok * U + (P - 1) % U, (int64_t)0), sos - 1);
        }
        x[(int64_t)m * ldx + c] = table[row * d + c];
    }
    if (tid == 0) {
        *posp = P;
        win[0] = next + advance;
        win[1] = next;
    }
}

// =====================================================================================================================
// decode_source_rows: the source rows of a decoder on continuous latents, src = z W^T + b on the live window of z_full.
// A workgroup owns kSrcRows source rows x kSrcThreads output columns: the latents of its rows go through LDS (every lane
// reads the same address: a broadcast), a thread streams its own row of W as float4 and keeps one accumulator per row.
// Per output element: acc = 0, fmaf over k ascending, + bias -- a function of the row's latents and W's row alone.
constexpr int kSrcRows = 8;
constexpr int kSrcThreads = 128;
constexpr int kSrcMaxDz = 256;
constexpr int kSrcMaxS = 1024;

__global__ __launch_bounds__(kSrcThreads) void decode_source_rows_kernel(const float* __restrict__ z_full, int64_t nb, int dz,
                                                                         const int32_t* __restrict__ win,
                                                                         const float* __restrict__ w,
                                                                         const float* __restrict__ bias,
                                                                         float* __restrict__ src, int64_t lds, int64_t rows_all,
                                                                         int S, int N) {
    __shared__ float4 zs[kSrcRows * (kSrcMaxDz / 4)];
    const int w0 = win ? win[1] : 0;
    if (w0 < 0 || (int64_t)w0 + S > nb) return;              // no live window (uniform): src stays as it is
    const int64_t r0 = (int64_t)blockIdx.y * kSrcRows;
    const int rows = (int)min((int64_t)kSrcRows, rows_all - r0);
    const int q = dz / 4;
    for (int e = threadIdx.x; e < rows * q; e += kSrcThreads) {
        const int64_t row = r0 + e / q;
        const int64_t b = row / S, j = row % S;
        zs[(e / q) * (kSrcMaxDz / 4) + e % q] = reinterpret_cast<const float4*>(z_full + (b * nb + w0 + j) * dz)[e % q];
    }
    __syncthreads();
    const int n = blockIdx.x * kSrcThreads + threadIdx.x;
    if (n >= N) return;
    const float4* wr = reinterpret_cast<const float4*>(w + (int64_t)n * dz);
    float acc[kSrcRows];
#pragma unroll
    for (int r = 0; r < kSrcRows; ++r) acc[r] = 0.0f;
#pragma unroll 4
    for (int k = 0; k < q; ++k) {
        const float4 wv = wr[k];
#pragma unroll
        for (int r = 0; r < kSrcRows; ++r) {
            const float4 zv = zs[r * (kSrcMaxDz / 4) + k];   // rows past `rows` hold stale LDS: computed, never stored
            float a = acc[r];
            a = fmaf(zv.x, wv.x, a);
            a = fmaf(zv.y, wv.y, a);
            a = fmaf(zv.z, wv.z, a);
            a = fmaf(zv.w, wv.w, a);
            acc[r] = a;
        }
    }
    const float bn = bias ? bias[n] : 0.0f;
#pragma unroll
    for (int r = 0; r < kSrcRows; ++r)
        if (r < rows) src[(r0 + r) * lds + n] = bn + acc[r];
}

// =====================================================================================================================
// decode_sample: one workgroup of 16 wavefronts; wavefront w takes rows w, w + 16, ...  Lane l owns tokens 4l .. 4l + 3
// of the row (V_c <= 256), so the cumulative sums are a lane-serial scan of four plus a wave scan of the lane totals.
constexpr int kSampWaves = 16;

struct VoiceOffsets {
    int off[kDecMaxVoices + 1];
};

__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// CONS (vqcpc_decode_sample_constrained): `teacher` is the constraint -- per (row, column) a token to emit, or < 0 for a draw --
// and the emitted token's log-probability under the UNFILTERED row (temperature 1) goes to logp.  Both are addressed at column
// col = pos (win == NULL) or win[1] * U + pos, the chorale coordinate of the live window's position: one captured step serves
// every window.  A column outside [0, ldteach) / [0, ldlogp) is free / not written.  The log-sum-exp is a lane-serial sum of
// four and a butterfly over the 64 lanes: its order depends on nothing but the lane layout, so a row's value is the same
// whatever M.  Without CONS the kernel is what it was before the flag: none of the added code is instantiated.
// MASK (vqcpc_decode_sample_masked, on top of CONS): `allowed` [M][ldallow][8] holds per (row, column) a 256-bit set of the tokens
// that may be drawn, read at the same column as the constraint; lane l's four tokens are bits 4 (l & 7) .. + 3 of word l >> 3.
// A token outside the set becomes -inf where `exclude` is applied, so top-k, top-p and probs act on the set; a forced token
// ignores it.  Only bits [0, V) count and a set without any is no restriction.  logmass gets, at logp's column rule, the log
// of the share of the UNFILTERED row's probability that the set leaves open: (m_a - m) + log(s_a) - log(s) with the maximum
// and exp-sum of the row (the logp code's) and of its allowed tokens, both summed in the same lane order -- the full set gives
// exactly 0.  Without MASK none of this is instantiated.
template <bool CONS, bool MASK = false>
__global__ __launch_bounds__(64 * kSampWaves) void decode_sample_kernel(
    const float* __restrict__ logits, int64_t ldl, VoiceOffsets vo, int nc, int M, float temperature, int top_k, float top_p,
    const uint32_t* __restrict__ exclude, const int64_t* __restrict__ seeds, const int64_t* __restrict__ teacher,
    int64_t ldteach, int64_t* __restrict__ tokens, int64_t ldtok, int T, const float* __restrict__ table, int64_t table_rows,
    int d, int U, float* __restrict__ next_in, int64_t ldn, float* __restrict__ probs, int64_t ldp, int32_t* __restrict__ posp,
    float* __restrict__ logp, int64_t ldlogp, const int32_t* __restrict__ win, const uint32_t* __restrict__ allowed,
    int64_t ldallow, float* __restrict__ logmass, int64_t ldmass) {
    static_assert(CONS || !MASK, "the mask is addressed at the constraint's column");
    __shared__ float sl[kSampWaves][kDecMaxVocab];            // a wave's (filtered) logits
    __shared__ float srt[kSampWaves][kDecMaxVocab];           // top-p: probabilities in descending order, then their cumsum
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pos = *posp;
    const bool live_pos = pos >= 0 && pos < T;
    const int c = live_pos ? pos % nc : 0;
    const int V = vo.off[c + 1] - vo.off[c];
    const float ninf = -INFINITY;
    int64_t col = -1;                                         // CONS: the column of constraint / logp, < 0 = no live window
    if constexpr (CONS) {
        const int w0 = win ? win[1] : 0;
        if (live_pos && w0 >= 0) col = (int64_t)w0 * U + pos;
    }
    for (int r0 = 0; r0 < M; r0 += kSampWaves) {             // uniform trip count: every wave reaches every barrier
        const int b = r0 + wave;
        const bool act = live_pos && b < M;
        float l[4];
        float raw[4] = {ninf, ninf, ninf, ninf};              // CONS: the row as the model gave it
        uint32_t ok = 0xFu;                                   // MASK: bit t = token 4 * lane + t may be drawn
        if constexpr (MASK) {
            if (act && allowed && col >= 0 && col < ldallow) {        // uniform over the wave: the ballot runs in every lane
                const uint32_t word = allowed[((int64_t)b * ldallow + col) * 8 + (lane >> 3)];
                const int mine = V - 4 * lane;                         // this lane's tokens below V
                const uint32_t bits = (word >> ((lane & 7) * 4)) & (mine >= 4 ? 0xFu : mine > 0 ? (1u << mine) - 1u : 0u);
                if (__ballot(bits != 0u) != 0ull) ok = bits;           // an empty set restricts nothing
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = 4 * lane + t;
            float v = ninf;
            if (act && i < V) {
                v = logits[(int64_t)b * ldl + vo.off[c] + i];
                if constexpr (CONS) raw[t] = v;
                v = v / temperature;
                if (exclude && ((exclude[c * 8 + (i >> 5)] >> (i & 31)) & 1u)) v = ninf;
                if constexpr (MASK) {
                    if (!((ok >> t) & 1u)) v = ninf;
                }
            }
            l[t] = v;
            sl[wave][i] = v;
        }
        __syncthreads();
        // top-k (utils.py:111-114): drop logits < the k-th largest, i.e. those with at least k strictly larger ones
        if (act && top_k > 0 && top_k < V) {
            int gt[4] = {0, 0, 0, 0};
            for (int j = 0; j < V; ++j) {
                const float o = sl[wave][j];
#pragma unroll
                for (int t = 0; t < 4; ++t) gt[t] += o > l[t];
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (gt[t] >= top_k) l[t] = ninf;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) sl[wave][4 * lane + t] = l[t];
        __syncthreads();
        // top-p (utils.py:116-126): softmax over the sorted survivors, drop entries whose cumulative probability BEFORE
        // them exceeds top_p (the shift by one), the first is always kept
        const bool nucleus = top_p > 0.0f && top_p < 1.0f;
        int rank[4];
        if (act && nucleus) {
            float mx = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3]));
            mx = wave_max(mx);
            float e[4], s = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                e[t] = l[t] > ninf ? expf(l[t] - mx) : 0.0f;
                s += e[t];
            }
            const float inv = 1.0f / wave_sum(s);
#pragma unroll
            for (int t = 0; t < 4; ++t) rank[t] = 4 * lane + t;          // tokens >= V keep their own slot
            int gt[4] = {0, 0, 0, 0};
            for (int j = 0; j < V; ++j) {
                const float o = sl[wave][j];
#pragma unroll
                for (int t = 0; t < 4; ++t) gt[t] += (o > l[t]) | ((o == l[t]) & (j < 4 * lane + t));
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (4 * lane + t < V) rank[t] = gt[t];
                srt[wave][rank[t]] = 4 * lane + t < V ? e[t] * inv : 0.0f;
            }
        }
        __syncthreads();
        if (act && nucleus) {
            float v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = srt[wave][4 * lane + t];
            v[1] += v[0];
            v[2] += v[1];
            v[3] += v[2];
            const float base = wave_incl_scan(v[3], lane) - v[3];
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] += base;
#pragma unroll
            for (int t = 0; t < 4; ++t) srt[wave][4 * lane + t] = v[t];
        }
        __syncthreads();
        if (act && nucleus) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (rank[t] >= 1 && rank[t] < V && srt[wave][rank[t] - 1] > top_p) l[t] = ninf;
        }
        // softmax of the filtered row and one draw: the first token whose inclusive cumulative weight exceeds u * total
        if (act) {
            float mx = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3]));
            mx = wave_max(mx);
            float e[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) e[t] = l[t] > ninf ? expf(l[t] - mx) : 0.0f;
            float cum[4];
            cum[0] = e[0];
            cum[1] = cum[0] + e[1];
            cum[2] = cum[1] + e[2];
            cum[3] = cum[2] + e[3];
            const float base = wave_incl_scan(cum[3], lane) - cum[3];
#pragma unroll
            for (int t = 0; t < 4; ++t) cum[t] += base;
            const float total = __shfl(cum[3], 63, 64);
            if (probs) {
                const float inv = 1.0f / total;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (4 * lane + t < V) probs[(int64_t)b * ldp + 4 * lane + t] = e[t] * inv;
            }
            int tok;
            int64_t forced = -1;
            if constexpr (CONS) {
                if (teacher && col >= 0 && col < ldteach) forced = teacher[(int64_t)b * ldteach + col];
            }
            if (CONS ? forced >= 0 : teacher != nullptr) {
                tok = CONS ? (int)min(forced, (int64_t)kDecMaxVocab) : (int)teacher[(int64_t)b * ldteach + pos];
            } else {
                const uint64_t sd = (uint64_t)seeds[b];
                const uint32_t r = rng_u24_from_x0(rng_x0(sd, (uint32_t)pos), (uint32_t)(sd >> 32));
                const float target = ((float)r + 0.5f) * (1.0f / 16777216.0f) * total;
                // the first token of non-zero weight whose cumulative weight exceeds the target (the cumulative sums
                // need not be monotone to the last bit across lanes: the scan rounds in tree order); none (u * total
                // rounded up to total): the last token of non-zero weight
                int first = 1 << 30, last = -1;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (e[t] > 0.0f) {
                        if (cum[t] > target) first = min(first, 4 * lane + t);
                        last = 4 * lane + t;
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    first = min(first, __shfl_xor(first, o, 64));
                    last = max(last, __shfl_xor(last, o, 64));
                }
                tok = first < (1 << 30) ? first : last;
            }
            tok = min(max(tok, 0), V - 1);
            if (lane == 0) tokens[(int64_t)b * ldtok + pos] = tok;
            const int64_t row = min((int64_t)tok * U + pos % U, table_rows - 1);     // _target_rows: input of position pos + 1
            for (int k = lane; k < d; k += 64) next_in[(int64_t)b * ldn + k] = table[row * d + k];
            if constexpr (MASK) {
                const bool wl = logp && col >= 0 && col < ldlogp, wm = logmass && col >= 0 && col < ldmass;
                if (wl || wm) {                               // uniform, as below; rmx, rs and logp are formed as below
                    const float rmx = wave_max(fmaxf(fmaxf(raw[0], raw[1]), fmaxf(raw[2], raw[3])));
                    float rs = 0.0f;
#pragma unroll
                    for (int t = 0; t < 4; ++t) rs += raw[t] > ninf ? expf(raw[t] - rmx) : 0.0f;
                    rs = wave_sum(rs);
                    if (wl) {
                        const int tt = tok & 3;
                        const float mine = tt == 0 ? raw[0] : tt == 1 ? raw[1] : tt == 2 ? raw[2] : raw[3];
                        const float rt = __shfl(mine, tok >> 2, 64);
                        if (lane == 0) logp[(int64_t)b * ldlogp + col] = (rt - rmx) - logf(rs);
                    }
                    if (wm) {
                        float ar[4];
#pragma unroll
                        for (int t = 0; t < 4; ++t) ar[t] = (ok >> t) & 1u ? raw[t] : ninf;
                        const float amx = wave_max(fmaxf(fmaxf(ar[0], ar[1]), fmaxf(ar[2], ar[3])));
                        float as = 0.0f;
#pragma unroll
                        for (int t = 0; t < 4; ++t) as += ar[t] > ninf ? expf(ar[t] - amx) : 0.0f;
                        as = wave_sum(as);
                        if (lane == 0) logmass[(int64_t)b * ldmass + col] = (amx - rmx) + logf(as) - logf(rs);
                    }
                }
            } else if constexpr (CONS) {
                if (logp && col >= 0 && col < ldlogp) {       // uniform: the shuffles below run in every lane or in none
                    const float rmx = wave_max(fmaxf(fmaxf(raw[0], raw[1]), fmaxf(raw[2], raw[3])));
                    float rs = 0.0f;
#pragma unroll
                    for (int t = 0; t < 4; ++t) rs += raw[t] > ninf ? expf(raw[t] - rmx) : 0.0f;
                    rs = wave_sum(rs);
                    const int tt = tok & 3;
                    const float mine = tt == 0 ? raw[0] : tt == 1 ? raw[1] : tt == 2 ? raw[2] : raw[3];
                    const float rt = __shfl(mine, tok >> 2, 64);
                    if (lane == 0) logp[(int64_t)b * ldlogp + col] = (rt - rmx) - logf(rs);
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && live_pos) *posp = pos + 1;      // after the barrier: every thread has read pos
}

}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_decode_linear(const float* x, int64_t ldx, const int64_t* gather, const float* w, const float* bias, const float* res,
                        int64_t ldr, float* y, int64_t ldy, int64_t M, int N, int K, int relu, void* stream) {
    VQ_REQUIRE(x && w && y && M >= 1 && M <= kDecMaxRows && N >= 1 && N <= kDecMaxDim && K >= 4 && K <= kDecMaxDim && K % 4 == 0,
               "decode_linear: bad arguments (1 <= M <= 64, 1 <= N <= 4096, 4 <= K <= 4096, K %% 4 == 0)");
    VQ_REQUIRE(ldx >= K && ldx % 4 == 0 && ldy >= N && (!res || ldr >= N) && aligned16(x) && aligned16(w),
               "decode_linear: bad leading dimensions or alignment");
    VQ_REQUIRE(x != y, "decode_linear: y may not alias x");
    const int cols = kLinWaves * kLinCols;
    const dim3 grid((unsigned)ceil_div(N, cols)), block(64 * kLinWaves);
    hipStream_t s = (hipStream_t)stream;
    if (M <= 8)
        hipLaunchKernelGGL(decode_linear_kernel<8>, grid, block, 0, s, x, ldx, gather, w, bias, res, ldr, y, ldy, (int)M, N, K,
                           relu);
    else
        hipLaunchKernelGGL(decode_linear_kernel<32>, grid, block, 0, s, x, ldx, gather, w, bias, res, ldr, y, ldy, (int)M, N, K,
                           relu);
    VQ_CHECK_LAUNCH("decode_linear");
    return VQCPC_OK;
}

// the two attention entry points share their checks and their launch; `name` is the one the caller's errors carry
static int decode_attn_launch(const char* name, const float* q, int64_t ldq, float* k_cache, float* v_cache, int64_t ldc,
                              const float* k_new, const float* v_new, int64_t ldn, const float* e1, const float* e2, float* ctx,
                              int64_t ldo, const int32_t* pos, int64_t M, int Lk, int ratio, int H, int hd, int mask, bool want_probs,
                              float* probs, int64_t ldp, int64_t rows, const int32_t* win, int win_stride, void* stream) {
    VQ_REQUIRE(q && k_cache && v_cache && e1 && e2 && ctx && pos && M >= 1 && M <= kDecMaxRows && Lk >= 1 && Lk <= kDecMaxLk &&
               ratio >= 1 && H >= 1 && mask >= 0 && mask <= 2,
               "%s: bad arguments (1 <= M <= 64, 1 <= Lk <= 1024, mask in {0, 1, 2})", name);
    VQ_REQUIRE(hd == 16 || hd == 32 || hd == 64 || hd == 128, "%s: hd must be 16, 32, 64 or 128 (got %d)", name, hd);
    const int64_t d = (int64_t)H * hd;
    VQ_REQUIRE(ldq >= d && ldc >= d && ldo >= d && ldq % 4 == 0 && ldc % 4 == 0 && aligned16(q) && aligned16(k_cache) &&
               aligned16(e1) && aligned16(e2), "%s: bad leading dimensions or alignment", name);
    VQ_REQUIRE((k_new == nullptr) == (v_new == nullptr), "%s: k_new and v_new go together", name);
    if (k_new)
        VQ_REQUIRE(mask == 1 && ratio == 1 && ldn >= d && ldn % 4 == 0 && aligned16(k_new),
                   "%s: self mode (k_new given) is causal with ratio 1", name);
    if (want_probs)
        VQ_REQUIRE(probs && ldp >= Lk && rows >= 1 && (!win || win_stride >= 1),
                   "%s: probs [M][H][rows][ldp] needs probs != NULL, ldp >= Lk, rows >= 1 (and win_stride >= 1 with win)", name);
    const float scale = 1.0f / sqrtf((float)hd);
    const dim3 grid((unsigned)(M * H)), block(256);
    hipStream_t s = (hipStream_t)stream;
#define DEC_ATTN(HD, PROBS)                                                                                                    \
    hipLaunchKernelGGL((decode_attn_kernel<HD, PROBS>), grid, block, 0, s, q, ldq, k_cache, v_cache, ldc, k_new, v_new, ldn,   \
                       e1, e2, ctx, ldo, pos, Lk, ratio, H, mask, scale, probs, ldp, rows, win, win_stride)
    if (want_probs) {
        switch (hd) {
            case 16: DEC_ATTN(16, true); break;
            case 32: DEC_ATTN(32, true); break;
            case 64: DEC_ATTN(64, true); break;
            default: DEC_ATTN(128, true); break;
        }
    } else {
        switch (hd) {
            case 16: DEC_ATTN(16, false); break;
            case 32: DEC_ATTN(32, false); break;
            case 64: DEC_ATTN(64, false); break;
            default: DEC_ATTN(128, false); break;
        }
    }
#undef DEC_ATTN
    VQ_CHECK_LAUNCH(name);
    return VQCPC_OK;
}

int vqcpc_decode_attn(const float* q, int64_t ldq, float* k_cache, float* v_cache, int64_t ldc, const float* k_new,
                      const float* v_new, int64_t ldn, const float* e1, const float* e2, float* ctx, int64_t ldo,
                      const int32_t* pos, int64_t M, int Lk, int ratio, int H, int hd, int mask, void* stream) {
    return decode_attn_launch("decode_attn", q, ldq, k_cache, v_cache, ldc, k_new, v_new, ldn, e1, e2, ctx, ldo, pos, M, Lk, ratio,
                              H, hd, mask, false, nullptr, 0, 0, nullptr, 0, stream);
}

int vqcpc_decode_attn_probs(const float* q, int64_t ldq, float* k_cache, float* v_cache, int64_t ldc, const float* k_new,
                            const float* v_new, int64_t ldn, const float* e1, const float* e2, float* ctx, int64_t ldo,
                            const int32_t* pos, int64_t M, int Lk, int ratio, int H, int hd, int mask, float* probs, int64_t ldp,
                            int64_t rows, const int32_t* win, int win_stride, void* stream) {
    return decode_attn_launch("decode_attn_probs", q, ldq, k_cache, v_cache, ldc, k_new, v_new, ldn, e1, e2, ctx, ldo, pos, M, Lk,
                              ratio, H, hd, mask, true, probs, ldp, rows, win, win_stride, stream);
}

// the three sampler entry points share their checks and their launch in the same way.  cons: the constrained forms -- `fixed` is the
// constraint (the plain form's teacher tokens otherwise) and seeds are required; mask: allowed / logmass on top of that
static int decode_sample_launch(const char* name, bool cons, bool mask, const float* logits, int64_t ldl, const int32_t* voice_offsets,
                                int nc, int64_t M, float temperature, int top_k, float top_p, const uint32_t* exclude,
                                const int64_t* seeds, const int64_t* fixed, int64_t ldfixed, float* logp, int64_t ldlogp,
                                const int32_t* win, const uint32_t* allowed, int64_t ldallow, float* logmass, int64_t ldmass,
                                int64_t* tokens, int64_t ldtok, int T, const float* table, int64_t table_rows, int d, int U,
                                float* next_in, int64_t ldn, float* probs, int64_t ldp, int32_t* pos, void* stream) {
    VQ_REQUIRE(logits && voice_offsets && tokens && table && next_in && pos && nc >= 1 && nc <= kDecMaxVoices && M >= 1 &&
               M <= kDecMaxRows && T >= 1 && d >= 1 && d <= kDecMaxDim && U >= 1 && table_rows >= 1,
               "%s: bad arguments (1 <= M <= 64, 1 <= nc <= 16, 1 <= d <= 4096)", name);
    VQ_REQUIRE(temperature > 0.0f && top_k >= 0 && top_p == top_p, "%s: temperature > 0, top_k >= 0", name);
    VQ_REQUIRE(seeds || (!cons && fixed), "%s: seeds are needed%s", name, cons ? "" : " unless the tokens are teacher-forced");
    VoiceOffsets vo;
    vo.off[0] = voice_offsets[0];
    VQ_REQUIRE(vo.off[0] >= 0, "%s: negative voice offset", name);
    int vmax = 0;
    for (int c = 0; c < nc; ++c) {
        const int V = voice_offsets[c + 1] - voice_offsets[c];
        VQ_REQUIRE(V >= 1 && V <= kDecMaxVocab, "%s: voice %d has %d tokens (1 <= V_c <= 256)", name, c, V);
        vo.off[c + 1] = voice_offsets[c + 1];
        vmax = std::max(vmax, V);
    }
    for (int c = nc + 1; c <= kDecMaxVoices; ++c) vo.off[c] = vo.off[nc];
    VQ_REQUIRE(ldl >= vo.off[nc] && ldtok >= T && ldn >= d && (!probs || ldp >= vmax), "%s: bad leading dimensions", name);
    // the window index lives on the device: with win the host can only ask for one window's columns, and the kernel
    // treats a column at or past the leading dimension as free / does not write it
    VQ_REQUIRE((!fixed || ldfixed >= T) && (!logp || ldlogp >= T), "%s: bad leading dimensions (%s >= T)", name,
               cons ? "ldcons, ldlogp" : "ldteach");
    VQ_REQUIRE((!allowed || ldallow >= T) && (!logmass || ldmass >= T), "%s: bad leading dimensions (ldallow, ldmass >= T)", name);
    VQ_REQUIRE((int64_t)(vmax - 1) * U + (U - 1) < table_rows, "%s: the table has too few rows for V_c * U", name);
    const auto kern = mask ? decode_sample_kernel<true, true> : cons ? decode_sample_kernel<true> : decode_sample_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(1), dim3(64 * kSampWaves), 0, (hipStream_t)stream, logits, ldl, vo, nc, (int)M, temperature, top_k,
                       top_p, exclude, seeds, fixed, ldfixed, tokens, ldtok, T, table, table_rows, d, U, next_in, ldn, probs, ldp, pos,
                       logp, ldlogp, win, allowed, ldallow, logmass, ldmass);
    VQ_CHECK_LAUNCH(name);
    return VQCPC_OK;
}

int vqcpc_decode_sample(const float* logits, int64_t ldl, const int32_t* voice_offsets, int nc, int64_t M, float temperature,
                        int top_k, float top_p, const uint32_t* exclude, const int64_t* seeds, const int64_t* teacher,
                        int64_t ldteach, int64_t* tokens, int64_t ldtok, int T, const float* table, int64_t table_rows, int d,
                        int U, float* next_in, int64_t ldn, float* probs, int64_t ldp, int32_t* pos, void* stream) {
    return decode_sample_launch("decode_sample", false, false, logits, ldl, voice_offsets, nc, M, temperature, top_k, top_p, exclude,
                                seeds, teacher, ldteach, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, tokens, ldtok, T, table,
                                table_rows, d, U, next_in, ldn, probs, ldp, pos, stream);
}

int vqcpc_decode_sample_constrained(const float* logits, int64_t ldl, const int32_t* voice_offsets, int nc, int64_t M,
                                    float temperature, int top_k, float top_p, const uint32_t* exclude, const int64_t* seeds,
                                    const int64_t* constraint, int64_t ldcons, float* logp, int64_t ldlogp, const int32_t* win,
                                    int64_t* tokens, int64_t ldtok, int T, const float* table, int64_t table_rows, int d, int U,
                                    float* next_in, int64_t ldn, float* probs, int64_t ldp, int32_t* pos, void* stream) {
    return decode_sample_launch("decode_sample_constrained", true, false, logits, ldl, voice_offsets, nc, M, temperature, top_k, top_p,
                                exclude, seeds, constraint, ldcons, logp, ldlogp, win, nullptr, 0, nullptr, 0, tokens, ldtok, T, table,
                                table_rows, d, U, next_in, ldn, probs, ldp, pos, stream);
}

int vqcpc_decode_sample_masked(const float* logits, int64_t ldl, const int32_t* voice_offsets, int nc, int64_t M, float temperature,
                               int top_k, float top_p, const uint32_t* exclude, const int64_t* seeds, const int64_t* constraint,
                               int64_t ldcons, float* logp, int64_t ldlogp, const int32_t* win, const uint32_t* allowed,
                               int64_t ldallow, float* logmass, int64_t ldmass, int64_t* tokens, int64_t ldtok, int T,
                               const float* table, int64_t table_rows, int d, int U, float* next_in, int64_t ldn, float* probs,
                               int64_t ldp, int32_t* pos, void* stream) {
    return decode_sample_launch("decode_sample_masked", true, true, logits, ldl, voice_offsets, nc, M, temperature, top_k, top_p,
                                exclude, seeds, constraint, ldcons, logp, ldlogp, win, allowed, ldallow, logmass, ldmass, tokens,
                                ldtok, T, table, table_rows, d, U, next_in, ldn, probs, ldp, pos, stream);
}

int vqcpc_decode_prefill_attn(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldk, float* k_cache,
                              float* v_cache, int64_t ldc, const float* e1, const float* e2, float* ctx, int64_t ldo, int64_t M,
                              int P, int Lk, int ratio, int H, int hd, int mask, void* stream) {
    VQ_REQUIRE(k && v && e1 && e2 && M >= 1 && M <= kDecMaxRows && Lk >= 1 && Lk <= kDecMaxLk && ratio >= 1 && H >= 1 &&
               mask >= 0 && mask <= 2 && P >= 0 && (int64_t)P <= (int64_t)ratio * Lk,
               "decode_prefill_attn: bad arguments (1 <= M <= 64, 1 <= Lk <= 1024, 0 <= P <= ratio * Lk, mask in {0, 1, 2})");
    VQ_REQUIRE(hd == 16 || hd == 32 || hd == 64 || hd == 128, "decode_prefill_attn: hd must be 16, 32, 64 or 128 (got %d)", hd);
    const int64_t d = (int64_t)H * hd;
    VQ_REQUIRE((k_cache == nullptr) == (v_cache == nullptr), "decode_prefill_attn: k_cache and v_cache go together");
    VQ_REQUIRE(ctx || k_cache, "decode_prefill_attn: ctx may be NULL in self mode only (store the prefix k | v and stop)");
    VQ_REQUIRE(!ctx || (q && ldq >= d && ldq % 4 == 0 && ldo >= d && aligned16(q)), "decode_prefill_attn: bad q / ctx");
    VQ_REQUIRE(ldk >= d && ldk % 4 == 0 && aligned16(k) && aligned16(v) && aligned16(e1) && aligned16(e2),
               "decode_prefill_attn: bad leading dimensions or alignment");
    if (k_cache)
        VQ_REQUIRE(mask == 1 && ratio == 1 && ldc >= d && ldc % 4 == 0 && aligned16(k_cache) && aligned16(v_cache),
                   "decode_prefill_attn: self mode (k_cache given) is causal with ratio 1");
    if (P == 0) return VQCPC_OK;
    const float scale = 1.0f / sqrtf((float)hd);
    const dim3 grid((unsigned)ceil_div(P, kPfRows), (unsigned)(M * H)), block(256);
    hipStream_t s = (hipStream_t)stream;
#define DEC_PF(HD, KT)                                                                                                         \
    hipLaunchKernelGGL((decode_prefill_attn_kernel<HD, KT>), grid, block, 0, s, q, ldq, k, v, ldk, k_cache, v_cache, ldc, e1,  \
                       e2, ctx, ldo, P, Lk, ratio, H, mask, scale)
    switch (hd) {
        case 16: DEC_PF(16, 32); break;
        case 32: DEC_PF(32, 32); break;
        case 64: DEC_PF(64, 32); break;
        default: DEC_PF(128, 16); break;
    }
#undef DEC_PF
    VQ_CHECK_LAUNCH("decode_prefill_attn");
    return VQCPC_OK;
}

int vqcpc_decode_window(const int64_t* codes_full, int64_t nb, int64_t* chorale, int64_t ldch, int32_t* win, int advance,
                        int64_t* codes_win, int S, int64_t* tokens, int T, int U, int P, int64_t* prefix_rows,
                        const float* table, int64_t table_rows, int d, float* x, int64_t ldx, const int64_t* seeds_in,
                        int64_t* seeds_out, int32_t* pos, int64_t M, void* stream) {
    VQ_REQUIRE(codes_full && chorale && win && codes_win && tokens && table && x && seeds_in && seeds_out && pos && M >= 1 &&
               M <= kDecMaxRows, "decode_window: bad arguments (1 <= M <= 64)");
    VQ_REQUIRE(S >= 1 && U >= 1 && T == S * U && nb >= S && ldch >= nb * U && P >= 0 && P < T && (P == 0 || prefix_rows) &&
               d >= 1 && d <= kDecMaxDim && ldx >= d && table_rows >= 2 && advance >= 0,
               "decode_window: T == S * U, nb >= S, ldch >= nb * U, 0 <= P < T, 1 <= d <= 4096");
    hipLaunchKernelGGL(decode_window_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, codes_full, nb, chorale, ldch, win,
                       advance, codes_win, S, tokens, T, U, P, prefix_rows, table, table_rows, d, x, ldx, seeds_in, seeds_out,
                       pos, (int)M);
    VQ_CHECK_LAUNCH("decode_window");
    return VQCPC_OK;
}

int vqcpc_decode_source_rows(const float* z_full, int64_t nb, int dz, const int32_t* win, const float* w, const float* bias,
                             float* src, int64_t lds, int64_t M, int S, int N, void* stream) {
    VQ_REQUIRE(z_full && w && src && M >= 1 && M <= kDecMaxRows && S >= 1 && S <= kSrcMaxS && N >= 1 && N <= kDecMaxDim &&
               dz >= 4 && dz <= kSrcMaxDz && dz % 4 == 0,
               "decode_source_rows: bad arguments (1 <= M <= 64, 1 <= S <= 1024, 1 <= N <= 4096, 4 <= dz <= 256, dz %% 4 == 0)");
    VQ_REQUIRE(nb >= S && lds >= N && aligned16(z_full) && aligned16(w),
               "decode_source_rows: nb >= S, lds >= N, z_full and w 16-byte aligned");
    const int64_t rows = M * S;
    const dim3 grid((unsigned)ceil_div(N, kSrcThreads), (unsigned)ceil_div(rows, (int64_t)kSrcRows)), block(kSrcThreads);
    hipLaunchKernelGGL(decode_source_rows_kernel, grid, block, 0, (hipStream_t)stream, z_full, nb, dz, win, w, bias, src, lds,
                       rows, S, N);
    VQ_CHECK_LAUNCH("decode_source_rows");
    return VQCPC_OK;
}

}  // extern "C"
