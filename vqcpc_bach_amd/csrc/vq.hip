// Product vector quantiser: LDS-staged codebook, four lanes per row, canonical (non-FMA, t-ascending, k-ascending) distances.
// Compiled with -ffp-contract=off; the distance uses explicitly rounded __fsub_rn/__fmul_rn/__fadd_rn so that the
// argmin is bit-identical to oracle/vqcpc_oracle.py:vq_distances_canonical (reference: vector_quantizer.py:105-116).
#include "common.h"

namespace vq {

constexpr int kVqThreads = 256;
constexpr int kVqLdsFloats = 36 * 1024;  // 144 KiB of codebook per workgroup at most

// ---------------------------------------------------------------------------------------------------------------------
// forward.  kVqLpr = 4 lanes share one row (64 rows per workgroup: 544 workgroups at C1's 34 816 rows, 2 waves per SIMD on
// every CU; one row per lane gave 136 workgroups on 256 CUs).  Lane j of a row scans the codes k = j, j + 4, j + 8, ...
// of the LDS-staged codebook -- the four lanes of a row read four consecutive codes (64 bytes apart at dsub = 16:
// distinct banks) and the 16 rows of a wave read the same addresses (broadcast) -- and the four partial results meet in a
// two-step shuffle.  Every distance is the canonical chain (t ascending, separately rounded sub / mul / add); a lane keeps
// the FIRST minimum of its ascending code list (strict '<') and the merge prefers the smaller distance, then the smaller
// index: exactly the sequential k-ascending scan with strict '<' (ties -> first index; a NaN distance never replaces,
// and a NaN at k = 0 stays, as in the sequential scan).  The z rows of a wave are 16 consecutive rows = one contiguous
// 16 * D * 4-byte stretch, read as float4 (the four lanes of a row read the same 64 bytes).
// DSUB > 0: sub-vector kept in registers; DSUB == 0: runtime dsub, sub-vector re-read from global (L1) per code.
constexpr int kVqLpr = 4;                          // lanes per row
constexpr int kVqRows = kVqThreads / kVqLpr;       // rows per workgroup

template <int DSUB>
__global__ __launch_bounds__(kVqThreads) void vq_fwd_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                            int64_t R, int ncb, int K, int dsub_rt, float beta,
                                                            int squared, int assign, int64_t* __restrict__ idx_out,
                                                            float* __restrict__ zq_out, float* __restrict__ loss_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int dsub = DSUB > 0 ? DSUB : dsub_rt;
    const int D = ncb * dsub;
    const int j = threadIdx.x & (kVqLpr - 1);
    const int64_t r = (int64_t)blockIdx.x * kVqRows + (threadIdx.x >> 2);
    const bool live = r < R;
    const float* zr = z + (live ? r : 0) * D;
    float lsum = 0.0f;   // sum over the whole row of (q - z)^2   or  ((q - z) + eps)^2   (lane 0 of the row)
    const float kInf = __builtin_inff();

    for (int c = 0; c < ncb; ++c) {
        __syncthreads();
        const float* src = cb + (int64_t)c * K * dsub;
        if ((K * dsub) % 4 == 0) {
            for (int i = threadIdx.x * 4; i < K * dsub; i += kVqThreads * 4)
                *reinterpret_cast<float4*>(lds + i) = *reinterpret_cast<const float4*>(src + i);
        } else {
            for (int i = threadIdx.x; i < K * dsub; i += kVqThreads) lds[i] = src[i];
        }
        __syncthreads();

        float x[DSUB > 0 ? DSUB : 1];
        if (DSUB > 0) {
            if (DSUB % 4 == 0) {
#pragma unroll
                for (int t = 0; t < DSUB; t += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(zr + c * DSUB + t);
                    x[t] = v.x, x[t + 1] = v.y, x[t + 2] = v.z, x[t + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int t = 0; t < DSUB; ++t) x[t] = zr[c * DSUB + t];
            }
        }
        // lane-local scan of the codes j, j + 4, ...: lane 0 starts from code 0 unconditionally (the sequential scan's
        // k == 0), the others from "nothing yet" = (+inf, -1): +inf never replaces anything in the sequential scan either
        float best = kInf;
        int bi = -1;
        if (assign) {
            int k = j;
            if (DSUB > 0) {
                // four codes at a time: four independent canonical chains whose latencies overlap; candidates are compared
                // in code order with the same strict '<'
                constexpr int KU = 4;
                for (; k + (KU - 1) * kVqLpr < K; k += KU * kVqLpr) {
                    float dd[KU];
#pragma unroll
                    for (int u = 0; u < KU; ++u) dd[u] = 0.0f;
#pragma unroll
                    for (int t = 0; t < DSUB; ++t) {
#pragma unroll
                        for (int u = 0; u < KU; ++u) {
                            const float df = __fsub_rn(x[t], lds[(k + u * kVqLpr) * DSUB + t]);
                            dd[u] = __fadd_rn(dd[u], __fmul_rn(df, df));
                        }
                    }
#pragma unroll
                    for (int u = 0; u < KU; ++u) {
                        const int kk = k + u * kVqLpr;
                        if (kk == 0 || dd[u] < best) {
                            best = dd[u];
                            bi = kk;
                        }
                    }
                }
            }
            for (; k < K; k += kVqLpr) {
                const float* e = lds + k * dsub;
                float d = 0.0f;
                if (DSUB > 0) {
#pragma unroll
                    for (int t = 0; t < DSUB; ++t) {
                        const float df = __fsub_rn(x[t], e[t]);
                        d = __fadd_rn(d, __fmul_rn(df, df));
                    }
                } else {
                    for (int t = 0; t < dsub; ++t) {
                        const float df = __fsub_rn(zr[c * dsub + t], e[t]);
                        d = __fadd_rn(d, __fmul_rn(df, df));
                    }
                }
                if (k == 0 || d < best) {   // strict '<': the first index wins ties; NaN never replaces
                    best = d;
                    bi = k;
                }
            }
            // merge the four lanes of the row: smaller distance, then smaller index; "nothing yet" never wins; a NaN kept
            // from code 0 (bi == 0 in lane 0) is never replaced because every comparison with it is false
#pragma unroll
            for (int o = 1; o < kVqLpr; o <<= 1) {
                const float od = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                const bool take = oi >= 0 && (bi < 0 || od < best || (od == best && oi < bi));
                // a NaN at code 0 must survive: it sits in the lane that holds bi == 0, and (x < NaN), (x == NaN) are false
                // there; the OTHER lanes see od = NaN, oi = 0 and must adopt it: sequentially nothing ever replaces it
                const bool other_is_stuck_nan = oi == 0 && od != od;
                const bool mine_is_stuck_nan = bi == 0 && best != best;
                if (!mine_is_stuck_nan && (take || other_is_stuck_nan)) {
                    best = od;
                    bi = oi;
                }
            }
        } else {
            bi = live ? (int)idx_out[r * ncb + c] : 0;       // assign == 0: indices are given (label corruption path)
        }
        if (!live || j != 0) continue;                        // one lane per row finishes the row
        if (assign) idx_out[r * ncb + c] = (int64_t)bi;
        if (!zq_out) continue;                                // index-only (inference) mode
        const float* q = lds + bi * dsub;
        for (int t = 0; t < dsub; ++t) {
            const float xv = zr[c * dsub + t];
            const float diff = __fsub_rn(q[t], xv);                 // (quantized - inputs)
            zq_out[r * D + c * dsub + t] = __fadd_rn(xv, diff);     // inputs + (quantized - inputs).detach()
            const float v = squared ? diff : __fadd_rn(diff, 1e-5f);
            lsum = __fadd_rn(lsum, __fmul_rn(v, v));
        }
    }
    if (live && j == 0 && loss_out) {
        const float l = squared ? lsum : sqrtf(lsum);
        loss_out[r] = __fadd_rn(l, __fmul_rn(beta, l));             // q_latent + commitment_cost * e_latent
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward.  Workgroup = chunk of 256 rows.  Phase A (lane = row): d_z and the per-row codebook contribution
// val = g_loss * dloss/dq, kept in LDS.  Phase B per codebook: cell (k, t) of an LDS accumulator is owned by exactly
// one lane, rows are applied in ascending order -> deterministic segment sum, no atomics.  Partials go to workspace.
__global__ __launch_bounds__(kVqThreads) void vq_bwd_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                            const int64_t* __restrict__ idx, const float* __restrict__ g_zq,
                                                            const float* __restrict__ g_loss, int64_t R, int ncb, int K,
                                                            int dsub, float beta, int squared, float* __restrict__ d_z,
                                                            float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = ncb * dsub;
    float* acc = lds;                               // [K][dsub]
    float* val = lds + K * dsub;                    // [256][dsub]  (current codebook)
    int* sidx = reinterpret_cast<int*>(val + kVqThreads * dsub);   // [256]
    const int64_t r = (int64_t)blockIdx.x * kVqThreads + threadIdx.x;
    const bool live = r < R;
    const int rows_here = (int)min((int64_t)kVqThreads, R - (int64_t)blockIdx.x * kVqThreads);

    // row norm for the non-squared variant: n = || (q - z) + eps || over the full D
    float inv_n = 0.0f;
    if (live && !squared) {
        float s = 0.0f;
        for (int c = 0; c < ncb; ++c) {
            const float* q = cb + ((int64_t)c * K + idx[r * ncb + c]) * dsub;
            for (int t = 0; t < dsub; ++t) {
                const float v = (q[t] - z[r * D + c * dsub + t]) + 1e-5f;
                s += v * v;
            }
        }
        inv_n = 1.0f / sqrtf(s);
    }
    const float gl = live ? g_loss[r] : 0.0f;

    for (int c = 0; c < ncb; ++c) {
        __syncthreads();
        for (int i = threadIdx.x; i < K * dsub; i += kVqThreads) acc[i] = 0.0f;
        if (live) {
            const int k = (int)idx[r * ncb + c];
            sidx[threadIdx.x] = k;
            const float* q = cb + ((int64_t)c * K + k) * dsub;
            for (int t = 0; t < dsub; ++t) {
                const int col = c * dsub + t;
                const float diff = q[t] - z[r * D + col];
                // dloss/dq_t  (q_latent term) and dloss/dz_t (commitment term)
                const float dq = squared ? 2.0f * diff : (diff + 1e-5f) * inv_n;
                val[threadIdx.x * dsub + t] = gl * dq;
                d_z[r * D + col] = g_zq[r * D + col] - gl * beta * dq;
            }
        }
        __syncthreads();
        // owner of cell (k, t): lane ((k % kgroups) * dsub + t)
        const int kgroups = kVqThreads / dsub;      // >= 1: the host's LDS check admits dsub <= 158 at most
        const int my_t = threadIdx.x % dsub, my_g = threadIdx.x / dsub;
        if (my_g < kgroups) {
            // k % kgroups per row is a scalar division (8 600 scalar instructions per wave at 256 rows x 2 codebooks:
            // profiles/r03_pmc_kernels_c1.txt); kgroups is a power of two for every dsub that divides 256
            const bool pow2 = (kgroups & (kgroups - 1)) == 0;
            const int kmask = kgroups - 1;
            for (int row = 0; row < rows_here; ++row) {
                const int k = sidx[row];
                const int kg = pow2 ? (k & kmask) : (k % kgroups);
                if (kg == my_g) acc[k * dsub + my_t] += val[row * dsub + my_t];
            }
        }
        __syncthreads();
        float* dst = ws + ((int64_t)blockIdx.x * ncb + c) * K * dsub;
        for (int i = threadIdx.x; i < K * dsub; i += kVqThreads) dst[i] = acc[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// EMA codebooks (EMAProductVectorQuantizer).  Three kernels; vq_fwd / vq_bwd above are untouched.
//
// statistics.  Per codebook c and code k: the number of rows assigned to k and the sum of their sub-vectors,
// stats [ncb][K][W], W = 1 + dsub (column 0 = count, columns 1.. = sum).  The scheme of vq_bwd_kernel's phase B: workgroup =
// chunk of 256 rows, the chunk's rows staged in LDS as val[256][W] = (1.0f, z sub-vector), cell (k, t) of the LDS accumulator
// owned by exactly one lane (lane (k % kgroups) * W + t), rows applied in ascending order -> deterministic segment sum, no
// atomics; partials go to the workspace and launch_reduce_splits adds the chunks in chunk order.  k % kgroups is taken once
// per row by the row's own lane (kgroups = 256 / W is rarely a power of two here: 15 at dsub = 16).  A row whose index is
// outside [0, K) is skipped (its group is -1: no lane owns it), never dereferenced.
__global__ __launch_bounds__(kVqThreads) void vq_ema_stats_kernel(const float* __restrict__ z, const int64_t* __restrict__ idx,
                                                                  int64_t R, int ncb, int K, int dsub, float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int W = dsub + 1;
    const int D = ncb * dsub;
    float* acc = lds;                                              // [K][W]
    float* val = lds + (size_t)K * W;                              // [256][W]
    int* sidx = reinterpret_cast<int*>(val + kVqThreads * W);      // [256] code of the row
    int* sgrp = sidx + kVqThreads;                                 // [256] code % kgroups, -1: skip the row
    const int64_t r = (int64_t)blockIdx.x * kVqThreads + threadIdx.x;
    const bool live = r < R;
    const int rows_here = (int)min((int64_t)kVqThreads, R - (int64_t)blockIdx.x * kVqThreads);
    const int kgroups = kVqThreads / W;                            // W <= 256 checked on the host
    const int my_t = threadIdx.x % W, my_g = threadIdx.x / W;

    for (int c = 0; c < ncb; ++c) {
        __syncthreads();
        for (int i = threadIdx.x; i < K * W; i += kVqThreads) acc[i] = 0.0f;
        if (live) {
            const int64_t k64 = idx[r * ncb + c];
            const bool ok = k64 >= 0 && k64 < (int64_t)K;
            sidx[threadIdx.x] = ok ? (int)k64 : 0;
            sgrp[threadIdx.x] = ok ? (int)(k64 % kgroups) : -1;
            val[threadIdx.x * W] = 1.0f;
            for (int t = 0; t < dsub; ++t) val[threadIdx.x * W + 1 + t] = z[r * D + c * dsub + t];
        }
        __syncthreads();
        if (my_g < kgroups) {
            for (int row = 0; row < rows_here; ++row) {
                if (sgrp[row] == my_g) acc[sidx[row] * W + my_t] += val[row * W + my_t];
            }
        }
        __syncthreads();
        float* dst = ws + ((int64_t)blockIdx.x * ncb + c) * K * W;
        for (int i = threadIdx.x; i < K * W; i += kVqThreads) dst[i] = acc[i];
    }
}

// commitment backward: d_z = g_zq + g_loss * beta * dl/dz only (lane = row, the arithmetic of vq_bwd_kernel's phase A, so the
// squared form gives vq_bwd's d_z bit for bit); no segment sum, no LDS.  A row with an index outside [0, K) gets d_z = g_zq.
__global__ __launch_bounds__(kVqThreads) void vq_commit_bwd_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                                   const int64_t* __restrict__ idx,
                                                                   const float* __restrict__ g_zq,
                                                                   const float* __restrict__ g_loss, int64_t R, int ncb, int K,
                                                                   int dsub, float beta, int squared, float* __restrict__ d_z) {
    const int D = ncb * dsub;
    const int64_t r = (int64_t)blockIdx.x * kVqThreads + threadIdx.x;
    if (r >= R) return;
    bool ok = true;
    for (int c = 0; c < ncb; ++c) {
        const int64_t k = idx[r * ncb + c];
        ok = ok && k >= 0 && k < (int64_t)K;
    }
    if (!ok) {
        for (int col = 0; col < D; ++col) d_z[r * D + col] = g_zq[r * D + col];
        return;
    }
    float inv_n = 0.0f;
    if (!squared) {
        float s = 0.0f;
        for (int c = 0; c < ncb; ++c) {
            const float* q = cb + ((int64_t)c * K + idx[r * ncb + c]) * dsub;
            for (int t = 0; t < dsub; ++t) {
                const float v = (q[t] - z[r * D + c * dsub + t]) + 1e-5f;
                s += v * v;
            }
        }
        inv_n = 1.0f / sqrtf(s);
    }
    const float gl = g_loss[r];
    for (int c = 0; c < ncb; ++c) {
        const float* q = cb + ((int64_t)c * K + idx[r * ncb + c]) * dsub;
        for (int t = 0; t < dsub; ++t) {
            const int col = c * dsub + t;
            const float diff = q[t] - z[r * D + col];
            const float dq = squared ? 2.0f * diff : (diff + 1e-5f) * inv_n;
            d_z[r * D + col] = g_zq[r * D + col] - gl * beta * dq;
        }
    }
}

// update, one workgroup per codebook:  N_k <- g N_k + h n_k ;  m_k <- g m_k + h s_k ;  T = sum_k N_k ;
// Nt_k = (N_k + eps) / (T + K eps) * T ;  e_k <- m_k / Nt_k.  Every product, sum and quotient is rounded separately
// (-ffp-contract=off, IEEE division).  T is a pairwise tree over the K values padded with zeros to P = 2^ceil(log2 K):
// level by level a[i] += a[i + half]; the order is a function of K alone, whatever the launch geometry.
__global__ __launch_bounds__(kVqThreads) void vq_ema_update_kernel(const float* __restrict__ stats, float* __restrict__ N,
                                                                   float* __restrict__ m, float* __restrict__ cb, int K,
                                                                   int dsub, int P, float g, float h, float eps) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* tree = lds;            // [P]
    float* nt = lds + P;          // [K]
    const int c = blockIdx.x;
    const int W = dsub + 1;
    const float* st = stats + (int64_t)c * K * W;
    float* Nc = N + (int64_t)c * K;
    for (int k = threadIdx.x; k < P; k += kVqThreads) {
        float v = 0.0f;
        if (k < K) {
            v = g * Nc[k] + h * st[(int64_t)k * W];
            Nc[k] = v;
            nt[k] = v;
        }
        tree[k] = v;
    }
    __syncthreads();
    for (int half = P >> 1; half >= 1; half >>= 1) {
        for (int i = threadIdx.x; i < half; i += kVqThreads) tree[i] += tree[i + half];
        __syncthreads();
    }
    const float T = tree[0];
    const float denom = T + (float)K * eps;
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += kVqThreads) nt[k] = (nt[k] + eps) / denom * T;
    __syncthreads();
    float* mc = m + (int64_t)c * K * dsub;
    float* ec = cb + (int64_t)c * K * dsub;
    for (int i = threadIdx.x; i < K * dsub; i += kVqThreads) {
        const int k = i / dsub, t = i - k * dsub;
        const float v = g * mc[i] + h * st[(int64_t)k * W + 1 + t];
        mc[i] = v;
        ec[i] = v / nt[k];
    }
}

// ---- dead-code restarts (opt-in companion of the EMA update) ---------------------------------------------------------------
// mix of include/vqcpc.h (the splitmix64 finaliser csrc/clusters.hip uses), all arithmetic mod 2^64
__device__ __forceinline__ uint64_t restart_mix(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// candidates, one lane per element of cand [ncb][K][dsub]: the row r mod (R world) of the ranks' concatenated z, this rank's
// value when it owns the row and +0.0f otherwise.  The lanes of one code recompute the same hash: ncb K dsub elements in all.
__global__ __launch_bounds__(kVqThreads) void vq_restart_candidates_kernel(const float* __restrict__ z, int64_t R, int ncb, int K,
                                                                           int dsub, uint64_t seed, uint64_t step,
                                                                           const uint64_t* __restrict__ step_dev, int rank,
                                                                           int world, float* __restrict__ cand) {
    const int64_t i = (int64_t)blockIdx.x * kVqThreads + threadIdx.x;
    if (i >= (int64_t)ncb * K * dsub) return;
    const int64_t code = i / dsub;              // c * K + k
    const int t = (int)(i - code * dsub);
    const int c = (int)(code / K);
    const uint64_t count = step_dev ? step_dev[0] : step;
    const uint64_t key = restart_mix(seed + (count + 1) * 0x9E3779B97F4A7C15ull);
    const uint64_t r = restart_mix(key + ((uint64_t)code + 1) * 0x9E3779B97F4A7C15ull);
    const uint64_t r_glob = r % ((uint64_t)R * (uint64_t)world);
    const int64_t owner = (int64_t)(r_glob / (uint64_t)R), row = (int64_t)(r_glob % (uint64_t)R);
    cand[i] = owner == rank ? z[row * ((int64_t)ncb * dsub) + (int64_t)c * dsub + t] : 0.0f;
}

// restart, one lane per code: N < thr (strict) -> e = m = cand, N = 1; every other cell keeps its bits.  The codes restarted by a
// workgroup are counted by wave ballot + popcount, summed over its waves in LDS and added to restarts[c] by ONE integer atomic.
__global__ __launch_bounds__(kVqThreads) void vq_ema_restart_kernel(const float* __restrict__ cand, float* __restrict__ N,
                                                                    float* __restrict__ m, float* __restrict__ cb, int K, int dsub,
                                                                    float thr, int* __restrict__ restarts) {
    __shared__ int wave_count[kVqThreads / kWave];
    const int c = blockIdx.y;
    const int k = blockIdx.x * kVqThreads + threadIdx.x;
    const int64_t code = (int64_t)c * K + k;
    const bool dead = k < K && N[code] < thr;
    if (dead) {
        const float* src = cand + code * dsub;
        float* mk = m + code * dsub;
        float* ek = cb + code * dsub;
        for (int t = 0; t < dsub; ++t) {
            const float v = src[t];
            ek[t] = v;
            mk[t] = v;
        }
        N[code] = 1.0f;
    }
    const uint64_t bal = __ballot(dead);         // every lane of the wave arrives here
    if ((threadIdx.x & (kWave - 1)) == 0) wave_count[threadIdx.x / kWave] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kVqThreads / kWave; ++w) total += wave_count[w];
        if (total > 0) atomicAdd(restarts + c, total);
    }
}

}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_vq_fwd(const float* z, const float* codebooks, int64_t R, int ncb, int K, int dsub, float beta, int squared,
                 int assign, int64_t* idx, float* zq_sg, float* loss, void* stream) {
    if (R == 0) return VQCPC_OK;
    VQ_REQUIRE(z && codebooks && idx && ((zq_sg != nullptr) == (loss != nullptr)), "vq_fwd: null pointer");
    VQ_REQUIRE(zq_sg || assign, "vq_fwd: index-only mode (zq_sg == loss == NULL) needs assign = 1");
    VQ_REQUIRE(R >= 0 && ncb >= 1 && K >= 1 && dsub >= 1, "vq_fwd: bad shape R=%lld ncb=%d K=%d dsub=%d", (long long)R, ncb,
               K, dsub);
    VQ_REQUIRE((int64_t)K * dsub <= kVqLdsFloats, "vq_fwd: codebook of %d x %d floats does not fit the LDS", K, dsub);
    VQ_REQUIRE(aligned16(z) && aligned16(codebooks), "vq_fwd: z and codebooks must be 16-byte aligned");
    const dim3 grid((unsigned)ceil_div(R, kVqRows)), block(kVqThreads);
    const size_t lds = (size_t)K * dsub * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
#define VQ_LAUNCH(DS)                                                                                                  \
    if (lds > 64 * 1024)                                                                                               \
        (void)hipFuncSetAttribute((const void*)vq_fwd_kernel<DS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    hipLaunchKernelGGL(vq_fwd_kernel<DS>, grid, block, lds, s, z, codebooks, R, ncb, K, dsub, beta, squared, assign, idx, \
                       zq_sg, loss)
    switch (dsub) {
        case 3: VQ_LAUNCH(3); break;
        case 4: VQ_LAUNCH(4); break;
        case 8: VQ_LAUNCH(8); break;
        case 16: VQ_LAUNCH(16); break;
        case 32: VQ_LAUNCH(32); break;
        case 64: VQ_LAUNCH(64); break;
        default: VQ_LAUNCH(0); break;
    }
#undef VQ_LAUNCH
    VQ_CHECK_LAUNCH("vq_fwd");
    return VQCPC_OK;
}

int64_t vqcpc_vq_bwd_workspace(int64_t R, int ncb, int K, int dsub) {
    return ceil_div(std::max<int64_t>(R, 1), kVqThreads) * ncb * K * dsub * (int64_t)sizeof(float);
}

int vqcpc_vq_bwd(const float* z, const float* codebooks, const int64_t* idx, const float* g_zq, const float* g_loss,
                 int64_t R, int ncb, int K, int dsub, float beta, int squared, float* d_z, float* d_codebooks,
                 void* workspace, int64_t workspace_bytes, void* stream) {
    VQ_REQUIRE(z && codebooks && idx && g_zq && g_loss && d_z && d_codebooks && workspace, "vq_bwd: null pointer");
    VQ_REQUIRE(R >= 1 && ncb >= 1 && K >= 1 && dsub >= 1, "vq_bwd: bad shape");
    // accumulator [K][dsub] + staged rows [256][dsub] + their codes: dsub <= 158 at K = 1, so a lane group (kgroups = 256 / dsub
    // >= 1) always exists; larger dsub is refused here with the numbers that do not fit
    const size_t lds = ((size_t)K * dsub + (size_t)kVqThreads * dsub + kVqThreads) * sizeof(float);
    VQ_REQUIRE(lds <= 160 * 1024, "vq_bwd: %d codes + %d staged rows of %d floats do not fit the LDS", K, kVqThreads, dsub);
    if (workspace_bytes < vqcpc_vq_bwd_workspace(R, ncb, K, dsub)) {
        set_error("vq_bwd: workspace too small");
        return VQCPC_EWORKSPACE;
    }
    const int nchunks = (int)ceil_div(R, kVqThreads);
    hipStream_t s = (hipStream_t)stream;
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)vq_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(vq_bwd_kernel, dim3(nchunks), dim3(kVqThreads), lds, s, z, codebooks, idx, g_zq, g_loss, R, ncb, K,
                       dsub, beta, squared, d_z, (float*)workspace);
    VQ_CHECK_LAUNCH("vq_bwd");
    const int64_t count = (int64_t)ncb * K * dsub;
    return launch_reduce_splits((const float*)workspace, count, nchunks, d_codebooks, count, 0, s);
}

int64_t vqcpc_vq_ema_stats_workspace(int64_t R, int ncb, int K, int dsub) {
    return ceil_div(std::max<int64_t>(R, 1), kVqThreads) * ncb * K * (dsub + 1) * (int64_t)sizeof(float);
}

int vqcpc_vq_ema_stats(const float* z, const int64_t* idx, int64_t R, int ncb, int K, int dsub, float* stats, void* workspace,
                       int64_t workspace_bytes, void* stream) {
    VQ_REQUIRE(z && idx && stats && workspace, "vq_ema_stats: null pointer");
    VQ_REQUIRE(R >= 1 && ncb >= 1 && K >= 1 && dsub >= 1, "vq_ema_stats: bad shape R=%lld ncb=%d K=%d dsub=%d", (long long)R, ncb,
               K, dsub);
    VQ_REQUIRE(R < ((int64_t)1 << 24), "vq_ema_stats: %lld rows: the counts of 2^24 rows and more are not exact in fp32",
               (long long)R);
    VQ_REQUIRE(dsub + 1 <= kVqThreads, "vq_ema_stats: dsub + 1 = %d columns exceed the %d lanes of a workgroup", dsub + 1,
               kVqThreads);
    const int W = dsub + 1;
    const size_t lds = ((size_t)K * W + (size_t)kVqThreads * W + 2 * kVqThreads) * sizeof(float);
    VQ_REQUIRE(lds <= 160 * 1024, "vq_ema_stats: accumulator of %d x %d floats does not fit the LDS", K, W);
    if (workspace_bytes < vqcpc_vq_ema_stats_workspace(R, ncb, K, dsub)) {
        set_error("vq_ema_stats: workspace too small");
        return VQCPC_EWORKSPACE;
    }
    const int nchunks = (int)ceil_div(R, kVqThreads);
    hipStream_t s = (hipStream_t)stream;
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)vq_ema_stats_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(vq_ema_stats_kernel, dim3(nchunks), dim3(kVqThreads), lds, s, z, idx, R, ncb, K, dsub, (float*)workspace);
    VQ_CHECK_LAUNCH("vq_ema_stats");
    const int64_t count = (int64_t)ncb * K * W;
    return launch_reduce_splits((const float*)workspace, count, nchunks, stats, count, 0, s);
}

int vqcpc_vq_commit_bwd(const float* z, const float* codebooks, const int64_t* idx, const float* g_zq, const float* g_loss,
                        int64_t R, int ncb, int K, int dsub, float beta, int squared, float* d_z, void* stream) {
    VQ_REQUIRE(z && codebooks && idx && g_zq && g_loss && d_z, "vq_commit_bwd: null pointer");
    VQ_REQUIRE(R >= 1 && ncb >= 1 && K >= 1 && dsub >= 1, "vq_commit_bwd: bad shape R=%lld ncb=%d K=%d dsub=%d", (long long)R, ncb,
               K, dsub);
    hipLaunchKernelGGL(vq_commit_bwd_kernel, dim3((unsigned)ceil_div(R, kVqThreads)), dim3(kVqThreads), 0, (hipStream_t)stream, z,
                       codebooks, idx, g_zq, g_loss, R, ncb, K, dsub, beta, squared, d_z);
    VQ_CHECK_LAUNCH("vq_commit_bwd");
    return VQCPC_OK;
}

int vqcpc_vq_ema_update(const float* stats, float* cluster_size, float* ema_sum, float* codebooks, int ncb, int K, int dsub,
                        float g, float h, float eps, void* stream) {
    VQ_REQUIRE(stats && cluster_size && ema_sum && codebooks, "vq_ema_update: null pointer");
    VQ_REQUIRE(ncb >= 1 && K >= 1 && dsub >= 1, "vq_ema_update: bad shape ncb=%d K=%d dsub=%d", ncb, K, dsub);
    VQ_REQUIRE(K <= 16 * 1024, "vq_ema_update: %d codes do not fit the LDS", K);
    int P = 1;
    while (P < K) P <<= 1;
    const size_t lds = ((size_t)P + K) * sizeof(float);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)vq_ema_update_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(vq_ema_update_kernel, dim3(ncb), dim3(kVqThreads), lds, (hipStream_t)stream, stats, cluster_size, ema_sum,
                       codebooks, K, dsub, P, g, h, eps);
    VQ_CHECK_LAUNCH("vq_ema_update");
    return VQCPC_OK;
}

int vqcpc_vq_restart_candidates(const float* z, int64_t R, int ncb, int K, int dsub, uint64_t seed, uint64_t step,
                                const uint64_t* step_dev, int rank, int world, float* cand, void* stream) {
    VQ_REQUIRE(z && cand, "vq_restart_candidates: null pointer");
    VQ_REQUIRE(R >= 1 && ncb >= 1 && K >= 1 && dsub >= 1, "vq_restart_candidates: bad shape R=%lld ncb=%d K=%d dsub=%d",
               (long long)R, ncb, K, dsub);
    VQ_REQUIRE(world >= 1 && rank >= 0 && rank < world, "vq_restart_candidates: rank %d outside [0, world = %d)", rank, world);
    VQ_REQUIRE(R < ((int64_t)1 << 31) && R * world < ((int64_t)1 << 31),
               "vq_restart_candidates: %lld rows on %d ranks: 2^31 rows and more are refused", (long long)R, world);
    const int64_t n = (int64_t)ncb * K * dsub;
    VQ_REQUIRE(n < ((int64_t)1 << 31) * kVqThreads, "vq_restart_candidates: %lld elements exceed the grid", (long long)n);
    hipLaunchKernelGGL(vq_restart_candidates_kernel, dim3((unsigned)ceil_div(n, kVqThreads)), dim3(kVqThreads), 0,
                       (hipStream_t)stream, z, R, ncb, K, dsub, seed, step, step_dev, rank, world, cand);
    VQ_CHECK_LAUNCH("vq_restart_candidates");
    return VQCPC_OK;
}

int vqcpc_vq_ema_restart(const float* cand, float* cluster_size, float* ema_sum, float* codebooks, int ncb, int K, int dsub,
                         float thr, int32_t* restarts, void* stream) {
    VQ_REQUIRE(cand && cluster_size && ema_sum && codebooks && restarts, "vq_ema_restart: null pointer");
    VQ_REQUIRE(ncb >= 1 && ncb <= 65535 && K >= 1 && dsub >= 1, "vq_ema_restart: bad shape ncb=%d K=%d dsub=%d", ncb, K, dsub);
    VQ_REQUIRE(thr >= 0.0f, "vq_ema_restart: threshold %g is negative (or NaN)", (double)thr);
    hipLaunchKernelGGL(vq_ema_restart_kernel, dim3((unsigned)ceil_div(K, kVqThreads), (unsigned)ncb), dim3(kVqThreads), 0,
                       (hipStream_t)stream, cand, cluster_size, ema_sum, codebooks, K, dsub, thr, restarts);
    VQ_CHECK_LAUNCH("vq_ema_restart");
    return VQCPC_OK;
}

}  // extern "C"
