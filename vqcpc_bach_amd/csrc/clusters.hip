// Cluster census: which rows a codeword collects, E deterministic examples per codeword, and every codeword's nearest neighbours
// (include/vqcpc.h, the "Cluster census" section, states the definitions; vqcpc_bach_amd/clusters.py is the caller; in place of the
// host loops of VQCPCB/encoder.py:112-185).
//   * cluster_count: one thread per (row, codebook).  SMALL tables (ncb * K <= kCountLdsWords) are counted per workgroup in LDS
//     (ds_add_u32; a block of 256 threads strides over its share of the rows) and flushed once, one global atomic per non-zero word;
//     LARGE tables (the merged code, K up to 2^24) go straight to global integer atomics, where rows spread over so many words that
//     a workgroup-private table would cost more to clear and flush than it saves.  Integer sums are order-independent.
//   * cluster_select: a CASCADING 64-bit atomicMin over the E slots of a code, see the argument at the kernel.
//   * codebook_knn: one lane per query codeword; candidate codewords are staged in LDS in tiles of at most kKnnTileFloats floats (a
//     codebook of K * d <= kKnnTileFloats is resident: one tile), every lane reads the SAME LDS word (broadcast, conflict-free),
//     kKnnGroup candidates share one pass over the query's d features, and a register-resident sorted list of k <= 16 (distance,
//     index) pairs takes each candidate by an unrolled insertion.  Distances are the canonical chain of vq.hip (this file is compiled
//     with -ffp-contract=off as well).
// Plain C++: vector loads and stores, LDS, global integer atomics.
#include <algorithm>

#include "common.h"

namespace vq {

constexpr int kClusterThreads = 256;
constexpr int kClusterMaxBlocks = 2048;       // cap the grid and stride the rest
constexpr int kCountLdsWords = 8192;          // 32 KiB of per-workgroup counts: up to 5 workgroups per CU
constexpr int kCountRowsPerBlock = 4096;      // LDS form: at least this many (row, codebook) pairs per clear + flush
constexpr int64_t kClusterMaxK = (int64_t)1 << 24;
constexpr int kClusterMaxBooks = 64;
constexpr int kSelectMaxE = 64;
constexpr uint64_t kSlotEmpty = ~0ull;
constexpr uint64_t kIdLimit = 0xFFFFFFFFull;  // ids are < 2^32 - 1, so that no packed key is the empty value

constexpr int kKnnThreads = 64;               // one wave of query codewords per block
constexpr int kKnnTileFloats = 8192;          // 32 KiB of candidate codewords per tile
constexpr int kKnnGroup = 8;                  // candidates per pass over the query's features
constexpr int kKnnMaxK = 16;
constexpr int kKnnMaxD = 1024;                // a tile holds at least kKnnGroup codewords

// h of include/vqcpc.h: the low 32 bits of the splitmix64 finaliser of key + id * 0x9E3779B97F4A7C15 (clusters.select_hash in Python)
__host__ __device__ __forceinline__ uint32_t cluster_hash(uint64_t key, uint64_t id) {
    uint64_t z = key + id * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)(z ^ (z >> 31));
}

// ---- counts -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kClusterThreads) void cluster_count_lds_kernel(const int64_t* __restrict__ codes, int64_t ld, int64_t n,
                                                                            int ncb, int K, int32_t* __restrict__ counts,
                                                                            int32_t* __restrict__ flag) {
    extern __shared__ int32_t s_counts[];      // ncb * K words
    const int words = ncb * K;
    for (int w = threadIdx.x; w < words; w += kClusterThreads) s_counts[w] = 0;
    __syncthreads();
    const int64_t total = n * ncb, step = (int64_t)gridDim.x * kClusterThreads;
    bool bad = false;
    for (int64_t g = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x; g < total; g += step) {
        const int64_t row = g / ncb;
        const int c = (int)(g - row * ncb);
        const int64_t k = codes[row * ld + c];
        if (k >= 0 && k < K) atomicAdd(&s_counts[c * K + (int)k], 1);
        else bad = true;
    }
    if (bad) *flag = 1;
    __syncthreads();
    for (int w = threadIdx.x; w < words; w += kClusterThreads) {
        const int32_t v = s_counts[w];
        if (v) atomicAdd(&counts[w], v);
    }
}

__global__ __launch_bounds__(kClusterThreads) void cluster_count_global_kernel(const int64_t* __restrict__ codes, int64_t ld, int64_t n,
                                                                               int ncb, int64_t K, int32_t* __restrict__ counts,
                                                                               int32_t* __restrict__ flag) {
    const int64_t total = n * ncb, step = (int64_t)gridDim.x * kClusterThreads;
    for (int64_t g = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x; g < total; g += step) {
        const int64_t row = g / ncb;
        const int c = (int)(g - row * ncb);
        const int64_t k = codes[row * ld + c];
        if (k >= 0 && k < K) atomicAdd(&counts[c * K + k], 1);
        else *flag = 1;
    }
}

// ---- examples ---------------------------------------------------------------------------------------------------------------------
// THE CASCADE.  The E slots of a code start empty (all ones) and a member's packed key v (unique: its id sits in the low bits)
// enters at slot 0:  old = atomicMin(&slot[e], v) leaves min(old, v) in the slot, and the thread carries max(old, v) on to slot
// e + 1; it stops when what it carries is the empty value or after slot E - 1.
//   (1) A value is, at any moment, in exactly one place -- one slot or one thread's hand -- and a slot's content only decreases.
//   (2) Every value that reaches slot e is carried on exactly once (by the thread that brought it, or by the thread whose smaller
//       value displaced it), except the slot's final minimum.  All members reach slot 0, so slot 0 ends as the smallest; the values
//       that reach slot e + 1 are those that reached slot e without its final minimum, so by induction slot e ends as the
//       (e + 1)-th smallest, whatever the interleaving.  With fewer than E members the tail stays empty.
//   (3) THE EARLY DROP.  When w leaves slot e - 1 it was the larger of the two values there, and each slot below holds, by (1),
//       something that was smaller than w when w passed it and has only decreased since: e distinct values below w.  So whatever
//       slot E - 1 holds at any time has E - 1 members below it, i.e. it is >= the E-th smallest, and a value -- fresh or carried --
//       that exceeds the current (or a stale, hence larger) content of slot E - 1 is not among the E smallest: it is dropped at once.
//       The E smallest are never dropped, and (2) goes through with "carried on or dropped".  Without the drop a code with n
//       members costs up to E atomics per member; with it, a member that loses against slot E - 1 costs one load.
// The result is a function of the SET of (code, id) pairs: row order, chunking and scheduling do not enter.
__global__ __launch_bounds__(kClusterThreads) void cluster_select_kernel(const int64_t* __restrict__ codes, int64_t ld, int64_t n, int ncb,
                                                                         int64_t K, const int64_t* __restrict__ ids, int64_t id0,
                                                                         uint64_t key, int E, unsigned long long* __restrict__ slots,
                                                                         int32_t* __restrict__ flag) {
    const int64_t total = n * ncb, step = (int64_t)gridDim.x * kClusterThreads;
    for (int64_t g = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x; g < total; g += step) {
        const int64_t row = g / ncb;
        const int c = (int)(g - row * ncb);
        const int64_t k = codes[row * ld + c];
        const uint64_t id = (uint64_t)(ids ? ids[row] : id0 + row);
        if (k < 0 || k >= K || id >= kIdLimit) {
            *flag = 1;
            continue;
        }
        unsigned long long* __restrict__ slot = slots + ((int64_t)c * K + k) * E;
        unsigned long long v = ((unsigned long long)cluster_hash(key, id) << 32) | id;
        for (int e = 0; e < E; ++e) {
            if (v > __hip_atomic_load(slot + E - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;      // (3)
            const unsigned long long old = atomicMin(slot + e, v);
            v = old > v ? old : v;
            if (v == kSlotEmpty) break;
        }
    }
}

// ---- nearest codewords ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kKnnThreads) void codebook_knn_kernel(const float* __restrict__ e, int K, int d, int k, int tile,
                                                                   int32_t* __restrict__ nn, float* __restrict__ dist2) {
    extern __shared__ float s_tile[];          // min(tile, K) codewords of d floats
    const int c = blockIdx.y;
    const int i = blockIdx.x * kKnnThreads + threadIdx.x;
    const bool live = i < K;
    const float* __restrict__ book = e + (int64_t)c * K * d;
    const float* __restrict__ q = book + (int64_t)(live ? i : 0) * d;
    float bd[kKnnMaxK];
    int bi[kKnnMaxK];
#pragma unroll
    for (int s = 0; s < kKnnMaxK; ++s) bd[s] = __builtin_inff(), bi[s] = -1;
    float worst = __builtin_inff();            // bd[k - 1]: what a candidate has to beat
    for (int j_base = 0; j_base < K; j_base += tile) {
        const int tj = min(tile, K - j_base);
        if (j_base) __syncthreads();           // the previous tile has been read
        const float* __restrict__ src = book + (int64_t)j_base * d;
        for (int w = threadIdx.x; w < tj * d; w += kKnnThreads) s_tile[w] = src[w];
        __syncthreads();
        if (!live) continue;
        for (int j0 = 0; j0 < tj; j0 += kKnnGroup) {
            float acc[kKnnGroup];
            int off[kKnnGroup];
#pragma unroll
            for (int u = 0; u < kKnnGroup; ++u) acc[u] = 0.0f, off[u] = min(j0 + u, tj - 1) * d;
            for (int t = 0; t < d; ++t) {      // t ascending, separately rounded sub / mul / add: the canonical chain
                const float x = q[t];
#pragma unroll
                for (int u = 0; u < kKnnGroup; ++u) {
                    const float df = __fsub_rn(x, s_tile[off[u] + t]);
                    acc[u] = __fadd_rn(acc[u], __fmul_rn(df, df));
                }
            }
#pragma unroll
            for (int u = 0; u < kKnnGroup; ++u) {
                const int j = j_base + j0 + u;
                const float dist = acc[u];
                // candidates arrive in ascending j, so strict '<' keeps the smaller index in front of an equal distance;
                // self is left out by INDEX (two coinciding codewords are each other's nearest, at distance 0)
                if (j0 + u >= tj || j == i || !(dist < worst)) continue;
#pragma unroll
                for (int s = kKnnMaxK - 1; s >= 0; --s) {      // top down: slot s - 1 is read before it changes
                    if (s < k && dist < bd[s]) {
                        const int below = s > 0 ? s - 1 : 0;
                        const bool shift = s > 0 && dist < bd[below];
                        bd[s] = shift ? bd[below] : dist;
                        bi[s] = shift ? bi[below] : j;
                    }
                    if (s == k - 1) worst = bd[s];
                }
            }
        }
    }
    if (!live) return;
    const int64_t o = ((int64_t)c * K + i) * k;
#pragma unroll
    for (int s = 0; s < kKnnMaxK; ++s) {
        if (s < k) nn[o + s] = bi[s], dist2[o + s] = bd[s];
    }
}

static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_cluster_count(const int64_t* codes, int64_t ld, int64_t n, int ncb, int64_t K, int32_t* counts, int32_t* flag, void* stream) {
    VQ_REQUIRE(ncb >= 1 && ncb <= kClusterMaxBooks && K >= 1 && K <= kClusterMaxK && ld >= ncb && n >= 0 && n < ((int64_t)1 << 31),
               "cluster_count: need 1 <= ncb <= 64, 1 <= K <= 2^24, ld >= ncb, 0 <= n < 2^31 (ncb=%d K=%lld ld=%lld n=%lld)", ncb,
               (long long)K, (long long)ld, (long long)n);
    if (n == 0) return VQCPC_OK;
    VQ_REQUIRE(codes && counts && flag, "cluster_count: null pointer");
    VQ_REQUIRE(aligned8(codes) && aligned4(counts) && aligned4(flag), "cluster_count: codes must be 8-byte, counts and flag 4-byte aligned");
    const int64_t total = n * ncb;
    if (K * ncb <= kCountLdsWords) {
        const int blocks = (int)std::min<int64_t>(ceil_div(total, kCountRowsPerBlock), kClusterMaxBlocks);
        hipLaunchKernelGGL(cluster_count_lds_kernel, dim3(blocks), dim3(kClusterThreads), (size_t)(K * ncb) * sizeof(int32_t),
                           (hipStream_t)stream, codes, ld, n, ncb, (int)K, counts, flag);
    } else {
        const int blocks = (int)std::min<int64_t>(ceil_div(total, kClusterThreads), kClusterMaxBlocks);
        hipLaunchKernelGGL(cluster_count_global_kernel, dim3(blocks), dim3(kClusterThreads), 0, (hipStream_t)stream, codes, ld, n, ncb, K,
                           counts, flag);
    }
    VQ_CHECK_LAUNCH("cluster_count");
    return VQCPC_OK;
}

int vqcpc_cluster_select(const int64_t* codes, int64_t ld, int64_t n, int ncb, int64_t K, const int64_t* ids, int64_t id0, uint64_t key,
                         int E, uint64_t* slots, int32_t* flag, void* stream) {
    VQ_REQUIRE(ncb >= 1 && ncb <= kClusterMaxBooks && K >= 1 && K <= kClusterMaxK && ld >= ncb && n >= 0 && n < ((int64_t)1 << 31) &&
                   E >= 1 && E <= kSelectMaxE,
               "cluster_select: need 1 <= ncb <= 64, 1 <= K <= 2^24, ld >= ncb, 0 <= n < 2^31, 1 <= E <= 64 (ncb=%d K=%lld ld=%lld "
               "n=%lld E=%d)", ncb, (long long)K, (long long)ld, (long long)n, E);
    VQ_REQUIRE(ids || (id0 >= 0 && id0 + n <= (int64_t)kIdLimit),
               "cluster_select: without an id array need id0 >= 0 and id0 + n <= 2^32 - 1 (id0=%lld n=%lld)", (long long)id0, (long long)n);
    if (n == 0) return VQCPC_OK;
    VQ_REQUIRE(codes && slots && flag, "cluster_select: null pointer");
    VQ_REQUIRE(aligned8(codes) && aligned8(ids) && aligned8(slots) && aligned4(flag),
               "cluster_select: codes, ids and slots must be 8-byte, flag 4-byte aligned");
    const int blocks = (int)std::min<int64_t>(ceil_div(n * ncb, kClusterThreads), kClusterMaxBlocks);
    hipLaunchKernelGGL(cluster_select_kernel, dim3(blocks), dim3(kClusterThreads), 0, (hipStream_t)stream, codes, ld, n, ncb, K, ids, id0,
                       key, E, reinterpret_cast<unsigned long long*>(slots), flag);
    VQ_CHECK_LAUNCH("cluster_select");
    return VQCPC_OK;
}

int vqcpc_codebook_knn(const float* e, int ncb, int K, int d, int k, int32_t* nn, float* dist2, void* stream) {
    VQ_REQUIRE(ncb >= 1 && ncb <= 65535 && K >= 2 && (int64_t)K <= kClusterMaxK && d >= 1 && d <= kKnnMaxD && k >= 1 && k <= kKnnMaxK &&
                   k < K,
               "codebook_knn: need 1 <= ncb <= 65535, 2 <= K <= 2^24, 1 <= d <= 1024, 1 <= k <= 16, k < K (ncb=%d K=%d d=%d k=%d)", ncb,
               K, d, k);
    VQ_REQUIRE(e && nn && dist2, "codebook_knn: null pointer");
    VQ_REQUIRE(aligned4(e) && aligned4(nn) && aligned4(dist2), "codebook_knn: pointers must be 4-byte aligned");
    const int tile = std::min(K, kKnnTileFloats / d);                           // >= kKnnGroup codewords, or the whole codebook
    hipLaunchKernelGGL(codebook_knn_kernel, dim3((unsigned)ceil_div(K, kKnnThreads), (unsigned)ncb), dim3(kKnnThreads),
                       (size_t)tile * d * sizeof(float), (hipStream_t)stream, e, K, d, k, tile, nn, dist2);
    VQ_CHECK_LAUNCH("codebook_knn");
    return VQCPC_OK;
}

}  // extern "C"
