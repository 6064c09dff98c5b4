// Duplicate check: the longest common run of a query (a generation) against the device-resident corpus (include/vqcpc.h, the
// "Duplicate check" section, states the definition; DeviceCorpus.longest_common_run in dataloaders/corpus.py is the caller).
// The longest common contiguous run between a query of n ticks and a framed corpus of N ticks lives on one of n + N - 1
// DIAGONALS (query tick t against framed tick t + delta), and a diagonal is one sequential scan.
//   * dup_frame: the corpus once, as one 64-bit word per tick (four 16-bit voices) with a sentinel tick (all ones) in front of every
//     piece and after the last.  Query tokens are < 0xFFFF, so a sentinel equals nothing: runs break at piece boundaries and at both
//     ends of the array without a branch in the scan.
//   * dup_pack: int64 (G, ticks, 4) query tokens -> the same word layout.
//   * dup_longest_run: grid (chunks of kDupThreads diagonals) x G.  A block stages, per pass of kDupTile query ticks, the query words
//     and the kDupThreads + tile - 1 framed words its diagonals touch in LDS (out of range reads as sentinel).  Lane l owns diagonal
//     k0 + l and reads s_c[l + t]: consecutive lanes read consecutive 8-byte words (ds_read_b64, the 32 lanes of a half cover the
//     64 banks once: conflict-free); the query word is one address for the whole wave (broadcast).  Per tick: one 64-bit XOR; zero
//     adds 4 to the running length; otherwise the run is closed with the tick's leading equal voices, a run strictly inside the tick
//     (voices 1 / 2 / 1-2) is scored, and the run reopens with the trailing equal voices.  A lane meets its runs in ascending query
//     position, so "strictly longer" keeps the smallest i; across lanes the packed key length << 48 | (0xFFFF - i) << 32 |
//     (0xFFFFFFFF - j) carries the tie rule through a wave shuffle maximum, an LDS maximum over the waves and one 64-bit atomicMax
//     per block into out[g].  A maximum is order-independent: the result is deterministic.
// LDS: (kDupTile + kDupThreads + kDupTile) words = 6 KiB per block whatever the query length, so the CU's occupancy is set by
// registers alone.  Plain C++, vector memory operations and one device-scope atomic only.
#include <algorithm>

#include "common.h"

namespace vq {

constexpr int kDupThreads = 256;              // diagonals per block: one per lane, 4 waves
constexpr int kDupTile = 256;                 // query ticks staged per pass
constexpr int kDupMaxBlocks = 2048;           // frame / pack are memory-bound: cap the grid and stride the rest
constexpr uint64_t kDupSentinel = ~0ull;

__device__ __forceinline__ uint64_t dup_word(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
    return (uint64_t)((v0 & 0xFFFFu) | (v1 << 16)) | ((uint64_t)((v2 & 0xFFFFu) | (v3 << 16)) << 32);
}

__global__ __launch_bounds__(kDupThreads) void dup_frame_kernel(const int4* __restrict__ tokens,
                                                               const int64_t* __restrict__ piece_start, int P,
                                                               uint64_t* __restrict__ framed, int64_t n_framed) {
    const int64_t step = (int64_t)gridDim.x * kDupThreads;
    for (int64_t f = (int64_t)blockIdx.x * kDupThreads + threadIdx.x; f < n_framed; f += step) {
        int lo = 0, hi = P + 1;               // the sentinel in front of piece p (after the last: p = P) sits at piece_start[p] + p
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (piece_start[mid] + mid <= f) lo = mid;
            else hi = mid;
        }
        uint64_t w = kDupSentinel;
        if (f != piece_start[lo] + lo) {
            const int4 v = tokens[f - lo - 1];
            w = dup_word((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w);
        }
        framed[f] = w;
    }
}

__global__ __launch_bounds__(kDupThreads) void dup_pack_kernel(const int64_t* __restrict__ x, int64_t ld_row, int64_t ld_tick,
                                                              int n_ticks, int64_t total, uint64_t* __restrict__ query,
                                                              int64_t ld_query) {
    const int64_t step = (int64_t)gridDim.x * kDupThreads;
    for (int64_t e = (int64_t)blockIdx.x * kDupThreads + threadIdx.x; e < total; e += step) {
        const int64_t g = e / n_ticks;
        const int t = (int)(e - g * n_ticks);
        const int64_t* __restrict__ s = x + g * ld_row + (int64_t)t * ld_tick;
        query[g * ld_query + t] = dup_word((uint32_t)s[0], (uint32_t)s[1], (uint32_t)s[2], (uint32_t)s[3]);
    }
}

__global__ __launch_bounds__(kDupThreads) void dup_longest_run_kernel(const uint64_t* __restrict__ framed, int64_t n_framed,
                                                                     const uint64_t* __restrict__ query, int64_t ld_query,
                                                                     int n_ticks, unsigned long long* __restrict__ out) {
    __shared__ uint64_t s_q[kDupTile];
    __shared__ uint64_t s_c[kDupThreads + kDupTile];
    __shared__ unsigned long long s_best[kDupThreads / kWave];
    const int lane = threadIdx.x;
    const uint64_t* __restrict__ q = query + (int64_t)blockIdx.y * ld_query;
    // diagonal k = blockIdx.x * kDupThreads + lane matches query tick t with framed tick t + k - (n_ticks - 1)
    const int64_t base = (int64_t)blockIdx.x * kDupThreads - (n_ticks - 1);      // framed tick of (t = 0, lane 0)
    uint32_t run = 0, best = 0, best_i = 0;
    for (int t0 = 0; t0 < n_ticks; t0 += kDupTile) {
        const int nt = min(kDupTile, n_ticks - t0);
        if (t0) __syncthreads();              // the previous pass has been read
        for (int idx = lane; idx < nt; idx += kDupThreads) s_q[idx] = q[t0 + idx];
        for (int idx = lane; idx < kDupThreads + nt - 1; idx += kDupThreads) {
            const int64_t f = base + t0 + idx;
            s_c[idx] = (f >= 0 && f < n_framed) ? framed[f] : kDupSentinel;
        }
        __syncthreads();
#pragma unroll 4
        for (int tt = 0; tt < nt; ++tt) {
            const uint64_t d = s_q[tt] ^ s_c[lane + tt];
            if (d == 0) {
                run += 4;
            } else {
                const uint32_t i_tick = 4u * (uint32_t)(t0 + tt);
                const uint32_t lead = (uint32_t)__builtin_ctzll(d) >> 4;
                const uint32_t len = run + lead;
                if (len > best) best = len, best_i = i_tick + lead - len;
                if (best < 2) {               // a run strictly inside the tick has 1 or 2 tokens
                    const uint32_t lo = (uint32_t)d, hi = (uint32_t)(d >> 32);
                    const bool e0 = (lo & 0xFFFFu) == 0, e1 = (lo >> 16) == 0, e2 = (hi & 0xFFFFu) == 0, e3 = (hi >> 16) == 0;
                    const bool in1 = e1 && !e0 && !(e2 && e3), in2 = e2 && !e3 && !(e1 && e0);
                    const uint32_t inner = (uint32_t)in1 + (uint32_t)in2;
                    if (inner > best) best = inner, best_i = i_tick + (in1 ? 1u : 2u);
                }
                run = (uint32_t)__builtin_clzll(d) >> 4;
            }
        }
    }
    if (run > best) best = run, best_i = 4u * (uint32_t)n_ticks - run;
    unsigned long long key = 0;
    if (best) {
        const uint64_t j = (uint64_t)((int64_t)best_i + 4 * (base + lane));      // a real match lies inside the framed array
        key = ((unsigned long long)best << 48) | ((unsigned long long)(0xFFFFu - best_i) << 32) | (0xFFFFFFFFull - j);
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, kWave);
        key = other > key ? other : key;
    }
    if ((lane & (kWave - 1)) == 0) s_best[lane / kWave] = key;
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int w = 1; w < kDupThreads / kWave; ++w) key = s_best[w] > key ? s_best[w] : key;
        if (key) atomicMax(out + blockIdx.y, key);
    }
}

static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_dup_frame(const int32_t* tokens, const int64_t* piece_start, int P, int64_t total_ticks, uint64_t* framed, void* stream) {
    VQ_REQUIRE(P >= 1 && total_ticks >= P && total_ticks + P + 1 < ((int64_t)1 << 30),
               "dup_frame: need P >= 1, total_ticks >= P and total_ticks + P + 1 < 2^30 (P=%d total_ticks=%lld)", P,
               (long long)total_ticks);
    VQ_REQUIRE(tokens && piece_start && framed, "dup_frame: null pointer");
    VQ_REQUIRE(aligned16(tokens) && aligned8(framed), "dup_frame: tokens must be 16-byte and framed 8-byte aligned");
    const int64_t n_framed = total_ticks + P + 1;
    const int blocks = (int)std::min<int64_t>(ceil_div(n_framed, kDupThreads), kDupMaxBlocks);
    hipLaunchKernelGGL(dup_frame_kernel, dim3(blocks), dim3(kDupThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const int4*>(tokens), piece_start, P, framed, n_framed);
    VQ_CHECK_LAUNCH("dup_frame");
    return VQCPC_OK;
}

int vqcpc_dup_pack(const int64_t* x, int64_t ld_row, int64_t ld_tick, int n_ticks, int G, uint64_t* query, int64_t ld_query,
                   void* stream) {
    VQ_REQUIRE(n_ticks >= 1 && G >= 1 && ld_tick >= 4 && ld_row >= 0 && ld_query >= n_ticks,
               "dup_pack: need n_ticks >= 1, G >= 1, ld_tick >= 4, ld_row >= 0, ld_query >= n_ticks (n_ticks=%d G=%d ld_tick=%lld "
               "ld_row=%lld ld_query=%lld)", n_ticks, G, (long long)ld_tick, (long long)ld_row, (long long)ld_query);
    VQ_REQUIRE(x && query, "dup_pack: null pointer");
    VQ_REQUIRE(aligned8(x) && aligned8(query), "dup_pack: pointers must be 8-byte aligned");
    const int64_t total = (int64_t)G * n_ticks;
    const int blocks = (int)std::min<int64_t>(ceil_div(total, kDupThreads), kDupMaxBlocks);
    hipLaunchKernelGGL(dup_pack_kernel, dim3(blocks), dim3(kDupThreads), 0, (hipStream_t)stream, x, ld_row, ld_tick, n_ticks, total,
                       query, ld_query);
    VQ_CHECK_LAUNCH("dup_pack");
    return VQCPC_OK;
}

int vqcpc_dup_longest_run(const uint64_t* framed, int64_t n_framed, const uint64_t* query, int64_t ld_query, int n_ticks, int G,
                          uint64_t* out, void* stream) {
    VQ_REQUIRE(n_ticks >= 1 && 4 * (int64_t)n_ticks <= 65535 && G >= 1 && G <= 65535 && n_framed >= 1 &&
                   n_framed < ((int64_t)1 << 30) && ld_query >= n_ticks,
               "dup_longest_run: need 1 <= n_ticks, 4 n_ticks <= 65535, 1 <= G <= 65535, 1 <= n_framed < 2^30 (framed tokens < 2^32), "
               "ld_query >= n_ticks (n_ticks=%d G=%d n_framed=%lld ld_query=%lld)", n_ticks, G, (long long)n_framed,
               (long long)ld_query);
    VQ_REQUIRE(framed && query && out, "dup_longest_run: null pointer");
    VQ_REQUIRE(aligned8(framed) && aligned8(query) && aligned8(out), "dup_longest_run: pointers must be 8-byte aligned");
    const int64_t chunks = ceil_div(n_framed + n_ticks - 1, kDupThreads);         // < 2^22 + 64
    hipLaunchKernelGGL(dup_longest_run_kernel, dim3((unsigned)chunks, (unsigned)G), dim3(kDupThreads), 0, (hipStream_t)stream, framed,
                       n_framed, query, ld_query, n_ticks, reinterpret_cast<unsigned long long*>(out));
    VQ_CHECK_LAUNCH("dup_longest_run");
    return VQCPC_OK;
}

}  // extern "C"
