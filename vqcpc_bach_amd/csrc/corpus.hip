// Device-resident window sampler over a tokenised corpus (vqcpc_bach_amd/dataloaders/corpus.py; the window rule restates
// VQCPCB/datasets/chorale_dataset.py:124-129 and :418-470).  The corpus stays in device memory as (total_ticks, 4) int32 -- one
// tick of 4 voices is 16 contiguous bytes -- with the tick offsets of its pieces; a WINDOW SET of W beats enumerates, piece-major,
// the start beats o = -(W - 1) .. last[p] of every piece p, and win_cum (P + 1 int64, device) holds the cumulative window counts.
//   * corpus_permute: positions q0 .. q0 + count - 1 of an epoch order -> window ids lo + pi_key(q mod n).  pi is a balanced Feistel
//     network on 2 * hb bits, 2^(2 hb - 2) < n <= 2^(2 hb) (hb >= 1), cycle-walked into [0, n): a true bijection for every n >= 1,
//     fewer than 4 expected walks, no materialised permutation and no random numbers from anywhere.
//   * corpus_gather: one thread per (id, tick): binary search of the id's piece in win_cum (the threads of a window read the same
//     words), one 16-byte load of the tick (or the START / END / PAD row of `special`), the 4 voices widened to int64 and written as
//     two 16-byte stores where the strides allow.  Consecutive threads write consecutive ticks, so a wave's stores cover one
//     contiguous 2 KiB run for dense outputs.  Ticks below `split` go to out, the others to out2 (x_left / x_right in one launch).
//     An id outside [0, win_cum[P]) writes nothing and raises *flag.
// Plain vector loads and stores, no atomics, no allocation or synchronisation in the launch functions (graph-capture safe).
#include <algorithm>

#include "common.h"

namespace vq {

constexpr int kCorpusThreads = 256;
constexpr int kCorpusMaxBlocks = 2048;        // memory-bound: cap the grid and stride the rest
constexpr int kFeistelRounds = 6;

struct FeistelKeys {
    uint32_t k[kFeistelRounds];
};

__host__ __device__ __forceinline__ uint32_t corpus_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// one pass of the network over the 2 * hb-bit value x: (L, R) -> (R, L ^ F_r(R)), a bijection whatever F is
__device__ __forceinline__ uint64_t feistel(uint64_t x, int hb, uint32_t mask, const FeistelKeys& keys) {
    uint32_t L = (uint32_t)(x >> hb) & mask, R = (uint32_t)x & mask;
#pragma unroll
    for (int r = 0; r < kFeistelRounds; ++r) {
        const uint32_t t = L ^ (corpus_mix32(R ^ keys.k[r]) & mask);
        L = R;
        R = t;
    }
    return ((uint64_t)L << hb) | R;
}

__global__ __launch_bounds__(kCorpusThreads) void corpus_permute_kernel(int64_t* __restrict__ ids, int64_t lo, int64_t n,
                                                                        int64_t q0, int64_t count, int hb, uint32_t mask,
                                                                        FeistelKeys keys) {
    const int64_t step = (int64_t)gridDim.x * kCorpusThreads;
    for (int64_t i = (int64_t)blockIdx.x * kCorpusThreads + threadIdx.x; i < count; i += step) {
        uint64_t x = (uint64_t)((q0 + i) % n);
        do {                                   // cycle walking: x < n lies on the cycle, so the walk comes back below n
            x = feistel(x, hb, mask, keys);
        } while (x >= (uint64_t)n);
        ids[i] = lo + (int64_t)x;
    }
}

__global__ __launch_bounds__(kCorpusThreads) void corpus_gather_kernel(
    const int4* __restrict__ tokens, const int64_t* __restrict__ piece_start, const int64_t* __restrict__ win_cum,
    const int32_t* __restrict__ special, int P, int W, int sub, const int64_t* __restrict__ ids, int64_t count,
    int64_t* __restrict__ out, int64_t ld_row, int64_t ld_tick, int split, int64_t* __restrict__ out2, int64_t ld_row2,
    int64_t ld_tick2, int vec, int32_t* __restrict__ flag) {
    const int Tw = W * sub;
    const int64_t total = count * Tw, step = (int64_t)gridDim.x * kCorpusThreads, n_windows = win_cum[P];
    for (int64_t g = (int64_t)blockIdx.x * kCorpusThreads + threadIdx.x; g < total; g += step) {
        const int64_t row = g / Tw;
        const int t = (int)(g - row * Tw);
        const int64_t id = ids[row];
        if (id < 0 || id >= n_windows) {
            if (t == 0) *flag = 1;
            continue;
        }
        int lo = 0, hi = P;                    // win_cum[lo] <= id < win_cum[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (win_cum[mid] <= id) lo = mid;
            else hi = mid;
        }
        const int64_t ps = piece_start[lo], len = piece_start[lo + 1] - ps;
        const int64_t rel = (id - win_cum[lo] - (W - 1)) * sub + t;          // tick of the piece, < 0 / >= len: padding
        int4 v;
        if (rel >= 0 && rel < len) {
            v = tokens[ps + rel];
        } else {
            const int32_t* __restrict__ s = special + (rel == -1 ? 0 : rel == len ? 4 : 8);    // START | END | PAD
            v = make_int4(s[0], s[1], s[2], s[3]);
        }
        int64_t* __restrict__ o = t < split ? out + row * ld_row + (int64_t)t * ld_tick
                                            : out2 + row * ld_row2 + (int64_t)(t - split) * ld_tick2;
        if (vec) {
            reinterpret_cast<longlong2*>(o)[0] = make_longlong2(v.x, v.y);
            reinterpret_cast<longlong2*>(o)[1] = make_longlong2(v.z, v.w);
        } else {
            o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
        }
    }
}

static inline uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_corpus_permute(int64_t* ids, int64_t lo, int64_t n, uint64_t key, int64_t q0, int64_t count, void* stream) {
    const int64_t big = (int64_t)1 << 61;      // lo + n and q0 + count stay below 2^63
    VQ_REQUIRE(n >= 1 && n <= big && q0 >= 0 && q0 <= big && count >= 0 && count <= big && lo >= 0 && lo <= big,
               "corpus_permute: need 1 <= n <= 2^61 and q0, count, lo in [0, 2^61] (n=%lld q0=%lld count=%lld lo=%lld)", (long long)n,
               (long long)q0, (long long)count, (long long)lo);
    if (count == 0) return VQCPC_OK;
    VQ_REQUIRE(ids, "corpus_permute: null pointer");
    int hb = 1;
    while (hb < 31 && ((uint64_t)1 << (2 * hb)) < (uint64_t)n) ++hb;
    const uint32_t mask = (uint32_t)(((uint64_t)1 << hb) - 1);
    FeistelKeys keys;
    uint64_t s = key;
    for (int r = 0; r < kFeistelRounds; ++r) keys.k[r] = (uint32_t)(splitmix64(s) >> 32);
    const int blocks = (int)std::min<int64_t>(ceil_div(count, kCorpusThreads), kCorpusMaxBlocks);
    hipLaunchKernelGGL(corpus_permute_kernel, dim3(blocks), dim3(kCorpusThreads), 0, (hipStream_t)stream, ids, lo, n, q0, count, hb,
                       mask, keys);
    VQ_CHECK_LAUNCH("corpus_permute");
    return VQCPC_OK;
}

int vqcpc_corpus_gather(const int32_t* tokens, const int64_t* piece_start, const int64_t* win_cum, const int32_t* special, int P,
                        int W, int subdivision, const int64_t* ids, int64_t count, int64_t* out, int64_t ld_row, int64_t ld_tick,
                        int split, int64_t* out2, int64_t ld_row2, int64_t ld_tick2, int32_t* flag, void* stream) {
    VQ_REQUIRE(P >= 1 && W >= 1 && subdivision >= 1 && count >= 0 && (int64_t)W * subdivision <= (1 << 20),
               "corpus_gather: need P >= 1, W >= 1, subdivision >= 1, W * subdivision <= 2^20, count >= 0 (P=%d W=%d sub=%d count=%lld)",
               P, W, subdivision, (long long)count);
    const int Tw = W * subdivision;
    VQ_REQUIRE(split >= 0 && split <= Tw, "corpus_gather: need 0 <= split <= W * subdivision (split=%d)", split);
    VQ_REQUIRE((split == 0 || (ld_tick >= 4 && ld_row >= 0)) && (split == Tw || (ld_tick2 >= 4 && ld_row2 >= 0)),
               "corpus_gather: a tick is 4 int64 words: need ld_tick >= 4 and ld_row >= 0 for every output in use");
    if (count == 0) return VQCPC_OK;
    VQ_REQUIRE(tokens && piece_start && win_cum && special && ids && flag && (split == 0 || out) && (split == Tw || out2),
               "corpus_gather: null pointer");
    VQ_REQUIRE(aligned16(tokens), "corpus_gather: tokens must be 16-byte aligned (one tick = one 16-byte load)");
    const int vec = (split == 0 || (aligned16(out) && ld_row % 2 == 0 && ld_tick % 2 == 0)) &&
                    (split == Tw || (aligned16(out2) && ld_row2 % 2 == 0 && ld_tick2 % 2 == 0));
    const int blocks = (int)std::min<int64_t>(ceil_div(count * Tw, kCorpusThreads), kCorpusMaxBlocks);
    hipLaunchKernelGGL(corpus_gather_kernel, dim3(blocks), dim3(kCorpusThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const int4*>(tokens), piece_start, win_cum, special, P, W, subdivision, ids, count, out, ld_row,
                       ld_tick, split, out2, ld_row2, ld_tick2, vec, flag);
    VQ_CHECK_LAUNCH("corpus_gather");
    return VQCPC_OK;
}

}  // extern "C"
