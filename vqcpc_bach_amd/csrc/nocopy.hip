// Copy guard: generation that cannot recite the corpus (decoders/generation.py `no_copy=`; include/vqcpc.h, "Copy guard", states
// the definition; tests/nocopy_reference.py restates it in numpy without any hashing).  Exact integer logic, no floating point, no LDS
// but the beam's column move.
// The corpus is the duplicate check's framed array (csrc/duplicates.hip) read as 16-bit tokens: token position j = 4 framed tick +
// voice, a sentinel tick (0xFFFF in every voice) in front of every piece and after the last.  With max_copy = n, token k is BANNED at
// column c of a row when some corpus position j of voice c % 4 follows n tokens equal to the row's last n tokens and holds k.
//   * the index (DeviceCorpus.copy_index): one entry per corpus position whose n-token context holds no sentinel, key =
//     copy_hash(voice, context) << 8 | next token, sorted; `where` keeps j.  vqcpc_copy_index_keys writes the keys (a thread per
//     position, -1: no entry), vqcpc_copy_index_unique marks, after the sort, the entries whose predecessor has the same key AND the
//     same context: they are dropped, so a context keeps one entry per distinct continuation however often it occurs.
//   * the hash is a SUM over the context of a position-salted mix of each token, so lanes strided over the context add partial sums in
//     any order.  It is not part of the contract: every candidate of a key range is compared token by token.
//   * copy_ban, one wavefront per (row, column): lane l keeps history tokens col - 1 - l, col - 65 - l, ... (8 registers for n <= 512),
//     hashes them, one uniform binary search finds the range's first key, and every candidate is verified by the WHOLE WAVE, 64
//     tokens per pass with an early exit on a mismatching pass (after the duplicate removal a range holds a context's distinct continuations,
//     a handful: a lane per candidate would leave the wave idle and walk n tokens serially).  Verified continuations are OR-ed into a
//     256-bit set held as four wave-uniform 64-bit words.
//   * vqcpc_decode_nocopy: the step form, ONE launch, a wavefront per row (M <= 64), inside the captured step immediately before the
//     sampler or the beam select and after vqcpc_decode_rules; vqcpc_nocopy_audit: the same device function over a whole token tensor.
//   * vqcpc_nocopy_beam_column: after vqcpc_decode_beam_select, the live column of the report follows the ancestors (the select writes
//     its own records in slot order; this one it does not know).
#include "common.h"

namespace vq {

constexpr int kCopyMaxRows = 64;
constexpr int kCopyMaxN = 512;
constexpr int kCopyRegs = kCopyMaxN / 64;     // history tokens per lane
constexpr int kCopyVoices = 4;
constexpr int kCopyMaxVocab = 256;
constexpr uint32_t kCopySentinel = 0xFFFFu;
constexpr int kCopyRelaxed = 1 << 16, kCopyForced = 1 << 17;
constexpr int kCopyThreads = 256;
constexpr int kCopyMaxBlocks = 4096;
constexpr int kCopyAuditCols = 16;            // columns of a row per audit workgroup (one wavefront)

struct CopyVocab {
    int V[kCopyVoices];
};

struct CopyIndexView {
    const int64_t* keys;                      // sorted
    const int64_t* where;
    int64_t entries;
    const uint16_t* tok;                      // the framed corpus, 4 tokens per tick
    int64_t ntok;
    int n;
};

// a row's history: column c lives in hi[c - base] (the live window's tokens) for c >= base, else in lo[c] (the chorale)
struct CopyHistory {
    const int64_t* lo;
    int64_t ldlo;
    const int64_t* hi;
    int64_t base;
};

__device__ __forceinline__ uint32_t copy_token(const CopyHistory& h, int64_t c) {
    int64_t t = -1;
    if (c >= h.base) t = h.hi[c - h.base];
    else if (c < h.ldlo) t = h.lo[c];
    return (t >= 0 && t < (int64_t)kCopySentinel) ? (uint32_t)t : kCopySentinel;      // what is no token equals nothing
}

// the contribution of context token `tok`, m tokens before the position (m = 1 .. n)
__device__ __forceinline__ uint64_t copy_mix(uint32_t m, uint32_t tok) {
    uint64_t z = (uint64_t)m * 0x9E3779B97F4A7C15ull + (uint64_t)(tok + 1u) * 0xBF58476D1CE4E5B9ull;
    z ^= z >> 29;
    z *= 0x94D049BB133111EBull;
    return z ^ (z >> 32);
}

// the first key of (voice, context): 55 hash bits above the 8 bits of the next token, non-negative as int64
__device__ __forceinline__ int64_t copy_key0(uint64_t sum, int voice) {
    uint64_t z = sum + (uint64_t)(voice + 1) * 0xD6E8FEB86659FD93ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (int64_t)((z >> 9) << 8);
}

__device__ __forceinline__ int64_t copy_lower_bound(const int64_t* __restrict__ keys, int64_t entries, int64_t key) {
    int64_t lo = 0, hi = entries;             // the first index whose key is >= key
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The tokens banned at column col (>= n) of the history h, as four wave-uniform words.  One wavefront, every lane calls it.
__device__ __forceinline__ void copy_ban(const CopyIndexView& ix, const CopyHistory& h, int64_t col, int lane,
                                         unsigned long long ban[4]) {
    ban[0] = ban[1] = ban[2] = ban[3] = 0ull;
    const int n = ix.n, v = (int)(col & 3);
    uint32_t hist[kCopyRegs];
    uint64_t sum = 0;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < kCopyRegs; ++i) {
        const int m = 64 * i + lane + 1;
        hist[i] = kCopySentinel;
        if (m <= n) {
            hist[i] = copy_token(h, col - m);
            bad = bad || hist[i] == kCopySentinel;
            sum += copy_mix((uint32_t)m, hist[i]);
        }
    }
    if (__ballot(bad) != 0ull) return;        // uniform: a column without a token matches nothing
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor((unsigned long long)sum, o, 64);
    const int64_t k0 = copy_key0(sum, v);
    const int64_t last = k0 | 255;            // the range's last key; k0 + 256 would overflow when every hash bit is set
    for (int64_t idx = copy_lower_bound(ix.keys, ix.entries, k0); idx < ix.entries && ix.keys[idx] <= last; ++idx) {    // uniform
        const int64_t w = ix.where[idx];
        if (w < n || w >= ix.ntok || (int)(w & 3) != v) continue;
        bool same = true;
#pragma unroll
        for (int i = 0; i < kCopyRegs; ++i) {
            if (same && 64 * i < n) {         // uniform
                const int m = 64 * i + lane + 1;
                const bool differs = m <= n && (uint32_t)ix.tok[w - m] != hist[i];
                same = __ballot(differs) == 0ull;
            }
        }
        if (!same) continue;
        const uint32_t k = ix.tok[w];
        if (k >= (uint32_t)kCopyMaxVocab) continue;
        const unsigned long long bit = 1ull << (k & 63u);
        const uint32_t q = k >> 6;
        ban[0] |= q == 0u ? bit : 0ull;
        ban[1] |= q == 1u ? bit : 0ull;
        ban[2] |= q == 2u ? bit : 0ull;
        ban[3] |= q == 3u ? bit : 0ull;
    }
}

__device__ __forceinline__ unsigned long long copy_vocab_word(int V, int j) {
    return V >= 64 * (j + 1) ? ~0ull : V > 64 * j ? (1ull << (V - 64 * j)) - 1ull : 0ull;
}

__global__ __launch_bounds__(64) void decode_nocopy_kernel(
    const int64_t* __restrict__ tokens, int64_t ldtok, int T, const int64_t* __restrict__ chorale, int64_t ldch,
    const int64_t* __restrict__ constraint, int64_t ldcons, CopyIndexView ix, CopyVocab vv, const uint32_t* __restrict__ exclude,
    const uint32_t* stat, int64_t ldstat, uint32_t* sets, int64_t ldsets, int32_t* __restrict__ report, int64_t ldrep,
    const int32_t* __restrict__ posp, const int32_t* __restrict__ win, int U) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int pos = *posp;
    if (pos < 0 || pos >= T) return;                          // uniform
    const int w0 = win ? win[1] : 0;
    if (w0 < 0) return;                                       // no live window
    const int64_t base = (int64_t)w0 * U, col = base + pos;
    const int v = (int)(col & 3), V = vv.V[v];
    CopyHistory h;
    h.lo = chorale ? chorale + (int64_t)b * ldch : nullptr;
    h.ldlo = chorale ? ldch : 0;
    h.hi = tokens + (int64_t)b * ldtok;
    h.base = base;
    unsigned long long ban[4] = {0ull, 0ull, 0ull, 0ull};
    if (col >= ix.n) copy_ban(ix, h, col, lane, ban);
    // the set that comes in (stat may be `sets` itself: the rule kernel wrote it this step), all of it read before the store
    const uint32_t* in = stat && col < ldstat ? stat + ((int64_t)b * ldstat + col) * 8 : nullptr;
    unsigned long long s[4], vm[4], ex[4];
    bool none = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        vm[j] = copy_vocab_word(V, j);
        s[j] = in ? (unsigned long long)in[2 * j] | ((unsigned long long)in[2 * j + 1] << 32) : vm[j];
        ex[j] = exclude ? (unsigned long long)exclude[v * 8 + 2 * j] | ((unsigned long long)exclude[v * 8 + 2 * j + 1] << 32) : 0ull;
        none = none && (s[j] & vm[j]) == 0ull;
    }
    if (none) {                                               // the samplers read such a set as the whole vocabulary: say so
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = vm[j];
    }
    int64_t forced = -1;
    if (constraint && col < ldcons) forced = constraint[(int64_t)b * ldcons + col];
    int rep = 0;
    unsigned long long out[4] = {s[0], s[1], s[2], s[3]};
    if (forced >= 0) {
        if (forced < kCopyMaxVocab && ((ban[forced >> 6] >> (forced & 63)) & 1ull)) rep = kCopyForced;
    } else {
        int removed = 0;
        bool left = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            removed += __popcll(s[j] & ban[j]);
            left = left || (s[j] & ~ban[j] & vm[j] & ~ex[j]) != 0ull;
        }
        if (removed != 0 && !left) rep = kCopyRelaxed;        // copying is the only way on: the sampler never meets an empty set
        else {
            rep = removed;
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = s[j] & ~ban[j];
        }
    }
    if (col < ldsets && lane < 8) {
        const int j = lane >> 1;
        const unsigned long long w = j == 0 ? out[0] : j == 1 ? out[1] : j == 2 ? out[2] : out[3];
        sets[((int64_t)b * ldsets + col) * 8 + lane] = (uint32_t)(w >> (32 * (lane & 1)));
    }
    if (report && col < ldrep && lane == 0) report[(int64_t)b * ldrep + col] = rep;
}

__global__ __launch_bounds__(64) void nocopy_audit_kernel(const int64_t* __restrict__ x, int64_t ld, int64_t width, CopyIndexView ix,
                                                          int32_t* __restrict__ report, int64_t ldrep) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.y, c0 = (int64_t)blockIdx.x * kCopyAuditCols;
    CopyHistory h;
    h.lo = x + b * ld;
    h.ldlo = width;
    h.hi = nullptr;
    h.base = INT64_MAX;                                       // every column comes from x
    for (int64_t col = c0; col < min(c0 + kCopyAuditCols, width); ++col) {
        const int64_t t = h.lo[col];
        int rep = 0;
        if (col >= ix.n && t >= 0 && t < kCopyMaxVocab) {     // uniform
            unsigned long long ban[4];
            copy_ban(ix, h, col, lane, ban);
            if ((ban[t >> 6] >> (t & 63)) & 1ull) rep = kCopyForced;
        }
        if (lane == 0) report[b * ldrep + col] = rep;
    }
}

__global__ __launch_bounds__(kCopyThreads) void copy_index_keys_kernel(const uint16_t* __restrict__ tok, int64_t ntok, int n,
                                                                      int64_t* __restrict__ keys) {
    const int64_t step = (int64_t)gridDim.x * kCopyThreads;
    for (int64_t j = (int64_t)blockIdx.x * kCopyThreads + threadIdx.x; j < ntok; j += step) {
        int64_t key = -1;
        const uint32_t k = tok[j];
        if (j >= n && k < (uint32_t)kCopyMaxVocab) {
            uint64_t sum = 0;
            bool ok = true;
            for (int m = 1; m <= n; ++m) {
                const uint32_t t = tok[j - m];
                if (t == kCopySentinel) {
                    ok = false;
                    break;
                }
                sum += copy_mix((uint32_t)m, t);
            }
            if (ok) key = copy_key0(sum, (int)(j & 3)) | (int64_t)k;
        }
        keys[j] = key;
    }
}

__global__ __launch_bounds__(kCopyThreads) void copy_index_unique_kernel(const uint16_t* __restrict__ tok, int64_t ntok, int n,
                                                                        const int64_t* __restrict__ keys,
                                                                        const int64_t* __restrict__ where, int64_t entries,
                                                                        uint8_t* __restrict__ keep) {
    const int64_t step = (int64_t)gridDim.x * kCopyThreads;
    for (int64_t i = (int64_t)blockIdx.x * kCopyThreads + threadIdx.x; i < entries; i += step) {
        bool same = i > 0 && keys[i] == keys[i - 1];
        if (same) {
            const int64_t a = where[i], p = where[i - 1];
            same = a >= n && a < ntok && p >= n && p < ntok && ((a ^ p) & 3) == 0;
            for (int m = 1; same && m <= n; ++m) same = tok[a - m] == tok[p - m];
        }
        keep[i] = same ? 0 : 1;
    }
}

__global__ __launch_bounds__(64) void nocopy_beam_column_kernel(int32_t* __restrict__ report, int64_t ld, const int32_t* __restrict__ anc,
                                                                const int32_t* __restrict__ flag,
                                                                const int32_t* __restrict__ bound, int M, int W) {
    if (*flag == 0) return;                                   // no row moved
    const int64_t col = bound[1];
    if (col < 0 || col >= ld) return;
    const int r = threadIdx.x;
    int32_t val = 0;
    bool move = false;
    if (r < M) {
        const int a = anc[r];
        move = a >= 0 && a < M && a / W == r / W;             // an ancestor outside the row's group leaves the row alone
        if (move) val = report[(int64_t)a * ld + col];
    }
    __syncthreads();                                          // every load before the first store
    if (move) report[(int64_t)r * ld + col] = val;
}

static bool copy_index_ok(const int64_t* keys, const int64_t* where, int64_t entries, const uint64_t* framed, int64_t n_framed,
                          int max_copy) {
    return framed && entries >= 0 && (entries == 0 || (keys && where)) && n_framed >= 1 && n_framed < ((int64_t)1 << 30) &&
           max_copy >= 1 && max_copy <= kCopyMaxN;
}

static CopyIndexView copy_view(const int64_t* keys, const int64_t* where, int64_t entries, const uint64_t* framed, int64_t n_framed,
                               int max_copy) {
    CopyIndexView ix;
    ix.keys = keys;
    ix.where = where;
    ix.entries = entries;
    ix.tok = reinterpret_cast<const uint16_t*>(framed);
    ix.ntok = 4 * n_framed;
    ix.n = max_copy;
    return ix;
}

}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_copy_index_keys(const uint64_t* framed, int64_t n_framed, int max_copy, int64_t* keys, void* stream) {
    VQ_REQUIRE(framed && keys, "copy_index_keys: null pointer");
    VQ_REQUIRE(n_framed >= 1 && n_framed < ((int64_t)1 << 30) && max_copy >= 1 && max_copy <= kCopyMaxN,
               "copy_index_keys: need 1 <= n_framed < 2^30 and 1 <= max_copy <= 512 (n_framed=%lld max_copy=%d)", (long long)n_framed,
               max_copy);
    const int64_t ntok = 4 * n_framed;
    const int blocks = (int)(ceil_div(ntok, kCopyThreads) < kCopyMaxBlocks ? ceil_div(ntok, kCopyThreads) : kCopyMaxBlocks);
    hipLaunchKernelGGL(copy_index_keys_kernel, dim3(blocks), dim3(kCopyThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint16_t*>(framed), ntok, max_copy, keys);
    VQ_CHECK_LAUNCH("copy_index_keys");
    return VQCPC_OK;
}

int vqcpc_copy_index_unique(const uint64_t* framed, int64_t n_framed, int max_copy, const int64_t* keys, const int64_t* where,
                            int64_t entries, uint8_t* keep, void* stream) {
    VQ_REQUIRE(keys && where && keep && entries >= 1, "copy_index_unique: keys, where, keep and at least one entry are needed");
    VQ_REQUIRE(copy_index_ok(keys, where, entries, framed, n_framed, max_copy),
               "copy_index_unique: need framed, 1 <= n_framed < 2^30 and 1 <= max_copy <= 512");
    const int blocks = (int)(ceil_div(entries, kCopyThreads) < kCopyMaxBlocks ? ceil_div(entries, kCopyThreads) : kCopyMaxBlocks);
    hipLaunchKernelGGL(copy_index_unique_kernel, dim3(blocks), dim3(kCopyThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint16_t*>(framed), 4 * n_framed, max_copy, keys, where, entries, keep);
    VQ_CHECK_LAUNCH("copy_index_unique");
    return VQCPC_OK;
}

int vqcpc_decode_nocopy(const int64_t* tokens, int64_t ldtok, int T, const int64_t* chorale, int64_t ldch, const int64_t* constraint,
                        int64_t ldcons, const int64_t* keys, const int64_t* where, int64_t entries, const uint64_t* framed,
                        int64_t n_framed, int max_copy, const int32_t* voice_offsets, int nc, const uint32_t* exclude,
                        const uint32_t* copy_static, int64_t ldstatic, uint32_t* sets, int64_t ldsets, int32_t* copy_report,
                        int64_t ldreport, const int32_t* pos, const int32_t* win, int U, int64_t M, void* stream) {
    VQ_REQUIRE(tokens && voice_offsets && sets && pos, "decode_nocopy: tokens, voice_offsets, sets and pos are needed");
    VQ_REQUIRE(copy_index_ok(keys, where, entries, framed, n_framed, max_copy),
               "decode_nocopy: an index (keys, where, framed; 1 <= n_framed < 2^30, 1 <= max_copy <= 512) is needed");
    VQ_REQUIRE(M >= 1 && M <= kCopyMaxRows && T >= 1 && U >= 1, "decode_nocopy: bad arguments (1 <= M <= 64, T >= 1, U >= 1)");
    VQ_REQUIRE(nc == kCopyVoices, "decode_nocopy: the corpus has 4 voices, nc = %d", nc);
    VQ_REQUIRE(!win || chorale, "decode_nocopy: a window index needs the chorale");
    CopyVocab vv;
    for (int c = 0; c < kCopyVoices; ++c) {
        vv.V[c] = voice_offsets[c + 1] - voice_offsets[c];
        VQ_REQUIRE(vv.V[c] >= 1 && vv.V[c] <= kCopyMaxVocab, "decode_nocopy: 1 <= V_c <= 256 for every voice (V_%d = %d)", c, vv.V[c]);
    }
    VQ_REQUIRE(ldtok >= T && (!chorale || ldch >= T) && (!constraint || ldcons >= T) && (!copy_static || ldstatic >= T) && ldsets >= T &&
                   (!copy_report || ldreport >= T),
               "decode_nocopy: bad leading dimensions (every one >= T)");
    hipLaunchKernelGGL(decode_nocopy_kernel, dim3((unsigned)M), dim3(64), 0, (hipStream_t)stream, tokens, ldtok, T, chorale, ldch,
                       constraint, ldcons, copy_view(keys, where, entries, framed, n_framed, max_copy), vv, exclude, copy_static, ldstatic,
                       sets, ldsets, copy_report, ldreport, pos, win, U);
    VQ_CHECK_LAUNCH("decode_nocopy");
    return VQCPC_OK;
}

int vqcpc_nocopy_audit(const int64_t* x, int64_t ld, int64_t width, const int64_t* keys, const int64_t* where, int64_t entries,
                       const uint64_t* framed, int64_t n_framed, int max_copy, int32_t* report, int64_t ldreport, int64_t rows,
                       void* stream) {
    VQ_REQUIRE(x && report, "nocopy_audit: x and report are needed");
    VQ_REQUIRE(copy_index_ok(keys, where, entries, framed, n_framed, max_copy),
               "nocopy_audit: an index (keys, where, framed; 1 <= n_framed < 2^30, 1 <= max_copy <= 512) is needed");
    VQ_REQUIRE(rows >= 1 && rows <= 65535 && width >= 1 && width % kCopyVoices == 0 && width <= (int64_t)INT32_MAX * kCopyAuditCols,
               "nocopy_audit: bad arguments (1 <= rows <= 65535, width a positive multiple of 4)");
    VQ_REQUIRE(ld >= width && ldreport >= width, "nocopy_audit: bad leading dimensions (ld, ldreport >= width)");
    const dim3 grid((unsigned)ceil_div(width, kCopyAuditCols), (unsigned)rows);
    hipLaunchKernelGGL(nocopy_audit_kernel, grid, dim3(64), 0, (hipStream_t)stream, x, ld, width,
                       copy_view(keys, where, entries, framed, n_framed, max_copy), report, ldreport);
    VQ_CHECK_LAUNCH("nocopy_audit");
    return VQCPC_OK;
}

int vqcpc_nocopy_beam_column(int32_t* copy_report, int64_t ldreport, const int32_t* ancestors, const int32_t* flag, const int32_t* bound,
                             int64_t M, int W, void* stream) {
    VQ_REQUIRE(copy_report && ancestors && flag && bound, "nocopy_beam_column: null pointer");
    VQ_REQUIRE(M >= 1 && M <= kCopyMaxRows && W >= 1 && W <= M && M % W == 0 && ldreport >= 1,
               "nocopy_beam_column: bad arguments (1 <= M <= 64, W dividing M, ldreport >= 1)");
    hipLaunchKernelGGL(nocopy_beam_column_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, copy_report, ldreport, ancestors, flag, bound,
                       (int)M, W);
    VQ_CHECK_LAUNCH("nocopy_beam_column");
    return VQCPC_OK;
}

}  // extern "C"
