// Voice-leading rules as context-dependent token sets (decoders/generation.py `rules=`; the rule is stated once, in numpy, in
// tests/rules_reference.py).  Exact integer logic, no floating point, no LDS.
//   * vqcpc_decode_rules: the step form.  ONE launch, a wavefront per row (M <= 64), issued immediately before the masked
//     sampler inside the captured step.  It reads `pos` and `win` from device memory as the sampler does, evaluates the
//     position's candidates against the tokens emitted so far and OVERWRITES the 256-bit set of the live column in the buffer
//     the sampler reads, and the column's report.  The caller's static sets stay in a second buffer.
//   * vqcpc_rules_audit: the same device function over a grid of (row, column range): every token is taken as forced and all
//     history comes from one token tensor; it writes the forced half of the report (the violated rules' bits << 4).
// Position: column col, tick e = col / nc, voice v = col % nc (voice 0 is the top voice).  kinds[u][tok] is a MIDI pitch >= 0,
// HOLD (-1) or anything below (REST, META: no pitch).
//   look-back: pitch_at(u, e') walks back from tick e' while voice u holds, 64 ticks per iteration (lane l looks at tick
//     e' - 64 i - l), and a ballot finds the most recent tick that does not hold; no bound but column 0.
//   voices: lane u keeps voice u's pitch of this tick (`now`, NONE unless the voice is known) and of the previous one (`prev`);
//     a candidate's test reads them with shuffles.
//   candidates: four per lane, k = 64 j + l, so that the ballot of pass j IS the words 2 j and 2 j + 1 of the set.
//   relaxation: E = static set minus exclude, D = the candidates that break no enabled rule; while E & D is empty (a wave-wide
//     any-reduction per level) PARALLEL, then LEAP, then CROSSING is dropped.  The set written is static & D_final with the bits
//     at and past V_v cleared; were it empty inside the vocabulary -- which the sampler would read as "no restriction" -- the
//     whole vocabulary is written instead, which says the same thing explicitly.
#include "common.h"

namespace vq {

constexpr int kRuleMaxRows = 64;
constexpr int kRuleMaxVoices = 16;
constexpr int kRuleMaxVocab = 256;
constexpr int kRuleHold = -1;
constexpr int kRuleMeta = -3;
constexpr int kRuleNone = INT32_MIN;         // no pitch
constexpr int kRuleCrossing = 1, kRuleLeap = 2, kRuleParallel = 4;
constexpr int kAuditWaves = 4;
constexpr int kAuditCols = 64;               // columns of a row per audit workgroup

struct RuleVocab {
    int V[kRuleMaxVoices];
};

// a row's history: column c lives in hi[c - base] (the live window's tokens) for c >= base, else in lo[c] (the chorale)
struct RuleHistory {
    const int64_t* lo;
    int64_t ldlo;
    const int64_t* hi;
    int64_t base;
};

__device__ __forceinline__ int64_t rule_token(const RuleHistory& h, int64_t c) {
    if (c >= h.base) return h.hi[c - h.base];
    return c < h.ldlo ? h.lo[c] : (int64_t)-1;
}

__device__ __forceinline__ int rule_kind(const int32_t* __restrict__ kinds, int ldk, int V, int u, int64_t tok) {
    return (tok >= 0 && tok < V) ? kinds[(int64_t)u * ldk + tok] : kRuleMeta;
}

// the pitch voice u sounds at tick e1 (wave-uniform result)
__device__ __forceinline__ int rule_pitch_at(const RuleHistory& h, const int32_t* __restrict__ kinds, int ldk, int V, int nc, int u,
                                             int64_t e1, int lane) {
    for (int64_t t0 = e1;; t0 -= 64) {
        const int64_t t = t0 - lane;
        int kd = kRuleMeta;                                   // before column 0: the walk stops without a pitch
        if (t >= 0) kd = rule_kind(kinds, ldk, V, u, rule_token(h, t * nc + u));
        const unsigned long long stop = __ballot(kd != kRuleHold);
        if (stop != 0ull) {                                   // uniform; some lane has t < 0 once t0 < 63
            const int k = __shfl(kd, __ffsll(stop) - 1, 64);
            return k >= 0 ? k : kRuleNone;
        }
    }
}

// the rules a candidate of kind ck breaks (all three, enabled or not); every lane calls it: the voices are read by shuffles
__device__ __forceinline__ int rule_violations(int ck, int prev_v, int leap_v, int v, int nc, int now_l, int prev_l) {
    const int p = ck >= 0 ? ck : ck == kRuleHold ? prev_v : kRuleNone;
    int bits = 0;
    if (ck >= 0 && prev_v != kRuleNone && leap_v >= 0 && abs(ck - prev_v) > leap_v) bits |= kRuleLeap;
    const bool moves = p != kRuleNone && prev_v != kRuleNone && p != prev_v;
    for (int u = 0; u < nc; ++u) {
        const int nu = __shfl(now_l, u, 64), pu = __shfl(prev_l, u, 64);
        if (nu == kRuleNone || p == kRuleNone) continue;      // unknown voices (and voice v itself) hold NONE
        if (u < v ? p > nu : p < nu) bits |= kRuleCrossing;
        if (moves && pu != kRuleNone && nu != pu && (nu > pu) == (p > prev_v)) {
            const int a = abs(nu - p) % 12, b = abs(pu - prev_v) % 12;
            if (a == b && (a == 0 || a == 7)) bits |= kRuleParallel;
        }
    }
    return bits;
}

// One position of one row, one wavefront.  constraint: the row's forced tokens (NULL: none), columns >= ldcons are free;
// stat: the 8 words of the column's static set or NULL; sets / report: where the column's set (8 words) and report go, or NULL.
__device__ __forceinline__ void rules_position(const RuleHistory& h, const int64_t* __restrict__ constraint, int64_t ldcons,
                                               const int32_t* __restrict__ kinds, int ldk, const RuleVocab& vv, int nc,
                                               const int32_t* __restrict__ max_leap, int enabled,
                                               const uint32_t* __restrict__ exclude, const uint32_t* __restrict__ stat,
                                               uint32_t* __restrict__ sets, int32_t* __restrict__ report, int64_t col, int lane) {
    const int v = (int)(col % nc);
    const int64_t e = col / nc;
    const int V = vv.V[v];
    int now_l = kRuleNone, prev_l = kRuleNone;                // lane u: voice u
    for (int u = 0; u < nc; ++u) {
        const int Vu = vv.V[u];
        const int pu = rule_pitch_at(h, kinds, ldk, Vu, nc, u, e - 1, lane);
        int nu = kRuleNone;
        if (u != v) {
            const int64_t c = e * nc + u;
            int64_t tok = -1;
            if (u < v) tok = rule_token(h, c);                // emitted at this tick
            else if (constraint && c < ldcons) tok = constraint[c];       // forced, not yet emitted
            if (tok >= 0) {
                const int kd = rule_kind(kinds, ldk, Vu, u, tok);
                nu = kd >= 0 ? kd : kd == kRuleHold ? pu : kRuleNone;
            }
        }
        if (lane == u) {
            now_l = nu;
            prev_l = pu;
        }
    }
    const int prev_v = __shfl(prev_l, v, 64);
    const int leap_v = max_leap ? max_leap[v] : -1;
    int64_t forced = -1;
    if (constraint && col < ldcons) forced = constraint[col];
    if (forced >= 0) {                                        // uniform
        const int bits = rule_violations(rule_kind(kinds, ldk, V, v, forced), prev_v, leap_v, v, nc, now_l, prev_l) & enabled;
        if (report && lane == 0) *report = bits << 4;
        if (sets && lane < 8) {
            const int left = V - 32 * lane;                   // no static set: the whole vocabulary, explicitly
            sets[lane] = stat ? stat[lane] : left >= 32 ? 0xFFFFFFFFu : left > 0 ? (1u << left) - 1u : 0u;
        }
        return;
    }
    int vi[4];
    bool inS[4], inE[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 64 * j + lane;
        const bool inV = k < V;
        const int ck = inV ? kinds[(int64_t)v * ldk + k] : kRuleMeta;
        vi[j] = rule_violations(ck, prev_v, leap_v, v, nc, now_l, prev_l) & enabled;
        const bool st = stat ? ((stat[k >> 5] >> (k & 31)) & 1u) != 0u : true;
        const bool ex = exclude ? ((exclude[v * 8 + (k >> 5)] >> (k & 31)) & 1u) != 0u : false;
        inS[j] = inV && st;
        inE[j] = inS[j] && !ex;
    }
    int drop = 0;
    for (int level = 0; level < 3; ++level) {                 // PARALLEL, then LEAP, then CROSSING
        bool mine = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) mine = mine || (inE[j] && (vi[j] & ~drop) == 0);
        if (__ballot(mine) != 0ull) break;                    // uniform
        drop |= kRuleParallel >> level;
    }
    unsigned long long m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = __ballot(inS[j] && (vi[j] & ~drop) == 0);
    if ((m[0] | m[1] | m[2] | m[3]) == 0ull) {                // nothing of the vocabulary in the static set
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = V >= 64 * (j + 1) ? ~0ull : V > 64 * j ? (1ull << (V - 64 * j)) - 1ull : 0ull;
    }
    if (sets && lane < 8) {
        const int j = lane >> 1;
        const unsigned long long w = j == 0 ? m[0] : j == 1 ? m[1] : j == 2 ? m[2] : m[3];
        sets[lane] = (uint32_t)(w >> (32 * (lane & 1)));
    }
    if (report && lane == 0) *report = drop & enabled;
}

__global__ __launch_bounds__(64) void decode_rules_kernel(
    const int64_t* __restrict__ tokens, int64_t ldtok, int T, const int64_t* __restrict__ chorale, int64_t ldch,
    const int64_t* __restrict__ constraint, int64_t ldcons, const int32_t* __restrict__ kinds, int ldk, RuleVocab vv, int nc,
    const int32_t* __restrict__ max_leap, int enabled, const uint32_t* __restrict__ exclude, const uint32_t* __restrict__ stat,
    int64_t ldstat, uint32_t* __restrict__ sets, int64_t ldsets, int32_t* __restrict__ report, int64_t ldrep,
    const int32_t* __restrict__ posp, const int32_t* __restrict__ win, int U) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int pos = *posp;
    if (pos < 0 || pos >= T) return;                          // uniform
    const int w0 = win ? win[1] : 0;
    if (w0 < 0) return;                                       // no live window
    const int64_t base = (int64_t)w0 * U, col = base + pos;
    RuleHistory h;
    h.lo = chorale ? chorale + (int64_t)b * ldch : nullptr;
    h.ldlo = chorale ? ldch : 0;
    h.hi = tokens + (int64_t)b * ldtok;
    h.base = base;
    rules_position(h, constraint ? constraint + (int64_t)b * ldcons : nullptr, ldcons, kinds, ldk, vv, nc, max_leap, enabled, exclude,
                   stat && col < ldstat ? stat + ((int64_t)b * ldstat + col) * 8 : nullptr,
                   col < ldsets ? sets + ((int64_t)b * ldsets + col) * 8 : nullptr,
                   report && col < ldrep ? report + (int64_t)b * ldrep + col : nullptr, col, lane);
}

__global__ __launch_bounds__(64 * kAuditWaves) void rules_audit_kernel(const int64_t* __restrict__ x, int64_t ld, int64_t width,
                                                                      const int32_t* __restrict__ kinds, int ldk, RuleVocab vv,
                                                                      int nc, const int32_t* __restrict__ max_leap, int enabled,
                                                                      int32_t* __restrict__ report, int64_t ldrep) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.y, c0 = (int64_t)blockIdx.x * kAuditCols;
    RuleHistory h;
    h.lo = x + b * ld;
    h.ldlo = width;
    h.hi = nullptr;
    h.base = INT64_MAX;                                       // every column comes from x
    for (int64_t col = c0 + wave; col < min(c0 + kAuditCols, width); col += kAuditWaves) {    // a wave's own trip count
        if (h.lo[col] < 0) {                                  // no token (uniform): nothing to judge
            if (lane == 0) report[b * ldrep + col] = 0;
            continue;
        }
        rules_position(h, h.lo, width, kinds, ldk, vv, nc, max_leap, enabled, nullptr, nullptr, nullptr, report + b * ldrep + col,
                       col, lane);
    }
}

static bool rule_vocab(const char* name, const int32_t* voice_offsets, int nc, int ldk, RuleVocab* vv) {
    for (int c = 0; c < kRuleMaxVoices; ++c) vv->V[c] = 0;
    for (int c = 0; c < nc; ++c) {
        const int V = voice_offsets[c + 1] - voice_offsets[c];
        if (V < 1 || V > kRuleMaxVocab || V > ldk) return false;
        vv->V[c] = V;
    }
    return true;
}

}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_decode_rules(const int64_t* tokens, int64_t ldtok, int T, const int64_t* chorale, int64_t ldch, const int64_t* constraint,
                       int64_t ldcons, const int32_t* kinds, int ldk, const int32_t* voice_offsets, int nc, const int32_t* max_leap,
                       int rules, const uint32_t* exclude, const uint32_t* static_sets, int64_t ldstatic, uint32_t* sets,
                       int64_t ldsets, int32_t* report, int64_t ldreport, const int32_t* pos, const int32_t* win, int U, int64_t M,
                       void* stream) {
    VQ_REQUIRE(tokens && kinds && voice_offsets && sets && pos, "decode_rules: tokens, kinds, voice_offsets, sets and pos are needed");
    VQ_REQUIRE(M >= 1 && M <= kRuleMaxRows && nc >= 1 && nc <= kRuleMaxVoices && T >= 1 && U >= 1,
               "decode_rules: bad arguments (1 <= M <= 64, 1 <= nc <= 16, T >= 1, U >= 1)");
    VQ_REQUIRE(rules >= 1 && rules <= 7 && (!(rules & kRuleLeap) || max_leap),
               "decode_rules: rules is a mask of CROSSING 1 | LEAP 2 | PARALLEL 4 (LEAP needs max_leap)");
    VQ_REQUIRE(!win || chorale, "decode_rules: a window index needs the chorale");
    RuleVocab vv;
    VQ_REQUIRE(rule_vocab("decode_rules", voice_offsets, nc, ldk, &vv), "decode_rules: 1 <= V_c <= 256 and V_c <= ldk for every voice");
    // the window index lives on the device: the kernel skips whatever lies at or past a leading dimension
    VQ_REQUIRE(ldtok >= T && (!chorale || ldch >= T) && (!constraint || ldcons >= T) && (!static_sets || ldstatic >= T) && ldsets >= T &&
                   (!report || ldreport >= T),
               "decode_rules: bad leading dimensions (every one >= T)");
    hipLaunchKernelGGL(decode_rules_kernel, dim3((unsigned)M), dim3(64), 0, (hipStream_t)stream, tokens, ldtok, T, chorale, ldch, constraint,
                       ldcons, kinds, ldk, vv, nc, max_leap, rules, exclude, static_sets, ldstatic, sets, ldsets, report, ldreport, pos, win,
                       U);
    VQ_CHECK_LAUNCH("decode_rules");
    return VQCPC_OK;
}

int vqcpc_rules_audit(const int64_t* x, int64_t ld, int64_t width, const int32_t* kinds, int ldk, const int32_t* voice_offsets, int nc,
                      const int32_t* max_leap, int rules, int32_t* report, int64_t ldreport, int64_t rows, void* stream) {
    VQ_REQUIRE(x && kinds && voice_offsets && report, "rules_audit: x, kinds, voice_offsets and report are needed");
    VQ_REQUIRE(rows >= 1 && rows <= 65535 && nc >= 1 && nc <= kRuleMaxVoices && width >= 1 && width % nc == 0 &&
                   width <= (int64_t)INT32_MAX * kAuditCols,
               "rules_audit: bad arguments (1 <= rows <= 65535, 1 <= nc <= 16, width a positive multiple of nc)");
    VQ_REQUIRE(rules >= 1 && rules <= 7 && (!(rules & kRuleLeap) || max_leap),
               "rules_audit: rules is a mask of CROSSING 1 | LEAP 2 | PARALLEL 4 (LEAP needs max_leap)");
    RuleVocab vv;
    VQ_REQUIRE(rule_vocab("rules_audit", voice_offsets, nc, ldk, &vv), "rules_audit: 1 <= V_c <= 256 and V_c <= ldk for every voice");
    VQ_REQUIRE(ld >= width && ldreport >= width, "rules_audit: bad leading dimensions (ld, ldreport >= width)");
    const dim3 grid((unsigned)ceil_div(width, kAuditCols), (unsigned)rows), block(64 * kAuditWaves);
    hipLaunchKernelGGL(rules_audit_kernel, grid, block, 0, (hipStream_t)stream, x, ld, width, kinds, ldk, vv, nc, max_leap, rules, report,
                       ldreport);
    VQ_CHECK_LAUNCH("rules_audit");
    return VQCPC_OK;
}

}  // extern "C"
