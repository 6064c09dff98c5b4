// Host check of vqcpc_bach_amd/csrc/relattn_forms.h (no HIP, no GPU; built and run by tests/test_attention_entry_refusals_cpu.py with
// the address and undefined-behaviour sanitizers): att_route() sends every call of the ten self-attention entry points to the kernel
// that include/vqcpc.h and the header's own comment document for it, every instantiation of the two kernel lists is reached by some
// call, and no call selects a kernel outside them.
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>

#include "../vqcpc_bach_amd/csrc/relattn_forms.h"

using namespace vq;
typedef std::set<std::pair<int, int>> FormSet;

template <class... T>
static FormSet entries(Forms<T...>, size_t* count) {
    *count = sizeof...(T);
    return FormSet{{T::a, T::b}...};
}

static int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++failures;                  \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");           \
        }                                \
    } while (0)

// The documented rule, written entry by entry without the table under test.  `al`: the aligned pointers.
static AttKernel documented(int family, bool bwd, int L, int H, int hd, bool force, unsigned al, bool tokens) {
    const bool qkv = al & P_QKV, e1 = al & P_E1, e2 = al & P_E2, out = al & P_OUT, dctx = !bwd || (al & P_DCTX), ws = al & P_WS;
    const bool hd3 = hd == 16 || hd == 32 || hd == 64;
    // "L = 16 and L = 4 run the one-wavefront-per-block kernels": 4 (L = 16) or 16 (L = 4) problems per workgroup, whole heads
    const bool wave = !force && hd3 && ((L == 16 && (H == 1 || H == 2 || H % 4 == 0)) || (L == 4 && (16 % H == 0 || H % 16 == 0)));
    const bool cores = L == 16;                                  // the matrix-core kernels, given aligned operands
    switch (family) {
        case ATT_F32:
            if (wave) return cores && qkv && e1 && e2 && out && dctx ? ATT_MFMA16 : ATT_LDS;
            // "any other L <= 1024 ... runs the strip kernels of relattn_x.hip"; force_general "routes every L through the latter"
            if (L < 1 || L > 1024 || !(hd3 || hd == 128)) return ATT_REFUSED;
            return (bwd ? qkv && dctx && ws : qkv && e1 && e2) ? ATT_STRIP : ATT_REFUSED;
        case ATT_B16:                                              // "L in {16, 4}; L = 16 is forwarded to the matrix-core kernels"
            if (!wave || !qkv || !out || !dctx) return ATT_REFUSED;
            return cores && e1 && e2 ? ATT_MFMA16 : ATT_LDS;
        case ATT16_B16:
        case ATT16_B16IO:                                          // L = 16 matrix-core attention only, any head count
            return !force && hd3 && H >= 1 && qkv && e1 && e2 && out && dctx ? ATT_MFMA16 : ATT_REFUSED;
        default:                                                   // ATT_TAB: "L in {16, 4} only", rows through the tokens
            if (!tokens || !wave) return ATT_REFUSED;
            return cores && qkv && e1 && e2 && out && dctx ? ATT_MFMA16 : ATT_LDS;
    }
}

int main() {
    // 1. the table: five families, forward then backward, io and token use as include/vqcpc.h declares them
    const char* names[10] = {"relattn_fwd",         "relattn_bwd",         "relattn_fwd_b16", "relattn_bwd_b16", "relattn16_fwd_b16",
                             "relattn16_bwd_b16",   "relattn16_fwd_b16io", "relattn16_bwd_b16io", "relattn_tab_fwd", "relattn_tab_bwd"};
    const int io[5] = {0, OUT16, OUT16, IN16 | OUT16, 0};
    const AttTokens tok[5] = {TOK_NONE, TOK_NONE, TOK_OPTIONAL, TOK_NONE, TOK_REQUIRED};
    for (int i = 0; i < 10; ++i) {
        const AttEntry& e = kAttEntries[i];
        CHECK(std::strcmp(e.name, names[i]) == 0 && e.bwd == (i % 2 == 1) && e.io == io[i / 2] && e.tokens == tok[i / 2] &&
                  e.has_L == (i / 2 != ATT16_B16 && i / 2 != ATT16_B16IO),
              "entry %d (%s) is not %s as declared", i, e.name, names[i]);
        CHECK((e.must & e.mfma) == e.must && !(e.must & P_WS) && (e.bwd || !((e.must | e.mfma | e.strips) & (P_DCTX | P_WS))),
              "entry %s: pointer sets", e.name);
    }
    size_t n_lds = 0, n_16 = 0;
    const FormSet lds = entries(AttLdsForms{}, &n_lds), m16 = entries(Att16Forms{}, &n_16);
    CHECK(n_lds == 6 && lds.size() == 6 && n_16 == 9 && m16.size() == 9, "the lists hold %zu and %zu instantiations", n_lds, n_16);

    // 2. every call
    const int Ls[6] = {1, 4, 16, 24, 1024, 1025}, Hs[4] = {1, 2, 3, 8}, hds[5] = {8, 16, 32, 64, 128};
    FormSet lds_reached, m16_reached;
    long calls = 0, count[4] = {0, 0, 0, 0};
    for (int i = 0; i < 10; ++i)
        for (int L : Ls)
            for (int H : Hs)
                for (int hd : hds)
                    for (int flags = 0; flags < 4; ++flags)
                        for (unsigned al = 0; al < 64; ++al) {
                            const AttEntry& e = kAttEntries[i];
                            const bool force = flags & 1, tokens = flags & 2;
                            const AttRoute r = att_route(e, L, H, hd, force, al, tokens);
                            const AttKernel want = documented(i / 2, e.bwd, e.has_L ? L : 16, H, hd, force, al, tokens);
                            ++calls, ++count[r.kernel];
                            CHECK(r.kernel == want, "%s L=%d H=%d hd=%d force=%d aligned=%#x tokens=%d: route %d, documented %d",
                                  e.name, L, H, hd, force, al, tokens, r.kernel, want);
                            CHECK((r.kernel == ATT_REFUSED) == (r.why != nullptr), "%s: a refusal and only a refusal says why", e.name);
                            if (r.kernel == ATT_LDS) {
                                CHECK(dispatch(AttLdsForms{}, L, hd, [&](auto) {}) && !(e.io & IN16), "%s: no LDS kernel <%d, %d>", e.name, L, hd);
                                lds_reached.insert({L, hd});
                            } else if (r.kernel == ATT_MFMA16) {
                                CHECK(dispatch(Att16Forms{}, hd, e.io, [&](auto) {}), "%s: no matrix-core kernel <%d, io %d>", e.name, hd, e.io);
                                m16_reached.insert({hd, e.io});
                            }
                        }
    CHECK(lds_reached == lds && m16_reached == m16, "%zu of %zu and %zu of %zu instantiations are reached", lds_reached.size(), lds.size(),
          m16_reached.size(), m16.size());
    std::printf("%ld calls: %ld refused, %ld strip, %ld matrix-core, %ld LDS; %zu + %zu forms reached, %d failures\n", calls, count[ATT_REFUSED],
                count[ATT_STRIP], count[ATT_MFMA16], count[ATT_LDS], lds_reached.size(), m16_reached.size(), failures);
    return failures ? 1 : 0;
}
