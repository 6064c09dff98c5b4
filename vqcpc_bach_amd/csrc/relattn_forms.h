// The public self-attention entry points (include/vqcpc.h: vqcpc_relattn_*, vqcpc_relattn16_*, vqcpc_relattn_tab_*), what each one
// takes, and how a call selects its kernel.  Plain C++17, no HIP: tests/relattn_forms_check.cpp walks these tables on the host.
//
// Ten entry points are two operations, self-attention forward and backward over blocks of length L; an AttEntry says in which four
// respects one differs from the next (io formats, token table, L an argument or 16, the strip kernels behind it) and which pointers
// it wants aligned.  relattn.hip has one checked launcher per direction (self_fwd, self_bwd) that reads the entry and takes the
// kernel from att_route().  The two Forms lists at the end instantiate the kernels.
//
// The entries were written one by one and differ in ways that nothing explains.  The table keeps every difference as it was:
//   - no backward checks drop_p; every forward does (self_bwd has no such line);
//   - relattn_fwd_b16 / _bwd_b16 refuse a misaligned q|k|v, ctx, d ctx or d q|k|v (`must`) ...
//   - ... while relattn_fwd / _bwd and relattn_tab_fwd / _bwd refuse nothing at L in {4, 16} (`must` = 0): a misaligned pointer
//     only sends the call from the matrix-core kernel to the LDS kernels, which read rows through float4 casts themselves;
//   - relattn16_* want every pointer aligned (`must` = `mfma`) and have no other kernel to fall to;
//   - the strip kernels behind relattn_fwd / _bwd want q|k|v, e1, e2 (forward) and q|k|v, d ctx, the workspace (backward).
// Whether any of this is a bug is for a later change to decide.  One difference is not kept: relattn_fwd_b16 and relattn_tab_fwd did
// not look at a negative n_blocks and computed a grid from it (zero or wrapped: an invalid launch); every forward now refuses it.
#pragma once

#include "gemm_forms.h"

namespace vq {

enum { IN16 = 1, OUT16 = 2 };      // io bits: q|k|v (and d ctx) are bf16, leading dimensions multiples of 8; ctx / d q|k|v are bf16
enum AttTokens { TOK_NONE, TOK_REQUIRED, TOK_OPTIONAL };      // rows fetched through a token table
// pointers of a call; P_OUT is ctx in the forward and d q|k|v in the backward, P_DCTX and P_WS exist in the backward only
enum { P_QKV = 1, P_E1 = 2, P_E2 = 4, P_OUT = 8, P_DCTX = 16, P_WS = 32 };
constexpr unsigned P_FWD = P_QKV | P_E1 | P_E2 | P_OUT, P_BWD = P_FWD | P_DCTX;

struct AttEntry {
    const char* name;
    bool bwd;
    int io;
    AttTokens tokens;
    bool has_L;        // L is an argument (else 16, and the matrix-core kernels are the only ones)
    unsigned strips;   // other L go to the strip kernels of relattn_x.hip, which want these pointers aligned (0: other L are refused)
    unsigned must;     // 16-byte aligned, or the call is refused
    unsigned mfma;     // all aligned: the matrix-core kernel (L = 16); else the LDS kernel
};

constexpr AttEntry kAttEntries[10] = {
    {"relattn_fwd", false, 0, TOK_NONE, true, P_QKV | P_E1 | P_E2, 0, P_FWD},
    {"relattn_bwd", true, 0, TOK_NONE, true, P_QKV | P_DCTX | P_WS, 0, P_BWD},
    {"relattn_fwd_b16", false, OUT16, TOK_NONE, true, 0, P_QKV | P_OUT, P_FWD},
    {"relattn_bwd_b16", true, OUT16, TOK_NONE, true, 0, P_QKV | P_DCTX | P_OUT, P_BWD},
    {"relattn16_fwd_b16", false, OUT16, TOK_OPTIONAL, false, 0, P_FWD, P_FWD},
    {"relattn16_bwd_b16", true, OUT16, TOK_OPTIONAL, false, 0, P_BWD, P_BWD},
    {"relattn16_fwd_b16io", false, IN16 | OUT16, TOK_NONE, false, 0, P_FWD, P_FWD},
    {"relattn16_bwd_b16io", true, IN16 | OUT16, TOK_NONE, false, 0, P_BWD, P_BWD},
    {"relattn_tab_fwd", false, 0, TOK_REQUIRED, true, 0, 0, P_FWD},
    {"relattn_tab_bwd", true, 0, TOK_REQUIRED, true, 0, 0, P_BWD},
};
enum { ATT_F32, ATT_B16, ATT16_B16, ATT16_B16IO, ATT_TAB };      // kAttEntries[2 * family + (backward ? 1 : 0)]

inline bool att_hd_ok(int hd) { return hd == 16 || hd == 32 || hd == 64; }
// the one-wavefront-per-block LDS kernels: 4 waves of 64 / (4 L) block slots each, heads and slots must divide one another
inline bool att_lds_ok(int L, int H, int hd) {
    if (!(L == 16 || L == 4) || !att_hd_ok(hd) || H < 1) return false;
    const int slots = 4 * (64 / (4 * L));
    return slots % H == 0 || H % slots == 0;
}
inline bool att_mfma16_ok(int L, int H, int hd) { return L == 16 && H >= 1 && att_hd_ok(hd); }
inline bool att_strip_ok(int L, int H, int hd) { return L >= 1 && L <= 1024 && H >= 1 && (att_hd_ok(hd) || hd == 128); }

enum AttKernel { ATT_REFUSED, ATT_STRIP, ATT_MFMA16, ATT_LDS };
struct AttRoute {
    AttKernel kernel;
    const char* why;      // ATT_REFUSED: what is wrong, to stand in front of "L=.. H=.. hd=.."
};

// force_general: vqcpc_relattn_force_general(1); aligned: P_ bits of the 16-byte
// aligned pointers.  L is ignored (16) by an entry that does not take it.
inline AttRoute att_route(const AttEntry& e, int L, int H, int hd, bool force_general, unsigned aligned,
                          bool tokens_given) {
    const auto all = [&](unsigned set) { return (aligned & set) == set; };
    if (e.tokens == TOK_REQUIRED && !tokens_given) return {ATT_REFUSED, "no tokens for"};
    if (!e.has_L) {
        if (force_general || !att_mfma16_ok(16, H, hd)) return {ATT_REFUSED, "unsupported"};
        return all(e.must) ? AttRoute{ATT_MFMA16, nullptr} : AttRoute{ATT_REFUSED, "a buffer is not 16-byte aligned for"};
    }
    if (force_general || !att_lds_ok(L, H, hd)) {
        if (!e.strips || !att_strip_ok(L, H, hd)) return {ATT_REFUSED, "unsupported"};
        return all(e.strips) ? AttRoute{ATT_STRIP, nullptr} : AttRoute{ATT_REFUSED, "a buffer is not 16-byte aligned for"};
    }
    if (!all(e.must)) return {ATT_REFUSED, "a buffer is not 16-byte aligned for"};
    return {att_mfma16_ok(L, H, hd) && all(e.mfma) ? ATT_MFMA16 : ATT_LDS, nullptr};
}

// relattn_fwd_kernel / relattn_bwd_kernel<L, HD> (relattn.hip) ...
using AttLdsForms = Forms<Form<16, 16>, Form<16, 32>, Form<16, 64>, Form<4, 16>, Form<4, 32>, Form<4, 64>>;
// ... and relattn16_fwd_kernel / relattn16_bwd_kernel<HD, B16 = io & OUT16, IN16 = io & IN16> (relattn16.hip): Form<HD, io>
using Att16Forms = Forms<Form<16, 0>, Form<32, 0>, Form<64, 0>, Form<16, OUT16>, Form<32, OUT16>, Form<64, OUT16>,
                         Form<16, IN16 | OUT16>, Form<32, IN16 | OUT16>, Form<64, IN16 | OUT16>>;

}  // namespace vq
