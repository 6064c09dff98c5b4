// Which template instantiations ("forms") of the GEMM kernels exist, and how a call's operands select one.  Plain C++17, no HIP:
// tests/gemm_forms_check.cpp walks these tables on the host.
//
// A form is a Form<A, B> of compile-time integers (epilogue bits, and a second parameter where the kernel has one); a kernel
// family's table is a Forms<...> list.  dispatch() turns run-time values into the compile-time entry that equals them, so a form
// that is not in its table cannot be launched.  To add a form: add its entry to the family's table -- that instantiates the kernel --
// and, for gemm_nt_g3_kernel, make g3_form() below produce it.
#pragma once

namespace vq {

// epilogue feature bits (compile-time); E_RUNTIME = decide everything from EpiParams at run time (rare combinations)
enum { E_BIAS = 1, E_RELU = 2, E_DROP = 4, E_GATE = 8, E_ADD = 16, E_RUNTIME = 32, E_ADD2 = 64, E_MASKOUT = 128, E_GATEBITS = 256 };
// gemm_nt_g3_kernel only: the residual already sits in C, accumulate in place (gemm_grad.hip)
constexpr int G_ACCUM = 512;

template <int A, int B = 0>
struct Form {
    static constexpr int a = A, b = B;
};
template <class... T>
struct Forms {};

// fn(Form<a, b>{}) for the entry of the table that equals (a, b); false, and no call, when there is none
template <class... T, class Fn>
inline bool dispatch(Forms<T...>, int a, int b, Fn&& fn) {
    return (((a == T::a && b == T::b) ? (fn(T{}), true) : false) || ...);
}
// lists joined, and a list with every entry's second parameter set to B
template <class... L>
struct Concat;
template <class... T>
struct Concat<Forms<T...>> {
    using type = Forms<T...>;
};
template <class... T, class... U, class... R>
struct Concat<Forms<T...>, Forms<U...>, R...> : Concat<Forms<T..., U...>, R...> {};
template <int B, class L>
struct WithB;
template <int B, class... T>
struct WithB<B, Forms<T...>> {
    using type = Forms<Form<T::a, B>...>;
};

// ---- bf16x6 / fp32 NT kernels (gemm.hip): epilogue forms with a compile-time instantiation -----------------------------------
// the 64-tile kernel's eight ...
using NtForms64 = Forms<Form<0>, Form<E_BIAS>, Form<E_BIAS | E_RELU>, Form<E_BIAS | E_RELU | E_DROP>, Form<E_GATE>, Form<E_ADD>,
                        // s = x + dropout(a W^T + b): the residual sum that LayerNorm normalises (transformer_custom.py:282-283,
                        // 288-289), produced by the out-proj / FFN2 epilogue so that the LayerNorm kernels read ONE input stream
                        Form<E_BIAS | E_ADD>, Form<E_BIAS | E_DROP | E_ADD>>;
// ... and the nine of the 128- and 256-tile kernels (any other combination: gemm_nt_kernel<.., E_RUNTIME, ..>)
using NtForms = Concat<NtForms64, Forms<Form<E_ADD | E_ADD2>>>::type;
// 256-tile ping-pong kernel: the forms that have a two-plane ("gradient arithmetic", NP = 2) instantiation ...
using NtGradForms = Forms<Form<0>, Form<E_ADD>, Form<E_ADD | E_ADD2>>;
// ... and its bit-mask forms (vqcpc_gemm_nt_relu_mask, vqcpc_gemm_nt_gatebits)
using NtMaskForms = Forms<Form<E_BIAS | E_RELU | E_MASKOUT>, Form<E_BIAS | E_RELU | E_DROP | E_MASKOUT>, Form<E_GATEBITS>>;

// ---- f16x3 256-tile kernel (gemm_grad.hip): gemm_nt_g3_kernel<EPI, PL> ------------------------------------------------------
// PL bit 0 / bit 1: operand A / B arrives pre-split ("P4").  Every epilogue takes an fp32 A, with B fp32 (PL 0) or P4 (PL 2) ...
using G3Epilogues = Forms<Form<0>, Form<E_ADD>, Form<E_ADD | E_ADD2>, Form<G_ACCUM>, Form<E_ADD | G_ACCUM>, Form<E_GATEBITS>,
                          Form<E_BIAS>, Form<E_BIAS | E_ADD>, Form<E_BIAS | E_DROP | E_ADD>, Form<E_BIAS | E_RELU | E_MASKOUT>,
                          Form<E_BIAS | E_RELU | E_DROP | E_MASKOUT>>;
// ... and these take a P4 A beside a P4 B (PL 3): the products whose A is written in P4 by its producer
using G3EpiloguesP4A = Forms<Form<0>, Form<E_ADD>, Form<G_ACCUM>, Form<E_BIAS>, Form<E_BIAS | E_ADD>, Form<E_BIAS | E_DROP | E_ADD>>;
using G3Forms = Concat<WithB<0, G3Epilogues>::type, WithB<2, G3Epilogues>::type, WithB<3, G3EpiloguesP4A>::type>::type;

// The operands of one product on gemm_nt_g3_kernel that select its form: which are present, and which residual is C itself (same
// pointer, same leading dimension).
struct G3Operands {
    bool bias, relu, drop, add, add2, add_is_c, add2_is_c, gate_mask, mask_out, pl_a, pl_b;
};
struct G3Form {
    int epi, pl;
};
inline G3Form g3_form(const G3Operands& o) {
    int epi = (o.bias ? E_BIAS : 0) | (o.relu ? E_RELU : 0) | (o.drop ? E_DROP : 0) | (o.add ? E_ADD : 0) | (o.add2 ? E_ADD2 : 0) |
              (o.gate_mask ? E_GATEBITS : 0) | (o.mask_out ? E_MASKOUT : 0);
    if (epi == E_ADD && o.add_is_c) epi = G_ACCUM;                                   // C += A . B^T
    else if (epi == (E_ADD | E_ADD2) && o.add2_is_c) epi = E_ADD | G_ACCUM;          // C += A . B^T + add
    return {epi, (o.pl_a ? 1 : 0) | (o.pl_b ? 2 : 0)};
}

}  // namespace vq
