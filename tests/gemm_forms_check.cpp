// Host check of vqcpc_bach_amd/csrc/gemm_forms.h (no HIP, no GPU; built and run by tests/test_gemm_forms.py, with the address and
// undefined-behaviour sanitizers): the table of gemm_nt_g3_kernel<EPI, PL> instantiations is the 28 forms written out below, the
// operands -> form mapping sends every combination of operands the entry points document to an entry and every other combination to
// none, and every entry is reached by some combination (no dead instantiation).
#include <cstdio>
#include <set>
#include <utility>

#include "../vqcpc_bach_amd/csrc/gemm_forms.h"

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

// what include/vqcpc.h documents for vqcpc_gemm_nt_grad / _f16x3 / _g3_pl, written without the mapping under test
static bool documented(const G3Operands& o) {
    if (o.pl_a && !o.pl_b) return false;                                  // a pre-split A comes with a pre-split B
    bool p4a_ok;                                                          // may A be pre-split in this form?
    if (o.bias) {                                                         // forward forms
        if (o.gate_mask || o.add2 || o.relu != o.mask_out || (o.relu && o.add)) return false;
        if (o.drop && !o.add && !o.relu) return false;                    // dropout goes with a residual or relu
        p4a_ok = !o.relu;
    } else {                                                              // input-gradient forms
        if (o.relu || o.drop || o.mask_out || (o.add2 && !o.add) || (o.gate_mask && o.add)) return false;
        p4a_ok = !o.gate_mask && !o.add2;
    }
    return p4a_ok || !o.pl_a;
}

int main() {
    // 1. the tables
    const int every[11] = {0,
                           E_ADD,
                           E_ADD | E_ADD2,
                           G_ACCUM,
                           E_ADD | G_ACCUM,
                           E_GATEBITS,
                           E_BIAS,
                           E_BIAS | E_ADD,
                           E_BIAS | E_DROP | E_ADD,
                           E_BIAS | E_RELU | E_MASKOUT,
                           E_BIAS | E_RELU | E_DROP | E_MASKOUT};
    const int p4a[6] = {0, E_ADD, G_ACCUM, E_BIAS, E_BIAS | E_ADD, E_BIAS | E_DROP | E_ADD};
    FormSet want;
    for (int e : every) want.insert({e, 0}), want.insert({e, 2});
    for (int e : p4a) want.insert({e, 3});
    size_t n = 0;
    const FormSet table = entries(G3Forms{}, &n);
    CHECK(n == 28 && table.size() == 28 && table == want, "G3Forms has %zu entries, %zu distinct: not the 28 instantiations", n,
          table.size());
    size_t n9 = 0, n8 = 0, n3 = 0;
    const FormSet nt9 = entries(NtForms{}, &n9), nt8 = entries(NtForms64{}, &n8), ntg = entries(NtGradForms{}, &n3);
    FormSet nt9_less = nt9;
    nt9_less.erase({E_ADD | E_ADD2, 0});
    CHECK(n9 == 9 && nt9.size() == 9 && n8 == 8 && nt8 == nt9_less, "NtForms64 is not NtForms without add + add2");
    for (const auto& f : ntg) CHECK(nt9.count(f) == 1, "NtGradForms entry %d is not in NtForms", f.first);

    // 2. every combination of present / absent operands
    FormSet reached;
    int accepted = 0;
    for (unsigned bits = 0; bits < (1u << 11); ++bits) {
        const auto bit = [&](int i) { return ((bits >> i) & 1u) != 0; };
        const G3Operands o{bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8), bit(9), bit(10)};
        if ((o.add_is_c && !o.add) || (o.add2_is_c && !o.add2)) continue;             // an absent operand is not C
        const G3Form f = g3_form(o);
        int calls = 0;
        const bool found = dispatch(G3Forms{}, f.epi, f.pl, [&](auto v) {
            ++calls;
            CHECK(decltype(v)::a == f.epi && decltype(v)::b == f.pl, "dispatch(%d, %d) called entry (%d, %d)", f.epi, f.pl,
                  decltype(v)::a, decltype(v)::b);
        });
        CHECK(calls == (found ? 1 : 0), "dispatch(%d, %d) made %d calls", f.epi, f.pl, calls);
        CHECK(found == documented(o), "operands %#x -> form (%d, %d): %s, but the combination is %s", bits, f.epi, f.pl,
              found ? "instantiated" : "not instantiated", documented(o) ? "documented" : "not documented");
        if (found) reached.insert({f.epi, f.pl}), ++accepted;
    }
    CHECK(reached == table, "%zu of the %zu instantiations are reached by some combination of operands", reached.size(), table.size());
    // the in-place forms: only a residual that IS C accumulates
    CHECK(g3_form({false, false, false, true, false, true, false, false, false, false, true}).epi == G_ACCUM, "add == C");
    CHECK(g3_form({false, false, false, true, true, false, true, false, false, false, true}).epi == (E_ADD | G_ACCUM), "add2 == C");
    CHECK(g3_form({false, false, false, true, true, true, false, false, false, false, true}).epi == (E_ADD | E_ADD2), "add == C beside add2");
    CHECK(g3_form({true, false, false, true, false, true, false, false, false, false, true}).epi == (E_BIAS | E_ADD), "bias + add == C");
    std::printf("%d accepted combinations, %zu forms reached, %d failures\n", accepted, reached.size(), failures);
    return failures ? 1 : 0;
}
