"""The float64 reference of the constrained sampler (tests/constrained_reference.py) against plain definitions, and the new
entry point's host-side argument checks (no GPU: the checks fail before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import constrained_reference as C
import decode_reference as R

SETTINGS = [(1.0, 0, 1.0, ()), (0.7, 5, 1.0, (1,)), (1.5, 0, 0.9, ()), (0.7, 4, 0.8, (0, 2))]


def _rows(M, V, seed):
    return torch.randn(M, V, generator=torch.Generator().manual_seed(seed)) * 2.0


@pytest.mark.parametrize('V', [3, 13, 256])
def test_all_free_is_the_filter_and_the_inverse_cdf_draw(V):
    M = 5
    lg = _rows(M, V, 100 + V)
    seeds = torch.arange(M, dtype=torch.int64) * 1000003 + 17
    for temperature, top_k, top_p, exclude in SETTINGS:
        for pos in (0, 7):
            for cons in (None, torch.full((M,), -1, dtype=torch.int64)):
                tok, pr, _ = C.constrained_step_ref(lg, temperature, top_k, top_p, exclude, seeds, pos, cons)
                for b in range(M):
                    want = R.filter_ref(lg[b], temperature, top_k, top_p, exclude)
                    assert torch.equal(pr[b], want)
                    u = (float(R.rng_u24_ref(int(seeds[b]), pos)) + 0.5) / 2.0 ** 24
                    cum = torch.cumsum(want, dim=0)
                    t = int(tok[b])
                    assert float(want[t]) > 0 and t not in exclude
                    assert float(cum[t]) - float(want[t]) <= u * float(cum[-1]) + 1e-15 and u * float(cum[-1]) < float(cum[t]) + 1e-15


def test_the_draw_is_keyed_by_seed_and_position_alone():
    """Forcing rows 0 and 2 leaves the draws of rows 1 and 3 as they are."""
    lg = _rows(4, 13, 7)
    seeds = torch.tensor([5, 6, 7, 8], dtype=torch.int64)
    free, _, _ = C.constrained_step_ref(lg, 1.0, 0, 1.0, (), seeds, 3, None)
    mixed, _, _ = C.constrained_step_ref(lg, 1.0, 0, 1.0, (), seeds, 3, torch.tensor([4, -1, 12, -5]))
    assert mixed.tolist() == [4, int(free[1]), 12, int(free[3])]


@pytest.mark.parametrize('V', [1, 2, 13, 256])
def test_all_forced_is_the_forced_tokens(V):
    M = 6
    lg = _rows(M, V, 200 + V)
    seeds = torch.zeros(M, dtype=torch.int64)
    cons = torch.tensor([0, V - 1, V // 2, V, V + 1000, 0], dtype=torch.int64)          # two past the vocabulary: clamped
    for temperature, top_k, top_p, exclude in SETTINGS:
        exclude = tuple(t for t in exclude if t < V and V > 3)
        tok, pr, _ = C.constrained_step_ref(lg, temperature, top_k, top_p, exclude, seeds, 1, cons)
        assert tok.tolist() == [0, V - 1, V // 2, V - 1, V - 1, 0]
        for b in range(M):                                                          # probs stay the filtered ones
            assert torch.equal(pr[b], R.filter_ref(lg[b], temperature, top_k, top_p, exclude))


@pytest.mark.parametrize('V', [1, 2, 13, 256])
def test_logp_is_log_softmax_of_the_unfiltered_row(V):
    M = 4
    lg = _rows(M, V, 300 + V)
    lg[1] = torch.linspace(-80.0, 80.0, V)[torch.randperm(V, generator=torch.Generator().manual_seed(1))] if V > 1 else lg[1]
    if V > 2:
        lg[2, ::2] = -float('inf')
    cons = torch.tensor([0, V - 1, min(1, V - 1), -1], dtype=torch.int64)
    seeds = torch.tensor([1, 2, 3, 4], dtype=torch.int64)
    for temperature, top_k, top_p, exclude in SETTINGS:
        exclude = tuple(t for t in exclude if t < V and V > 3)
        tok, _, lp = C.constrained_step_ref(lg, temperature, top_k, top_p, exclude, seeds, 2, cons)
        want = torch.log_softmax(lg.double(), dim=-1).gather(1, tok.view(-1, 1)).view(-1)
        assert torch.allclose(lp, want, rtol=0, atol=1e-12), (lp, want)              # filters and temperature do not enter
        if V > 2:
            assert float(lp[2]) > -float('inf') and float(C.logp_ref(lg[2], 0)) == -float('inf')


def test_logp_bound_covers_plain_fp32():
    """The bound holds for the same chain evaluated in fp32 numpy on the CPU (sequential sum: fewer roundings per term than
    gamma_255 allows but more than the kernel's nine -- so it is checked against gamma_V here), and is not vacuous."""
    g = torch.Generator().manual_seed(9)
    for V, scale in ((13, 2.0), (256, 2.0), (256, 40.0)):
        row = (torch.randn(V, generator=g) * scale).float()
        r = row.numpy()
        d = (r - r.max()).astype(np.float32)
        s = np.float32(0)
        for v in np.exp(d).astype(np.float32):
            s = np.float32(s + v)
        for tok in (0, V - 1, int(r.argmax())):
            got = float(np.float32(d[tok] - np.log(s, dtype=np.float32)))
            b = C.logp_bound(row, tok)
            assert 0 < b < 1e-4, b
            assert abs(got - C.logp_ref(row, tok)) <= b + V * C.U_FP32, (V, scale, tok)


@pytest.fixture(scope='module')
def lib():
    import torch  # noqa: F401  (loads the process-wide libamdhip64.so.7 first)
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    return hip.load()


def test_constrained_entry_point_rejects_bad_arguments(lib):
    P, Q = 4096, 8192                     # stand-ins: nothing is dereferenced before the checks fail
    f = lib.vqcpc_decode_sample_constrained
    offs = (ctypes.c_int32 * 2)(0, 40)

    def call(M=4, temperature=1.0, seeds=Q, cons=Q, ldcons=8, logp=P, ldlogp=8, offsets=offs, nc=1, ldl=40, rows=40 * 16 + 1):
        return f(P, ldl, offsets, nc, M, temperature, 0, 1.0, None, seeds, cons, ldcons, logp, ldlogp, None, P, 8, 8, Q, rows, 32,
                 16, P, 32, None, 0, P, None)
    for kw in (dict(M=65), dict(M=0), dict(seeds=None), dict(temperature=0.0), dict(ldcons=7), dict(ldlogp=7), dict(ldl=39),
               dict(rows=40 * 16 - 1), dict(offsets=(ctypes.c_int32 * 3)(0, 40, 297), nc=2, ldl=297, rows=257 * 16 + 1)):
        assert call(**kw) == -1, kw
        assert b'decode_sample_constrained' in lib.vqcpc_last_error(), (kw, lib.vqcpc_last_error())
