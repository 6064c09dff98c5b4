"""Anchors tests/attention_reference.py (the float64 reference of csrc/relattn_x.hip) before any GPU is involved: the oracle's
closed form and masks, the reference project's recorded outputs under tests/golden/, torch float64 autograd of its own forward,
and the structural zeros of the relative tables' gradients.  CPU only.

The last test is the host-only refusal test of the alignment requirements of vqcpc_relattn_x_fwd / _bwd: it must run where
there is NO GPU (dummy addresses), so it cannot live in the gpu-marked tests/test_relattn_x_kernels_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import attention_reference as A
from conftest import load_golden, rel_err
from oracle import decoder_oracle as D

T = torch.from_numpy
TOL = 1e-6            # the fixtures are fp32: the bound tests/test_decoder_oracle_golden.py uses for the relative term
F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def data(n, H, Lq, Lk, hd, seed):
    g = gen(seed)
    d = H * hd
    return dict(q=torch.randn(n * Lq, d, generator=g, dtype=F64), k=torch.randn(n * Lk, d, generator=g, dtype=F64),
                v=torch.randn(n * Lk, d, generator=g, dtype=F64), e1=torch.randn(H * Lk, hd, generator=g, dtype=F64) * 0.5,
                e2=torch.randn(H * Lk, hd, generator=g, dtype=F64) * 0.5, go=torch.randn(n * Lq, d, generator=g, dtype=F64))


@pytest.mark.parametrize('Lq,Lk', [(1, 1), (2, 2), (7, 7), (48, 3), (12, 6), (80, 40), (33, 33)])
def test_bias_and_masks_are_the_oracles(Lq, Lk):
    n, H, hd = 2, 3, 8
    g = gen(Lq + Lk)
    qs = torch.randn(n, H, Lq, hd, generator=g, dtype=F64)
    e1, e2 = torch.randn(H * Lk, hd, generator=g, dtype=F64), torch.randn(H * Lk, hd, generator=g, dtype=F64)
    got, want = A.rel_bias(qs, e1, e2, Lk), D.relative_bias_cross(qs, e1, e2, Lk)
    assert got.dtype == F64 and float((got - want).abs().max()) < 1e-13
    assert A.rel_bias(qs, e1, e2, Lk, dtype=torch.float32).dtype == torch.float32
    for mask in (1, 2):
        assert torch.equal(A.keep_rule(mask, Lq, Lk), D.additive_mask(mask, Lk, Lq) == 0)
    assert bool(A.keep_rule(0, Lq, Lk).all()) and D.additive_mask(0, Lk, Lq) is None
    # every row keeps at least one key under every mask (the softmax never meets an empty row)
    assert all(bool(A.keep_rule(m, Lq, Lk).any(1).all()) for m in (0, 1, 2))


@pytest.mark.parametrize('name', ['relbias_cross_S3_T48', 'relbias_cross_S6_T12', 'relbias_cross_S40_T80', 'relbias_L24'])
def test_bias_reproduces_the_recorded_relative_term(name):
    g = load_golden(name)
    q = T(g['q'])
    H = int(g['H'])
    S = int(g['S']) if 'S' in g else q.shape[1]
    n = q.shape[0] // H
    got = A.rel_bias(q.view(n, H, q.shape[1], q.shape[2]), g['e1'], g['e2'], S).reshape(g['bias'].shape)
    assert got.dtype == F64 and rel_err(got, g['bias']) < TOL


@pytest.mark.parametrize('name,mask', [('mha_self_causal_T24', 1), ('mha_cross_anticausal_S6_T12', 2)])
def test_forward_and_backward_reproduce_the_recorded_attention_module(name, mask):
    """in_proj and out_proj restated in float64 around attn_fwd / attn_bwd: the module's output, its per-head weights, and the
    gradients of its inputs, of in_proj and of the relative tables."""
    g = load_golden(name)
    H, S, Tq = int(g['H']), int(g['S']), int(g['T'])
    xq = T(g['q']).double().transpose(0, 1)                                  # fixtures are time-first
    xkv = T(g['mem']).double().transpose(0, 1) if 'mem' in g else xq
    n, _, d = xq.shape
    W, b = T(g['sd/in_proj_weight']).double(), T(g['sd/in_proj_bias']).double()
    Wo, bo = T(g['sd/out_proj.weight']).double(), T(g['sd/out_proj.bias']).double()
    assert np.array_equal(np.isfinite(g['attn_mask']), A.keep_rule(mask, Tq, S).numpy())
    xq2, xkv2 = xq.reshape(n * Tq, d), xkv.reshape(n * S, d)
    q = xq2 @ W[:d].t() + b[:d]
    k, v = (xkv2 @ W[d:].t() + b[d:]).split(d, dim=-1)
    e1, e2 = g['sd/attn_bias.e1'], g['sd/attn_bias.e2']
    ctx, probs = A.attn_fwd(q, k, v, e1, e2, n, Tq, S, H, mask)
    out = ctx @ Wo.t() + bo
    assert rel_err(probs, g['weights']) < TOL
    assert rel_err(out.reshape(n, Tq, d).transpose(0, 1), g['out']) < TOL
    d_ctx = T(g['g']).double().transpose(0, 1).reshape(n * Tq, d) @ Wo
    dq, dk, dv, de1, de2, _, _ = A.attn_bwd(d_ctx, q, k, v, probs, e1, e2, n, Tq, S, H, mask)
    assert rel_err(de1, g['grad/attn_bias.e1']) < 10 * TOL
    if float(np.abs(g['grad/attn_bias.e2']).max()) == 0.0:
        assert float(de2.abs().max()) == 0.0
    else:
        assert rel_err(de2, g['grad/attn_bias.e2']) < 10 * TOL
    dkv = torch.cat([dk, dv], dim=1)
    dW = torch.cat([dq.t() @ xq2, dkv.t() @ xkv2])
    assert rel_err(dW, g['grad/in_proj_weight']) < 10 * TOL
    dxq, dxkv = dq @ W[:d], dkv @ W[d:]
    if 'mem' in g:
        assert rel_err(dxq.reshape(n, Tq, d).transpose(0, 1), g['d_q']) < 10 * TOL
        assert rel_err(dxkv.reshape(n, S, d).transpose(0, 1), g['d_mem']) < 10 * TOL
    else:
        assert rel_err((dxq + dxkv).reshape(n, Tq, d).transpose(0, 1), g['d_q']) < 10 * TOL


@pytest.mark.parametrize('mask', [0, 1, 2])
@pytest.mark.parametrize('r', [1, 4])
@pytest.mark.parametrize('p', [0.0, 0.25])
def test_explicit_backward_is_autograd_of_the_forward(mask, r, p):
    n, H, Lk, hd = 2, 3, 7, 8
    Lq = r * Lk
    Dt = data(n, H, Lq, Lk, hd, 10 * mask + r)
    scale = A.keep_scale(0x5EED0001, n, H, Lq, Lk, p)
    if p:
        assert scale.shape == (n, H, Lq, Lk) and 0.1 < float((scale == 0).double().mean()) < 0.4
        assert set(scale.unique().tolist()) == {0.0, float(np.float32(1.0) / np.float32(0.75))}
    leaves = {key: Dt[key].clone().requires_grad_(True) for key in ('q', 'k', 'v', 'e1', 'e2')}
    ctx, probs = A.attn_fwd(leaves['q'], leaves['k'], leaves['v'], leaves['e1'], leaves['e2'], n, Lq, Lk, H, mask, scale)
    (ctx * Dt['go']).sum().backward()
    assert float((probs.detach().sum(-1) - 1).abs().max()) < 1e-14
    assert bool((probs.detach()[:, :, ~A.keep_rule(mask, Lq, Lk)] == 0).all())
    got = A.attn_bwd(Dt['go'], Dt['q'], Dt['k'], Dt['v'], probs.detach(), Dt['e1'], Dt['e2'], n, Lq, Lk, H, mask, scale)
    for name, a in zip(('q', 'k', 'v', 'e1', 'e2'), got[:5]):
        w = leaves[name].grad
        assert a.dtype == F64 and a.shape == w.shape
        assert float((a - w).abs().max()) <= 1e-13 * max(1.0, float(w.abs().max())), name
    # the norms of the summands bound the sums, and vanish exactly where the sums are structurally zero
    for a, nn in ((got[3], got[5]), (got[4], got[6])):
        assert bool((a.abs() <= nn * np.sqrt(n * Lq) * (1 + 1e-12) + 1e-300).all())
        assert bool((a[nn == 0] == 0).all())
    # fp32 evaluation of the same formulas: an fp32-accurate copy
    c32, p32 = A.attn_fwd(Dt['q'], Dt['k'], Dt['v'], Dt['e1'], Dt['e2'], n, Lq, Lk, H, mask, scale, dtype=torch.float32)
    assert c32.dtype == p32.dtype == torch.float32 and 0.0 < rel_err(c32, ctx.detach()) < 1e-5
    b32 = A.attn_bwd(Dt['go'], Dt['q'], Dt['k'], Dt['v'], probs.detach(), Dt['e1'], Dt['e2'], n, Lq, Lk, H, mask, scale,
                     dtype=torch.float32)
    assert all(t.dtype == torch.float32 for t in b32[:5]) and 0.0 < rel_err(b32[0], got[0]) < 1e-5


@pytest.mark.parametrize('r', [1, 4])
@pytest.mark.parametrize('Lk', [1, 2, 5])
def test_structural_zeros_are_exact(r, Lk):
    n, H, hd = 2, 2, 4
    Lq = r * Lk
    Dt = data(n, H, Lq, Lk, hd, 77 + Lk)
    for mask in (0, 1, 2):
        _, probs = A.attn_fwd(Dt['q'], Dt['k'], Dt['v'], Dt['e1'], Dt['e2'], n, Lq, Lk, H, mask)
        # masked entries of the INPUT probs are never read: poison them
        poisoned = torch.where(A.keep_rule(mask, Lq, Lk), probs, torch.full_like(probs, float('nan')))
        out = A.attn_bwd(Dt['go'], Dt['q'], Dt['k'], Dt['v'], poisoned, Dt['e1'], Dt['e2'], n, Lq, Lk, H, mask)
        assert all(bool(torch.isfinite(t).all()) for t in out)
        d_e1, d_e2, n1, n2 = (t.view(H, Lk, hd) for t in out[3:])
        assert bool((d_e2[:, 0] == 0).all()) and bool((n2[:, 0] == 0).all())          # e2 row 0 is never read
        if mask == 1:
            assert bool((d_e2 == 0).all()) and bool((n2 == 0).all())                  # causal: j <= p never meets e2
        if mask == 2:
            assert bool((d_e1[:, :Lk - 1] == 0).all()) and bool((n1[:, :Lk - 1] == 0).all())   # anticausal: of e1 only row Lk - 1
        if mask == 0 and Lk > 1:
            assert bool((n1 > 0).all()) and bool((n2[:, 1:] > 0).all())
    # de_err: zero scale -> 0 for an exact zero, inf otherwise
    e = A.de_err(torch.tensor([0.0, 1e-30, 1.0]), torch.tensor([0.0, 0.0, 0.5]), torch.tensor([0.0, 0.0, 2.0]))
    assert e.tolist() == [0.0, float('inf'), 0.25]


def test_misaligned_relative_tables_are_refused_before_any_launch():
    """vqcpc_relattn_x_fwd loads e1 / e2 rows as float4 (xload_row on xerel_row); the tables must be 16-byte aligned, and the
    backward asks the same of the tables it is given.  Dummy addresses, never dereferenced: host-only, as
    test_gemm_forms.py::test_p4_a_operand_with_a_form_that_has_no_instantiation_is_refused."""
    if torch.cuda.is_available():
        pytest.skip('host-only: a missing refusal must not become a launch on dummy addresses')
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    lib = hip.load()
    q, k, v, e1, e2, ctx, probs, dq, dk, dv, de1, de2, ws, dctx = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(14)]
    n, Lq, Lk, H, hd = 1, 8, 8, 1, 16
    d = H * hd
    wsb = lib.vqcpc_relattn_x_bwd_workspace(n, Lq, Lk, H, hd)
    for bad1, bad2 in ((4, 0), (0, 8), (12, 12)):
        e1b, e2b = ctypes.c_void_p(e1.value + bad1), ctypes.c_void_p(e2.value + bad2)
        rc = lib.vqcpc_relattn_x_fwd(q, d, k, d, v, d, e1b, e2b, ctx, d, probs, n, Lq, Lk, H, hd, 0, 0.0, 0, None)
        assert rc != 0 and b'relattn_x_fwd: e1 / e2 must be 16-byte aligned' in lib.vqcpc_last_error(), (rc, lib.vqcpc_last_error())
        rc = lib.vqcpc_relattn_x_bwd(dctx, d, q, d, k, d, v, d, probs, e1b, e2b, dq, d, dk, d, dv, d, de1, de2, n, Lq, Lk, H, hd, 0,
                                     0.0, 0, ws, wsb, None)
        assert rc != 0 and b'relattn_x_bwd: e1 / e2 must be 16-byte aligned' in lib.vqcpc_last_error(), (rc, lib.vqcpc_last_error())
