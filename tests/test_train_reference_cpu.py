"""tests/train_reference.py against independent statements of the same operations, on the CPU: torch float64 autograd on the
library formula (F.layer_norm, F.selu, nn.GRU, log_softmax, torch.optim.Adam + clip_grad_norm_) within 1e-12, and the matching
function of oracle/ where one exists.  A reference that is wrong here would make the GPU tests of test_train_kernels_gpu.py
compare the kernels with the wrong thing."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decode_reference as DR
import train_reference as T
from oracle import student_oracle as SO
from oracle import vqcpc_oracle as O

TOL = 1e-12
F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def close(a, b, tol=TOL):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * scale, (err, scale)


@pytest.mark.parametrize('M,d,with_r', [(1, 4, False), (5, 36, True), (3, 260, True)])
def test_layernorm_reference(M, d, with_r):
    g = gen(M * 1000 + d)
    x = torch.randn(M, d, generator=g, dtype=F64).requires_grad_()
    r = torch.randn(M, d, generator=g, dtype=F64).requires_grad_() if with_r else None
    scale = T.dropout_scale(0x1234567800000005, (M, d), 0.25) if with_r else None
    gamma = torch.randn(d, generator=g, dtype=F64).requires_grad_()
    beta = torch.randn(d, generator=g, dtype=F64).requires_grad_()
    dy = torch.randn(M, d, generator=g, dtype=F64)
    eps = 1e-5
    y, mean, rstd, s = T.ln_fwd(x, r, scale, gamma, beta, eps)
    s_t = x + r * scale if with_r else x
    y_t = F.layer_norm(s_t, (d,), gamma, beta, eps)
    close(y, y_t)
    close(y, O.layer_norm(s_t, gamma, beta, eps))
    close(mean, s_t.mean(-1))
    close(rstd, 1 / torch.sqrt(s_t.var(-1, unbiased=False) + eps))
    grads = torch.autograd.grad(y_t, [x, gamma, beta] + ([r] if with_r else []), dy)
    d_s, d_r, d_gamma, d_beta = T.ln_bwd(dy, s.detach(), gamma.detach(), mean.detach(), rstd.detach(), scale)
    close(d_s, grads[0])
    close(d_gamma, grads[1])
    close(d_beta, grads[2])
    if with_r:
        close(d_r, grads[3])
        assert float((scale == 0).double().mean()) > 0.05           # the mask drops something
    else:
        close(d_r, d_s)


def test_selu_reference():
    x = torch.cat([torch.logspace(-7, math.log10(30), 200, dtype=F64), -torch.logspace(-7, math.log10(30), 200, dtype=F64),
                   torch.tensor([0.0, -0.0], dtype=F64)]).requires_grad_()
    y = T.selu(x)
    # F.selu and the oracle use exp(x) - 1: absolute agreement only (that form is what loses accuracy near 0-)
    close(y, F.selu(x), 1e-15 + 4e-16)
    close(y, O.selu(x.detach()), 1e-15 + 4e-16)
    (gx,) = torch.autograd.grad(F.selu(x), x, torch.ones_like(x))
    close(T.selu_grad(x.detach()), gx)
    # expm1: relative accuracy for small negative x, against the series x + x^2 / 2 + x^3 / 6
    xs = -torch.logspace(-7, -3, 50, dtype=F64)
    series = T.SELU_SCALE * T.SELU_ALPHA * (xs + xs ** 2 / 2 + xs ** 3 / 6 + xs ** 4 / 24)
    assert float(((T.selu(xs) - series).abs() / series.abs()).max()) < 1e-13
    assert float(T.selu(torch.tensor([0.0]))[0]) == 0.0 and float(T.selu(torch.tensor([-0.0]))[0]) == 0.0
    h = torch.randn(300, generator=gen(3), dtype=F64).requires_grad_()
    scale = T.dropout_scale(77, (300,), 0.25)
    g = torch.randn(300, generator=gen(4), dtype=F64)
    (gh,) = torch.autograd.grad(F.selu(h * scale), h, g)
    close(T.dropout_selu_bwd(h.detach(), g, scale), gh)
    close(T.dropout_selu_fwd(h.detach(), scale), F.selu(h * scale).detach(), 1e-15 + 4e-16)


@pytest.mark.parametrize('B,H', [(1, 1), (5, 3), (4, 64)])
def test_gru_reference_against_nn_gru(B, H):
    g = gen(B * 100 + H)
    I = 7
    gru = torch.nn.GRU(I, H, batch_first=True).double()
    x = torch.randn(B, 1, I, generator=g, dtype=F64)
    h0 = torch.randn(1, B, H, generator=g, dtype=F64).requires_grad_()
    w_ih, w_hh, b_ih, b_hh = (p.detach() for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0))
    gi = (x[:, 0] @ w_ih.t() + b_ih).requires_grad_()
    out, _ = gru(x, h0)
    gh, h, y = T.gru_step_fwd(gi.detach(), w_hh, b_hh, h0[0].detach())
    close(h, out[:, 0])
    close(y, h)
    gh0, h_zero, _ = T.gru_step_fwd(gi.detach(), w_hh, b_hh, None)
    out0, _ = gru(x)
    close(h_zero, out0[:, 0])
    close(gh0, b_hh.expand(B, -1))
    # the cell, and its backward against autograd through the same formula
    scale = T.dropout_scale(5, (B, H), 0.3, idx_base=1000)
    ghr = gh.clone().requires_grad_()
    h_t, y_t = T.gru_cell_fwd(gi, ghr, h0[0], scale)
    d_y = torch.randn(B, H, generator=g, dtype=F64)
    d_h = torch.randn(B, H, generator=g, dtype=F64)
    a_gi, a_gh, a_h0 = torch.autograd.grad([y_t, h_t], [gi, ghr, h0], [d_y, d_h])
    d_gi, d_gh, d_hp = T.gru_cell_bwd(gi.detach(), gh, h0[0].detach(), d_y, d_h, scale)
    close(d_gi, a_gi)
    close(d_gh, a_gh)
    close(d_hp, a_h0[0])
    # the fused backward step: dh arrives as dgh_next . W_hh + dhp
    dgh_next = torch.randn(B, 3 * H, generator=g, dtype=F64)
    dhp = torch.randn(B, H, generator=g, dtype=F64)
    s_gi, s_gh, s_hp = T.gru_step_bwd(dgh_next, w_hh.t().contiguous(), dhp, gi.detach(), gh, h0[0].detach(), d_y, scale)
    c_gi, c_gh, c_hp = T.gru_cell_bwd(gi.detach(), gh, h0[0].detach(), d_y, dgh_next @ w_hh + dhp, scale)
    close(s_gi, c_gi)
    close(s_gh, c_gh)
    close(s_hp, c_hp)
    # the oracle's recurrence (one layer, one step, h0 = 0)
    P = {'c.g_ar_fwd.weight_ih_l0': w_ih, 'c.g_ar_fwd.weight_hh_l0': w_hh, 'c.g_ar_fwd.bias_ih_l0': b_ih,
         'c.g_ar_fwd.bias_hh_l0': b_hh, 'c.output_linear.weight': torch.eye(H, dtype=F64), 'c.output_linear.bias': torch.zeros(H, dtype=F64)}
    close(h_zero, O.gru_context(x, P, 'c.', 1))


@pytest.mark.parametrize('B,K,N,zdim,cdim', [(1, 1, 1, 1, 1), (3, 5, 7, 6, 10)])
def test_nce_reference(B, K, N, zdim, cdim):
    g = gen(B + K + N)
    c = torch.randn(B, cdim, generator=g, dtype=F64).requires_grad_()
    W = torch.randn(zdim, cdim, K, generator=g, dtype=F64).requires_grad_()
    zp = torch.randn(B, K, zdim, generator=g, dtype=F64).requires_grad_()
    zn = torch.randn(B, N, K, zdim, generator=g, dtype=F64).requires_grad_()
    gb = torch.randn(B, generator=g, dtype=F64)
    f_pos, f_neg, loss_b, hits = T.nce_fwd(c, W, zp, zn)
    o_pos, o_neg = O.fks_scores(c, W, zp, zn)
    close(f_pos, o_pos)
    close(f_neg, o_neg)
    close(loss_b.mean(), O.nce_loss(o_pos, o_neg))
    lse = torch.logsumexp(torch.cat([o_neg, o_pos.unsqueeze(2)], 2), 2)
    close(loss_b, -(o_pos - lse).sum(1))
    assert torch.equal(hits.bool(), o_pos > o_neg.max(2)[0])
    grads = torch.autograd.grad(-(o_pos - lse).sum(1), [c, W, zp, zn], gb)
    mine = T.nce_bwd(c.detach(), W.detach(), zp.detach(), zn.detach(), f_pos.detach(), f_neg.detach(), gb)
    for a, b in zip(mine, grads):
        close(a, b)


def test_nce_reference_tie_is_no_hit():
    f_pos, f_neg, _, hits = T.nce_fwd(torch.ones(1, 1), torch.ones(1, 1, 1), torch.full((1, 1, 1), 2.0), torch.full((1, 3, 1, 1), 2.0))
    assert float(f_pos[0, 0]) == 2.0 and float(hits[0, 0]) == 0.0


@pytest.mark.parametrize('R,V', [(1, 1), (5, 63), (9, 130)])
def test_softmax_ce_reference(R, V):
    g = gen(R * 1000 + V)
    x = (torch.randn(R, V, generator=g, dtype=F64) * 3).requires_grad_()
    tgt = torch.randint(0, V, (R,), generator=g)
    loss, grad = T.softmax_ce(x, target=tgt)
    lp = torch.log_softmax(x, -1)
    close(loss, F.nll_loss(lp, tgt, reduction='none'))
    close(grad, torch.autograd.grad(F.nll_loss(lp, tgt, reduction='sum'), x)[0])
    tl = torch.randn(R, V, generator=g, dtype=F64) * 2
    loss_s, grad_s = T.softmax_ce(x, target_logits=tl)
    ref_s = -(torch.softmax(tl, -1) * torch.log_softmax(x, -1)).sum(-1)
    close(loss_s, ref_s)
    close(grad_s, torch.autograd.grad(ref_s.sum(), x)[0])
    assert float(grad_s.sum(-1).abs().max()) < 1e-14
    # the oracle's per-channel losses: one channel, every position selected
    mask = torch.ones(R, 1, 1)
    close(loss, SO.categorical_crossentropy([x.detach().view(R, 1, V)], tgt.view(R, 1, 1), mask))
    close(loss_s, SO.distilled_categorical_crossentropy([x.detach().view(R, 1, V)], [tl.view(R, 1, V)], mask))
    # shift invariance at large logits
    big, _ = T.softmax_ce(x.detach() + 1e4, target=tgt)
    close(big, loss.detach(), 1e-10)


@pytest.mark.parametrize('rows,f,d', [(1, 1, 4), (6, 8, 36)])
def test_upscale_reference(rows, f, d):
    g = gen(rows + f)
    x = torch.randn(rows, d, generator=g, dtype=F64).requires_grad_()
    emb = torch.randn(f, d, generator=g, dtype=F64).requires_grad_()
    out = T.upscale_fwd(x, emb)
    close(out, SO.upscale(x.view(1, rows, d), f, emb)[0])
    close(out, x.repeat_interleave(f, 0) + emb.repeat(rows, 1))
    go = torch.randn(rows * f, d, generator=g, dtype=F64)
    a_x, a_e = torch.autograd.grad(out, [x, emb], go)
    dx, de = T.upscale_bwd(go, f)
    close(dx, a_x)
    close(de, a_e)


@pytest.mark.parametrize('max_norm', [None, 5.0, 0.5])
def test_adam_reference_against_torch_optim(max_norm):
    g = gen(11)
    n, steps, lr, b1, b2, eps = 50, 6, 1e-3, 0.9, 0.999, 1e-8
    p0 = torch.randn(n, generator=g, dtype=F64)
    grads = [torch.randn(n, generator=g, dtype=F64) * (0.1 if t % 2 else 3.0) for t in range(steps)]
    prm = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([prm], lr=lr, betas=(b1, b2), eps=eps)
    for gt in grads:
        prm.grad = gt.clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([prm], max_norm)
        opt.step()
    p, m, v = T.adam_steps(p0, grads, lr, b1, b2, eps, max_norm)
    close(p, prm.detach())
    close(m, opt.state[prm]['exp_avg'])
    close(v, opt.state[prm]['exp_avg_sq'])
    # the oracle's clip + Adam (fp32 state): agreement at fp32 level only
    P = {'w': p0.float().clone()}
    st = {}
    for gt in grads:
        gg = [gt.float().clone()]
        if max_norm is not None:
            O.clip_grad_norm(gg, max_norm)
        O.adam_step(P, {'w': gg[0]}, st, lr, (b1, b2), eps)
    close(P['w'], p, 1e-5)


def test_adam_single_step_and_clip_coef():
    assert T.clip_coef(None, 5.0, 0.5) == 0.5
    assert T.clip_coef(4.0, 5.0) == 1.0                                  # norm 2 < 5
    assert abs(T.clip_coef(100.0, 5.0) - 5.0 / (10.0 + 1e-6)) < 1e-15
    assert abs(T.sumsq(torch.tensor([3.0, 4.0]), 0.5) - 6.25) < 1e-15
    p, g, m, v = T.adam_step(torch.ones(3), torch.full((3,), 2.0), torch.zeros(3), torch.zeros(3), 0.1, 0.9, 0.999, 1e-8, 1, 0.5)
    close(g, torch.ones(3))
    close(m, torch.full((3,), 0.1, dtype=F64))
    close(v, torch.full((3,), 0.001, dtype=F64))
    close(p, torch.full((3,), 1.0 - 0.1 / (1.0 + 1e-8), dtype=F64))               # the first step moves by lr * sign(g)


def test_bf16_rne_reference():
    g = gen(9)
    x = torch.cat([torch.randn(5000, generator=g), torch.randn(2000, generator=g) * 1e-30, torch.randn(2000, generator=g) * 1e30,
                   torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3.3895314e38, 1e-40, -1e-40])])
    # exact ties: a bf16 value plus half its spacing -> the even neighbour
    base = torch.randn(1000, generator=g).bfloat16().float()
    ties = (base.view(torch.int32) | 0x8000).view(torch.float32)
    x = torch.cat([x, ties])
    want = x.bfloat16().view(torch.int16).to(torch.int32) & 0xFFFF
    got = T.bf16_rne(x)
    assert torch.equal(got, want)
    assert torch.equal(T.bf16_to_f32(got), x.bfloat16().float())


def test_dropout_generator_keep_rate():
    """The numpy statement of the generator keeps 1 - p of the elements within 5 binomial standard deviations, for the seeds
    and probabilities the GPU test of vqcpc_dropout_mask uses; p = 0 keeps everything; the scale is 1 / (1 - p) in fp32."""
    n = 100000
    for seed in (0x9E3779B97F4A7C15, 0x0123456700000001, 0xFFFFFFFF00000000):
        for p in (0.0, 0.1, 0.5, 0.999):
            keep = T.dropout_keep(seed, n, p)
            if p == 0.0:
                assert keep.all()
                continue
            q = 1.0 - T.drop_threshold(p) / 2.0 ** 24
            assert abs(float(keep.mean()) - q) <= 5.0 * math.sqrt(q * (1.0 - q) / n), (seed, p, float(keep.mean()))
        assert not np.array_equal(T.dropout_keep(seed, 1000, 0.5), T.dropout_keep(seed ^ (1 << 40), 1000, 0.5))   # the high word matters
    # idx_base shifts the stream
    assert np.array_equal(T.dropout_keep(5, 100, 0.5, idx_base=40), T.dropout_keep(5, 140, 0.5)[40:])
    sc = T.dropout_scale(5, (10, 10), 0.25)
    assert set(sc.unique().tolist()) == {0.0, float(np.float32(1.0) / np.float32(0.75))}
    assert T.drop_threshold(0.25) == 1 << 22 and T.drop_threshold(0.0) == 0
    # and the generator is the one of decode_reference, not a second statement of it
    assert T.rng_u24_ref is DR.rng_u24_ref


def test_error_statistics():
    ref = torch.tensor([[3.0, 4.0], [0.0, 0.0], [0.0, 0.0], [1e-20, 1e-20]], dtype=F64)
    out = torch.tensor([[3.0, 4.5], [0.0, 0.0], [0.0, 1e-30], [1e-20, 2e-20]], dtype=F64)
    e = T.row_err(out, ref)
    assert abs(float(e[0]) - 0.5 / math.sqrt(12.5)) < 1e-15 and float(e[1]) == 0.0 and math.isinf(float(e[2]))
    assert abs(float(e[3]) - 1.0) < 1e-12                               # a small row is judged by its own size
    assert torch.allclose(T.row_err(torch.tensor([1.1, 2.0]), torch.tensor([1.0, 2.0], dtype=F64)),
                          torch.tensor([0.1, 0.0], dtype=F64), atol=1e-7)
    terms = torch.tensor([[1.0, 0.0], [-1.0, 0.0]], dtype=F64)
    c = T.col_err(torch.tensor([1e-3, 0.0]), terms.sum(0), terms)
    assert abs(float(c[0]) - 1e-3 / math.sqrt(2.0)) < 1e-9 and float(c[1]) == 0.0
