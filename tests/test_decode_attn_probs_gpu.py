"""vqcpc_decode_attn_probs (csrc/decode.hip) by direct calls: vqcpc_decode_attn's kernel body with a compile-time flag, which
also writes the row of attention probabilities it multiplies V by.  Conventions of tests/test_decode_kernels_gpu.py (guard
rows, sentinel / NaN fills, fixed seeds), whose helpers are imported; the float64 reference is
decode_reference.attn_ref(..., return_weights=True).

Exact: ctx (and, in self mode, both caches) bit-identical to vqcpc_decode_attn on the same inputs; masked keys and j > pos are
+0.0; nothing but [0, Lk) of the one row changes in a NaN-filled buffer with guard rows; dead launches change nothing.
Bounds: |sum_j p_j - 1| <= (Lk + 3) 2^-24 in float64 (one rounding per product p_j = e_j * inv, one for the reciprocal, at
most Lk - 1 in the kernel's own sum of the e_j, whatever its order), and the attention tests' statistic on the weights:
max |p - p64| / rms(p64) <= C_ATTN x the same figure of the plain fp32 evaluation (each case prints `PROBS ...: ratio`).

Shapes.  Self mode: every hd x Lk, and at each every (M, H, ldp) of {1, 3} x {1, 3} x {Lk, Lk + 3}; the reference is computed
once per (hd, Lk) at M = H = 3 and sliced (rows and heads are independent).  Cross mode: every hd x ratio x mask, each at two
of the six Lk so that every (hd, ratio) meets every Lk and every mask meets every Lk; (M, H, ldp) cycle with the case and are
reduced while M * H * ratio * Lk^2 > 2^24, because attn_ref holds float64 arrays of that many elements (134 MB)."""
import pytest
import torch

import decode_reference as R
from test_decode_kernels_gpu import C_ATTN, GR, NAN, Buf, _attn_data, call, gen, same_bits

pytestmark = pytest.mark.gpu

HDS = [16, 32, 64, 128]
LKS = [1, 3, 255, 256, 257, 1024]
U24 = 2.0 ** -24


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


class ProbsBuf:
    """probs [M][H][rows][ldp] inside a NaN-filled allocation with GR guard rows of ldp floats on both sides."""

    def __init__(self, M, H, rows, ldp):
        self.shape = (M, H, rows, ldp)
        self.full = torch.full((2 * GR + M * H * rows, ldp), NAN, device='cuda')
        self.arg = self.full[GR:]
        self.before = self.full.clone()

    def view(self):
        M, H, rows, ldp = self.shape
        return self.full[GR:GR + M * H * rows].view(M, H, rows, ldp)

    def only_row(self, r, Lk):
        """Everything outside columns [0, Lk) of row r of every (b, h) has its bits unchanged -> those rows (M, H, Lk), host."""
        exp = self.before.clone()
        M, H, rows, ldp = self.shape
        ev = exp[GR:GR + M * H * rows].view(M, H, rows, ldp)
        ev[:, :, r, :Lk] = self.view()[:, :, r, :Lk]
        assert same_bits(exp, self.full)
        return self.view()[:, :, r, :Lk].cpu()

    def untouched(self):
        assert same_bits(self.before, self.full)


def _slice(q, k, v, e1, e2, M, H, Lk):
    """The first M sequences and H heads of data drawn at (3, ., 3, .)"""
    H0, hd = q.shape[2], q.shape[3]
    cut = lambda e: e.view(H0, Lk, hd)[:H].reshape(H * Lk, hd).contiguous()
    return q[:M, :, :H].contiguous(), k[:M, :, :H].contiguous(), v[:M, :, :H].contiguous(), cut(e1), cut(e2)


def _attn(entry, q, ldq, kdat, vdat, knew, vnew, ldn, e1d, e2d, pos, M, Lk, ratio, H, hd, mask, extra=()):
    d = H * hd
    kc, vc, ctx = Buf(M * Lk, d, d + 4, kdat), Buf(M * Lk, d, d + 4, vdat), Buf(M, d, d + 3)
    posd = torch.tensor([pos], dtype=torch.int32, device='cuda')
    call(entry, q, ldq, kc.view, vc.view, d + 4, knew, vnew, ldn, e1d, e2d, ctx.view, d + 3, posd, M, Lk, ratio, H, hd, mask, *extra)
    torch.cuda.synchronize()
    assert int(posd.item()) == pos
    return ctx, kc, vc


def _both(self_mode, q, k, v, e1d, e2d, pos, ratio, mask, M, H, hd, Lk, ldp, rows=None, win=None, stride=0):
    """The plain entry and the probs entry on the same inputs -> (ProbsBuf, ctx Buf of the probs entry); asserts that ctx and
    both caches have the plain entry's bits, guards included."""
    d = H * hd
    live = 0 <= pos < ratio * Lk
    p = pos // ratio
    kdat, vdat = k.reshape(M, Lk, d).clone(), v.reshape(M, Lk, d).clone()
    if self_mode:                                             # cache rows >= pos are NaN, the step's k / v row is row pos
        qkv = torch.randn(M, 3 * d, generator=gen(pos + 17))
        qkv[:, :d] = q.reshape(M, d)
        if live:
            qkv[:, d:2 * d], qkv[:, 2 * d:] = k[:, pos].reshape(M, d), v[:, pos].reshape(M, d)
        cut = min(max(pos, 0), Lk)
        kdat[:, cut:], vdat[:, cut:] = NAN, NAN
        qd = qkv.cuda()
        a = (qd[:, :d], 3 * d, kdat, vdat, qd[:, d:2 * d], qd[:, 2 * d:], 3 * d)
    else:                                                     # the memory rows the mask rules out are NaN
        if live and mask == 1:
            kdat[:, p + 1:], vdat[:, p + 1:] = NAN, NAN
        if live and mask == 2:
            kdat[:, :p], vdat[:, :p] = NAN, NAN
        qd = torch.full((M, d + 8), NAN)
        qd[:, :d] = q.reshape(M, d)
        a = (qd.cuda(), d + 8, kdat, vdat, None, None, 0)
    tail = (e1d, e2d, pos, M, Lk, ratio, H, hd, mask)
    plain = _attn('vqcpc_decode_attn', *a, *tail)
    pb = ProbsBuf(M, H, Lk * ratio if rows is None else rows, ldp)
    got = _attn('vqcpc_decode_attn_probs', *a, *tail, extra=(pb.arg, ldp, pb.shape[2], win, stride))
    for x, y in zip(plain, got):
        assert same_bits(x.full, y.full)
    if not live:
        got[0].assert_untouched(), got[1].assert_untouched(), got[2].assert_untouched()
    return pb, got[0]


def _check_rows(label, rows_got, w64, w32, keep, Lk):
    """rows_got (M, H, R, Lk) fp32 against the float64 weights; keep (R, Lk) bool: the keys the mask admits."""
    assert not bool(torch.isnan(rows_got).any()), label
    bits = rows_got.contiguous().view(torch.int32)
    assert bool((bits[:, :, ~keep] == 0).all()), label                 # +0.0, bit-exactly
    assert bool((rows_got[:, :, keep] >= 0).all()), label
    s = float((rows_got.double().sum(-1) - 1.0).abs().max())
    assert s <= (Lk + 3) * U24, (label, s, (Lk + 3) * U24)
    rms = float(w64.pow(2).mean().sqrt())
    ek = float((rows_got.double() - w64).abs().max()) / rms
    ep = float((w32.double() - w64).abs().max()) / rms
    ratio_ = ek / ep if ep > 0 else (0.0 if ek == 0 else float('inf'))
    print(f'PROBS {label}: kernel {ek:.3e} plain {ep:.3e} ratio {ratio_:.2f} |sum - 1| {s:.2e}')
    assert ek <= C_ATTN * ep, (label, ek, ep)


@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('Lk', LKS)
def test_self_mode(hd, Lk):
    i = HDS.index(hd) * len(LKS) + LKS.index(Lk)
    data = _attn_data(gen(7000 + i), 3, 3, hd, Lk)
    poss = sorted({0, min(1, Lk - 1), Lk // 2, Lk - 1})
    q, kt, vt, e1, e2 = data
    _, w64 = R.attn_ref(q.expand(3, len(poss), 3, hd), kt, vt, e1, e2, Lk, 1, 1, poss, return_weights=True)
    _, w32 = R.attn_ref(q.expand(3, len(poss), 3, hd), kt, vt, e1, e2, Lk, 1, 1, poss, dtype=torch.float32, return_weights=True)
    keep = torch.arange(Lk).view(1, Lk) <= torch.tensor(poss).view(-1, 1)
    for M in (1, 3):
        for H in (1, 3):
            qs, ks, vs, e1s, e2s = _slice(*data, M, H, Lk)
            e1d, e2d = e1s.cuda(), e2s.cuda()
            for ldp in (Lk, Lk + 3):
                rows = []
                for pos in poss:
                    pb, _ = _both(True, qs, ks, vs, e1d, e2d, pos, 1, 1, M, H, hd, Lk, ldp)
                    rows.append(pb.only_row(pos, Lk))
                _check_rows(f'self hd{hd} Lk{Lk} M{M} H{H} ldp{ldp} pos{poss}', torch.stack(rows, dim=2), w64[:M, :H], w32[:M, :H],
                            keep, Lk)
            for pos in (-1, Lk):                                        # dead launches change nothing
                pb, _ = _both(True, qs, ks, vs, e1d, e2d, pos, 1, 1, M, H, hd, Lk, Lk + 3)
                pb.untouched()


def _cross_lks(a, b, mask):
    """The two Lk of case (hd index a, ratio index b, mask): x and x + 3 of the six, x = a + b + mask."""
    x = (a + b + mask) % 6
    return LKS[x], LKS[(x + 3) % 6]


def _cross_shape(i, k, Lk, ratio):
    M, H = [(3, 3), (1, 3), (3, 1), (1, 1)][(i + k) % 4]
    while M * H * ratio * Lk * Lk > 1 << 24 and M > 1:
        M = 1
    while M * H * ratio * Lk * Lk > 1 << 24 and H > 1:
        H = 1
    return M, H, Lk + 3 * ((i // 4 + k) % 2)


def test_the_cross_grid_keeps_every_size():
    seen = {}
    for a in range(4):
        for b, ratio in enumerate((1, 4, 16)):
            for mask in range(3):
                i = (a * 3 + b) * 3 + mask
                for k, Lk in enumerate(_cross_lks(a, b, mask)):
                    M, H, ldp = _cross_shape(i, k, Lk, ratio)
                    seen.setdefault(('hd-ratio', a, ratio), set()).add(Lk)
                    seen.setdefault(('mask', mask), set()).add(Lk)
                    seen.setdefault('M', set()).add(M), seen.setdefault('H', set()).add(H)
                    seen.setdefault('pad', set()).add(ldp - Lk)
    assert all(v == set(LKS) for key, v in seen.items() if isinstance(key, tuple))
    assert seen['M'] == {1, 3} and seen['H'] == {1, 3} and seen['pad'] == {0, 3}


@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('ratio', [1, 4, 16])
@pytest.mark.parametrize('mask', [0, 1, 2])
def test_cross_mode(hd, ratio, mask):
    i = (HDS.index(hd) * 3 + (1, 4, 16).index(ratio)) * 3 + mask
    for k, Lk in enumerate(_cross_lks(HDS.index(hd), (1, 4, 16).index(ratio), mask)):
        M, H, ldp = _cross_shape(i, k, Lk, ratio)
        q, km, vm, e1, e2 = _attn_data(gen(8000 + i + Lk), M, H, hd, Lk)
        e1d, e2d = e1.cuda(), e2.cuda()
        poss = sorted({0, ratio - 1, min(ratio, ratio * Lk - 1), ratio * (Lk - 1), ratio * Lk - 1})
        qe = q.expand(M, len(poss), H, hd)
        _, w64 = R.attn_ref(qe, km, vm, e1, e2, Lk, ratio, mask, poss, return_weights=True)
        _, w32 = R.attn_ref(qe, km, vm, e1, e2, Lk, ratio, mask, poss, dtype=torch.float32, return_weights=True)
        p = (torch.tensor(poss) // ratio).view(-1, 1)
        j = torch.arange(Lk).view(1, Lk)
        keep = torch.ones(len(poss), Lk, dtype=torch.bool) if mask == 0 else (j <= p if mask == 1 else j >= p)
        rows = []
        for pos in poss:
            pb, _ = _both(False, q, km, vm, e1d, e2d, pos, ratio, mask, M, H, hd, Lk, ldp)
            rows.append(pb.only_row(pos, Lk))
        _check_rows(f'cross hd{hd} Lk{Lk} ratio{ratio} mask{mask} M{M} H{H} ldp{ldp} pos{poss}', torch.stack(rows, dim=2), w64, w32,
                    keep, Lk)
        for pos in (-1, ratio * Lk):
            pb, _ = _both(False, q, km, vm, e1d, e2d, pos, ratio, mask, M, H, hd, Lk, ldp)
            pb.untouched()


@pytest.mark.parametrize('self_mode', [True, False])
def test_window_rows_and_repeats(self_mode):
    """win = {., w}, win_stride = U: the row is w * U + pos; a row at or past `rows`, or no live window (w < 0), writes no
    probability and leaves ctx the plain entry's; the row does not depend on where it is written; calls repeat bit for bit."""
    M, H, hd, Lk, U = 3, 3, 32, 257, 16
    ratio, mask = (1, 1) if self_mode else (4, 2)
    pos = 100
    q, k, v, e1, e2 = _attn_data(gen(9000 + self_mode), M, H, hd, Lk)
    e1d, e2d = e1.cuda(), e2.cuda()
    run = lambda **kw: _both(self_mode, q, k, v, e1d, e2d, pos, ratio, mask, M, H, hd, Lk, Lk + 3, **kw)
    pb0, ctx0 = run()
    base = pb0.only_row(pos, Lk)
    pb1, ctx1 = run()
    assert same_bits(base, pb1.only_row(pos, Lk)) and same_bits(ctx0.full, ctx1.full)
    for w in (0, 3, 7):
        win = torch.tensor([w + 1, w], dtype=torch.int32, device='cuda')
        pb, _ = run(rows=7 * U + pos + 1, win=win, stride=U)
        assert same_bits(base, pb.only_row(w * U + pos, Lk)), w
    win = torch.tensor([8, 7], dtype=torch.int32, device='cuda')
    for rows in (7 * U + pos, 1):                                        # r >= rows (the last row is r - 1)
        pb, ctx = run(rows=rows, win=win, stride=U)
        pb.untouched()
        assert same_bits(ctx.full, ctx0.full)
    pb, ctx = run(rows=pos, win=None)                                    # win == NULL: r = pos == rows
    pb.untouched()
    assert same_bits(ctx.full, ctx0.full)
    win = torch.tensor([0, -1], dtype=torch.int32, device='cuda')        # no live window, as the constrained sampler's column
    pb, ctx = run(rows=2 * Lk * ratio, win=win, stride=U)
    pb.untouched()
    assert same_bits(ctx.full, ctx0.full)
