"""The training step's pointwise and row kernels (csrc/embed_ln.hip, util.hip, gru.hip, nce.hip, student.hip) one by one, by
direct calls, against the float64 references of tests/train_reference.py, at the shapes and edges the model-level tests
never reach.

Conventions of every test here:
  * outputs live in sentinel-filled allocations with guard elements on both sides; the guards must be bit-unchanged after the
    call; where the ABI has a stride the leading dimension exceeds the width;
  * every input the result must not depend on is NaN (the gaps of a strided x, r when the form has none, h_prev rows past
    B): a NaN in an output is a wrong read;
  * seeds are fixed.

Statistic.  Per row: max |out - out64| / rms(out64 of that row); per column of a column sum (d_gamma, d_beta):
|out - out64| / ||summands of that column||_2 (train_reference.row_err / col_err) -- never a tensor-wide maximum, so a wrong
element of a small row or of one ragged column counts in full.

Tolerances that are not derived (LayerNorm, GRU, InfoNCE, softmax-CE, SELU gradient: expf / tanhf / __expf and a summation
order of their own).  The yardstick is the SAME formula in plain fp32 torch on the CPU against the float64 reference: a group
of rows passes when max err(kernel) <= C * max err(plain fp32); where plain fp32 is exact (err = 0) the bound is 4 ulp of
each output, and outputs that are ALL within 4 ulp pass in any case (a group of one scalar has no statistics).  C = 4 for every family (`C_FAMILY`).  Every case prints `<FAMILY> <label>: kernel .. plain .. ratio ..`; the
measured medians and maxima and the cases above 2 are in profiles/train_kernel_tests_log.md.

Derived bounds: SELU forward (4 * 2^-24 relative), sum of squares (2^-23 relative), Adam (componentwise, `_adam_bounds`),
upscale backward (sequential fp32 sums).  Exact: dropout mask, token check, accumulate8, scale_rows, upscale forward, the
bf16 roundings and the bit identities include/vqcpc.h states for the bf16 LayerNorm forms.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import decode_reference as DR
import train_reference as T

pytestmark = pytest.mark.gpu

C_FAMILY = {'LN': 4.0, 'SELU': 4.0, 'GRU': 4.0, 'NCE': 4.0, 'CE': 4.0}
NAN = float('nan')
U = 2.0 ** -24
SENT_I32 = 0xDEADBEEF - (1 << 32)            # as fp32: -6.26e18, finite, never produced by these kernels
SENT = {torch.float32: (torch.int32, SENT_I32), torch.int16: (torch.int16, 0x5A5A), torch.int32: (torch.int32, 0x5A5A5A5A),
        torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A), torch.float64: (torch.int64, 0x5A5A5A5A5A5A5A5A)}
PAD = 256                                    # guard elements on each side
F32 = torch.float32
RATIOS = {}


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    yield hip
    for fam, rs in sorted(RATIOS.items()):
        r = sorted(x for _, x in rs if math.isfinite(x))
        if r:
            print(f'SUMMARY {fam}: {len(rs)} groups, median ratio {r[len(r) // 2]:.2f}, max {r[-1]:.2f}, C = {C_FAMILY[fam]:g}; above 2: '
                  + ', '.join(f'{lab} {x:.2f}' for lab, x in rs if x > 2.0))


def call(name, *args):
    from vqcpc_bach_amd import hip
    hip.call(name, *args)


def query(name, *args):
    from vqcpc_bach_amd import hip
    return hip.query(name, *args)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    t = t.contiguous()
    return t.view(SENT[t.dtype][0]) if t.dtype in (torch.float32, torch.float64) else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Guard:
    """A contiguous tensor of `shape` inside a sentinel-filled allocation with PAD guard elements before and after."""

    def __init__(self, shape, dtype=F32, data=None):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.n = int(np.prod(shape)) if shape else 1
        st, sv = SENT[dtype]
        self.full = torch.full((self.n + 2 * PAD,), sv, dtype=st, device='cuda').view(dtype)
        self.view = self.full[PAD:PAD + self.n].view(shape)
        if data is not None:
            self.view.copy_(torch.as_tensor(data).to(dtype).reshape(shape))
        self.before = self.full.clone()

    def check(self, written=True):
        """Guards bit-unchanged; `written`: no element of the tensor still holds the sentinel; False: nothing changed at all."""
        f, b = bits(self.full), bits(self.before)
        assert torch.equal(f[:PAD], b[:PAD]) and torch.equal(f[PAD + self.n:], b[PAD + self.n:]), 'guard overwritten'
        if written is False:
            assert torch.equal(f, b), 'an output that must stay untouched was written'
        elif written and self.n:
            assert not bool((f[PAD:PAD + self.n] == SENT[self.view.dtype][1]).any()), 'an output element was never written'
        return self.view

    def cpu(self):
        return self.view.cpu()


def strided(data, ld, dtype=F32, fill=NAN):
    """(rows, width) -> device (rows, ld) with `fill` (NaN) in the gap columns; returns the whole device tensor."""
    rows, width = data.shape
    full = torch.full((rows, ld), fill, dtype=dtype)
    full[:, :width] = data.to(dtype)
    return full.cuda()


def ulp32(ref64):
    a = torch.as_tensor(ref64).double().abs().float().numpy()
    return torch.from_numpy(np.spacing(np.maximum(a, np.float32(2.0 ** -126))).astype(np.float64))


def judge(fam, label, kernel, plain, ref64, groups=None, terms=None):
    """The yardstick of the module docstring.  kernel / plain / ref64 (rows, ...) (or vectors of per-row scalars); `terms`: the
    column-sum statistic instead (kernel (cols,)).  groups: lists of row indices judged separately (default: all rows at once)."""
    k = torch.as_tensor(kernel).detach().cpu().double()
    p = torch.as_tensor(plain).detach().double()
    ref = torch.as_tensor(ref64).detach().double()
    assert bool(torch.isfinite(k).all()), f'{fam} {label}: non-finite output'
    if terms is None:
        ek, ep = T.row_err(k, ref), T.row_err(p, ref)
    else:
        ek, ep = T.col_err(k, ref, terms), T.col_err(p, ref, terms)
    within4 = ((k.reshape(ref.shape) - ref).abs() <= 4.0 * ulp32(ref)).reshape(ek.shape[0], -1).all(1)
    bad = []
    for gi, sel in enumerate(groups if groups is not None else [list(range(ek.shape[0]))]):
        sel = torch.as_tensor(sel, dtype=torch.long)
        Ek, Ep = float(ek[sel].max()), float(ep[sel].max())
        if Ep == 0.0:
            ok, ratio = bool(within4[sel].all()), (0.0 if Ek == 0.0 else float('inf'))
        else:
            ratio = Ek / Ep
            # the 4-ulp floor of the exact case holds next to it too: without it the bound jumps from 4 ulp at err(plain) = 0 to a
            # hundredth of an ulp at err(plain) = 0.0025 ulp, which is what a group of ONE scalar (rstd of M = 1, a row's loss) meets
            # whenever plain fp32 happens to round well there
            ok = ratio <= C_FAMILY[fam] or bool(within4[sel].all())
        tag = f'{label}[{gi}]' if groups is not None else label
        print(f'{fam} {tag}: kernel {Ek:.3e} plain {Ep:.3e} ratio {ratio:.2f}')
        RATIOS.setdefault(fam, []).append((tag, ratio))
        if not ok:
            bad.append((tag, Ek, Ep, ratio))
    assert not bad, bad


# =====================================================================================================================
# LayerNorm family
LN_DS = [4, 32, 252, 256, 260, 512, 516, 1020, 1024]
LN_EPS = 1e-5
LN_SEED = 0x5EED000100000000 + 77
LN_FWD_M2 = 4 * 2048 + 1        # ln_blocks: at most 2048 workgroups of 4 rows -> row 8192 is the second row of block 0, wave 0


def ln_bwd_m2(d, has_r):
    """Smallest M at which a wave of the backward takes a second row: 4 * (the cap of ln_bwd_blocks) + 1, the cap read from
    vqcpc_add_layernorm_bwd_partials."""
    cap = query('vqcpc_add_layernorm_bwd_partials', 1 << 24, d, int(has_r))
    assert query('vqcpc_add_layernorm_bwd_partials', 4 * cap, d, int(has_r)) == cap
    assert query('vqcpc_add_layernorm_bwd_partials', 4 * cap - 4, d, int(has_r)) == cap - 1
    return 4 * cap + 1


def ln_data(M, d, seed, bf16=False):
    g = gen(seed)
    x = torch.randn(M, d, generator=g) * 1.5 + 0.3
    r = torch.randn(M, d, generator=g)
    dy = torch.randn(M, d, generator=g)
    if bf16:
        x, dy = x.bfloat16().float(), dy.bfloat16().float()
    return dict(x=x, r=r, dy=dy, gamma=1.0 + 0.5 * torch.randn(d, generator=g), beta=torch.randn(d, generator=g))


def ln_fwd_call(entry, x_dev, ldx, r_dev, gamma, beta, M, d, p, want_y=True, want_b16=False):
    y = Guard((M, d)) if want_y else None
    yb = Guard((M, d), torch.int16) if want_b16 else None
    mean, rstd = Guard(M), Guard(M)
    yv, ybv = (None if y is None else y.view), (None if yb is None else yb.view)
    if entry == 'fwd':
        call('vqcpc_add_layernorm_fwd', x_dev, ldx, r_dev, gamma, beta, yv, mean.view, rstd.view, M, d, LN_EPS, p, LN_SEED)
    elif entry == 'fwd_b16':
        call('vqcpc_add_layernorm_fwd_b16', x_dev, ldx, r_dev, gamma, beta, yv, ybv, mean.view, rstd.view, M, d, LN_EPS, p, LN_SEED)
    else:
        call('vqcpc_layernorm_fwd_xb16', x_dev, ldx, gamma, beta, yv, ybv, mean.view, rstd.view, M, d, LN_EPS)
    torch.cuda.synchronize()
    for o in (y, yb, mean, rstd):
        if o is not None:
            o.check()
    return (None if y is None else y.cpu()), (None if yb is None else yb.cpu()), mean.cpu(), rstd.cpu()


def ln_fwd_check(label, D, M, d, p, with_r, y, mean, rstd, groups=None):
    scale = T.dropout_scale(LN_SEED, (M, d), p) if with_r else None
    r = D['r'] if with_r else None
    ref = T.ln_fwd(D['x'], r, scale, D['gamma'], D['beta'], LN_EPS)
    pl = T.ln_fwd(D['x'], r, scale, D['gamma'], D['beta'], LN_EPS, dtype=F32)
    judge('LN', f'fwd y {label}', y, pl[0], ref[0], groups)
    s_rms = torch.sqrt((ref[3] * ref[3]).mean(1))
    judge('LN', f'fwd mean {label}', mean.double() / s_rms, pl[1].double() / s_rms, ref[1] / s_rms, groups)   # a mean near 0: the row's scale
    judge('LN', f'fwd rstd {label}', rstd, pl[2], ref[2], groups)
    return ref


def _ln_small_cases(d):
    for M in (1, 3, 5):
        for ldx in (d, 4 * d):
            for p in (0.0, 0.25):
                yield M, ldx, p


@pytest.mark.parametrize('d', LN_DS)
def test_layernorm_fwd_every_form(d):
    cases = list(_ln_small_cases(d)) + [(LN_FWD_M2, (4 * d, d)[LN_DS.index(d) % 2], (0.25, 0.0)[LN_DS.index(d) % 2])]
    for M, ldx, p in cases:
        D = ln_data(M, d, 1000 + 7 * M + d)
        gm, bt = D['gamma'].cuda(), D['beta'].cuda()
        xd, rd = strided(D['x'], ldx), D['r'].cuda()
        lab = f'd{d} M{M} ldx{ldx} p{p}'
        # separate r
        y, _, mean, rstd = ln_fwd_call('fwd', xd, ldx, rd, gm, bt, M, d, p)
        ln_fwd_check('r ' + lab, D, M, d, p, True, y, mean, rstd)
        # r == NULL: x is the residual sum, the dropout arguments are not used
        y0, _, mean0, rstd0 = ln_fwd_call('fwd', xd, ldx, None, gm, bt, M, d, p)
        ln_fwd_check('s ' + lab, D, M, d, p, False, y0, mean0, rstd0)
        # _b16 with both outputs: the fp32 output is the one above, the bf16 one its round-to-nearest-even
        for rr, yref, mref in ((rd, y, mean), (None, y0, mean0)):
            y2, yb2, mean2, rstd2 = ln_fwd_call('fwd_b16', xd, ldx, rr, gm, bt, M, d, p, True, True)
            assert same_bits(y2, yref) and same_bits(mean2, mref), lab
            assert torch.equal(yb2.to(torch.int32) & 0xFFFF, T.bf16_rne(y2)), lab
            _, yb3, mean3, rstd3 = ln_fwd_call('fwd_b16', xd, ldx, rr, gm, bt, M, d, p, False, True)
            assert torch.equal(yb3, yb2) and same_bits(mean3, mean2) and same_bits(rstd3, rstd2), lab
        # bf16 x: bit-identical to the fp32-input kernel on the same values
        Db = ln_data(M, d, 1000 + 7 * M + d, bf16=True)
        xb = strided(T.bf16_rne(Db['x']).to(torch.int16), ldx, torch.int16, 0x7FC0)
        x32 = strided(Db['x'], ldx)
        ya, _, ma, ra = ln_fwd_call('fwd', x32, ldx, None, gm, bt, M, d, 0.0)
        yx, ybx, mx, rx = ln_fwd_call('xb16', xb, ldx, None, gm, bt, M, d, 0.0, True, True)
        assert same_bits(yx, ya) and same_bits(mx, ma) and same_bits(rx, ra), lab
        assert torch.equal(ybx.to(torch.int32) & 0xFFFF, T.bf16_rne(ya)), lab
        _, ybx2, _, _ = ln_fwd_call('xb16', xb, ldx, None, gm, bt, M, d, 0.0, False, True)
        assert torch.equal(ybx2, ybx), lab
        if M <= 5:
            ln_fwd_check('xb16 ' + lab, Db, M, d, 0.0, False, yx, mx, rx)


def ln_bwd_call(entry, dy_dev, x_dev, ldx, r_dev, gamma, mean, rstd, M, d, p, ds=True, dsb=False, dr=True, drb=False,
                direct=True):
    """-> dict of host tensors (None where not asked for) + the workspace Guard.  entry: 'bwd' | 'b16' | 'xb16' | 'b16io'."""
    o = dict(d_s=Guard((M, d)) if ds else None, d_s_b=Guard((M, d), torch.int16) if dsb else None,
             d_r=Guard((M, d)) if dr else None, d_r_b=Guard((M, d), torch.int16) if drb else None,
             d_gamma=Guard(d) if direct else None, d_beta=Guard(d) if direct else None)
    wsb = query('vqcpc_add_layernorm_bwd_workspace', M, d)
    assert wsb % 4 == 0
    ws = Guard(wsb // 4)
    v = {k: (None if g is None else g.view) for k, g in o.items()}
    tail = (M, d, p, LN_SEED, ws.view, wsb)
    if entry == 'bwd':
        call('vqcpc_add_layernorm_bwd', dy_dev, x_dev, ldx, r_dev, gamma, mean, rstd, v['d_s'], v['d_r'], v['d_gamma'], v['d_beta'], *tail)
    elif entry == 'b16':
        call('vqcpc_add_layernorm_bwd_b16', dy_dev, x_dev, ldx, r_dev, gamma, mean, rstd, v['d_s'], v['d_r'], v['d_r_b'], v['d_gamma'],
             v['d_beta'], *tail)
    else:
        call('vqcpc_layernorm_bwd_xb16' if entry == 'xb16' else 'vqcpc_layernorm_bwd_b16io', dy_dev, x_dev, ldx, gamma, mean, rstd,
             v['d_s'], v['d_s_b'], v['d_r'], v['d_r_b'], v['d_gamma'], v['d_beta'], *tail)
    torch.cuda.synchronize()
    out = {}
    for k, g in o.items():
        out[k] = None if g is None else g.check().cpu()
    ws.check(written=None)
    out['ws'] = ws
    return out


def ln_bwd_ref(D, M, d, p, form, dtype=torch.float64):
    """form 'r': s = x + r * scale, d_r = d_s * scale; 's': s = x, d_r = d_s * scale (the regenerated mask; p = 0: d_s).
    mean / rstd are INPUTS of the backward: the float64 forward's, rounded to fp32."""
    scale = T.dropout_scale(LN_SEED, (M, d), p)
    f = T.ln_fwd(D['x'], D['r'] if form == 'r' else None, scale, D['gamma'], D['beta'], LN_EPS)
    mean, rstd = f[1].float(), f[2].float()
    s = f[3] if dtype == torch.float64 else T.ln_fwd(D['x'], D['r'] if form == 'r' else None, scale, D['gamma'], D['beta'], LN_EPS, dtype=F32)[3]
    return mean, rstd, T.ln_bwd(D['dy'], s, D['gamma'], mean, rstd, scale, dtype=dtype), f[3]


def ln_bwd_judge(label, D, M, d, p, form, out, groups=None, with_dr=True):
    mean, rstd, ref, s64 = ln_bwd_ref(D, M, d, p, form)
    _, _, pl, _ = ln_bwd_ref(D, M, d, p, form, dtype=F32)
    judge('LN', f'bwd d_s {label}', out['d_s'], pl[0], ref[0], groups)
    if with_dr:
        judge('LN', f'bwd d_r {label}', out['d_r'], pl[1], ref[1], groups)
    if out.get('d_gamma') is not None:
        xh = (s64 - mean.double().unsqueeze(1)) * rstd.double().unsqueeze(1)
        judge('LN', f'bwd d_gamma {label}', out['d_gamma'], pl[2], ref[2], terms=D['dy'].double() * xh)
        judge('LN', f'bwd d_beta {label}', out['d_beta'], pl[3], ref[3], terms=D['dy'].double())
    return ref


@pytest.mark.parametrize('d', LN_DS)
def test_layernorm_bwd_fp32_forms(d):
    i = LN_DS.index(d)
    big = [(ln_bwd_m2(d, True), (d, 4 * d)[i % 2], (0.0, 0.25)[i % 2], ('r',)), (ln_bwd_m2(d, False), (4 * d, d)[i % 2], 0.25, ('s',))]
    for M, ldx, p, forms in [c + (('r', 's'),) for c in _ln_small_cases(d)] + big:
        D = ln_data(M, d, 2000 + 7 * M + d)
        gm, dyd, xd, rd = D['gamma'].cuda(), D['dy'].cuda(), strided(D['x'], ldx), D['r'].cuda()
        for form in forms:
            mean, rstd = ln_bwd_ref(D, M, d, p, form)[:2]
            md, sd = mean.cuda(), rstd.cuda()
            lab = f'{form} d{d} M{M} ldx{ldx} p{p}'
            if form == 'r':
                out = ln_bwd_call('bwd', dyd, xd, ldx, rd, gm, md, sd, M, d, p)
                ln_bwd_judge(lab, D, M, d, p, form, out)
                # the same through the _b16 entry point: same fp32 bits, and the bf16 copy of d_r is its rounding
                o2 = ln_bwd_call('b16', dyd, xd, ldx, rd, gm, md, sd, M, d, p, drb=True)
                assert all(same_bits(o2[k], out[k]) for k in ('d_s', 'd_r', 'd_gamma', 'd_beta')), lab
                assert torch.equal(o2['d_r_b'].to(torch.int32) & 0xFFFF, T.bf16_rne(out['d_r'])), lab
            elif p > 0:
                out = ln_bwd_call('bwd', dyd, xd, ldx, None, gm, md, sd, M, d, p)          # d_r = d_s * the regenerated mask
                ref = ln_bwd_judge(lab, D, M, d, p, form, out)
                keep = T.dropout_scale(LN_SEED, (M, d), p) != 0
                assert bool((out['d_r'][~keep] == 0).all()) and same_bits(out['d_r'][keep], (out['d_s'] * np.float32(T.inv_keep(p)))[keep]), lab
                o2 = ln_bwd_call('bwd', dyd, xd, ldx, None, gm, md, sd, M, d, p, dr=False)   # no d_r asked for: same d_s
                assert same_bits(o2['d_s'], out['d_s']) and same_bits(o2['d_gamma'], out['d_gamma']), lab
                o3 = ln_bwd_call('b16', dyd, xd, ldx, None, gm, md, sd, M, d, p, dr=False, drb=True)
                assert same_bits(o3['d_s'], out['d_s']) and torch.equal(o3['d_r_b'].to(torch.int32) & 0xFFFF, T.bf16_rne(out['d_r'])), lab
            else:
                out = ln_bwd_call('bwd', dyd, xd, ldx, None, gm, md, sd, M, d, 0.0, dr=False)
                ln_bwd_judge(lab, D, M, d, 0.0, form, out, with_dr=False)
                o3 = ln_bwd_call('b16', dyd, xd, ldx, None, gm, md, sd, M, d, 0.0, dr=False, drb=True)   # p = 0: bf16(d_s)
                assert same_bits(o3['d_s'], out['d_s']) and torch.equal(o3['d_r_b'].to(torch.int32) & 0xFFFF, T.bf16_rne(out['d_s'])), lab


# (d_s, d_s_bf16, d_r, d_r_bf16) of the bf16-input forms: at least one of the first two (include/vqcpc.h)
LN_B16_COMBOS = [(1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0), (1, 0, 0, 0), (0, 1, 1, 0)]


@pytest.mark.parametrize('d', LN_DS)
def test_layernorm_bwd_bf16_forms(d):
    """vqcpc_layernorm_bwd_xb16 / _b16io: bit-identical to vqcpc_add_layernorm_bwd (r == NULL) on the upcast values, whatever
    subset of outputs is asked for; every bf16 output is the round-to-nearest-even of the fp32 one."""
    i = LN_DS.index(d)
    for M, ldx, p in list(_ln_small_cases(d)) + [(ln_bwd_m2(d, False), (d, 4 * d)[i % 2], (0.25, 0.0)[i % 2])]:
        D = ln_data(M, d, 3000 + 7 * M + d, bf16=True)
        mean, rstd = ln_bwd_ref(D, M, d, p, 's')[:2]
        gm, md, sd = D['gamma'].cuda(), mean.cuda(), rstd.cuda()
        x32, dy32 = strided(D['x'], ldx), D['dy'].cuda()
        xb = strided(T.bf16_rne(D['x']).to(torch.int16), ldx, torch.int16, 0x7FC0)
        dyb = T.bf16_rne(D['dy']).to(torch.int16).cuda()
        base = ln_bwd_call('bwd', dy32, x32, ldx, None, gm, md, sd, M, d, p, dr=p > 0)
        lab = f'd{d} M{M} ldx{ldx} p{p}'
        if M <= 5:
            ln_bwd_judge('xb16-values ' + lab, D, M, d, p, 's', base, with_dr=p > 0)
        want_r = base['d_r'] if p > 0 else base['d_s']
        for entry, dyv in (('xb16', dy32), ('b16io', dyb)):
            for ds, dsb, dr, drb in LN_B16_COMBOS:
                dr = dr and p > 0                                    # p == 0: d_r is d_s, NULL is passed (include/vqcpc.h)
                o = ln_bwd_call(entry, dyv, xb, ldx, None, gm, md, sd, M, d, p, ds=bool(ds), dsb=bool(dsb), dr=bool(dr), drb=bool(drb))
                tag = f'{entry} {lab} {(ds, dsb, dr, drb)}'
                assert same_bits(o['d_gamma'], base['d_gamma']) and same_bits(o['d_beta'], base['d_beta']), tag
                if ds:
                    assert same_bits(o['d_s'], base['d_s']), tag
                if dsb:
                    assert torch.equal(o['d_s_b'].to(torch.int32) & 0xFFFF, T.bf16_rne(base['d_s'])), tag
                if dr:
                    assert same_bits(o['d_r'], base['d_r']), tag
                if drb:
                    assert torch.equal(o['d_r_b'].to(torch.int32) & 0xFFFF, T.bf16_rne(want_r)), tag


def _reduce(items, accumulate):
    n = len(items)
    vp, i64, i32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    call('vqcpc_reduce_grouped', n, vp(*[it[0] for it in items]), i64(*[it[1] for it in items]), i32(*[it[2] for it in items]),
         vp(*[it[3] for it in items]), i64(*[it[4] for it in items]), accumulate)
    torch.cuda.synchronize()


@pytest.mark.parametrize('d,form', [(4, 'r'), (260, 's'), (516, 'r'), (1024, 's')])
def test_layernorm_deferred_partials(d, form):
    """d_gamma == d_beta == NULL leaves exactly vqcpc_add_layernorm_bwd_partials(M, d, has_r) rows of [d gamma | d beta] in the
    workspace; vqcpc_reduce_grouped sums them.  Bit identity with the direct form is ASSERTED: reduce_many_kernel walks the
    partials of a column in the order of reduce_splits_kernel (group g: splits g, g + 16, ..., the same four-at-a-time
    association, then the 16 group sums in ascending order), which is what the direct form launches for d < 65536."""
    has_r = form == 'r'
    for M in (5, ln_bwd_m2(d, has_r)):
        D = ln_data(M, d, 4000 + M + d)
        p = 0.25
        mean, rstd = ln_bwd_ref(D, M, d, p, form)[:2]
        args = (D['dy'].cuda(), strided(D['x'], d), d, D['r'].cuda() if has_r else None, D['gamma'].cuda(), mean.cuda(), rstd.cuda(), M, d, p)
        direct = ln_bwd_call('bwd', *args)
        lab = f'deferred {form} d{d} M{M}'
        ln_bwd_judge(lab, D, M, d, p, form, direct)
        deferred = ln_bwd_call('bwd', *args, direct=False)
        assert same_bits(deferred['d_s'], direct['d_s']) and same_bits(deferred['d_r'], direct['d_r'])
        npart = query('vqcpc_add_layernorm_bwd_partials', M, d, int(has_r))
        ws = deferred['ws']
        wb = bits(ws.view)
        assert not bool((wb[:npart * 2 * d] == SENT_I32).any()), 'a partial row was not written'
        assert bool((wb[npart * 2 * d:] == SENT_I32).all()), 'more than partials(M, d, has_r) rows were written'
        base = ws.view.data_ptr()
        seg_g, seg_b = (base, 2 * d, npart), (base + 4 * d, 2 * d, npart)

        def run(items, accumulate, init=None):
            outs = [Guard(d, data=init) for _ in items]
            _reduce([seg + (o.view.data_ptr(), d) for seg, o in zip(items, outs)], accumulate)
            return [o.check().cpu() for o in outs]

        g0, b0 = run([seg_g, seg_b], 0)
        identical = same_bits(g0, direct['d_gamma']) and same_bits(b0, direct['d_beta'])
        print(f'LN {lab}: reduce_grouped(accumulate = 0) bit-identical to the direct form: {identical}')
        assert identical
        # accumulate = 1 onto a given start: the sum enters the chain first, so compare against float64 under the yardstick
        mean_, rstd_, ref, s64 = ln_bwd_ref(D, M, d, p, form)
        pl = ln_bwd_ref(D, M, d, p, form, dtype=F32)[2]
        xh = (s64 - mean_.double().unsqueeze(1)) * rstd_.double().unsqueeze(1)
        init = torch.randn(d, generator=gen(d))
        g1, b1 = run([seg_g, seg_b], 1, init)
        tg = torch.cat([D['dy'].double() * xh, init.double().unsqueeze(0)])
        tb = torch.cat([D['dy'].double(), init.double().unsqueeze(0)])
        judge('LN', f'{lab} accumulate d_gamma', g1, (pl[2] + init), ref[2] + init.double(), terms=tg)
        judge('LN', f'{lab} accumulate d_beta', b1, (pl[3] + init), ref[3] + init.double(), terms=tb)
        # two groups naming the same output, accumulated in argument order: out = init + sum + sum
        out = Guard(d, data=init)
        _reduce([seg_g + (out.view.data_ptr(), d), seg_g + (out.view.data_ptr(), d)], 1)
        g2 = out.check().cpu()
        judge('LN', f'{lab} same output twice', g2, (pl[2] * 2 + init), 2 * ref[2] + init.double(), terms=torch.cat([tg, D['dy'].double() * xh]))
        # more than 32 groups in one call: every output carries the direct form's bits
        many = run([seg_g, seg_b] * 20, 0)
        assert all(same_bits(o, direct['d_gamma'] if j % 2 == 0 else direct['d_beta']) for j, o in enumerate(many)), lab


@pytest.mark.parametrize('d', [32, 260, 516, 1024])
def test_layernorm_conditioning(d):
    """Badly conditioned rows beside Gaussian rows in one call, each kind judged on its own: mean 1e3 with unit spread, constant
    rows (y == beta exactly, d_s finite), rows scaled by 1e-20 (eps dominates) and by 1e15, one-hot rows."""
    g = gen(50 + d)
    M = 18
    x = torch.randn(M, d, generator=g)
    x[3:6] += 1.0e3
    x[6], x[7], x[8] = 3.0, -0.5, 1024.0
    x[9:12] *= 1.0e-20
    x[12:15] *= 1.0e15
    x[15:18] = 0.0
    x[15, 0], x[16, d - 1], x[17, d // 2] = 1.0, -2.0, 1.0e4
    groups = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14], [15, 16, 17]]
    D = dict(x=x, r=None, dy=torch.randn(M, d, generator=g), gamma=1.0 + 0.5 * torch.randn(d, generator=g),
             beta=torch.randn(d, generator=g))
    ldx = d + 8
    gm, bt, xd = D['gamma'].cuda(), D['beta'].cuda(), strided(x, ldx)
    y, _, mean, rstd = ln_fwd_call('fwd', xd, ldx, None, gm, bt, M, d, 0.0)
    ln_fwd_check(f'conditioning d{d}', D, M, d, 0.0, False, y, mean, rstd, groups)
    assert same_bits(y[6:9], D['beta'].expand(3, d)), 'a constant row must give y == beta exactly'
    m_in, r_in = ln_bwd_ref(D, M, d, 0.0, 's')[:2]
    out = ln_bwd_call('bwd', D['dy'].cuda(), xd, ldx, None, gm, m_in.cuda(), r_in.cuda(), M, d, 0.0, dr=False)
    assert bool(torch.isfinite(out['d_s']).all())
    ln_bwd_judge(f'conditioning d{d}', D, M, d, 0.0, 's', out, groups, with_dr=False)


# =====================================================================================================================
# SELU
def _selu_inputs(n):
    grid = torch.logspace(-7, math.log10(30.0), 2499, dtype=torch.float64)
    full = torch.cat([torch.tensor([0.0, -0.0], dtype=torch.float64), torch.stack([-grid, grid], 1).reshape(-1)]).float()
    if n == 1:
        return torch.tensor([-1.0e-5])
    return full if n == full.numel() else full[torch.linspace(0, full.numel() - 1, n).long()]


@pytest.mark.parametrize('n', [1, 255, 257, 5000])
@pytest.mark.parametrize('p', [0.0, 0.25])
def test_dropout_selu(n, p):
    """Forward: |out - ref64| <= 4 * 2^-24 |ref64| + one fp32 denormal, for x over +-[1e-7, 30], 0 and -0 (the `__expf(x) - 1`
    form this kernel had misses it for every small negative x: relative error 6e-5 at -1e-3, several per cent at -1e-6).
    Backward: the yardstick."""
    seed = 0xABCDEF0100000003
    h = _selu_inputs(n)
    assert h.numel() == n
    scale = T.dropout_scale(seed, (n,), p)
    out = Guard(n)
    call('vqcpc_dropout_selu_fwd', h.cuda(), out.view, n, p, seed)
    torch.cuda.synchronize()
    o = out.check().cpu()
    ref = T.dropout_selu_fwd(h, scale)
    err = (o.double() - ref).abs()
    bound = 4.0 * U * ref.abs() + 2.0 ** -149
    worst = float((err / bound).max())
    print(f'SELU fwd n{n} p{p}: max err / bound = {worst:.3f}')
    assert bool(torch.isfinite(o).all()) and bool((err <= bound).all()), (worst, h[(err > bound)][:5])
    g = torch.randn(n, generator=gen(n))
    gh = Guard(n)
    call('vqcpc_dropout_selu_bwd', h.cuda(), g.cuda(), gh.view, n, p, seed)
    torch.cuda.synchronize()
    judge('SELU', f'bwd n{n} p{p}', gh.check().cpu().reshape(1, n), T.dropout_selu_bwd(h, g, scale, dtype=F32).reshape(1, n),
          T.dropout_selu_bwd(h, g, scale).reshape(1, n))


# =====================================================================================================================
# GRU
GRU_SEED = 0x1357924600000009


def _gru_cell_data(B, H, seed, saturate):
    g = gen(seed)
    gi, gh = torch.randn(B, 3 * H, generator=g), torch.randn(B, 3 * H, generator=g)
    if saturate and H >= 3:                                          # a quarter of the pre-activations at +-40: sigmoid and tanh saturate
        m = torch.rand(B, 3 * H, generator=g) < 0.25
        gi = torch.where(m, torch.where(torch.rand(B, 3 * H, generator=g) < 0.5, 40.0, -40.0) - gh, gi)
    return gi, gh, torch.randn(B, H, generator=g), torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)


@pytest.mark.parametrize('H', [1, 3, 64, 100])
@pytest.mark.parametrize('B', [1, 5, 33])
def test_gru_cell(B, H):
    for hp_given in (False, True):
        for p, base in ((0.0, 0), (0.3, 123457)):
            gi, gh, hp, d_y, d_h = _gru_cell_data(B, H, 100 * B + H, saturate=p > 0)
            hp_ = hp if hp_given else None
            scale = T.dropout_scale(GRU_SEED, (B, H), p, idx_base=base)
            lab = f'B{B} H{H} hprev{int(hp_given)} p{p}'
            ho, yo = Guard((B, H)), Guard((B, H))
            gid, ghd, hpd = gi.cuda(), gh.cuda(), (hp.cuda() if hp_given else None)
            call('vqcpc_gru_cell_fwd', gid, ghd, hpd, ho.view, yo.view, B, H, p, GRU_SEED, base)
            torch.cuda.synchronize()
            ref, pl = T.gru_cell_fwd(gi, gh, hp_, scale), T.gru_cell_fwd(gi, gh, hp_, scale, dtype=F32)
            judge('GRU', f'cell h {lab}', ho.check().cpu(), pl[0], ref[0])
            judge('GRU', f'cell y {lab}', yo.check().cpu(), pl[1], ref[1])
            ho2 = Guard((B, H))
            call('vqcpc_gru_cell_fwd', gid, ghd, hpd, ho2.view, None, B, H, p, GRU_SEED, base)       # y_out is nullable
            torch.cuda.synchronize()
            assert same_bits(ho2.check().cpu(), ho.cpu())
            for dy_, dh_ in ((d_y, None), (None, d_h), (d_y, d_h)):
                o = [Guard((B, 3 * H)), Guard((B, 3 * H)), Guard((B, H))]
                call('vqcpc_gru_cell_bwd', gid, ghd, hpd, None if dy_ is None else dy_.cuda(), None if dh_ is None else dh_.cuda(),
                     o[0].view, o[1].view, o[2].view, B, H, p, GRU_SEED, base)
                torch.cuda.synchronize()
                rb = T.gru_cell_bwd(gi, gh, hp_, dy_, dh_, scale)
                pb = T.gru_cell_bwd(gi, gh, hp_, dy_, dh_, scale, dtype=F32)
                for name, oo, a, b in zip(('d_gi', 'd_gh', 'd_hprev'), o, pb, rb):
                    judge('GRU', f'cell {name} {lab} dy{int(dy_ is not None)} dh{int(dh_ is not None)}', oo.check().cpu(), a, b)


def _gemm_nt_fp32(A, Bm, M, N, K, bias=None, add=None):
    """C = A . B^T (+ bias) (+ add) with vqcpc_gemm_nt in mode 0 (fp32 MFMA)."""
    from vqcpc_bach_amd import hip
    st = hip.gemm_mode_state()
    hip.set_gemm_mode(0)
    try:
        Cm = Guard((M, N))
        call('vqcpc_gemm_nt', A, K, Bm, K, Cm.view, N, M, N, K, bias, 0, 0.0, 0, None, 0, 1.0, add, N if add is not None else 0, None, 0)
        torch.cuda.synchronize()
        return Cm.check()
    finally:
        hip.restore_gemm_mode_state(st)


def test_gru_step_supported():
    for H, want in ((63, 0), (64, 1), (96, 0), (100, 0), (128, 1), (192, 1)):
        assert query('vqcpc_gru_step_supported', 8, H) == want, H
    assert query('vqcpc_gru_step_supported', 0, 64) == 0


@pytest.mark.parametrize('H', [64, 128, 192])
@pytest.mark.parametrize('B', [1, 31, 32, 33, 65])
def test_gru_step(B, H):
    """One fused launch against the float64 step, and against vqcpc_gemm_nt (mode 0) + the cell kernel under the same bound.
    h_prev / dgh_next carry NaN rows past B: the 32-row tile must not read them into a result."""
    g = gen(7 * B + H)
    w = torch.randn(3 * H, H, generator=g) / math.sqrt(H)
    b = torch.randn(3 * H, generator=g)
    gi = torch.randn(B, 3 * H, generator=g)
    hp = torch.randn(B, H, generator=g)
    pad = torch.full((3, H), NAN)
    wd, bd, gid, hpd = w.cuda(), b.cuda(), gi.cuda(), torch.cat([hp, pad]).cuda()
    for hp_given, p, base in ((True, 0.0, 0), (True, 0.3, 99), (False, 0.3, 1 << 33)):
        lab = f'B{B} H{H} hprev{int(hp_given)} p{p}'
        scale = T.dropout_scale(GRU_SEED, (B, H), p, idx_base=base)
        o = [Guard((B, 3 * H)), Guard((B, H)), Guard((B, H))]
        call('vqcpc_gru_step_fwd', gid, wd, bd, hpd if hp_given else None, o[0].view, o[1].view, o[2].view, B, H, p, GRU_SEED, base)
        torch.cuda.synchronize()
        ref = T.gru_step_fwd(gi, w, b, hp if hp_given else None, scale)
        pl = T.gru_step_fwd(gi, w, b, hp if hp_given else None, scale, dtype=F32)
        got = [x.check().cpu() for x in o]
        for name, a, c, r in zip(('gh', 'h', 'y'), got, pl, ref):
            judge('GRU', f'step {name} {lab}', a, c, r)
        if hp_given:
            gh2 = _gemm_nt_fp32(hpd, wd, B, 3 * H, H, bias=bd)
            h2, y2 = Guard((B, H)), Guard((B, H))
            call('vqcpc_gru_cell_fwd', gid, gh2, hpd, h2.view, y2.view, B, H, p, GRU_SEED, base)
            torch.cuda.synchronize()
            for name, a, c, r in zip(('gh', 'h', 'y'), got, pl, (gh2.cpu(), h2.check().cpu(), y2.check().cpu())):
                ek, ep = float(T.row_err(a, r.double()).max()), float(T.row_err(c, ref[('gh', 'h', 'y').index(name)]).max())
                print(f'GRU step-vs-unfused {name} {lab}: difference {ek:.3e} plain {ep:.3e}')
                assert ek <= C_FAMILY['GRU'] * ep, (name, lab, ek, ep)
    # backward step
    gh = T.gru_step_fwd(gi, w, b, hp)[0].float()
    whh_t = w.t().contiguous()
    dgh = torch.randn(B, 3 * H, generator=g)
    dhp = torch.randn(B, H, generator=g)
    d_y = torch.randn(B, H, generator=g)
    dghd, wtd, ghd = torch.cat([dgh, torch.full((3, 3 * H), NAN)]).cuda(), whh_t.cuda(), gh.cuda()
    for dy_given, p, base in ((False, 0.0, 0), (True, 0.3, 99)):
        lab = f'B{B} H{H} dy{int(dy_given)} p{p}'
        scale = T.dropout_scale(GRU_SEED, (B, H), p, idx_base=base)
        dy_ = d_y if dy_given else None
        o = [Guard((B, 3 * H)), Guard((B, 3 * H)), Guard((B, H), data=dhp)]
        call('vqcpc_gru_step_bwd', dghd, wtd, o[2].view, gid, ghd, hpd, None if dy_ is None else dy_.cuda(), o[0].view, o[1].view, B, H,
             p, GRU_SEED, base)
        torch.cuda.synchronize()
        ref = T.gru_step_bwd(dgh, whh_t, dhp, gi, gh, hp, dy_, scale)
        pl = T.gru_step_bwd(dgh, whh_t, dhp, gi, gh, hp, dy_, scale, dtype=F32)
        got = [x.check().cpu() for x in o]
        for name, a, c, r in zip(('d_gi', 'd_gh', 'dhp'), got, pl, ref):
            judge('GRU', f'step {name} {lab}', a, c, r)
        dh2 = _gemm_nt_fp32(dghd, wtd, B, H, 3 * H, add=dhp.cuda())
        o2 = [Guard((B, 3 * H)), Guard((B, 3 * H)), Guard((B, H))]
        call('vqcpc_gru_cell_bwd', gid, ghd, hpd, None if dy_ is None else dy_.cuda(), dh2, o2[0].view, o2[1].view, o2[2].view, B, H, p,
             GRU_SEED, base)
        torch.cuda.synchronize()
        for name, a, c, r, o2_ in zip(('d_gi', 'd_gh', 'dhp'), got, pl, ref, o2):
            ek, ep = float(T.row_err(a, o2_.check().cpu().double()).max()), float(T.row_err(c, r).max())
            print(f'GRU step-vs-unfused {name} {lab}: difference {ek:.3e} plain {ep:.3e}')
            assert ek <= C_FAMILY['GRU'] * ep, (name, lab, ek, ep)


# =====================================================================================================================
# InfoNCE
# the last shape: the backward's dynamic LDS (2 K zdim + K (N + 1) + cdim floats) is 65 520 bytes of the 65 536 it may ask for
NCE_SHAPES = [(1, 1, 1, 1, 1), (3, 5, 7, 6, 10), (2, 256, 2, 4, 4), (2, 16, 3, 500, 316)]


@pytest.mark.parametrize('B,K,N,zdim,cdim', NCE_SHAPES)
def test_nce(B, K, N, zdim, cdim):
    assert (2 * K * zdim + K * (N + 1) + cdim) * 4 <= 65536
    g = gen(B + K + N + zdim)
    c = torch.randn(B, cdim, generator=g)
    W = torch.randn(zdim, cdim, K, generator=g) / math.sqrt(zdim * cdim)
    zp = torch.randn(B, K, zdim, generator=g)
    zn = torch.randn(B, N, K, zdim, generator=g)
    # an exact tie between the positive and the largest negative at (b, k) = (0, 0): the same vector, hence the same fp32 chain
    # (not in the 1 x 1 x 1 shape: with its only negative equal to the positive every gradient cancels to exactly nothing)
    tie = B * K > 1
    f0 = T.nce_fwd(c, W, zp, zn)
    if tie:
        zp[0, 0] = zn[0, int(f0[1][0, 0].argmax()), 0]
    # scores up to |f| = 80: exp() of the raw scores would overflow fp32, the log-sum-exp must not
    fmax = max(float(T.nce_fwd(c, W, zp, zn)[0].abs().max()), float(T.nce_fwd(c, W, zp, zn)[1].abs().max()))
    zp, zn = zp * (80.0 / fmax), zn * (80.0 / fmax)
    ref = T.nce_fwd(c, W, zp, zn)
    pl = T.nce_fwd(c, W, zp, zn, dtype=F32)
    assert 79.0 < max(float(ref[0].abs().max()), float(ref[1].abs().max())) < 81.0
    cd, Wd, zpd, znd = c.cuda(), W.cuda(), zp.cuda(), zn.cuda()
    o = [Guard((B, K)), Guard((B, K, N)), Guard(B), Guard((B, K))]
    call('vqcpc_nce_fwd', cd, Wd, zpd, znd, B, K, N, zdim, cdim, *[x.view for x in o])
    torch.cuda.synchronize()
    f_pos, f_neg, loss_b, hits = [x.check().cpu() for x in o]
    lab = f'B{B} K{K} N{N} z{zdim} c{cdim}'
    judge('NCE', f'f_pos {lab}', f_pos, pl[0], ref[0])
    judge('NCE', f'f_neg {lab}', f_neg, pl[1], ref[1])
    judge('NCE', f'loss_b {lab}', loss_b, pl[2], ref[2])
    # hits: exact wherever the float64 margin exceeds the fp32 score error (a (cdim + zdim)-term chain), and at the planted tie
    wc = torch.einsum('bc,zck->bkz', c.double().abs(), W.double().abs())
    mag = torch.maximum((wc * zp.double().abs()).sum(-1), torch.einsum('bkz,bnkz->bkn', wc, zn.double().abs()).max(2)[0])
    margin = ref[0] - ref[1].max(2)[0]
    sure = margin.abs() > 4.0 * (cdim + zdim + 2) * U * mag
    if tie:
        assert abs(float(margin[0, 0])) < 1e-9 and float(hits[0, 0]) == 0.0, 'an exact tie is no hit'
        sure[0, 0] = False                                               # float64 sums the two copies in different orders: no sign to compare
    assert float(sure.double().mean()) > 0.9 or B * K < 4
    assert torch.equal(hits[sure], ref[3][sure].float()), lab
    assert bool(((hits == 0) | (hits == 1)).all())
    # backward from the kernel's own saved scores
    gb = torch.randn(B, generator=g)
    wsb = query('vqcpc_nce_bwd_workspace', B, K, N, zdim, cdim)
    outs = []
    for _ in range(2):
        ws = Guard(wsb // 4)
        ob = [Guard((B, cdim)), Guard((zdim, cdim, K)), Guard((B, K, zdim)), Guard((B, N, K, zdim))]
        call('vqcpc_nce_bwd', cd, Wd, zpd, znd, o[0].view, o[1].view, gb.cuda(), B, K, N, zdim, cdim, *[x.view for x in ob], ws.view, wsb)
        torch.cuda.synchronize()
        ws.check()
        outs.append([x.check().cpu() for x in ob])
    assert same_bits(outs[0][1], outs[1][1]), 'd_W must be bit-reproducible'
    rb = T.nce_bwd(c, W, zp, zn, f_pos, f_neg, gb)
    pb = T.nce_bwd(c, W, zp, zn, f_pos, f_neg, gb, dtype=F32)
    for name, a, b_, r in zip(('d_c', 'd_W', 'd_z_pos', 'd_z_neg'), outs[0], pb, rb):
        judge('NCE', f'{name} {lab}', a, b_, r)


# =====================================================================================================================
# softmax cross-entropy, scale_rows
def _ce_logits(R, V, seed, shift=0):
    """Row kinds, cycling: 0 N(0, 9) | 1 1e4 + N(0, 1) | 2 N(0, 1e8) | 3 equal logits | 4 -1e4 + N(0, 1)."""
    g = gen(seed)
    x = torch.randn(R, V, generator=g) * 3.0
    kinds = [(r + V + shift) % 5 for r in range(R)]
    for r, k in enumerate(kinds):
        if k == 1:
            x[r] = 1.0e4 + torch.randn(V, generator=g)
        elif k == 2:
            x[r] = torch.randn(V, generator=g) * 1.0e4
        elif k == 3:
            x[r] = 7.0
        elif k == 4:
            x[r] = -1.0e4 + torch.randn(V, generator=g)
    groups = [[r for r in range(R) if kinds[r] == k] for k in sorted(set(kinds))]
    return x, groups, g


@pytest.mark.parametrize('V', [1, 5, 63, 64, 65, 130])
@pytest.mark.parametrize('R', [1, 3, 4, 5, 9])
def test_softmax_ce(R, V):
    """Loss and gradient, hard and soft targets, each row kind judged on its own.  (With the fp32 evaluation this kernel had, five
    gradient cases measured 4.03 - 6.21 x the plain-fp32 error -- [1-130], [3-63], [5-64], [5-65], [9-65] -- which is why the
    kernel now evaluates the row in double; see profiles/train_kernel_tests_log.md.)"""
    x, groups, g = _ce_logits(R, V, 31 * R + V)
    tl, _, _ = _ce_logits(R, V, 77 * R + V, shift=2)        # never the kind of the logits: equal rows on both sides cancel to 0
    tgt = torch.randint(0, V, (R,), generator=g)
    ld, ldt = V + 3, V + 5
    xd, tld = strided(x, ld), strided(tl, ldt)
    for soft in (False, True):
        loss, grad = Guard(R), Guard((R, V))
        call('vqcpc_softmax_ce', xd, ld, None if soft else tgt.cuda(), tld if soft else None, ldt if soft else 0, loss.view, grad.view, R, V)
        torch.cuda.synchronize()
        kw = dict(target_logits=tl) if soft else dict(target=tgt)
        ref, pl = T.softmax_ce(x, **kw), T.softmax_ce(x, dtype=F32, **kw)
        lab = f'R{R} V{V} {"soft" if soft else "hard"}'
        lo, gr = loss.check().cpu(), grad.check().cpu()
        judge('CE', f'loss {lab}', lo, pl[0], ref[0], groups)
        judge('CE', f'grad {lab}', gr, pl[1], ref[1], groups)
        # the gradient rows sum to 0: each of the V elements may err by C * (plain fp32's largest error in that row, at least 2^-24)
        per_el = torch.clamp((pl[1].double() - ref[1]).abs().max(1)[0], min=U)
        assert bool((gr.double().sum(1).abs() <= V * C_FAMILY['CE'] * per_el).all()), lab


@pytest.mark.parametrize('R,V', [(1, 1), (255, 1), (257, 1), (5, 51), (1, 257), (3, 130)])
def test_scale_rows_is_exact(R, V):
    g = gen(R + V)
    a, s = torch.randn(R, V, generator=g), torch.randn(R, generator=g)
    out = Guard((R, V))
    call('vqcpc_scale_rows', a.cuda(), s.cuda(), out.view, R, V)
    torch.cuda.synchronize()
    assert same_bits(out.check().cpu(), a * s.unsqueeze(1))


# =====================================================================================================================
# optimiser
SUMSQ_BLOCKS = 1024                           # kSumsqBlocks of csrc/util.hip: vqcpc_sumsq_workspace(n) / sizeof(double)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1025, 100003, SUMSQ_BLOCKS * 256 * 4 + 1, SUMSQ_BLOCKS * 256 * 4 + 4])
def test_sumsq(n):
    """n past kSumsqBlocks * 256 * 4: at + 1 the tail element follows a full single pass, at + 4 the block loop takes a second
    pass.  Bound 2^-23 relative: each float4 term is rounded in fp32 before the double accumulation."""
    wsb = query('vqcpc_sumsq_workspace', n)
    assert wsb == SUMSQ_BLOCKS * 8
    gv = torch.randn(n, generator=gen(n % 1000 + 1))
    gd = gv.cuda()
    for gs in (1.0, 0.125):
        res = []
        for _ in range(2):
            out, ws = Guard(1, torch.float64), Guard(wsb // 8, torch.float64)
            call('vqcpc_sumsq', gd, n, gs, out.view, ws.view, wsb)
            torch.cuda.synchronize()
            ws.check(written=None)
            res.append(out.check().cpu())
        assert same_bits(res[0], res[1]), 'two calls must give the same bits'
        ref = T.sumsq(gv, gs)
        rel = abs(float(res[0][0]) - ref) / ref
        print(f'SUMSQ n{n} scale{gs}: relative error {rel:.3e} (bound {2.0 ** -23:.3e})')
        assert rel <= 2.0 ** -23, (n, gs, rel)


ADAM = dict(lr=float(np.float32(1e-3)), b1=float(np.float32(0.9)), b2=float(np.float32(0.999)), eps=float(np.float32(1e-8)),
            max_norm=5.0)                    # the ABI takes floats: the reference works with the fp32 values of the constants


def _adam_state(n, kind, seed):
    g = gen(seed)
    p, m = torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
    v = 0.01 * (1.0 + torch.rand(n, generator=g))
    if kind == 'zero':
        gr = torch.zeros(n)
    elif kind == 'tiny':
        gr = torch.full((n,), 1.0e-20) * torch.sign(torch.randn(n, generator=g))
    elif kind == 'at_max_norm':                                      # ||g|| = 5 = max_norm exactly: the clip just engages (1e-6 in the denominator)
        gr = torch.zeros(n)
        gr[0], gr[n - 1] = (3.0, 4.0) if n > 1 else (5.0, 5.0)
    else:
        gr = torch.randn(n, generator=g) * (3.0 if kind == 'clipped' else 0.01)
    return p, gr, m, v


def _adam_bounds(p, g, m, v, t, coef, new):
    """Componentwise bounds on |fp32 - float64| from the update formula, u = 2^-24 per rounding:
      g' = g coef              coef is 5 roundings from sumsq (sqrt, + 1e-6, /, min, * grad_scale), the product one more: 6u |g'|
      m' = b1 m + (1 - b1) g'  two products, one sum, the error of g': 4u b1 |m| + 10u (1 - b1) |g'|  <=  10u (b1 |m| + (1 - b1) |g'|)
      v' = b2 v + (1 - b2) g'^2   g'^2 carries 12u, three more roundings: 16u v'
      p' = p - a m' / (sqrt(v') s + eps), a = lr / bc1 and s = 1 / sqrt(bc2) rounded once each: the quotient inherits the ABSOLUTE
           error of m' (which does not shrink when b1 m and (1 - b1) g' cancel) over the denominator; the denominator carries
           16u / 2 from v' and one rounding each from sqrt, s, the product and + eps: 12u; a, the quotient and the product: 3u;
           the subtraction rounds once more:
           a 10u (b1 |m| + (1 - b1) |g'|) / den + 15u |upd| + u |p'|  <=  u (|p'| + 26 lr A), A = a (b1 |m| + (1 - b1) |g'|) / (lr den)
           -- relative to |p| + lr, with A the uncancelled update in units of lr (A <= 4 for the states drawn here).
    A denormal (2^-149) is added to each."""
    b1, b2, lr, eps = ADAM['b1'], ADAM['b2'], ADAM['lr'], ADAM['eps']
    pn, gn, mn, vn = new
    mag = b1 * m.double().abs() + (1 - b1) * gn.abs()
    den = torch.sqrt(vn) / math.sqrt(1 - b2 ** t) + eps
    A = (1.0 / (1 - b1 ** t)) * mag / den
    tiny = 2.0 ** -149
    return (U * (pn.abs() + 26.0 * lr * A) + tiny, 6 * U * gn.abs() + tiny, 10 * U * mag + tiny, 16 * U * vn + tiny)


def _adam_run(entry, state, n, t, gs, sumsq_val):
    bufs = [Guard(n, data=a) for a in state]
    sq = None if sumsq_val is None else torch.tensor([sumsq_val], dtype=torch.float64).cuda()
    if entry == 'host':
        call('vqcpc_adam_step', *[b.view for b in bufs], n, ADAM['lr'], ADAM['b1'], ADAM['b2'], ADAM['eps'], t, gs, ADAM['max_norm'], sq)
    else:
        lr_dev = torch.tensor([ADAM['lr']], dtype=F32).cuda()
        step_dev = torch.tensor([t], dtype=torch.int64).cuda()
        call('vqcpc_adam_step_dev', *[b.view for b in bufs], n, lr_dev, ADAM['b1'], ADAM['b2'], ADAM['eps'], step_dev, gs, ADAM['max_norm'], sq)
    torch.cuda.synchronize()
    return [b.check().cpu() for b in bufs]


def _within_ulps(a, b, k=1):
    ia, ib = a.view(torch.int32).to(torch.int64), b.view(torch.int32).to(torch.int64)
    fa = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    fb = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return bool(((fa - fb).abs() <= k).all())


@pytest.mark.parametrize('t', [1, 2, 10, 1000, 10 ** 6])
def test_adam_step_and_adam_step_dev(t):
    cases = [('small', 1000, 1.0, True), ('clipped', 1000, 1.0, True), ('clipped', 257, 0.125, True), ('small', 1, 1.0, True),
             ('zero', 300, 1.0, True), ('tiny', 300, 1.0, True), ('at_max_norm', 300, 1.0, True), ('clipped', 1000, 1.0, False)]
    if t == 1:
        cases.append(('small', 4096 * 256 + 5, 1.0, True))            # past the grid cap of 4096 workgroups: the element loop runs twice
    for kind, n, gs, clip in cases:
        state = _adam_state(n, kind, 10 * t + n)
        sq = T.sumsq(state[1], gs) if clip else None                   # sumsq == NULL: no clipping
        coef = T.clip_coef(sq, ADAM['max_norm'], gs)
        if kind == 'at_max_norm':
            assert sq == 25.0 and coef < 1.0
        if kind == 'clipped' and clip:
            assert coef < gs
        new = T.adam_step(*state, ADAM['lr'], ADAM['b1'], ADAM['b2'], ADAM['eps'], t, coef)
        bounds = _adam_bounds(*state, t, coef, new)
        lab = f't{t} {kind} n{n} gs{gs} clip{int(clip)}'
        got = {}
        for entry in ('host', 'dev'):
            got[entry] = _adam_run(entry, state, n, t, gs, sq)
            for name, a, r, bd in zip('pgmv', got[entry], new, bounds):
                assert bool(torch.isfinite(a).all()), (entry, name, lab)
                worst = float(((a.double() - r).abs() / bd).max())
                print(f'ADAM {entry} {name} {lab}: max err / bound = {worst:.3f}')
                assert worst <= 1.0, (entry, name, lab, worst)
        if kind == 'zero':
            assert bool((got['host'][1] == 0).all())                   # g is left clipped in place: zeros stay zeros
        same = all(same_bits(a, b) for a, b in zip(got['host'], got['dev']))
        print(f'ADAM dev-vs-host {lab}: bit-identical {same}')
        assert all(_within_ulps(a, b) for a, b in zip(got['host'], got['dev'])), lab


def test_adam_step_dev_chained_through_rng_salt_advance():
    """Three steps whose step count is the counter vqcpc_rng_salt_advance increments reproduce vqcpc_adam_step at t = 1, 2, 3."""
    n = 500
    state = _adam_state(n, 'small', 5)
    grads = [torch.randn(n, generator=gen(60 + i)) * 0.1 for i in range(3)]
    counter = torch.zeros(1, dtype=torch.int64).cuda()
    lr_dev = torch.tensor([ADAM['lr']], dtype=F32).cuda()
    dev = [Guard(n, data=a) for a in state]
    host = [Guard(n, data=a) for a in state]
    ref = [a.double() for a in state]
    try:
        for t in (1, 2, 3):
            call('vqcpc_rng_salt_advance', counter, 0x1234, )
            dev[1].view.copy_(grads[t - 1])
            host[1].view.copy_(grads[t - 1])
            call('vqcpc_adam_step_dev', *[b.view for b in dev], n, lr_dev, ADAM['b1'], ADAM['b2'], ADAM['eps'], counter, 1.0, ADAM['max_norm'], None)
            call('vqcpc_adam_step', *[b.view for b in host], n, ADAM['lr'], ADAM['b1'], ADAM['b2'], ADAM['eps'], t, 1.0, ADAM['max_norm'], None)
            torch.cuda.synchronize()
            assert int(counter.cpu()[0]) == t
            ref = list(T.adam_step(ref[0], grads[t - 1], ref[2], ref[3], ADAM['lr'], ADAM['b1'], ADAM['b2'], ADAM['eps'], t))
            for a, b in zip(dev, host):
                assert _within_ulps(a.check().cpu(), b.check().cpu(), t), t       # one ulp per chained step
        assert float((dev[0].cpu().double() - ref[0]).abs().max()) <= 3 * 40 * U * (1.0 + float(ref[0].abs().max()))
    finally:
        call('vqcpc_rng_salt_set', 0)
        torch.cuda.synchronize()


# =====================================================================================================================
# small exact kernels
MASK_SEEDS = (0x9E3779B97F4A7C15, 0x0123456700000001, 0xFFFFFFFF00000000)      # nonzero high words (checked on the CPU too)


@pytest.mark.parametrize('n', [1, 257, 100000])
def test_dropout_mask_equals_the_numpy_generator(n):
    for seed in MASK_SEEDS:
        for p in (0.0, 0.1, 0.5, 0.999):
            m = Guard(n)
            call('vqcpc_dropout_mask', m.view, n, p, seed)
            torch.cuda.synchronize()
            got = m.check().cpu()
            want = torch.from_numpy(T.dropout_keep(seed, n, p).astype(np.float32))
            assert same_bits(got, want), (n, hex(seed), p)
            if n == 100000 and p > 0:
                q = 1.0 - T.drop_threshold(p) / 2.0 ** 24
                assert abs(float(got.mean()) - q) <= 5.0 * math.sqrt(q * (1.0 - q) / n), (hex(seed), p, float(got.mean()))


CHECK_GRID_CAP = 2048 * 256                   # check_tokens launches at most 2048 workgroups of 256


@pytest.mark.parametrize('nv', [1, 4, 16])
@pytest.mark.parametrize('n', [1, 255, 257, CHECK_GRID_CAP + 1])
def test_check_tokens(nv, n):
    limits = [5 + 3 * v for v in range(nv)]                           # a different table size per voice
    lim_t = torch.tensor(limits, dtype=torch.int64)[torch.arange(n) % nv]
    g = gen(n + nv)
    good = (torch.rand(n, generator=g) * lim_t.double()).long().clamp_(max=lim_t - 1)
    good[-1] = lim_t[-1] - 1                                          # limit - 1 is inside
    if n > 1:
        good[0] = 0
    harr = (ctypes.c_int32 * nv)(*limits)

    def run(tok):
        out, flag = Guard(n, torch.int64), torch.zeros(1, dtype=torch.int32).cuda()
        call('vqcpc_check_tokens', tok.cuda(), n, nv, harr, out.view, flag)
        torch.cuda.synchronize()
        return out.check().cpu(), int(flag.cpu()[0])

    out, flag = run(good)
    assert torch.equal(out, good) and flag == 0, 'nothing to clamp: the copy is the input and the flag stays 0'
    for bad_value in (-1, None, 1 << 40):                            # None: the voice's limit itself
        tok = good.clone()
        tok[-1] = int(lim_t[-1]) if bad_value is None else bad_value   # a single id, in the last element
        out, flag = run(tok)
        assert torch.equal(out, torch.minimum(tok.clamp(min=0), lim_t - 1)) and flag == 1, (nv, n, bad_value)
    tok = good.clone()
    sel = torch.rand(n, generator=g) < 0.3
    tok[sel] = torch.tensor([-1, 1 << 40, 7, 1000, -(1 << 40)])[torch.randint(0, 5, (int(sel.sum()),), generator=g)]
    out, flag = run(tok)
    want = torch.minimum(tok.clamp(min=0), lim_t - 1)
    assert torch.equal(out, want) and flag == int(not torch.equal(want, tok))


@pytest.mark.parametrize('counts', [[], [257], [0], [0, 1, 255, 257, 5000, 20000, 1, 0], [5000, 257, 255, 1, 0, 3, 4, 64 * 256 + 1]])
def test_accumulate8(counts):
    g = gen(len(counts) + 1)
    nt = len(counts)
    src = [torch.randn(max(c, 1), generator=g) for c in counts]
    dst0 = [torch.randn(max(c, 1), generator=g) for c in counts]
    dst = [Guard(max(c, 1), data=d) for c, d in zip(counts, dst0)]
    srcd = [s.cuda() for s in src]
    pad = [0] * (8 - nt)
    call('vqcpc_accumulate8', (ctypes.c_void_p * 8)(*([d.view.data_ptr() for d in dst] + pad)),
         (ctypes.c_void_p * 8)(*([s.data_ptr() for s in srcd] + pad)), (ctypes.c_int * 8)(*(list(counts) + pad)), nt)
    torch.cuda.synchronize()
    for c, d, d0, s in zip(counts, dst, dst0, src):
        want = d0.clone()
        want[:c] = d0[:c] + s[:c]
        d.check(written=None)
        assert same_bits(d.cpu(), want), c


@pytest.mark.parametrize('f', [1, 8])
@pytest.mark.parametrize('d', [4, 36])
@pytest.mark.parametrize('rows', [1, 1000])
def test_upscale(rows, f, d):
    g = gen(rows + f + d)
    x, emb = torch.randn(rows, d, generator=g), torch.randn(f, d, generator=g)
    out = Guard((rows * f, d))
    call('vqcpc_upscale_fwd', x.cuda(), emb.cuda(), out.view, rows, f, d)
    torch.cuda.synchronize()
    assert same_bits(out.check().cpu(), T.upscale_fwd(x, emb, dtype=F32)), 'one fp32 addition per element: exact'
    go = torch.randn(rows * f, d, generator=g)
    wsb = query('vqcpc_upscale_bwd_workspace', rows, f, d)
    dx, de, ws = Guard((rows, d)), Guard((f, d)), Guard(max(wsb // 4, 1))
    call('vqcpc_upscale_bwd', go.cuda(), dx.view, de.view, rows, f, d, ws.view, wsb)
    torch.cuda.synchronize()
    ws.check(written=None)
    rx, re = T.upscale_bwd(go, f)
    ax, ae = T.upscale_bwd(go.abs(), f)
    # fp32 sums of f (dx) and of `rows` (d_emb) terms in some order: gamma_n sum |terms|, n the number of terms (Higham, lemma 3.1)
    assert bool(((dx.check().cpu().double() - rx).abs() <= f * U * ax + 2.0 ** -149).all())
    assert bool(((de.check().cpu().double() - re).abs() <= (rows + 16) * U * ae + 2.0 ** -149).all())


def test_rng_salt_advance_from_counter_and_set():
    n, p, seed, base = 1000, 0.5, 0x00C0FFEE00000011, 0x5EED

    def mask():
        m = Guard(n)
        call('vqcpc_dropout_mask', m.view, n, p, seed)
        torch.cuda.synchronize()
        return m.check().cpu()

    counter = torch.tensor([41], dtype=torch.int64).cuda()
    try:
        call('vqcpc_rng_salt_set', 0)
        plain = mask()
        assert same_bits(plain, torch.from_numpy(T.dropout_keep(seed, n, p).astype(np.float32)))
        call('vqcpc_rng_salt_advance', counter, base)
        salted = mask()
        assert int(counter.cpu()[0]) == 42, 'the counter must increment'
        assert not same_bits(salted, plain)
        salt = DR.splitmix64(base ^ 42) or 1
        assert same_bits(salted, torch.from_numpy(T.dropout_keep(seed ^ salt, n, p).astype(np.float32))), 'salt = splitmix64(base ^ counter)'
        call('vqcpc_rng_salt_set', 0)
        assert same_bits(mask(), plain), '_set(0) restores the unsalted mask'
        call('vqcpc_rng_salt_from_counter', counter, base)
        assert same_bits(mask(), salted) and int(counter.cpu()[0]) == 42, '_from_counter gives the same salt and leaves the counter'
    finally:
        call('vqcpc_rng_salt_set', 0)
        torch.cuda.synchronize()
    assert same_bits(mask(), plain)
