"""The three kernels of the EMA quantiser (csrc/vq.hip: vqcpc_vq_ema_stats, vqcpc_vq_commit_bwd, vqcpc_vq_ema_update) by direct
calls against the float64 references and the derived bounds of tests/vq_ema_reference.py.

Conventions (those of tests/test_train_kernels_gpu.py): outputs live in sentinel-filled allocations with guard elements on both
sides which must be bit-unchanged after the call; workspaces are NaN-poisoned; seeds are fixed.

Statistics: counts exact, sums within n u sum|z| per cell (order-free), two calls bit-identical.
Update: the bounds of vq_ema_reference.ema_bounds.
commit_bwd: not derived (a division and a square root in the non-squared form).  The yardstick is the SAME formula in plain fp32
torch on the CPU against float64: per case max over rows of max |d_z - d_z64| / rms(d_z64 of the row); the kernel passes when
its figure is <= C_DZ = 4 times plain fp32's, or every element is within 4 ulp (the rule and the constant of
tests/test_train_kernels_gpu.py).  Each case prints `DZ <label>: kernel .. plain .. ratio ..`; the measured ratios are in
profiles/vq_ema_perf_log.md.  In the squared form d_z must equal vqcpc_vq_bwd's bit for bit.
"""
import numpy as np
import pytest
import torch

import train_reference as T
import vq_ema_reference as E

pytestmark = pytest.mark.gpu

C_DZ = 4.0
PAD = 256
SENT_I32 = 0xDEADBEEF - (1 << 32)            # as fp32: -6.26e18, finite, never produced by these kernels
NAN = float('nan')
G, H, EPS = E.constants()

# (R, ncb, K, dsub): R around the 256-row chunk and over several chunks; dsub = 3 (odd), K = 3, K = 1; K * (1 + dsub) from 4 to
# 8704 cells; kgroups = 256 // (1 + dsub) both a power of two (dsub = 3) and not (4, 16, 64)
SHAPES = [(1, 1, 1, 3), (255, 2, 3, 4), (256, 1, 64, 16), (257, 2, 3, 3), (257, 1, 64, 64), (513, 4, 64, 16), (513, 2, 512, 16),
          (513, 4, 3, 64), (255, 1, 512, 4)]


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


def call(name, *args):
    from vqcpc_bach_amd import hip
    hip.call(name, *args)


def query(name, *args):
    from vqcpc_bach_amd import hip
    return hip.query(name, *args)


def bits(t):
    return t.contiguous().view(torch.int32)


class Guard:
    """A contiguous fp32 tensor of `shape` inside a sentinel-filled allocation with PAD guard elements before and after."""

    def __init__(self, shape, data=None):
        self.n = int(np.prod(shape))
        self.full = torch.full((self.n + 2 * PAD,), SENT_I32, dtype=torch.int32, device='cuda').view(torch.float32)
        self.view = self.full[PAD:PAD + self.n].view(shape)
        if data is not None:
            self.view.copy_(torch.as_tensor(data, dtype=torch.float32).reshape(shape))
        self.before = self.full.clone()

    def check(self, written=True):
        f, b = bits(self.full), bits(self.before)
        assert torch.equal(f[:PAD], b[:PAD]) and torch.equal(f[PAD + self.n:], b[PAD + self.n:]), 'guard overwritten'
        if written:
            assert not bool((f[PAD:PAD + self.n] == SENT_I32).any()), 'an output element was never written'
        else:
            assert torch.equal(f, b), 'an output that must stay untouched was written'
        return self.view


def nan_workspace(nbytes):
    return torch.full((max(nbytes // 4, 4) + PAD,), NAN, dtype=torch.float32, device='cuda')


def case(R, ncb, K, dsub, seed=0):
    g = torch.Generator().manual_seed(1000 + 7 * R + 3 * K + dsub + seed)
    z = torch.randn(R, ncb * dsub, generator=g)
    cb = torch.randn(ncb, K, dsub, generator=g)
    idx = torch.randint(0, K, (R, ncb), generator=g)
    g_zq = torch.randn(R, ncb * dsub, generator=g)
    g_loss = torch.randn(R, generator=g)
    return z, cb, idx, g_zq, g_loss


def run_stats(z, idx, K):
    R, D = z.shape
    ncb = idx.shape[1]
    dsub = D // ncb
    out = Guard((ncb, K, dsub + 1))
    nbytes = query('vqcpc_vq_ema_stats_workspace', R, ncb, K, dsub)
    assert nbytes == -(-R // 256) * ncb * K * (dsub + 1) * 4
    ws = nan_workspace(nbytes)
    call('vqcpc_vq_ema_stats', z.cuda(), idx.cuda(), R, ncb, K, dsub, out.view, ws, nbytes)
    torch.cuda.synchronize()
    return out


def check_stats(out, z, idx, K):
    st = out.check().cpu().double()
    n, s, a = E.stats(z, idx, K)
    assert torch.equal(st[..., 0], n), 'counts must be exact'
    err, bound = (st[..., 1:] - s).abs(), E.sum_bound(n, a)
    assert bool((err <= bound).all()), float((err - bound).max())
    empty = n == 0
    assert bool((st[..., 1:][empty] == 0).all()) and not bool(torch.signbit(st[..., 1:][empty]).any()), 'empty codes: sum +0.0'
    return st


# =====================================================================================================================
@pytest.mark.parametrize('R,ncb,K,dsub', SHAPES)
def test_statistics(R, ncb, K, dsub):
    z, _, idx, _, _ = case(R, ncb, K, dsub)
    a = run_stats(z, idx, K)
    check_stats(a, z, idx, K)
    b = run_stats(z, idx, K)
    assert torch.equal(bits(a.view), bits(b.view)), 'two calls must be bit-identical'


def test_statistics_every_row_on_one_code_and_empty_codes():
    R, ncb, K, dsub = 513, 2, 64, 16
    z = case(R, ncb, K, dsub, seed=1)[0]
    idx = torch.full((R, ncb), 5, dtype=torch.int64)
    idx[:, 1] = 63
    st = check_stats(run_stats(z, idx, K), z, idx, K)
    assert float(st[0, 5, 0]) == R and float(st[1, 63, 0]) == R and float(st[..., 0].sum()) == 2 * R
    assert int((st[..., 0] == 0).sum()) == 2 * (K - 1)


def test_statistics_skip_indices_outside_the_codebook():
    R, ncb, K, dsub = 300, 2, 3, 4
    z, _, idx, _, _ = case(R, ncb, K, dsub, seed=2)
    idx[7, 0], idx[256, 1], idx[299, 0] = K, -1, 1 << 40
    st = check_stats(run_stats(z, idx, K), z, idx, K)
    assert float(st[..., 0].sum()) == 2 * R - 3


@pytest.mark.parametrize('R,ncb,K,dsub,needle', [(10, 1, 4, 256, 'columns'), (10, 1, 4096, 16, 'LDS'), (10, 2, 640, 63, 'LDS')])
def test_statistics_refusals_launch_nothing(R, ncb, K, dsub, needle):
    from vqcpc_bach_amd import hip
    z = torch.zeros(R, ncb * dsub, device='cuda')
    idx = torch.zeros(R, ncb, dtype=torch.int64, device='cuda')
    out = Guard((8,))
    ws = nan_workspace(64)
    with pytest.raises(hip.VqcpcHipError, match=needle):
        call('vqcpc_vq_ema_stats', z, idx, R, ncb, K, dsub, out.view, ws, 1 << 40)
    torch.cuda.synchronize()
    out.check(written=False)
    assert bool(torch.isnan(ws).all())


# =====================================================================================================================
@pytest.mark.parametrize('squared', [1, 0])
@pytest.mark.parametrize('R,ncb,K,dsub', SHAPES)
def test_commit_bwd(R, ncb, K, dsub, squared):
    z, cb, idx, g_zq, g_loss = case(R, ncb, K, dsub, seed=3)
    beta = 0.25
    dev = [t.cuda() for t in (z, cb, idx, g_zq, g_loss)]
    out = Guard((R, ncb * dsub))
    call('vqcpc_vq_commit_bwd', *dev, R, ncb, K, dsub, beta, squared, out.view)
    torch.cuda.synchronize()
    got = out.check().cpu()
    ref = E.d_z(z, cb, idx, g_zq, g_loss, beta, squared)
    plain = E.d_z(z, cb, idx, g_zq, g_loss, beta, squared, dtype=torch.float32)
    ek, ep = float(T.row_err(got, ref).max()), float(T.row_err(plain, ref).max())
    ulp = torch.from_numpy(np.spacing(np.maximum(ref.abs().float().numpy(), np.float32(2.0 ** -126))).astype(np.float64))
    within4 = bool(((got.double() - ref).abs() <= 4.0 * ulp).all())
    ratio = ek / ep if ep > 0 else (0.0 if ek == 0 else float('inf'))
    print(f'DZ R{R}_ncb{ncb}_K{K}_d{dsub}_sq{squared}: kernel {ek:.3e} plain {ep:.3e} ratio {ratio:.2f}')
    assert bool(torch.isfinite(got).all())
    assert ratio <= C_DZ or within4, (ek, ep, ratio)
    if squared:
        dz2, dcb = Guard((R, ncb * dsub)), Guard((ncb, K, dsub))
        nbytes = query('vqcpc_vq_bwd_workspace', R, ncb, K, dsub)
        call('vqcpc_vq_bwd', *dev, R, ncb, K, dsub, beta, squared, dz2.view, dcb.view, nan_workspace(nbytes), nbytes)
        torch.cuda.synchronize()
        assert torch.equal(bits(out.view), bits(dz2.check())), 'squared form: d_z must equal vqcpc_vq_bwd bit for bit'


# =====================================================================================================================
def run_update(N, m, e, n, s):
    ncb, K, dsub = m.shape
    st = torch.cat([n.unsqueeze(-1), s], dim=-1).contiguous().cuda()
    gN, gm, ge = Guard((ncb, K), N), Guard((ncb, K, dsub), m), Guard((ncb, K, dsub), e)
    call('vqcpc_vq_ema_update', st, gN.view, gm.view, ge.view, ncb, K, dsub, G, H, EPS)
    torch.cuda.synchronize()
    return gN.check().cpu(), gm.check().cpu(), ge.check().cpu()


@pytest.mark.parametrize('dsub', [3, 16])
@pytest.mark.parametrize('K', [1, 3, 512])
def test_update_within_the_derived_bounds(K, dsub):
    ncb = 2
    g = torch.Generator().manual_seed(50 + K + dsub)
    N = (torch.rand(ncb, K, generator=g) * 40).float()
    m = (torch.randn(ncb, K, dsub, generator=g) * N.unsqueeze(-1)).float()
    n = torch.randint(0, 200, (ncb, K), generator=g).float()
    n[:, ::3] = 0                                                   # unused codes
    s = (torch.randn(ncb, K, dsub, generator=g) * n.unsqueeze(-1)).float()
    e_old = torch.randn(ncb, K, dsub, generator=g)                  # must be overwritten, never read
    N1, m1, e1 = run_update(N, m, e_old, n, s)
    rN, rm, re = E.update(N, m, n, s, G, H, EPS)
    bN, bm, be = E.ema_bounds(N, m, n, s, G, H, EPS)
    for name, got, ref, bound in (('N', N1, rN, bN), ('m', m1, rm, bm), ('e', e1, re, be)):
        err = (got.double() - ref).abs()
        print(f'UPDATE K{K}_d{dsub} {name}: max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
        assert bool((err <= bound).all()), (name, float((err - bound).max()))
    unused = n == 0
    f = np.float32
    assert np.array_equal(N1.numpy()[unused.numpy()], (f(G) * N.numpy())[unused.numpy()]), 'unused codes: N shrinks by exactly g'
    assert np.array_equal(m1.numpy()[unused.numpy()], (f(G) * m.numpy())[unused.numpy()]), 'unused codes: m shrinks by exactly g'
    assert bool(torch.isfinite(e1).all())


@pytest.mark.parametrize('K', [1, 3, 512])
def test_update_without_data_keeps_the_initial_codebook(K):
    """From N = 1, m = e an update with n = 0, s = 0 leaves e unchanged within the bound (exactly so in exact arithmetic)."""
    ncb, dsub = 2, 4
    e0 = torch.randn(ncb, K, dsub, generator=torch.Generator().manual_seed(60 + K)).float()
    N, n, s = torch.ones(ncb, K), torch.zeros(ncb, K), torch.zeros(ncb, K, dsub)
    N1, m1, e1 = run_update(N, e0, e0.clone(), n, s)
    be = E.ema_bounds(N, e0, n, s, G, H, EPS)[2]
    assert bool(((e1.double() - e0.double()).abs() <= be).all())
    assert bool((N1 == np.float32(G)).all()) and np.array_equal(m1.numpy(), np.float32(G) * e0.numpy())
