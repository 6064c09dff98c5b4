"""The kernels of the aligned ("diagonal") cross block (csrc/aligned.hip) one by one, by direct calls, against the float64
references of tests/aligned_reference.py.

Conventions (those of tests/test_train_kernels_gpu.py): outputs live in sentinel-filled allocations with guard elements on
both sides, which must be bit-unchanged after the call; every input the result must not depend on is NaN, so a NaN in an
output is a wrong read; seeds are fixed.

Bounds.  Expand is a copy and the step add ONE fp32 add: compared bit for bit.  Reduce sums epc terms sequentially in fp32:
|out - ref64| <= (epc - 1) * 2^-24 * sum_e |term| + 2^-24 |ref64| (one relative rounding per addition, each partial sum bounded
by the sum of the magnitudes, plus the final rounding of the comparison), and it must be bit-identical between two runs and
between n = 1 and the same rows inside n = 3.  ELU forward and backward evaluate expm1 / exp in double and round once, as
util.hip's SELU forward does, and take its bound: 4 * 2^-24 |ref64| + one fp32 denormal.  Every case prints its measured
maximum as a fraction of the bound; the maxima are in profiles/decoder_aligned_perf_log.md.
"""
import numpy as np
import pytest
import torch

import aligned_reference as A

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
PAD = 256
SENT_I32 = 0xDEADBEEF - (1 << 32)            # as fp32: -6.26e18, finite, never produced by these kernels
NAN = float('nan')
VOICES = [(1, 1), (1, 4), (4, 1), (4, 4), (3, 2)]                    # (nc, epc)
DIMS = [4, 32, 252, 260, 5]                                           # 5: no vector path anywhere
BATCHES = [(1, 1), (1, 3), (3, 1), (3, 3)]                            # (n, S)


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


def call(name, *args):
    from vqcpc_bach_amd import hip
    hip.call(name, *args)


def bits(t):
    return t.contiguous().view(torch.int32)


class Guard:
    """A contiguous fp32 tensor of `shape` inside a sentinel-filled allocation with PAD guard elements before and after."""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.full = torch.full((self.n + 2 * PAD,), SENT_I32, dtype=torch.int32, device='cuda').view(torch.float32)
        self.view = self.full[PAD:PAD + self.n].view(shape)
        self.before = self.full.clone()

    def check(self, written=True):
        f, b = bits(self.full), bits(self.before)
        assert torch.equal(f[:PAD], b[:PAD]) and torch.equal(f[PAD + self.n:], b[PAD + self.n:]), 'guard overwritten'
        if not written:
            assert torch.equal(f, b), 'an output that must stay untouched was written'
        elif self.n:
            assert not bool((f[PAD:PAD + self.n] == SENT_I32).any()), 'an output element was never written'
        return self.view.cpu()


def rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# =====================================================================================================================
@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('nc,epc', VOICES)
def test_expand(nc, epc, d):
    U = nc * epc
    for n, S in BATCHES:
        T = S * U
        C = rnd((n * S, nc * d), 11 * d + nc)
        for P in sorted({0, 1, U - 1, min(U + 1, T), T}):
            used = -(-P // U)
            Cp = C.clone().view(n, S, nc * d)
            Cp[:, used:] = NAN                                          # codes past the prefix are never read
            out = Guard((n * P, d))
            call('vqcpc_aligned_expand', Cp.cuda(), out.view, n, S, P, U, nc, d)
            torch.cuda.synchronize()
            o = out.check(written=P > 0)
            ref = torch.from_numpy(A.expand(C.numpy(), n, S, P, U, nc, dtype=np.float32))
            assert same(o, ref), (n, S, P)


@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('nc,epc', VOICES)
def test_reduce(nc, epc, d):
    U = nc * epc
    worst = 0.0
    per_n = {}
    for n, S in BATCHES:
        G = rnd((3 * S * U, d), 13 * d + epc)[:n * S * U] * 3.0           # n = 1 is sequence 0 of n = 3
        runs = []
        for _ in range(2):
            out = Guard((n * S, nc * d))
            call('vqcpc_aligned_reduce', G.cuda(), out.view, n, S, U, nc, d)
            torch.cuda.synchronize()
            runs.append(out.check())
        assert same(runs[0], runs[1]), 'two runs differ'
        per_n[(n, S)] = runs[0]
        ref = A.reduce(G.numpy(), n, S, U, nc)
        bound = (epc - 1) * U24 * A.reduce_abs(G.numpy(), n, S, U, nc) + U24 * np.abs(ref)
        err = np.abs(runs[0].double().numpy() - ref)
        assert np.isfinite(runs[0].numpy()).all()
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (n, S, float((err / bound).max()))
        if epc == 1:
            assert same(runs[0], torch.from_numpy(ref.astype(np.float32))), 'epc = 1 is a transposed copy'
    for S in (1, 3):
        assert same(per_n[(1, S)], per_n[(3, S)][:S]), 'a sequence alone differs from the same rows inside n = 3'
    print(f'REDUCE nc{nc} epc{epc} d{d}: max err / bound = {worst:.3f}')


# =====================================================================================================================
def _elu_inputs(n):
    grid = torch.logspace(-7, np.log10(30.0), 1200, dtype=torch.float64)
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, -88.0, 88.0, 1e-40, -1e-40, -1e-7, 1e-7, -1.0, 1.0], dtype=torch.float64)
    full = torch.cat([special, torch.stack([-grid, grid], 1).reshape(-1)]).float()
    if n <= full.numel():
        return full[:n]
    return torch.cat([full, rnd(n - full.numel(), n) * 3.0])


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('n', [1, 12, 255, 1027, 3 * 64 * 17 + 2])
def test_elu(n, offset):
    """offset = 1: pointers that are not 16-byte aligned (scalar path); n % 4 != 0: the scalar tail."""
    x = _elu_inputs(n)
    assert x.numel() == n and (n < 12 or bool((x.abs() < 1e-38).any() and (x == -88.0).any() and (x == 88.0).any()))
    g = rnd(n, n + 5)
    xd = torch.cat([torch.full((offset,), NAN), x]).cuda()[offset:]
    gd = torch.cat([torch.full((offset,), NAN), g]).cuda()[offset:]
    assert xd.data_ptr() % 16 == 4 * offset
    y = Guard(n + offset)
    call('vqcpc_elu_fwd', xd, y.view[offset:], n)
    torch.cuda.synchronize()
    assert bits(y.view[:offset]).eq(SENT_I32).all()
    o = y.view[offset:].cpu()
    y.view[:offset].copy_(y.view[offset:offset + 1].expand(offset))     # so that check() sees every element written
    y.check()
    ref = A.elu(x.numpy())
    bound = 4.0 * U24 * np.abs(ref) + 2.0 ** -149
    err = np.abs(o.double().numpy() - ref)
    worst_f = float((err / bound).max())
    print(f'ELU fwd n{n} offset{offset}: max err / bound = {worst_f:.3f}')
    assert np.isfinite(o.numpy()).all() and (err <= bound).all(), (worst_f, x[torch.from_numpy(err > bound)][:5])
    gx = Guard(n + offset)
    call('vqcpc_elu_bwd', xd, gd, gx.view[offset:], n)
    torch.cuda.synchronize()
    assert bits(gx.view[:offset]).eq(SENT_I32).all()
    o = gx.view[offset:].cpu()
    gx.view[:offset].copy_(gx.view[offset:offset + 1].expand(offset))
    gx.check()
    ref = A.elu_grad(x.numpy(), g.numpy())
    bound = 4.0 * U24 * np.abs(ref) + 2.0 ** -149
    err = np.abs(o.double().numpy() - ref)
    worst_b = float((err / bound).max())
    print(f'ELU bwd n{n} offset{offset}: max err / bound = {worst_b:.3f}')
    assert np.isfinite(o.numpy()).all() and (err <= bound).all(), (worst_b, x[torch.from_numpy(err > bound)][:5])
    pos = x > 0
    assert same(o[pos], g[pos]), 'x > 0 passes the gradient through unchanged'


# =====================================================================================================================
@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('nc,epc', VOICES)
def test_step_add(nc, epc, d):
    U = nc * epc
    for M, S in BATCHES:
        T = S * U
        C = rnd((M * S, nc * d), 17 * d + nc)
        h = rnd((M, d), 19 * d + epc)
        ldh = d + 4
        hd = torch.full((M, ldh), NAN)
        hd[:, :d] = h
        hd = hd.cuda()
        pos = torch.zeros(1, dtype=torch.int32, device='cuda')
        for p in sorted({0, U - 1, min(U, T - 1), T - 1}):
            Cp = torch.full((M, S, d, nc), NAN)                          # only this code's row, this voice's columns are read
            Cp[:, p // U, :, p % nc] = C.view(M, S, d, nc)[:, p // U, :, p % nc]
            pos.fill_(p)
            s = Guard((M, d))
            call('vqcpc_decode_aligned_add', hd, ldh, Cp.view(M * S, nc * d).cuda(), s.view, d, pos, M, S, U, nc, d)
            torch.cuda.synchronize()
            ref = torch.from_numpy(A.step_add(h.numpy(), C.numpy(), p, S, U, nc, dtype=np.float32))
            assert same(s.check(), ref), (M, S, p)
        for p in (T, -1):                                                # past the end: nothing is written
            pos.fill_(p)
            s = Guard((M, d))
            call('vqcpc_decode_aligned_add', hd, ldh, C.cuda(), s.view, d, pos, M, S, U, nc, d)
            torch.cuda.synchronize()
            s.check(written=False)


def test_arguments_are_validated():
    from vqcpc_bach_amd import hip
    x = torch.zeros(64, device='cuda')
    with pytest.raises(hip.VqcpcHipError, match='aligned_expand'):
        call('vqcpc_aligned_expand', x, x, 1, 1, 5, 4, 4, 4)             # P > S * U
    with pytest.raises(hip.VqcpcHipError, match='aligned_reduce'):
        call('vqcpc_aligned_reduce', x, x, 1, 1, 6, 4, 4)                # U % nc != 0
    with pytest.raises(hip.VqcpcHipError, match='aligned_expand'):
        call('vqcpc_aligned_expand', x, x, 1, 1, 4, 4, 4, 8192)          # nc * d beyond the LDS row
