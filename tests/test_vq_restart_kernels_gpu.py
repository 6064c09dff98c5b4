"""The two kernels of the dead-code restarts (csrc/vq.hip: vqcpc_vq_restart_candidates, vqcpc_vq_ema_restart) by direct calls
against tests/vq_restart_reference.py.  Both copy rows and set constants: every comparison is on the bits.  Outputs live in
allocations with guard elements on both sides which must be bit-unchanged after the call."""
import itertools

import numpy as np
import pytest
import torch

import vq_restart_reference as Rr

pytestmark = pytest.mark.gpu

PAD = 256
SENT_I32 = 0xDEADBEEF - (1 << 32)


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
    """A contiguous 4-byte tensor of `shape` in the middle of an allocation: PAD sentinel elements before and after it, the
    tensor itself filled with `data` or, without data, with NaN."""

    def __init__(self, shape, data=None, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.full = torch.full((self.n + 2 * PAD,), SENT_I32, dtype=torch.int32, device='cuda').view(dtype)
        self.view = self.full[PAD:PAD + self.n].view(shape)
        if data is None:
            self.view.fill_(float('nan'))
        else:
            self.view.copy_(torch.as_tensor(data, dtype=dtype).reshape(shape))
        self.before = self.full.clone()

    def check(self, untouched=False):
        f, b = bits(self.full), bits(self.before)
        assert torch.equal(f[:PAD], b[:PAD]) and torch.equal(f[PAD + self.n:], b[PAD + self.n:]), 'guard overwritten'
        if untouched:
            assert torch.equal(f, b), 'an output that must stay untouched was written'
        return self.view


def run_candidates(z_dev, ncb, K, dsub, seed, step, rank, world, step_dev=None):
    out = Guard((ncb, K, dsub))
    call('vqcpc_vq_restart_candidates', z_dev, z_dev.shape[0], ncb, K, dsub, seed, step, step_dev, rank, world, out.view)
    torch.cuda.synchronize()
    got = out.check().cpu().numpy()
    assert not np.isnan(got).any(), 'every element of cand is written'
    return got


SEED, STEP = 0xFEDCBA9876543210, 12


def test_candidates_equal_the_reference_bit_for_bit():
    """R x K x ncb x dsub x (world, rank), 288 launches: one lane per element, so K dsub ncb from 1 (one lane of one wave) to
    33792 (132 workgroups), with dsub = 33 and K = 5 no multiple of anything."""
    for R, ncb, dsub in itertools.product((1, 3, 257), (1, 2), (1, 4, 16, 33)):
        g = torch.Generator().manual_seed(100 * R + 10 * ncb + dsub)
        zs = [torch.randn(R, ncb * dsub, generator=g) for _ in range(3)]
        zs[0][0, 0] = -0.0                                          # a copied -0.0 keeps its sign; an unowned cell is +0.0
        zs_dev = [z.cuda() for z in zs]
        for K in (1, 5, 512):
            refs = {1: Rr.candidates([zs[0].numpy()], SEED, STEP, ncb, K), 3: Rr.candidates([z.numpy() for z in zs], SEED, STEP, ncb, K)}
            for world, rank in ((1, 0), (3, 0), (3, 1), (3, 2)):
                got = run_candidates(zs_dev[rank], ncb, K, dsub, SEED, STEP, rank, world)
                assert got.tobytes() == refs[world][rank].tobytes(), (R, ncb, dsub, K, world, rank)


def test_device_counter_form_equals_the_host_form_and_steps_differ():
    R, ncb, K, dsub = 257, 2, 512, 16
    z = torch.randn(R, ncb * dsub, generator=torch.Generator().manual_seed(1))
    zd = z.cuda()
    host = {t: run_candidates(zd, ncb, K, dsub, SEED, t, 1, 3) for t in (1, 2, (1 << 40) + 5)}
    for t, want in host.items():
        assert want.tobytes() == Rr.candidates([z.numpy()] * 3, SEED, t, ncb, K)[1].tobytes()
        counter = torch.tensor([t], dtype=torch.int64).cuda()
        got = run_candidates(zd, ncb, K, dsub, SEED, 999, 1, 3, step_dev=counter)        # the host value is ignored
        assert got.tobytes() == want.tobytes(), t
        assert int(counter[0]) == t, 'the counter is read, never written'
    assert host[1].tobytes() != host[2].tobytes(), 'two steps draw different rows'
    other_seed = run_candidates(zd, ncb, K, dsub, SEED + 1, 1, 1, 3)
    assert other_seed.tobytes() != host[1].tobytes()


# =====================================================================================================================
@pytest.mark.parametrize('dsub', [1, 33])
@pytest.mark.parametrize('K', [1, 5, 512, 513])
def test_restart_rule(K, dsub):
    """N below, equal to and above the threshold in the same codebook (K = 1: one of them per codebook); K = 513 = two full
    workgroups of four waves + one lane, K = 5 a partial first wave: the count must include the partial last wave."""
    ncb, thr = 2, 0.5
    rng = np.random.RandomState(K + dsub)
    kinds = np.arange(ncb * K).reshape(ncb, K) % 4              # K = 1: codebook 0 below, codebook 1 equal
    below = np.where(rng.rand(ncb, K) < 0.5, np.float32(0.1), np.nextafter(np.float32(thr), np.float32(0)))
    N = np.select([kinds == 0, kinds == 1, kinds == 2], [below, np.float32(thr), np.float32(0.9)], np.float32(37.5)).astype(np.float32)
    N[-1, -1] = 0.0 if K > 1 else N[-1, -1]                      # the very last lane of the launch is dead too
    m, e, cand = (rng.randn(ncb, K, dsub).astype(np.float32) for _ in range(3))
    start = np.array([7, 1000], dtype=np.int32)
    gN, gm, ge = Guard((ncb, K), N), Guard((ncb, K, dsub), m), Guard((ncb, K, dsub), e)
    gc, gr = Guard((ncb, K, dsub), cand), Guard((ncb,), start, dtype=torch.int32)
    call('vqcpc_vq_ema_restart', gc.view, gN.view, gm.view, ge.view, ncb, K, dsub, thr, gr.view)
    torch.cuda.synchronize()
    gc.check(untouched=True)
    rN, rm, re, cnt = Rr.restart(cand, N, m, e, thr)
    assert int(cnt.sum()) > 0
    dead = N < np.float32(thr)
    assert not dead[N == np.float32(thr)].any() and np.array_equal(dead.sum(1), cnt)
    for name, guard, ref, old, new in (('N', gN, rN, N, None), ('m', gm, rm, m, cand), ('e', ge, re, e, cand)):
        got = guard.check().cpu().numpy()
        assert got.tobytes() == ref.tobytes(), name
        assert got[~dead].tobytes() == old[~dead].tobytes(), f'{name}: untouched cells keep their bits'
        if new is not None:
            assert got[dead].tobytes() == new[dead].tobytes()
    assert bool((gN.view.cpu().numpy()[dead] == 1.0).all())
    assert gr.check().cpu().numpy().tolist() == (start + cnt).tolist(), 'the counter accumulates, exactly'
    # a second launch on the restarted state restarts nothing (N = 1 >= thr) and leaves the counter alone
    call('vqcpc_vq_ema_restart', gc.view, gN.view, gm.view, ge.view, ncb, K, dsub, thr, gr.view)
    torch.cuda.synchronize()
    assert gr.check().cpu().numpy().tolist() == (start + cnt).tolist() and gN.check().cpu().numpy().tobytes() == rN.tobytes()


def test_zero_threshold_changes_nothing():
    ncb, K, dsub = 2, 300, 4
    rng = np.random.RandomState(0)
    N = rng.rand(ncb, K).astype(np.float32)
    N[0, :5] = 0.0
    gs = [Guard((ncb, K), N)] + [Guard((ncb, K, dsub), rng.randn(ncb, K, dsub)) for _ in range(3)]
    gr = Guard((ncb,), [3, 4], dtype=torch.int32)
    call('vqcpc_vq_ema_restart', gs[3].view, gs[0].view, gs[1].view, gs[2].view, ncb, K, dsub, 0.0, gr.view)
    torch.cuda.synchronize()
    for g in gs + [gr]:
        g.check(untouched=True)


def test_refusals_launch_nothing():
    from vqcpc_bach_amd import hip
    z = torch.zeros(4, 8, device='cuda')
    out = Guard((2, 3, 4))
    for R, rank, world, needle in ((4, 0, 0, 'rank'), (4, -1, 2, 'rank'), (4, 2, 2, 'rank'), (1 << 30, 0, 2, '2\\^31'),
                                   ((1 << 31) - 1, 0, 2, '2\\^31'), (1 << 31, 0, 1, '2\\^31')):
        with pytest.raises(hip.VqcpcHipError, match=needle):
            call('vqcpc_vq_restart_candidates', z, R, 2, 3, 4, 0, 1, None, rank, world, out.view)
    gN, gm, ge, gr = Guard((2, 3), np.zeros((2, 3))), Guard((2, 3, 4)), Guard((2, 3, 4)), Guard((2,), [0, 0], dtype=torch.int32)
    with pytest.raises(hip.VqcpcHipError, match='negative'):
        call('vqcpc_vq_ema_restart', out.view, gN.view, gm.view, ge.view, 2, 3, 4, -0.5, gr.view)
    torch.cuda.synchronize()
    for g in (out, gN, gm, ge, gr):
        g.check(untouched=True)
