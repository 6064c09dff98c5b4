"""vqcpc_product_gather and vqcpc_product_gather_bwd (csrc/product_codes.hip) by direct calls and through ops.ProductEmbeddingFn,
against tests/product_codes_reference.py.

Gather: BIT-equal to the numpy fp32 chain (same adds in the same order; the first link is a copy).  Outputs live in a
sentinel-filled allocation with guard elements on both sides and guard columns [C, ldo); table rows and extra rows no index refers
to are NaN-poisoned, so a read of a wrong row shows.
Backward: against the float64 segment sums within product_codes_reference.sum_bound = n u sum|g| per element (n summands of a
cell, added in ascending m from an exact first add: at most n - 1 roundings each, the bound of tests/vq_ema_reference.py); cells
nobody refers to exactly 0; two runs bit-identical; d res is the incoming gradient's bits."""
import numpy as np
import pytest
import torch

import product_codes_reference as R

pytestmark = pytest.mark.gpu

PAD = 64
SENT = 0xDEADBEEF - (1 << 32)                # as fp32: -6.26e18, finite, never produced by these kernels
SHAPES = [(1, 1), (1, 5), (2, 3), (3, 4), (4, 8), (2, 512), (2, 4096)]
CASES = [(ncb, K, C) for ncb, K in SHAPES for C in ((4,) if K == 4096 else (36, 256, 260, 512))]
ROWS = (1, 2, 63, 257)


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


def _indices(pattern, M, lo, hi, rng):
    """M indices in [lo, hi): all equal, consecutive (wrapping), or random."""
    if pattern == 'equal':
        return np.full(M, lo + (hi - lo) * 2 // 3, dtype=np.int64)
    if pattern == 'arange':
        return lo + (np.arange(M, dtype=np.int64) * max((hi - lo) // max(M, 1), 1) + (hi - lo) // 2) % (hi - lo)
    return rng.integers(lo, hi, M)


def _poisoned(tables, extra, idx, nj):
    """Copies with NaN in every table row / extra row that the gather of `idx` must not read."""
    ncb, K, _ = tables.shape
    V = K ** ncb
    t = np.full_like(tables, np.nan)
    dig = R.digits(idx[idx < V], ncb, K)
    for j in range(nj):
        t[j, dig[j]] = tables[j, dig[j]]
    e = None
    if extra is not None:
        e = np.full_like(extra, np.nan)
        e[idx[idx >= V] - V] = extra[idx[idx >= V] - V]
    return t, e


def _gather(tables, idx, nj, res, extra, ldo):
    """One direct call on poisoned inputs; returns the (M, C) output after the guard checks."""
    from vqcpc_bach_amd import hip
    ncb, K, C = tables.shape
    M = len(idx)
    t, e = _poisoned(tables, extra, idx, nj)
    full = torch.full((M * ldo + 2 * PAD,), SENT, dtype=torch.int32, device='cuda')
    out = full[PAD:PAD + M * ldo].view(torch.float32)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    hip.call('vqcpc_product_gather', dev(t), dev(idx), dev(res), C, dev(e), 0 if extra is None else len(extra), out, ldo, M, ncb, K,
             nj, C)
    got = full.cpu()
    assert bool((got[:PAD] == SENT).all()) and bool((got[PAD + M * ldo:] == SENT).all()), 'guard overwritten'
    body = got[PAD:PAD + M * ldo].view(M, ldo)
    assert bool((body[:, C:] == SENT).all()), 'a column in [C, ldo) was written'
    return body[:, :C].contiguous().view(torch.float32).numpy()


@pytest.mark.parametrize('ncb,K,C', CASES)
def test_gather_is_bit_equal_to_the_fp32_chain(ncb, K, C):
    rng = np.random.default_rng(1000 * ncb + K + C)
    V = K ** ncb
    tables = rng.standard_normal((ncb, K, C)).astype(np.float32)
    extra = rng.standard_normal((3, C)).astype(np.float32)
    for M in ROWS:
        res = rng.standard_normal((M, C)).astype(np.float32)
        for pattern in ('equal', 'arange', 'random'):
            codes = _indices(pattern, M, 0, V, rng)
            sos = _indices(pattern, M, V, V + 3, rng)
            mixed = np.where(rng.random(M) < 0.4, sos, codes)
            variants = [(codes, ncb, None, None, C), (codes, ncb, res, None, C), (codes, ncb, None, None, C + 8),
                        (codes, ncb, None, extra, C), (sos, ncb, None, extra, C + 4), (mixed, ncb, None, extra, C)]
            if ncb > 1:
                variants += [(codes, nj, r, None, C) for nj in range(1, ncb) for r in (None, res)]
                variants += [(mixed, ncb - 1, None, extra, C)]
            for idx, nj, r, ex, ldo in variants:
                want = R.gather(tables, idx, nj=nj, res=r, extra=ex)
                got = _gather(tables, idx, nj, r, ex, ldo)
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (M, pattern, nj, r is not None, ex is not None, ldo)
    # one digit, no residual: a bit-exact row copy, whatever the bits are (a NaN payload, -0.0, a subnormal)
    odd = tables.copy()
    odd.view(np.int32)[0, :, 0] = 0x7FC12345
    odd[0, :, 1], odd[0, :, 2] = -0.0, 1e-41
    idx = _indices('random', 63, 0, V, rng)
    assert np.array_equal(_gather(odd, idx, 1, None, None, C).view(np.int32), odd[0][idx % K].view(np.int32))


def _backward(tables, extra, idx, nj, res, g):
    from vqcpc_bach_amd import ops
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(True)
    t, e, r = dev(tables), dev(extra), dev(res)
    out = ops.ProductEmbeddingFn.apply(t, e, torch.from_numpy(idx).cuda(), nj, r)
    out.backward(torch.from_numpy(g).cuda())
    return t.grad.cpu().numpy(), None if e is None else e.grad.cpu().numpy(), None if r is None else r.grad.cpu().numpy()


@pytest.mark.parametrize('ncb,K,C', CASES)
def test_backward_sums_within_the_derived_bound(ncb, K, C):
    rng = np.random.default_rng(2000 * ncb + K + C)
    V = K ** ncb
    tables = rng.standard_normal((ncb, K, C)).astype(np.float32)
    extra = rng.standard_normal((2, C)).astype(np.float32)
    worst = 0.0
    for M in ROWS:
        g = (rng.standard_normal((M, C)) * np.exp(rng.standard_normal((M, 1)))).astype(np.float32)
        res = rng.standard_normal((M, C)).astype(np.float32)
        for pattern in ('equal', 'arange', 'random'):       # 'equal': ONE segment of M rows per codebook, the longest
            codes = _indices(pattern, M, 0, V, rng)
            mixed = np.where(rng.random(M) < 0.4, _indices(pattern, M, V, V + 2, rng), codes)
            for idx, nj, r, ex in ((codes, ncb, None, None), (codes, max(ncb - 1, 1), res, None), (mixed, ncb, None, extra),
                                   (np.full(M, V + 1, dtype=np.int64), ncb, None, extra)):
                d_t, d_e, d_r = _backward(tables, ex, idx, nj, r, g)
                again = _backward(tables, ex, idx, nj, r, g)
                n_extra = 0 if ex is None else len(ex)
                ref_t, ref_e, (n_t, a_t), (n_e, a_e) = R.segment_sums(g, idx, ncb, K, nj=nj, n_extra=n_extra)
                err = np.abs(d_t.astype(np.float64) - ref_t)
                assert (err <= R.sum_bound(n_t, a_t)).all(), (M, pattern, nj, float(err.max()))
                assert (d_t[n_t == 0] == 0).all() and not np.signbit(d_t[n_t == 0]).any()
                assert np.array_equal(d_t.view(np.int32), again[0].view(np.int32))
                worst = max(worst, float((err / np.maximum(R.sum_bound(n_t, a_t), 1e-300)).max()))
                if ex is not None:
                    err_e = np.abs(d_e.astype(np.float64) - ref_e)
                    assert (err_e <= R.sum_bound(n_e, a_e)).all() and (d_e[n_e == 0] == 0).all()
                    assert np.array_equal(d_e.view(np.int32), again[1].view(np.int32))
                if r is not None:
                    assert np.array_equal(d_r.view(np.int32), g.view(np.int32))
    print(f'{ncb} x {K}, C = {C}: largest error / bound {worst:.3f}')


def test_module_and_merged_table():
    from vqcpc_bach_amd.quantizer.product_embedding import ProductEmbedding
    torch.manual_seed(0)
    emb = ProductEmbedding(3, 4, 8).cuda()
    table = emb.merged_table()
    w = emb.weight.detach().cpu().numpy()
    assert table.shape == (64, 8) and not table.requires_grad
    assert np.array_equal(table.cpu().numpy().view(np.int32), R.gather(w, np.arange(64)).view(np.int32))
    codes = torch.tensor([[63, 0, 17], [5, 5, 42]]).cuda()
    rows = emb(codes)
    assert rows.shape == (6, 8) and torch.equal(rows, table[codes.reshape(-1)])
    rows.sum().backward()
    assert emb.weight.grad.shape == (3, 4, 8)
    h = torch.randn(6, 8, device='cuda')
    assert np.array_equal(emb(codes, nj=2, res=h).detach().cpu().numpy().view(np.int32),
                          R.gather(w, codes.reshape(-1).cpu().numpy(), nj=2, res=h.cpu().numpy()).view(np.int32))
    with pytest.raises(ValueError):
        emb(codes, nj=4)
    with pytest.raises(ValueError):
        from vqcpc_bach_amd import ops
        ops.ProductEmbeddingFn.apply(emb.weight, torch.zeros(1, 8, device='cuda'), codes, None, h)


def test_empty_input_zeroes_the_gradients():
    from vqcpc_bach_amd import hip
    d_t = torch.full((2, 3, 8), 7.0, device='cuda')
    d_e = torch.full((1, 8), 7.0, device='cuda')
    idx = torch.empty(0, dtype=torch.int64, device='cuda')
    hip.call('vqcpc_product_gather_bwd', None, 8, idx, idx, d_t, d_e, 0, 0, 2, 3, 1, 8)
    assert float(d_t.abs().max()) == 0.0 and float(d_e.abs().max()) == 0.0


# =============================================================================================================================
# vqcpc_prior_sample_product / vqcpc_prior_window_product
# =============================================================================================================================
import prior_constrained_reference as C  # noqa: E402

D_IN = 12                                    # width of the input rows / head inputs in these tests


class Step:
    """The device state of `steps` positions of M rows: ncb stages per position on given per-stage logits (ncb, M, K)."""

    def __init__(self, logits, K, ncb, N, seeds, seed=0, teacher=None, cons=None, want_logp=False, win=None, pos0=0, probs=True):
        self.K, self.ncb, self.N = K, ncb, N
        self.M = M = logits.shape[1]
        g = torch.Generator().manual_seed(100 + seed)
        dev = 'cuda'
        self.logits = logits.cuda().contiguous()
        self.tables = torch.randn(ncb, K, D_IN, generator=g).to(dev)
        self.dtab = torch.randn(max(ncb - 1, 1), K, D_IN, generator=g).to(dev)
        self.h = torch.randn(M, D_IN, generator=g).to(dev)
        self.hn = [torch.full((M, D_IN), float('nan'), device=dev) for _ in range(ncb)]
        self.seeds = seeds.cuda()
        self.teacher = None if teacher is None else teacher.cuda()
        self.cons = None if cons is None else cons.cuda()
        self.ldcons = 0 if cons is None else cons.shape[1]
        self.logp = torch.full((M, self.ldcons or N), float('nan'), device=dev) if want_logp else None
        self.win = None if win is None else torch.tensor(win, dtype=torch.int32, device=dev)
        self.codes = torch.full((M, N), -1, dtype=torch.int64, device=dev)
        self.nxt = torch.full((M, D_IN), float('nan'), device=dev)
        self.probs = torch.zeros(ncb, M, K, device=dev) if probs else None
        self.pos = torch.full((1,), pos0, dtype=torch.int32, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.digits = torch.full((M, ncb), -7, dtype=torch.int32, device=dev)
        self.acc = torch.full((M,), float('nan'), device=dev)

    def stage(self, j, temperature=1.0, top_k=0, top_p=1.0):
        from vqcpc_bach_amd import hip
        K, ncb, N, M = self.K, self.ncb, self.N, self.M
        last = j == ncb - 1
        h = self.h if j == 0 else self.hn[j - 1]
        hip.call('vqcpc_prior_sample_product', self.logits[j], K, K, ncb, j, M, float(temperature), int(top_k), float(top_p),
                 self.seeds, self.teacher, N, self.cons, self.ldcons or N, self.logp, self.ldcons or N, self.win, self.digits,
                 self.acc, None if last else h, D_IN, None if last else self.dtab, None if last else self.hn[j], D_IN, self.codes, N,
                 N, self.tables, D_IN, self.nxt, D_IN, None if self.probs is None else self.probs[j], K, self.pos, self.ticket)

    def position(self, **kw):
        for j in range(self.ncb):
            self.stage(j, **kw)


@pytest.mark.parametrize('V', [1, 2, 33, 1024, 4096])
def test_one_codebook_is_the_merged_sampler_bit_for_bit(V):
    from vqcpc_bach_amd import hip
    M, N = 5, 4
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(1, M, V, generator=g) * 2).cuda()
    seeds = torch.arange(M, dtype=torch.int64) * 977 + 13
    cons = torch.randint(-1, V, (M, N + 3), generator=g)
    cons[:, 1] = -1
    cons[0, 0], cons[1, 2] = V + 5, 10 ** 12                          # beyond the vocabulary: clamped
    teacher = torch.randint(0, V, (M, N), generator=g)
    for name, kw, filt in (('plain', dict(), dict(temperature=1.3, top_k=7, top_p=0.8)),
                           ('plain', dict(teacher=teacher), dict()),
                           ('cons', dict(cons=cons, want_logp=True, win=[3, 2]), dict(temperature=0.7, top_p=0.9)),
                           ('cons', dict(cons=cons, want_logp=True), dict(top_k=3)),
                           ('cons', dict(want_logp=True, win=[0, -1]), dict())):
        s = Step(logits, V, 1, N, seeds, **kw)
        table = torch.cat([s.tables[0], torch.zeros(1, D_IN, device='cuda')])
        codes = torch.full((M, N), -1, dtype=torch.int64, device='cuda')
        nxt = torch.full((M, D_IN), float('nan'), device='cuda')
        probs = torch.zeros(M, V, device='cuda')
        logp = None if s.logp is None else torch.full_like(s.logp, float('nan'))
        pos, ticket = torch.zeros(1, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
        for step in range(N + 1):                                      # the last call is past the window: a no-op in both
            s.position(**filt)
            f = (float(filt.get('temperature', 1.0)), int(filt.get('top_k', 0)), float(filt.get('top_p', 1.0)))
            if name == 'plain':
                hip.call('vqcpc_prior_sample', s.logits[0], V, V, M, *f, s.seeds, s.teacher, N, codes, N, N, table, V + 1, D_IN, nxt,
                         D_IN, probs, V, pos, ticket)
            else:
                hip.call('vqcpc_prior_sample_constrained', s.logits[0], V, V, M, *f, s.seeds, s.cons, s.ldcons or N, logp,
                         s.ldcons or N, s.win, codes, N, N, table, V + 1, D_IN, nxt, D_IN, probs, V, pos, ticket)
            assert torch.equal(s.codes, codes) and torch.equal(bits(s.nxt), bits(nxt)) and torch.equal(bits(s.probs[0]), bits(probs))
            assert int(s.pos.item()) == int(pos.item()) == min(step + 1, N) and int(s.ticket.item()) == int(ticket.item()) == 0
            if logp is not None:
                assert torch.equal(bits(s.logp), bits(logp))
        assert bool((s.codes >= 0).all())


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('K,ncb', [(5, 2), (4, 3), (512, 2)])
def test_stages_digits_conditioning_and_position(K, ncb):
    M, N, V = 64, 5, K ** ncb
    g = torch.Generator().manual_seed(K + ncb)
    logits = torch.randn(ncb, M, K, generator=g) * 2
    seeds = torch.arange(M, dtype=torch.int64) * 31 + 7
    cons = torch.where(torch.rand(M, N, generator=g) < 0.5, torch.randint(0, V, (M, N), generator=g), torch.tensor(-1))
    cons[0, 0], cons[1, 0] = V + 3, -1
    free = Step(logits, K, ncb, N, seeds)
    forced = Step(logits, K, ncb, N, seeds, cons=cons, want_logp=True)
    one = Step(logits[:, 9:10], K, ncb, N, seeds[9:10], cons=cons[9:10], want_logp=True)
    one.h.copy_(forced.h[9:10])
    for p in range(N):
        for s in (free, forced, one):
            for j in range(ncb):
                s.stage(j, temperature=1.2, top_p=0.95)
                assert int(s.pos.item()) == (p + 1 if j == ncb - 1 else p) and int(s.ticket.item()) == 0    # only the last stage
        code = forced.codes[:, p].cpu()
        want = torch.where(cons[:, p] >= 0, cons[:, p].clamp(max=V - 1), free.codes[:, p].cpu())
        assert torch.equal(code, want)                                # forced digits are the constraint's, free ones the free run's
        dig = R.digits(code.numpy(), ncb, K)
        assert np.array_equal(forced.digits[:, :ncb - 1].cpu().numpy(), dig[:ncb - 1].T)
        h = forced.h.cpu().numpy()
        for j in range(ncb - 1):                                       # h_next = h + D[j][digit], one fp32 add
            h = h + forced.dtab[j].cpu().numpy()[dig[j]]
            assert np.array_equal(forced.hn[j].cpu().numpy().view(np.int32), h.view(np.int32)), j
        nxt = R.gather(forced.tables.cpu().numpy(), code.numpy())
        assert np.array_equal(forced.nxt.cpu().numpy().view(np.int32), nxt.view(np.int32))
        assert torch.equal(one.codes[0], forced.codes[9]) and torch.equal(bits(one.nxt[0]), bits(forced.nxt[9]))     # M = 1 against 64
        assert torch.equal(bits(one.logp[0]), bits(forced.logp[9]))
    before = [t.clone() for t in (forced.codes, forced.nxt, forced.logp, forced.digits, forced.acc, forced.probs, *forced.hn[:ncb - 1])]
    forced.position()                                                  # pos == N: nothing happens at any stage
    after = [forced.codes, forced.nxt, forced.logp, forced.digits, forced.acc, forced.probs, *forced.hn[:ncb - 1]]
    assert all(torch.equal(bits(a), bits(b)) if a.is_floating_point() else torch.equal(a, b) for a, b in zip(after, before))
    assert int(forced.pos.item()) == N and int(forced.ticket.item()) == 0
    # logp: per stage within prior_constrained_reference.logp_bound of the float64 value, summed, plus ncb - 1 roundings of the
    # partial sums (u |partial|, |partial| <= |logp| as every term is <= 0)
    codes = forced.codes.cpu()
    dig = [(codes // K ** j) % K for j in range(ncb)]
    got = forced.logp.cpu().double()
    for b in range(0, M, 7):
        ref = sum(float(torch.log_softmax(logits[j, b].double(), -1)[int(dig[j][b, 2])]) for j in range(ncb))
        tol = sum(C.logp_bound(logits[j, b], int(dig[j][b, 2])) for j in range(ncb)) + (ncb - 1) * R.U * abs(ref)
        assert abs(float(got[b, 2]) - ref) <= tol, (b, float(got[b, 2]), ref, tol)


def test_teacher_forcing_and_window_columns():
    K, ncb, M, N = 4, 3, 3, 4
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(ncb, M, K, generator=g)
    seeds = torch.tensor([1, 2, 3], dtype=torch.int64)
    teacher = torch.randint(0, K ** ncb, (M, N), generator=g)
    s = Step(logits, K, ncb, N, seeds, teacher=teacher)
    for _ in range(N):
        s.position(top_k=1)
    assert torch.equal(s.codes.cpu(), teacher)
    cons = torch.full((M, 9), -1, dtype=torch.int64)
    cons[:, 6] = 21
    s = Step(logits, K, ncb, N, seeds, cons=cons, want_logp=True, win=[7, 5])      # the live window starts at column 5
    for _ in range(2):
        s.position()
    assert bool((s.codes[:, 1] == 21).all()) and bool(torch.isnan(s.logp[:, :5]).all()) and bool(torch.isfinite(s.logp[:, 5:7]).all())
    s = Step(logits, K, ncb, N, seeds, cons=cons, want_logp=True, win=[0, -1])     # no live window: nothing forced, no logp
    s.position()
    assert bool(torch.isnan(s.logp).all()) and bool((s.codes[:, 0] >= 0).all())


def test_later_stage_draws_follow_the_probabilities():
    """The method and threshold of tests/test_prior_gpu.py::test_draws_follow_the_probabilities for digit 1 of a 2 x 32 code: n =
    200 000 draws (64 rows x 3 125 positions) of one fixed 32-way distribution, every frequency within 5 sqrt(p (1 - p) / n); and
    the two digits of a code are drawn with different keys (their agreement rate is that of independent draws)."""
    K, ncb, M, N, n = 32, 2, 64, 1024, 200000
    row = (np.random.default_rng(5).standard_normal(K) * 1.5).astype(np.float32)
    logits = torch.from_numpy(np.tile(row, (ncb, M, 1)))
    counts = torch.zeros(ncb, K, dtype=torch.float64)
    same, left, pas = 0, n // M, 0
    while left > 0:
        steps = min(N, left)
        s = Step(logits, K, ncb, N, torch.arange(M, dtype=torch.int64) * 7919 + 1000003 * (pas + 1), probs=False)
        for _ in range(steps):
            s.position()
        assert int(s.pos.item()) == steps
        drawn = s.codes[:, :steps].reshape(-1).cpu()
        assert bool(((drawn >= 0) & (drawn < K ** ncb)).all()) and bool((s.codes[:, steps:] == -1).all())
        for j in range(ncb):
            counts[j] += torch.bincount((drawn // K ** j) % K, minlength=K).double()
        same += int(((drawn % K) == (drawn // K)).sum())
        left -= steps
        pas += 1
    p = torch.softmax(torch.from_numpy(row).double(), dim=-1)
    lim = 5 * (p * (1 - p) / n).sqrt()
    for j in range(ncb):
        dev = (counts[j] / n - p).abs()
        print(f'digit {j}: worst deviation {float((dev / lim).max()) * 5:.2f} sigma')
        assert bool((dev <= lim).all()), (j, (dev / lim).max())
    q = float((p * p).sum())
    assert abs(same / n - q) <= 5 * (q * (1 - q) / n) ** 0.5


@pytest.mark.parametrize('K,ncb', [(4, 3), (3, 2), (7, 1)])
def test_window_kernel_equals_the_merged_one_on_the_merged_table(K, ncb):
    """The scenarios of tests/test_decode_kernels_gpu.py's window cases: vqcpc_prior_window on the (V + 1, d) table of all sums
    (vqcpc_product_gather over arange(V), then the start-of-sentence row) against vqcpc_prior_window_product, every output
    compared exactly."""
    from vqcpc_bach_amd import hip, ops
    V, M, N, nt, d = K ** ncb, 5, 6, 14, D_IN
    g = torch.Generator().manual_seed(K)
    tables = torch.randn(ncb, K, d, generator=g).cuda()
    sos = torch.randn(1, d, generator=g).cuda()
    table = torch.cat([ops.ProductEmbeddingFn.apply(tables, None, torch.arange(V).cuda()), sos])
    for win, pos0, P, adv in (([0, -1], 0, 0, 0), ([3, 0], N, N - 1, 1), ([4, 2], 3, 2, 4), ([8, 5], N, 0, 2), ([-1, 6], 4, 0, 0),
                              ([9, 1], 2, 5, 1)):
        outs = []
        for product in (False, True):
            seq = torch.randint(0, V, (M, nt), generator=torch.Generator().manual_seed(3)).cuda()
            seq[0, 5], seq[1, 6] = V + 9, -4                          # out of range in the sequence: clamped for the rows
            w = torch.tensor(win, dtype=torch.int32).cuda()
            codes_win = torch.randint(0, V, (M, N), generator=torch.Generator().manual_seed(4)).cuda()
            prefix = torch.full((M * N,), -9, dtype=torch.int64).cuda()
            x = torch.full((M, d), float('nan')).cuda()
            seeds_in = (torch.arange(M, dtype=torch.int64) * 101 + 5).cuda()
            seeds_out = torch.zeros(M, dtype=torch.int64).cuda()
            pos = torch.full((1,), pos0, dtype=torch.int32).cuda()
            if product:
                hip.call('vqcpc_prior_window_product', seq, nt, nt, w, adv, codes_win, N, P, prefix, tables, ncb, K, sos, d, x, d,
                         seeds_in, seeds_out, pos, M)
            else:
                hip.call('vqcpc_prior_window', seq, nt, nt, w, adv, codes_win, N, P, prefix, table, V + 1, d, x, d, seeds_in,
                         seeds_out, pos, M)
            outs.append((seq, w, codes_win, prefix, bits(x), seeds_out, pos))
        for a, b in zip(*outs):
            assert torch.equal(a, b), (win, pos0, P, adv)
