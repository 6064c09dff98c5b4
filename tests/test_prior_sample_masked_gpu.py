"""vqcpc_prior_sample_masked (csrc/prior.hip) and vqcpc_prior_sample_product_masked (csrc/product_codes.hip) by direct calls, with
the conventions of tests/test_prior_sample_constrained_gpu.py: sentinel-filled outputs with guard rows and wider leading
dimensions, NaN in the logits columns [V, ldl), sentinel bits in the set columns no step may read.
  (1) a full set or NULL == vqcpc_prior_sample_constrained bit for bit, logmass exactly 0,
  (2) a set S == the constrained sampler fed -inf outside S; a one-hot set == forcing; a forced code outside its set is emitted,
  (3) logmass against float64 within tests/prior_masked_reference.py::logmass_bound, -inf sets, invariance under M,
  (4) the column rule through the window index, the guards on the leading dimensions, repeated launches,
  (5) product stages: one codebook == the merged kernel, the stage chain in fp32 bits, the draws of vqcpc_prior_sample_product."""
import numpy as np
import pytest
import torch

import prior_masked_reference as R
from test_decode_kernels_gpu import GR, NAN, Buf, call, gen, same_bits

pytestmark = pytest.mark.gpu

VS = [1, 2, 15, 16, 17, 31, 32, 33, 65, 1000, 4095, 4096]    # the half-word a thread owns, the word, and the limits
N = 5
OFF = 5                                                  # the live window's first code in the windowed calls
W = N + OFF + 2                                          # columns of constraint / logp / allowed / logmass
FILTERS = [(1.5, 0, 1.0), (0.7, 5, 1.0), (1.5, 0, 0.9), (0.7, 5, 0.9)]      # temperature != 1, top-k, top-p, both
INF = float('inf')


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


def _logits(rows):
    M, V = rows.shape
    lg = torch.full((M, V + 3), NAN)
    lg[:, :V] = rows
    return lg.cuda()


def _seeds(M):
    return (torch.arange(1, M + 1, dtype=torch.int64) * 104729 * 1000003 + 11).cuda()


class Sets:
    """Packed sets (M, width[, ncb], words) inside a sentinel-filled allocation of leading dimension ld with guard rows."""

    def __init__(self, allowed, ld=None):
        packed = torch.from_numpy(R.pack_ref(allowed.numpy()).view(np.int32).copy())
        M, width = packed.shape[:2]
        self.ld = width + 2 if ld is None else ld
        self.full = torch.full((M + 2 * GR, self.ld) + tuple(packed.shape[2:]), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
        self.view = self.full[GR:GR + M, :width]
        self.view.copy_(packed)
        self.before = self.full.clone()

    def assert_untouched(self):
        assert torch.equal(self.before, self.full)


class Run:
    """`steps` calls of one entry point on fresh sentinel-filled outputs.  entry 'cons': vqcpc_prior_sample_constrained; 'mask':
    vqcpc_prior_sample_masked with sets (Sets or None) and mass (Buf or None) on top."""

    def __init__(self, entry, lg, V, d, temperature, top_k, top_p, seeds, steps=N, pos0=0, cons=None, logp=None, win=None,
                 sets=None, mass=None, table=None):
        M = lg.shape[0]
        self.pos = torch.full((1,), pos0, dtype=torch.int32, device='cuda')
        self.ticket = torch.zeros(1, dtype=torch.int32, device='cuda')
        self.codes = Buf(M, N, N + 3, dtype=torch.int64)
        self.nxt, self.pr = Buf(M, d, d + 3), Buf(M, V, V + 5)
        self.table = torch.randn(V + 1, d, generator=gen(3)).cuda() if table is None else table
        self.win = None if win is None else torch.tensor(win, dtype=torch.int32).cuda()
        head = (lg, V + 3, V, M, float(temperature), int(top_k), float(top_p), seeds, None if cons is None else cons.view,
                0 if cons is None else cons.ld, None if logp is None else logp.view, 0 if logp is None else logp.ld, self.win)
        tail = (self.codes.view, N + 3, N, self.table, V + 1, d, self.nxt.view, d + 3, self.pr.view, V + 5, self.pos, self.ticket)
        for i in range(steps):
            if entry == 'cons':
                call('vqcpc_prior_sample_constrained', *head, *tail)
            else:
                call('vqcpc_prior_sample_masked', *head, None if sets is None else sets.view, 0 if sets is None else sets.ld,
                     None if mass is None else mass.view, 0 if mass is None else mass.ld, *tail)
            torch.cuda.synchronize()
            assert int(self.ticket.item()) == 0 and int(self.pos.item()) == min(pos0 + i + 1, max(N, pos0)), (entry, i)

    def same_outputs(self, other):
        return (same_bits(self.codes.full, other.codes.full) and same_bits(self.nxt.full, other.nxt.full) and
                same_bits(self.pr.full, other.pr.full) and torch.equal(self.pos, other.pos) and
                torch.equal(self.ticket, other.ticket))


def _cons_buf(M, data):
    return Buf(M, W, W + 2, data=data, dtype=torch.int64)


def _random_cons(M, V, seed, free_share):
    g = gen(seed)
    cons = torch.randint(0, V, (M, W), generator=g)
    return torch.where(torch.rand(M, W, generator=g) < free_share, torch.full_like(cons, -1), cons)


def _random_sets(M, V, seed, share=0.4):
    """bool (M, W, V): every set has at least one code."""
    g = gen(seed)
    a = torch.rand(M, W, V, generator=g) < share
    a.scatter_(2, torch.randint(0, V, (M, W, 1), generator=g), True)
    return a


def _only_columns(buf, lo, hi):
    """Nothing but columns [lo, hi) of the logical rows of `buf` was written."""
    exp = buf.before.clone()
    exp[GR:GR + buf.rows, lo:hi] = buf.view[:, lo:hi]
    return same_bits(exp, buf.full)


# =====================================================================================================================
# (1) a full set or no set: the constrained sampler, and a mass of exactly zero
@pytest.mark.parametrize('V', VS)
def test_a_full_or_absent_set_is_the_constrained_sampler_bit_for_bit(V):
    n = 0
    for M in (1, 3, 64):
        lg = _logits(torch.randn(M, V, generator=gen(60 + V + M)) * 2.0)
        seeds = _seeds(M)
        cons = _random_cons(M, V, 70 + V, 0.6)
        full = Sets(torch.ones(M, W, V, dtype=torch.bool))
        for temperature, top_k, top_p in FILTERS:
            args = (lg, V, 4, temperature, min(top_k, V), top_p, seeds)
            lp0 = Buf(M, W, W + 1)
            ref = Run('cons', *args, cons=_cons_buf(M, cons), logp=lp0, win=[9, OFF])
            for sets, want_mass in ((None, False), (None, True), (full, False), (full, True)):
                lp, mass = Buf(M, W, W + 1), Buf(M, W, W + 3) if want_mass else None
                run = Run('mask', *args, cons=_cons_buf(M, cons), logp=lp, win=[9, OFF], sets=sets, mass=mass)
                assert run.same_outputs(ref) and same_bits(lp.full, lp0.full), (M, top_k, top_p, sets is None, want_mass)
                if want_mass:
                    live = mass.view[:, OFF:OFF + N]
                    assert same_bits(live, torch.zeros_like(live)) and _only_columns(mass, OFF, OFF + N)       # +0.0f, every bit
                n += 1
        full.assert_untouched()
    assert n == 48


# =====================================================================================================================
# (2) a set S: the constrained sampler on the row closed outside S
@pytest.mark.parametrize('V', VS)
def test_a_set_is_the_constrained_sampler_fed_minus_infinity_outside_it(V):
    for M in (1, 3, 64):
        rows = torch.randn(M, V, generator=gen(160 + V + M)) * 2.0
        seeds = _seeds(M)
        allowed = _random_sets(M, V, 170 + V + M)
        sets = Sets(allowed)
        cons = _random_cons(M, V, 180 + V, 0.7)
        for temperature, top_k, top_p in FILTERS:
            for p in (0, N - 1):
                a = allowed[:, OFF + p]
                args = (4, temperature, min(top_k, V), top_p, seeds)
                kw = dict(steps=1, pos0=p, win=[9, OFF])
                lp = Buf(M, W, W + 1)
                run = Run('mask', _logits(rows), V, *args, cons=_cons_buf(M, cons), logp=lp, sets=sets, **kw)
                closed = Run('cons', _logits(rows.masked_fill(~a, -INF)), V, *args, cons=_cons_buf(M, cons), **kw)
                assert run.same_outputs(closed), (M, temperature, top_k, top_p, p)
                codes = run.codes.view[:, p].cpu()
                free = cons[:, OFF + p] < 0
                assert bool(a[free].gather(1, codes[free].unsqueeze(1)).all())                # a drawn code lies in its set
                assert torch.equal(codes[~free], cons[~free, OFF + p])                         # a forced one wins
                # logp: the emitted code under the UNMODIFIED row -- the constrained sampler forced to the same codes
                force = torch.full((M, W), -1, dtype=torch.int64)
                force[:, OFF + p] = codes
                lp2 = Buf(M, W, W + 1)
                Run('cons', _logits(rows), V, *args, cons=_cons_buf(M, force), logp=lp2, **kw)
                assert same_bits(lp.full, lp2.full)
        sets.assert_untouched()


@pytest.mark.parametrize('V', [2, 17, 33, 4096])
def test_a_one_hot_set_is_forcing_and_a_forced_code_outside_its_set_is_emitted(V):
    M = 3
    rows = torch.randn(M, V, generator=gen(190 + V)) * 2.0
    seeds = _seeds(M)
    pick = torch.randint(0, V, (M, W), generator=gen(191 + V))
    one = torch.zeros(M, W, V, dtype=torch.bool).scatter_(2, pick.unsqueeze(2), True)
    lp, mass = Buf(M, W, W + 1), Buf(M, W, W + 1)
    run = Run('mask', _logits(rows), V, 4, 1.3, min(5, V), 0.9, seeds, logp=lp, sets=Sets(one), mass=mass, win=[0, OFF])
    lp2 = Buf(M, W, W + 1)
    forced = Run('cons', _logits(rows), V, 4, 1.3, min(5, V), 0.9, seeds, cons=_cons_buf(M, pick), logp=lp2, win=[0, OFF])
    assert same_bits(run.codes.full, forced.codes.full) and same_bits(run.nxt.full, forced.nxt.full) and same_bits(lp.full, lp2.full)
    assert torch.equal(run.codes.view.cpu(), pick[:, OFF:OFF + N])
    # the mass of a one-hot set is the code's log-probability up to the two chains' roundings (both bounds)
    for b in range(M):
        for p in range(N):
            ref = R.logmass_ref(rows[b], one[b, OFF + p])
            assert abs(float(mass.view[b, OFF + p]) - ref) <= R.logmass_bound(rows[b], one[b, OFF + p])
    # a forced code outside its set: emitted, and logmass is still the set's (the bits of the run that forces nothing)
    other = (pick + 1) % V
    mass2 = Buf(M, W, W + 1)
    out = Run('mask', _logits(rows), V, 4, 1.3, min(5, V), 0.9, seeds, cons=_cons_buf(M, other), sets=Sets(one), mass=mass2,
              win=[0, OFF])
    assert torch.equal(out.codes.view.cpu(), other[:, OFF:OFF + N])
    assert same_bits(mass2.full, mass.full)


# =====================================================================================================================
# (3) logmass
def _score_rows(V):
    """Rows of scale 2, of scale 40, and one holding -inf entries (every other code; V = 1 has none)."""
    g = gen(90 + V)
    rows = torch.stack([torch.randn(V, generator=g) * 2.0, torch.randn(V, generator=g) * 40.0, torch.randn(V, generator=g) * 2.0])
    if V >= 2:
        rows[2, ::2] = -INF
    return rows


@pytest.mark.parametrize('V', VS)
def test_logmass_is_within_its_bound_of_float64(V):
    rows = _score_rows(V)
    M = rows.shape[0]
    allowed = _random_sets(M, V, 200 + V, 0.3)
    if V >= 2:
        allowed[2, 1] = False
        allowed[2, 1, ::2] = True                                                 # row 2, column 1: every allowed logit is -inf
    allowed[:, 3] = True                                                          # column 3: the full set
    cons = torch.full((M, W), -1, dtype=torch.int64)
    cons[:, 2] = 0                                                                # written at forced columns too
    worst = 0.0
    for temperature, top_k, top_p in FILTERS[::3]:                                # neither the filter nor the temperature enters
        mass = Buf(M, W, W + 1)
        Run('mask', _logits(rows), V, 4, temperature, min(top_k, V), top_p, _seeds(M), cons=_cons_buf(M, cons), sets=Sets(allowed),
            mass=mass)
        got = mass.view.cpu()
        for b in range(M):
            for p in range(N):
                ref, bound = R.logmass_ref(rows[b], allowed[b, p]), R.logmass_bound(rows[b], allowed[b, p])
                if bound == 0.0:
                    assert float(got[b, p]) == ref, (V, b, p)                     # exactly 0.0f, or exactly -inf
                    continue
                err = abs(float(got[b, p]) - ref)
                worst = max(worst, err / bound)
                assert err <= bound, (V, b, p, float(got[b, p]), ref, bound)
        if V >= 2:
            assert float(got[2, 1]) == -INF
        assert bool((got[:, 3] == 0.0).all()) and _only_columns(mass, 0, N)
    print(f'V {V}: worst |logmass - float64| / bound = {worst:.3f}')


@pytest.mark.parametrize('V', [17, 1000, 4096])
def test_a_row_has_the_same_bits_alone_and_among_64(V):
    M = 64
    rows = torch.randn(M, V, generator=gen(110 + V)) * 3.0
    seeds = _seeds(M)
    cons = _random_cons(M, V, 120 + V, 0.6)
    allowed = _random_sets(M, V, 125 + V)
    table = torch.randn(V + 1, 4, generator=gen(3)).cuda()

    def run(sel):
        lp, mass = Buf(len(sel), W, W + 1), Buf(len(sel), W, W + 1)
        r = Run('mask', _logits(rows[sel]), V, 4, 1.3, min(7, V), 0.9, seeds[sel].contiguous(), cons=_cons_buf(len(sel), cons[sel]),
                logp=lp, sets=Sets(allowed[sel]), mass=mass, win=[0, 1], table=table)
        return r.codes.view.clone(), lp.view[:, 1:1 + N].clone(), mass.view[:, 1:1 + N].clone()
    codes, logp, mass = run(list(range(M)))
    assert bool(torch.isfinite(mass).all())
    for b in (0, 37, 63):
        c1, l1, m1 = run([b])
        assert torch.equal(c1[0], codes[b]) and same_bits(l1[0], logp[b]) and same_bits(m1[0], mass[b]), b


# =====================================================================================================================
# (4) the column rule, the guards, repeated launches
def test_the_set_is_read_and_the_mass_written_at_the_window_column_alone():
    """Every column holds another one-hot set, so a read anywhere else shows in the codes; window 0, a middle window, and no live
    window (no restriction, no mass)."""
    V, M = 257, 3
    rows = torch.randn(M, V, generator=gen(130)) * 2.0
    pick = (torch.arange(M).view(M, 1) * 31 + torch.arange(W).view(1, W) * 17 + 3) % V
    one = torch.zeros(M, W, V, dtype=torch.bool).scatter_(2, pick.unsqueeze(2), True)
    for live in (0, OFF):
        sets, mass = Sets(one), Buf(M, W, W + 1)
        run = Run('mask', _logits(rows), V, 4, 1.0, 0, 1.0, _seeds(M), sets=sets, mass=mass, win=[77, live])
        assert torch.equal(run.codes.view.cpu(), pick[:, live:live + N])
        sets.assert_untouched()
        assert _only_columns(mass, live, live + N) and run.win.tolist() == [77, live]
    sets, mass = Sets(one), Buf(M, W, W + 1)
    run = Run('mask', _logits(rows), V, 4, 1.0, 0, 1.0, _seeds(M), sets=sets, mass=mass, win=[0, -1])
    assert run.same_outputs(Run('cons', _logits(rows), V, 4, 1.0, 0, 1.0, _seeds(M)))
    mass.assert_untouched()
    nowin = Run('mask', _logits(rows), V, 4, 1.0, 0, 1.0, _seeds(M), sets=Sets(one))          # win == NULL: the column is pos
    assert torch.equal(nowin.codes.view.cpu(), pick[:, :N])


def test_columns_past_the_leading_dimensions_are_unrestricted_and_unwritten():
    """ldallow = ldmass = 7 >= N with win = {., 5}: columns 5 and 6 are restricted / written, positions 2 .. 4 (columns 7 .. 9) are
    drawn from the whole row and leave no mass (the guard rows behind the narrow buffers take what a missing guard would do)."""
    V, M = 255, 3
    rows = torch.randn(M, V, generator=gen(132)) * 2.0
    one = torch.zeros(M, 7, V, dtype=torch.bool)
    one[:, :, 200] = True
    sets, mass = Sets(one, ld=7), Buf(M, 7, 7)
    run = Run('mask', _logits(rows), V, 4, 1.0, 0, 1.0, _seeds(M), sets=sets, mass=mass, win=[0, OFF])
    plain = Run('cons', _logits(rows), V, 4, 1.0, 0, 1.0, _seeds(M))
    assert bool((run.codes.view[:, :2] == 200).all()) and torch.equal(run.codes.view[:, 2:], plain.codes.view[:, 2:])
    assert _only_columns(mass, OFF, 7) and bool(torch.isfinite(mass.view[:, OFF:7]).all())
    sets.assert_untouched()


def test_a_set_without_a_code_of_the_vocabulary_restricts_nothing():
    """Bits [V, 32 * words) set and none below: the kernel reads no restriction (the host refuses such a set)."""
    V, M = 17, 3
    rows = torch.randn(M, V, generator=gen(133)) * 2.0
    sets = Sets(torch.ones(M, W, V, dtype=torch.bool))
    sets.view.fill_(-(1 << 31) >> 14)                                    # bits 17 .. 31
    mass = Buf(M, W, W + 1)
    run = Run('mask', _logits(rows), V, 4, 1.2, 3, 0.9, _seeds(M), sets=sets, mass=mass)
    assert run.same_outputs(Run('cons', _logits(rows), V, 4, 1.2, 3, 0.9, _seeds(M)))
    assert bool((mass.view[:, :N] == 0.0).all())


def test_two_launches_give_equal_bits_and_nothing_is_written_past_the_window():
    V, M = 1000, 5
    rows = torch.randn(M, V, generator=gen(134)) * 2.0
    allowed, cons = _random_sets(M, V, 135), _random_cons(M, V, 136, 0.5)

    def run(**kw):
        lp, mass = Buf(M, W, W + 1), Buf(M, W, W + 1)
        r = Run('mask', _logits(rows), V, 4, 1.4, 9, 0.95, _seeds(M), cons=_cons_buf(M, cons), logp=lp, sets=Sets(allowed), mass=mass,
                win=[0, 2], **kw)
        return r, lp, mass
    a, b = run(), run()
    assert a[0].same_outputs(b[0]) and same_bits(a[1].full, b[1].full) and same_bits(a[2].full, b[2].full)
    r, lp, mass = run(steps=2, pos0=N)
    for buf in (r.codes, r.nxt, r.pr, lp, mass):
        buf.assert_untouched()
    assert int(r.pos.item()) == N and int(r.ticket.item()) == 0


# =====================================================================================================================
# (5) product stages
from test_product_codes_kernels_gpu import D_IN, Step  # noqa: E402


def _bits(t):
    return t.contiguous().view(torch.int32)


class MaskedStep(Step):
    """`Step` of tests/test_product_codes_kernels_gpu.py on vqcpc_prior_sample_product_masked: digit sets (M, W, ncb, K) bool or
    None, and the mass."""

    def __init__(self, *a, sets=None, want_mass=False, width=None, **kw):
        super().__init__(*a, **kw)
        width = width or self.ldcons or self.N
        self.sets = None if sets is None else Sets(sets)
        self.ldmass = width
        self.mass = torch.full((self.M, width), float('nan'), device='cuda') if want_mass else None
        self.macc = torch.full((self.M,), float('nan'), device='cuda')

    def stage(self, j, temperature=1.0, top_k=0, top_p=1.0):
        from vqcpc_bach_amd import hip
        K, ncb, N, M = self.K, self.ncb, self.N, self.M
        last = j == ncb - 1
        h = self.h if j == 0 else self.hn[j - 1]
        hip.call('vqcpc_prior_sample_product_masked', self.logits[j], K, K, ncb, j, M, float(temperature), int(top_k), float(top_p),
                 self.seeds, self.teacher, N, self.cons, self.ldcons or N, self.logp, self.ldcons or N, self.win,
                 None if self.sets is None else self.sets.view, 0 if self.sets is None else self.sets.ld, self.mass, self.ldmass,
                 self.digits, self.acc, self.macc, None if last else h, D_IN, None if last else self.dtab,
                 None if last else self.hn[j], D_IN, self.codes, N, N, self.tables, D_IN, self.nxt, D_IN,
                 None if self.probs is None else self.probs[j], K, self.pos, self.ticket)


@pytest.mark.parametrize('K', [1, 4, 33])
def test_one_codebook_is_the_merged_masked_sampler_bit_for_bit(K):
    M, Np = 5, 4
    g = gen(K)
    logits = torch.randn(1, M, K, generator=g) * 2
    seeds = torch.arange(M, dtype=torch.int64) * 977 + 13
    width = Np + 3
    cons = torch.where(torch.rand(M, width, generator=g) < 0.7, torch.tensor(-1), torch.randint(0, K, (M, width), generator=g))
    allowed = torch.rand(M, width, 1, K, generator=g) < 0.5
    allowed.scatter_(3, torch.randint(0, K, (M, width, 1, 1), generator=g), True)
    s = MaskedStep(logits, K, 1, Np, seeds, cons=cons, want_logp=True, win=[3, 2], sets=allowed, want_mass=True)
    table = torch.cat([s.tables[0], torch.zeros(1, D_IN, device='cuda')])
    codes = torch.full((M, Np), -1, dtype=torch.int64, device='cuda')
    nxt = torch.full((M, D_IN), float('nan'), device='cuda')
    probs = torch.zeros(M, K, device='cuda')
    logp, mass = torch.full_like(s.logp, float('nan')), torch.full_like(s.mass, float('nan'))
    pos, ticket = torch.zeros(1, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    merged = Sets(allowed[:, :, 0])
    for step in range(Np + 1):                                         # the last call is past the window: a no-op in both
        s.position(temperature=0.7, top_k=min(3, K), top_p=0.9)
        call('vqcpc_prior_sample_masked', s.logits[0], K, K, M, 0.7, min(3, K), 0.9, s.seeds, s.cons, width, logp, width, s.win,
             merged.view, merged.ld, mass, width, codes, Np, Np, table, K + 1, D_IN, nxt, D_IN, probs, K, pos, ticket)
        assert torch.equal(s.codes, codes) and torch.equal(_bits(s.nxt), _bits(nxt)) and torch.equal(_bits(s.probs[0]), _bits(probs))
        assert torch.equal(_bits(s.logp), _bits(logp)) and torch.equal(_bits(s.mass), _bits(mass))
        assert int(s.pos.item()) == int(pos.item()) == min(step + 1, Np) and int(s.ticket.item()) == int(ticket.item()) == 0
    assert bool((s.codes >= 0).all()) and bool(torch.isfinite(s.mass[:, 2:2 + Np]).all())


@pytest.mark.parametrize('K,ncb', [(1, 2), (4, 2), (33, 2), (4, 3), (33, 3)])
def test_the_stage_chain_in_fp32_bits_and_the_draws_of_the_plain_product_sampler(K, ncb):
    M, Np, V = 64, 4, K ** ncb
    g = gen(10 * K + ncb)
    logits = torch.randn(ncb, M, K, generator=g) * 2
    seeds = torch.arange(M, dtype=torch.int64) * 31 + 7
    cons = torch.where(torch.rand(M, Np, generator=g) < 0.7, torch.tensor(-1), torch.randint(0, V, (M, Np), generator=g))
    allowed = torch.rand(M, Np, ncb, K, generator=g) < 0.5
    allowed.scatter_(3, torch.randint(0, K, (M, Np, ncb, 1), generator=g), True)
    filt = dict(temperature=1.2, top_k=min(3, K), top_p=0.95)
    s = MaskedStep(logits, K, ncb, Np, seeds, cons=cons, want_logp=True, sets=allowed, want_mass=True)
    one = MaskedStep(logits[:, 9:10], K, ncb, Np, seeds[9:10], cons=cons[9:10], want_logp=True, sets=allowed[9:10], want_mass=True)
    one.h.copy_(s.h[9:10])
    for p in range(Np):
        # the draws: vqcpc_prior_sample_product fed -inf outside the position's digit sets
        closed = Step(logits.masked_fill(~allowed[:, p].transpose(0, 1), -INF), K, ncb, Np, seeds, cons=cons, want_logp=False, pos0=p)
        closed.h.copy_(s.h)
        for r in (s, one, closed):
            r.position(**filt)
        assert torch.equal(s.codes[:, p], closed.codes[:, p]) and torch.equal(_bits(s.nxt), _bits(closed.nxt))
        assert torch.equal(_bits(s.probs), _bits(closed.probs))
        assert torch.equal(one.codes[0], s.codes[9]) and torch.equal(_bits(one.logp[0]), _bits(s.logp[9])) and \
            torch.equal(_bits(one.mass[0]), _bits(s.mass[9]))                                  # M = 1 against 64
        # logp and logmass: each stage's value from the MERGED masked kernel on the stage's row (one codebook == merged, above),
        # added in ascending stage order by numpy in fp32
        code = s.codes[:, p].cpu()
        dig = [(code // K ** j) % K for j in range(ncb)]
        acc_lp = acc_lm = None
        for j in range(ncb):
            lp, lm = torch.full((M, 1), NAN, device='cuda'), torch.full((M, 1), NAN, device='cuda')
            stage_sets = Sets(allowed[:, p:p + 1, j])
            out = torch.full((M, 1), -1, dtype=torch.int64, device='cuda')
            call('vqcpc_prior_sample_masked', s.logits[j], K, K, M, 1.0, 0, 1.0, s.seeds, dig[j].view(M, 1).cuda(), 1, lp, 1, None,
                 stage_sets.view, stage_sets.ld, lm, 1, out, 1, 1, torch.zeros(K + 1, D_IN, device='cuda'), K + 1, D_IN,
                 torch.empty(M, D_IN, device='cuda'), D_IN, None, 0, torch.zeros(1, dtype=torch.int32, device='cuda'),
                 torch.zeros(1, dtype=torch.int32, device='cuda'))
            lp, lm = lp.cpu().numpy()[:, 0], lm.cpu().numpy()[:, 0]
            acc_lp, acc_lm = (lp, lm) if j == 0 else (acc_lp + lp, acc_lm + lm)
        assert acc_lp.dtype == np.float32
        assert np.array_equal(s.logp[:, p].cpu().numpy().view(np.int32), acc_lp.view(np.int32))
        assert np.array_equal(s.mass[:, p].cpu().numpy().view(np.int32), acc_lm.view(np.int32))
        # and against the float64 chain: the free digits lie in their sets, the forced code is emitted whole
        ref_codes, ref_dig, _, ref_mass = R.product_chain_ref(logits, 1.2, min(3, K), 0.95, seeds, p, cons[:, p], allowed[:, p])
        forced = cons[:, p] >= 0
        assert torch.equal(code[forced], cons[forced, p])
        for j in range(ncb):
            assert bool(allowed[~forced, p, j].gather(1, dig[j][~forced].unsqueeze(1)).all())
        tol = [sum(R.logmass_bound(logits[j, b], allowed[b, p, j]) for j in range(ncb)) + (ncb - 1) * 2.0 ** -24 * abs(float(ref_mass[b]))
               for b in range(M)]
        assert all(abs(float(s.mass[b, p]) - float(ref_mass[b])) <= tol[b] for b in range(M))
    s.sets.assert_untouched()
