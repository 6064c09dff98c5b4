"""vqcpc_prior_sample_constrained (csrc/prior.hip) by direct calls, with the conventions of tests/test_decode_kernels_gpu.py:
sentinel-filled outputs with guard rows and wider leading dimensions, NaN in the logits columns [V, ldl).
  (1) bit-identity with vqcpc_prior_sample: nothing forced, everything forced (== teacher forcing), a mixed constraint,
  (2) logp against float64 within tests/prior_constrained_reference.py::logp_bound, -inf codes, invariance under M,
  (3) addressing through the window index, the guards on the leading dimensions, clamping, the no-op past the window."""
import pytest
import torch

import prior_constrained_reference as C
from test_decode_kernels_gpu import GR, NAN, Buf, call, gen, same_bits

pytestmark = pytest.mark.gpu

VS = [1, 2, 15, 16, 17, 255, 257, 1000, 4095, 4096]      # thread ownership (16 codes per thread) and wave (1024) boundaries
N = 5
OFF = 5                                                  # the live window's first code in the windowed calls
W = N + OFF + 2                                          # columns of constraint / logp
FILTERS = [(0, 1.0), (5, 0.9)]


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


class Run:
    """`steps` calls of one entry point on fresh sentinel-filled outputs.  entry 'plain': vqcpc_prior_sample with `teacher`
    (M, N) or None; 'cons': vqcpc_prior_sample_constrained with cons / logp (Buf or None) and win (two int32 or None).  After
    every call the ticket is 0 and pos has advanced by one (live calls) or stayed (pos >= N)."""

    def __init__(self, entry, lg, V, d, temperature, top_k, top_p, seeds, steps=N, pos0=0, teacher=None, cons=None, logp=None,
                 win=None, table=None):
        M = lg.shape[0]
        self.pos = torch.full((1,), pos0, dtype=torch.int32, device='cuda')
        self.ticket = torch.zeros(1, dtype=torch.int32, device='cuda')
        self.codes = Buf(M, N, N + 3, dtype=torch.int64)
        self.nxt, self.pr = Buf(M, d, d + 3), Buf(M, V, V + 5)
        self.table = torch.randn(V + 1, d, generator=gen(3)).cuda() if table is None else table
        self.win = None if win is None else torch.tensor(win, dtype=torch.int32).cuda()
        for i in range(steps):
            if entry == 'plain':
                call('vqcpc_prior_sample', lg, V + 3, V, M, float(temperature), int(top_k), float(top_p), seeds, teacher, N,
                     self.codes.view, N + 3, N, self.table, V + 1, d, self.nxt.view, d + 3, self.pr.view, V + 5, self.pos,
                     self.ticket)
            else:
                call('vqcpc_prior_sample_constrained', lg, V + 3, V, M, float(temperature), int(top_k), float(top_p), seeds,
                     None if cons is None else cons.view, 0 if cons is None else cons.ld, None if logp is None else logp.view,
                     0 if logp is None else logp.ld, self.win, self.codes.view, N + 3, N, self.table, V + 1, d, self.nxt.view,
                     d + 3, self.pr.view, V + 5, self.pos, self.ticket)
            torch.cuda.synchronize()
            assert int(self.ticket.item()) == 0 and int(self.pos.item()) == min(pos0 + i + 1, max(N, pos0)), (entry, i)

    def same_outputs(self, other):
        return (same_bits(self.codes.full, other.codes.full) and same_bits(self.nxt.full, other.nxt.full) and
                same_bits(self.pr.full, other.pr.full) and torch.equal(self.pos, other.pos) and
                torch.equal(self.ticket, other.ticket))


def _cons_buf(M, data=None, width=W, ld=W + 2):
    return Buf(M, width, ld, data=data, dtype=torch.int64)


def _random_cons(M, V, seed, free_share):
    g = gen(seed)
    cons = torch.randint(0, V, (M, W), generator=g)
    return torch.where(torch.rand(M, W, generator=g) < free_share, torch.full_like(cons, -1), cons)


# =====================================================================================================================
# (1) bit-identity with the plain sampler
@pytest.mark.parametrize('V', VS)
def test_free_forced_and_mixed_against_the_plain_sampler(V):
    n = 0
    for M in (1, 3, 64):
        lg = _logits(torch.randn(M, V, generator=gen(60 + V + M)) * 2.0)
        seeds = _seeds(M)
        for d in (4, 516):
            for top_k, top_p in FILTERS:
                args = (lg, V, d, 1.5, min(top_k, V), top_p, seeds)
                plain = Run('plain', *args)
                # nothing forced: no constraint, an all-free one, with and without a window index and logp
                free = _cons_buf(M, torch.full((M, W), -1, dtype=torch.int64))
                for kw in (dict(), dict(cons=free), dict(cons=free, win=[9, OFF], logp=Buf(M, W, W + 1)), dict(logp=Buf(M, W, W + 1))):
                    assert Run('cons', *args, **kw).same_outputs(plain), (M, d, top_k, sorted(kw))
                free.assert_untouched()
                # everything forced == teacher forcing with teacher[b][pos] = constraint[b][win[1] + pos]
                full = _random_cons(M, V, 70 + V, 0.0)
                teacher = full[:, OFF:OFF + N].contiguous().cuda()
                forced = Run('cons', *args, cons=_cons_buf(M, full), win=[9, OFF])
                assert forced.same_outputs(Run('plain', *args, teacher=teacher)), (M, d, top_k)
                assert torch.equal(forced.codes.view, teacher)
                # mixed: the free positions keep the plain sampler's codes (the rows do not depend on earlier codes here), the
                # probabilities stay the filtered distribution whatever is forced
                mixed_c = _random_cons(M, V, 80 + V, 0.5)
                mixed = Run('cons', *args, cons=_cons_buf(M, mixed_c), win=[9, OFF])
                mc = mixed_c[:, OFF:OFF + N].cuda()
                assert torch.equal(mixed.codes.view, torch.where(mc < 0, plain.codes.view, mc)), (M, d, top_k)
                assert same_bits(mixed.pr.full, plain.pr.full)
                assert torch.equal(mixed.nxt.view, mixed.table[mixed.codes.view[:, N - 1]])
                n += 1
    assert n == 12


# =====================================================================================================================
# (2) logp
def _score_rows(V):
    """Rows of scale 2, of scale 40, and one holding -inf entries (every other code; V = 1 has none)."""
    g = gen(90 + V)
    rows = torch.stack([torch.randn(V, generator=g) * 2.0, torch.randn(V, generator=g) * 40.0, torch.randn(V, generator=g) * 2.0])
    if V >= 2:
        rows[2, ::2] = -float('inf')
    return rows


@pytest.mark.parametrize('V', VS)
def test_logp_is_within_its_bound_of_float64(V):
    rows = _score_rows(V)
    M = rows.shape[0]
    lg, seeds = _logits(rows), _seeds(M)
    cons = torch.full((M, W), -1, dtype=torch.int64)
    cons[:, 1] = torch.tensor([0, V - 1, 1 if V >= 2 else 0])                     # row 2: a finite code (odd)
    cons[:, 3] = torch.tensor([V // 2, int(rows[1].argmin()), 0])                 # row 2: a code of logit -inf (V >= 2)
    worst = 0.0
    for top_k, top_p in FILTERS:                                                  # neither the filter nor the temperature enters
        logp = Buf(M, W, W + 1)
        run = Run('cons', lg, V, 4, 1.7, min(top_k, V), top_p, seeds, cons=_cons_buf(M, cons), logp=logp)
        codes, got = run.codes.view.cpu(), logp.view.cpu()
        for b in range(M):
            for p in range(N):
                code = int(codes[b, p])
                ref, bound = C.logp_ref(rows[b], code), C.logp_bound(rows[b], code)
                if rows[b, code] == -float('inf'):
                    assert (b, p) == (2, 3) and float(got[b, p]) == -float('inf') and bound == 0.0
                    continue
                err = abs(float(got[b, p]) - ref)
                worst = max(worst, err / bound)
                assert err <= bound, (V, b, p, code, float(got[b, p]), ref, bound)
        if V >= 2:
            assert float(got[2, 3]) == -float('inf')
        exp = logp.before.clone()                                                 # columns [0, N) of the rows, nothing else
        exp[GR:GR + M, :N] = logp.view[:, :N]
        assert same_bits(exp, logp.full)
    print(f'V {V}: worst |logp - float64| / bound = {worst:.3f}')


@pytest.mark.parametrize('V', [17, 1000, 4096])
def test_a_row_has_the_same_bits_alone_and_among_64(V):
    M = 64
    rows = torch.randn(M, V, generator=gen(110 + V)) * 3.0
    seeds = _seeds(M)
    cons = _random_cons(M, V, 120 + V, 0.6)
    table = torch.randn(V + 1, 4, generator=gen(3)).cuda()

    def run(sel):
        logp = Buf(len(sel), W, W + 1)
        r = Run('cons', _logits(rows[sel]), V, 4, 1.3, min(7, V), 0.9, seeds[sel].contiguous(), cons=_cons_buf(len(sel), cons[sel]),
                logp=logp, win=[0, 1], table=table)
        return r.codes.view.clone(), logp.view[:, 1:1 + N].clone()
    codes, logp = run(list(range(M)))
    assert bool(torch.isfinite(logp).all())
    for b in (0, 37, 63):
        c1, l1 = run([b])
        assert torch.equal(c1[0], codes[b]) and same_bits(l1[0], logp[b]), b


# =====================================================================================================================
# (3) addressing, guards, clamping, the end of the window
def test_reads_and_writes_happen_at_the_window_column_alone():
    """win = {., 5}: the forced code of position pos is constraint[b][5 + pos] -- every column holds another code, so a read
    anywhere else shows in the codes -- and logp is written at columns 5 + pos, nowhere else."""
    V, M = 257, 3
    rows = torch.randn(M, V, generator=gen(130)) * 2.0
    cons = (torch.arange(M).view(M, 1) * 31 + torch.arange(W).view(1, W) * 17 + 3) % V
    cb, logp = _cons_buf(M, cons), Buf(M, W, W + 1)
    run = Run('cons', _logits(rows), V, 4, 1.0, 0, 1.0, _seeds(M), cons=cb, logp=logp, win=[77, OFF])
    assert torch.equal(run.codes.view.cpu(), cons[:, OFF:OFF + N])
    cb.assert_untouched()
    exp = logp.before.clone()
    exp[GR:GR + M, OFF:OFF + N] = logp.view[:, OFF:OFF + N]
    assert same_bits(exp, logp.full)
    got = logp.view[:, OFF:OFF + N].cpu()
    for b in range(M):
        for p in range(N):
            code = int(cons[b, OFF + p])
            assert abs(float(got[b, p]) - C.logp_ref(rows[b], code)) <= C.logp_bound(rows[b], code)
    assert run.win.tolist() == [77, OFF]                                           # the sampler never writes the window index


def test_without_a_live_window_nothing_is_forced_and_no_logp_is_written():
    V, M = 17, 3
    lg, seeds = _logits(torch.randn(M, V, generator=gen(131)) * 2.0), _seeds(M)
    logp = Buf(M, W, W + 1)
    run = Run('cons', lg, V, 4, 1.0, 0, 1.0, seeds, cons=_cons_buf(M, torch.zeros(M, W, dtype=torch.int64)), logp=logp,
              win=[0, -1])
    assert run.same_outputs(Run('plain', lg, V, 4, 1.0, 0, 1.0, seeds))
    logp.assert_untouched()


def test_columns_past_the_leading_dimensions_are_free_and_unwritten():
    """ldcons = ldlogp = 7 >= N with win = {., 5}: columns 5 and 6 are forced / written, positions 2 .. 4 (columns 7 .. 9) are
    drawn and leave no logp (the guard rows behind the narrow buffers take what a missing guard would write)."""
    V, M = 255, 3
    lg, seeds = _logits(torch.randn(M, V, generator=gen(132)) * 2.0), _seeds(M)
    cons = torch.full((M, 7), 200, dtype=torch.int64)
    logp = Buf(M, 7, 7)
    run = Run('cons', lg, V, 4, 1.0, 0, 1.0, seeds, cons=_cons_buf(M, cons, width=7, ld=7), logp=logp, win=[0, OFF])
    plain = Run('plain', lg, V, 4, 1.0, 0, 1.0, seeds)
    assert bool((run.codes.view[:, :2] == 200).all()) and torch.equal(run.codes.view[:, 2:], plain.codes.view[:, 2:])
    exp = logp.before.clone()
    exp[GR:GR + M, OFF:7] = logp.view[:, OFF:7]
    assert same_bits(exp, logp.full) and bool(torch.isfinite(logp.view[:, OFF:7]).all())


def test_forced_codes_past_the_vocabulary_are_clamped():
    V, M = 15, 2
    rows = torch.randn(M, V, generator=gen(133)) * 2.0
    cons = torch.full((M, W), -1, dtype=torch.int64)
    cons[0, 0], cons[1, 0], cons[0, 2], cons[1, 2] = V + 7, 2 ** 40, V, V - 1
    logp = Buf(M, W, W + 1)
    run = Run('cons', _logits(rows), V, 4, 1.0, 0, 1.0, _seeds(M), cons=_cons_buf(M, cons), logp=logp)
    codes = run.codes.view.cpu()
    assert codes[:, 0].tolist() == [V - 1, V - 1] and codes[:, 2].tolist() == [V - 1, V - 1]
    assert bool(((codes >= 0) & (codes < V)).all())
    for b, p in ((0, 0), (1, 0)):
        assert abs(float(logp.view[b, p]) - C.logp_ref(rows[b], V - 1)) <= C.logp_bound(rows[b], V - 1)


def test_past_the_window_nothing_at_all_is_written():
    V, M = 17, 3
    lg, seeds = _logits(torch.randn(M, V, generator=gen(134)) * 2.0), _seeds(M)
    cb, logp = _cons_buf(M, torch.zeros(M, W, dtype=torch.int64)), Buf(M, W, W + 1)
    run = Run('cons', lg, V, 4, 1.0, 0, 1.0, seeds, steps=2, pos0=N, cons=cb, logp=logp, win=[0, 0])
    for buf in (run.codes, run.nxt, run.pr, logp, cb):
        buf.assert_untouched()
    assert int(run.pos.item()) == N and int(run.ticket.item()) == 0
