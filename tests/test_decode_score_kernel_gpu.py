"""vqcpc_decode_score (csrc/score.hip) by direct calls: the six outputs against the float64 reference of tests/score_reference.py
within the derived bounds (rank and best exactly), the fused gather / scatter through (row_b, row_col), and the bit relations that
tie the kernel to the samplers it restates -- logp == vqcpc_decode_sample_constrained's with the target forced, logmass ==
vqcpc_decode_sample_masked's -- and to itself (a row alone == the row among 257, two launches).  Conventions as in
tests/test_decode_kernels_gpu.py: outputs sit in sentinel-filled allocations with guard rows and a wider leading dimension, every
input the result must not depend on is NaN or garbage, seeds are fixed."""
import ctypes

import numpy as np
import pytest
import torch

import constrained_reference as C
import masked_reference as MR
import score_reference as SR
from test_decode_kernels_gpu import GR, NAN, Buf, call, gen, same_bits
from test_decode_sample_constrained_gpu import Case, _nan_logp
from test_decode_sample_masked_gpu import mask_buf, put, random_sets
from test_decode_sample_masked_gpu import run as run_sampler

pytestmark = pytest.mark.gpu

VS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256]
VOICES = (1, 37, 256, 60)                     # nc = 4, unequal vocabularies
SPREADS = (0.0, 1e-3, 2.0, 80.0)
OUTPUTS = (('logp', torch.float32), ('logmass', torch.float32), ('entropy', torch.float32), ('rank', torch.int32),
           ('best', torch.int64), ('best_logp', torch.float32))


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


class ScoreCase:
    """R rows of logits for `widths` voices scattered over the cells of B pieces x cols columns.  A fifth of the rows is skipped
    (negative column, a piece index far outside, NaN logits).  Live row r: logits NaN outside its voice, spread SPREADS[r % 4],
    and for V >= 4 equal logits planted below and above the target index (every sixth row: at the row's maximum, so the arg-max
    ties too); its set is full / empty inside the vocabulary / one-hot / random by r % 4."""

    def __init__(self, widths, R, seed, B=3):
        g = gen(seed)
        self.widths, self.nc, self.R, self.B = tuple(widths), len(widths), R, B
        self.off = np.concatenate([[0], np.cumsum(widths)]).astype(int)
        self.offs = (ctypes.c_int32 * (self.nc + 1))(*self.off.tolist())
        self.vtot = int(self.off[-1])
        self.ldl = self.vtot + 6
        self.cols = cols = max(2 * self.nc, -(-R // B) + 3)
        self.ld, self.ldch, self.ldallow = cols + 3, cols + 2, cols + 1
        cells = torch.randperm(B * cols, generator=g)[:R]
        self.b, self.col = (cells // cols).tolist(), (cells % cols).tolist()
        self.live = [not (R >= 3 and r % 5 == 2) for r in range(R)]
        lg = torch.full((R, self.ldl), NAN)
        chorale = torch.randint(1 << 40, 1 << 41, (B, cols), generator=g)          # garbage wherever no live row points
        self.allowed = mask_buf(B, cols, self.ldallow, seed + 1)
        self.rows, self.tok, self.sets = [None] * R, [None] * R, [None] * R
        for r in range(R):
            if not self.live[r]:
                continue
            c = self.col[r] % self.nc
            V = self.widths[c]
            row = torch.randn(V, generator=g) * SPREADS[r % 4]
            tok = int(torch.randint(0, V, (1,), generator=g))
            if V >= 4:
                tok = V // 2 if r % 3 == 0 else tok
                if r % 3 == 0:
                    row[0] = row[V - 1] = row[tok]
                if r % 6 == 0:
                    row[0] = row[V - 1] = row[tok] = row.max() + 1.0
            kind = r % 4
            s = torch.ones(256, dtype=torch.bool) if kind == 0 else torch.zeros(256, dtype=torch.bool)
            if kind == 1:
                s[V:] = torch.rand(256 - V, generator=g) < 0.5                     # bits at or past V only: no restriction
            elif kind == 2:
                s[int(torch.randint(0, V, (1,), generator=g))] = True
            elif kind == 3:
                s = random_sets(1, V, g)[0]
            lg[r, self.off[c]:self.off[c + 1]] = row
            chorale[self.b[r], self.col[r]] = tok
            self.rows[r], self.tok[r], self.sets[r] = row, tok, s
            self.allowed.view[self.b[r], self.col[r] * 8:(self.col[r] + 1) * 8] = torch.from_numpy(_pack(s.numpy())).cuda()
        self.allowed.before = self.allowed.full.clone()
        self.lg = lg.cuda()
        self.chorale = Buf(B, cols, self.ldch, data=chorale, dtype=torch.int64)
        self.row_b = torch.tensor([self.b[r] if self.live[r] else 10 ** 6 + r for r in range(R)], dtype=torch.int32).cuda()
        self.row_col = torch.tensor([self.col[r] if self.live[r] else -1 - r for r in range(R)], dtype=torch.int32).cuda()

    def launch(self, skip=(), allowed=True, rows=None):
        """One launch; skip: outputs passed as NULL; rows: these rows only, as an R' = len(rows) call.  -> {name: Buf}."""
        idx = torch.arange(self.R) if rows is None else torch.as_tensor(rows)
        outs = {name: (None if name in skip else Buf(self.B, self.cols, self.ld, dtype=dt)) for name, dt in OUTPUTS}
        ptr = lambda name: None if outs[name] is None else outs[name].view
        call('vqcpc_decode_score', self.lg[idx.cuda()].contiguous(), self.ldl, self.offs, self.nc, len(idx),
             self.row_b[idx.cuda()].contiguous(), self.row_col[idx.cuda()].contiguous(), self.chorale.view, self.ldch,
             self.allowed.view if allowed else None, self.ldallow if allowed else 0, self.B, self.cols, self.ld,
             *[ptr(name) for name, _ in OUTPUTS])
        torch.cuda.synchronize()
        self.chorale.assert_untouched(), self.allowed.assert_untouched()
        return outs

    def assert_written_cells(self, outs, rows=None):
        """Exactly the live rows' cells were written: everything else, guards and padding included, keeps its bits."""
        rows = range(self.R) if rows is None else rows
        cells = [(self.b[r], self.col[r]) for r in rows if self.live[r]]
        for name, buf in outs.items():
            if buf is None:
                continue
            exp = buf.before.clone()
            for b, col in cells:
                exp[GR + b, col] = buf.full[GR + b, col]
                assert not same_bits(buf.full[GR + b, col], buf.before[GR + b, col]), (name, b, col, 'not written')
            assert same_bits(exp, buf.full), name


def _pack(bits):
    """bool (256,) -> int32 words (8,), bit i & 31 of word i >> 5."""
    return np.packbits(np.asarray(bits, dtype=bool), bitorder='little').view('<i4').copy()


def _check_values(case, outs):
    """Every live row against float64 within the derived bounds; rank and best exactly.  -> the worst |error| / bound per output."""
    host = {k: v.view.cpu() for k, v in outs.items() if v is not None}
    worst = dict(logp=0.0, logmass=0.0, entropy=0.0, best_logp=0.0)
    for r in range(case.R):
        if not case.live[r]:
            continue
        row, tok, b, col = case.rows[r], case.tok[r], case.b[r], case.col[r]
        ref = SR.score_ref(row.numpy(), tok, case.sets[r].numpy())
        rank, best = SR.rank_best_fp32(row.numpy(), tok)
        label = (case.widths, r, tok)
        assert int(host['rank'][b, col]) == rank == ref['rank'], label
        assert int(host['best'][b, col]) == best == ref['best'], label
        bounds = dict(logp=C.logp_bound(row, tok), best_logp=C.logp_bound(row, best), entropy=SR.entropy_bound(row.numpy()),
                      logmass=MR.logmass_bound(row, case.sets[r]))
        for key, bound in bounds.items():
            got, want = float(host[key][b, col]), ref[key]
            if bound == 0.0 or want == -float('inf'):
                assert got == want, (label, key, got, want)
                continue
            assert abs(got - want) <= bound, (label, key, got, want, bound)
            worst[key] = max(worst[key], abs(got - want) / bound)
        ent = float(host['entropy'][b, col])
        assert -bounds['entropy'] <= ent <= np.log(len(row)) + bounds['entropy'], label
        assert float(host['best_logp'][b, col]) >= float(host['logp'][b, col]), label
        assert (rank == 0) == (best == tok), label
    return worst


@pytest.mark.parametrize('R', [1, 3, 4, 5, 257])
def test_outputs_against_float64(R):
    """Every vocabulary size alone (nc = 1) and four unequal voices, R rows each: the partial last workgroup (four rows per
    workgroup), skipped rows, NaN outside the row's voice, guards, wide leading dimensions."""
    total = dict(logp=0.0, logmass=0.0, entropy=0.0, best_logp=0.0)
    for widths in [(V,) for V in VS] + [VOICES]:
        case = ScoreCase(widths, R, seed=3000 + 7 * R + sum(widths))
        outs = case.launch()
        case.assert_written_cells(outs)
        for key, share in _check_values(case, outs).items():
            total[key] = max(total[key], share)
    print(f'R = {R}: worst |error| / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in total.items()))


def test_each_output_may_be_null_and_two_launches_agree():
    case = ScoreCase(VOICES, 37, seed=3100)
    full = case.launch()
    again = case.launch()
    for name, _ in OUTPUTS:
        assert same_bits(full[name].full, again[name].full), name
    for name, _ in OUTPUTS:
        part = case.launch(skip=(name,))
        case.assert_written_cells(part)
        for other, _ in OUTPUTS:
            if other != name:
                assert same_bits(part[other].full, full[other].full), (name, other)
    only = case.launch(skip=tuple(n for n, _ in OUTPUTS if n != 'rank'))
    assert same_bits(only['rank'].full, full['rank'].full)
    free = case.launch(allowed=False)                              # no sets at all: the full set, exactly +0.0f
    case.assert_written_cells(free)
    for r in range(case.R):
        if case.live[r]:
            assert same_bits(free['logmass'].view[case.b[r], case.col[r]].cpu(), torch.zeros(())), r
    for name, _ in OUTPUTS:
        if name != 'logmass':
            assert same_bits(free[name].full, full[name].full), name


def test_a_row_alone_equals_the_row_among_257():
    case = ScoreCase(VOICES, 257, seed=3200)
    full = case.launch()
    for r in (0, 1, 3, 128, 255, 256):                             # first / last wave of a workgroup, the partial last workgroup
        assert case.live[r]
        alone = case.launch(rows=[r])
        case.assert_written_cells(alone, rows=[r])
        for name, _ in OUTPUTS:
            assert same_bits(alone[name].view[case.b[r], case.col[r]], full[name].view[case.b[r], case.col[r]]), (r, name)


def _score_rows(case, step, chorale, ld, allowed=None, ldallow=0):
    """The sampler case's rows of one step through vqcpc_decode_score: piece b = row b, column = the step's position."""
    M, col = case.M, case.pos0 + step
    lp, lm = _nan_logp(M, case.T, ld), _nan_logp(M, case.T, ld)
    call('vqcpc_decode_score', case.lg[step], case.ldl, case.offs, case.nc, M, torch.arange(M, dtype=torch.int32).cuda(),
         torch.full((M,), col, dtype=torch.int32).cuda(), chorale, case.T, allowed, ldallow, M, case.T, ld, lp.view, lm.view,
         None, None, None, None)
    torch.cuda.synchronize()
    return lp, lm


@pytest.mark.parametrize('M', [1, 17, 64])
def test_logp_has_the_bits_of_the_constrained_sampler(M):
    """The same logits rows through vqcpc_decode_sample_constrained with the target forced: logp bit for bit."""
    steps = 3
    for widths in [(V,) for V in VS] + [VOICES]:
        case = Case(M, widths, steps, U=1, T_=steps + 2, seed=4000 * M + sum(widths))
        T_ = case.T
        g = gen(41 * M + sum(widths))
        forced = torch.stack([torch.randint(0, widths[s % len(widths)], (M,), generator=g) if s < steps else
                              torch.zeros(M, dtype=torch.int64) for s in range(T_)], dim=1).cuda()
        want = _nan_logp(M, T_, T_ + 2)
        out = run_sampler(case, 'cons', constraint=forced, ldcons=T_, logp=want.view, ldlogp=T_ + 2)
        assert torch.equal(out['tok'][:, :steps], forced[:, :steps].cpu())
        for s in range(steps):
            lp, lm = _score_rows(case, s, forced, T_ + 2)
            assert same_bits(lp.view[:, s], want.view[:, s]), (M, widths, s)
            exp = lp.before.clone()
            exp[GR:GR + M, s] = lp.view[:, s]
            assert same_bits(exp, lp.full), (M, widths, s)                          # one column written, nothing else
            assert bool((lm.view[:, s] == 0.0).all())                              # no sets: the full set


@pytest.mark.parametrize('M', [1, 17, 64])
def test_logmass_has_the_bits_of_the_masked_sampler(M):
    """Full, empty, one-hot and random sets (by row) through vqcpc_decode_sample_masked: logmass bit for bit, logp too."""
    steps = 2
    for widths in [(V,) for V in VS] + [VOICES]:
        case = Case(M, widths, steps, U=1, T_=steps + 2, seed=5000 * M + sum(widths))
        T_ = case.T
        g = gen(43 * M + sum(widths))
        al = mask_buf(M, T_, T_ + 1, 44 * M + sum(widths))
        forced = torch.zeros(M, T_, dtype=torch.int64)
        for s in range(steps):
            V = widths[s % len(widths)]
            sets = random_sets(M, V, g)
            sets[0::4] = True                                                        # full
            sets[1::4] = False                                                       # empty: no restriction
            hot = torch.randint(0, V, (M,), generator=g)
            sets[2::4] = False
            sets[torch.arange(M)[2::4], hot[2::4]] = True                            # one-hot
            forced[:, s] = torch.where(sets[torch.arange(M), hot], hot, sets[:, :V].int().argmax(1))      # inside the set, or any
            forced[1::4, s] = hot[1::4]
            put(al, s, sets)
        forced = forced.cuda()
        want_lp, want_lm = _nan_logp(M, T_, T_ + 2), _nan_logp(M, T_, T_ + 2)
        run_sampler(case, 'masked', constraint=forced, ldcons=T_, logp=want_lp.view, ldlogp=T_ + 2, allowed=al.view, ldallow=T_ + 1,
                    logmass=want_lm.view, ldmass=T_ + 2)
        for s in range(steps):
            lp, lm = _score_rows(case, s, forced, T_ + 2, allowed=al.view, ldallow=T_ + 1)
            assert same_bits(lm.view[:, s], want_lm.view[:, s]), (M, widths, s)
            assert same_bits(lp.view[:, s], want_lp.view[:, s]), (M, widths, s)
            assert bool((lm.view[0::4, s] == 0.0).all()) and bool((lm.view[1::4, s] == 0.0).all())
        al.assert_untouched()


def test_bad_arguments_are_refused_before_any_launch():
    from vqcpc_bach_amd import hip
    case = ScoreCase((13,), 4, seed=3300)
    lp = Buf(case.B, case.cols, case.ld)

    def go(logits=case.lg, ldl=case.ldl, offs=case.offs, nc=1, R=4, row_b=case.row_b, row_col=case.row_col,
           chorale=case.chorale.view, ldch=case.ldch, allowed=case.allowed.view, ldallow=case.ldallow, B=case.B, cols=case.cols,
           ld=case.ld):
        call('vqcpc_decode_score', logits, ldl, offs, nc, R, row_b, row_col, chorale, ldch, allowed, ldallow, B, cols, ld,
             lp.view, None, None, None, None, None)
    wide = (ctypes.c_int32 * 2)(0, 257)
    for kw in (dict(logits=None), dict(row_b=None), dict(row_col=None), dict(chorale=None), dict(nc=0), dict(nc=17), dict(R=0),
               dict(B=0), dict(cols=0), dict(ldl=12), dict(ldch=case.cols - 1), dict(ld=case.cols - 1),
               dict(ldallow=case.cols - 1), dict(offs=wide)):
        with pytest.raises(hip.VqcpcHipError, match='decode_score'):
            go(**kw)
    torch.cuda.synchronize()
    lp.assert_untouched()
    go()
    torch.cuda.synchronize()
    assert not same_bits(lp.full, lp.before)
