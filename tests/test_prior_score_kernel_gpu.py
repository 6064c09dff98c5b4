"""vqcpc_prior_score (csrc/prior_score.hip) by direct calls: the five outputs against the float64 reference of
tests/prior_score_reference.py within the derived bounds (rank and best exactly), the fused gather / scatter through (row_b, row_col),
and the bit relations that tie the kernel to the samplers it restates -- logp == vqcpc_prior_sample_constrained's with the target
forced, the ncb ascending-stage launches == vqcpc_prior_sample_product's chain -- and to itself (a row alone == the row among 70, two
launches).  Conventions as in tests/test_decode_kernels_gpu.py: outputs sit in sentinel-filled allocations with guard rows and a wider
leading dimension, every input the result must not depend on is NaN or garbage, seeds are fixed.  The logits' leading dimension is
V + 3: row r starts on a 16-byte boundary only when r is a multiple of 4, so both load forms of the kernel run in every case."""
import numpy as np
import pytest
import torch

import prior_constrained_reference as C
import prior_score_reference as PS
from test_decode_kernels_gpu import GR, NAN, Buf, call, gen, same_bits
from test_prior_sample_constrained_gpu import Run, _cons_buf, _seeds
from test_product_codes_kernels_gpu import Step

pytestmark = pytest.mark.gpu

VS = [1, 2, 15, 16, 17, 255, 256, 257, 1024, 1025, 4095, 4096]      # thread ownership (16 codes per thread), the two forms (1024)
RS = [1, 3, 70]
SPREADS = (0.0, 1e-3, 2.0, 80.0)
NINF = -float('inf')
OUTPUTS = (('logp', torch.float32), ('entropy', torch.float32), ('rank', torch.int32), ('best', torch.int64),
           ('best_logp', torch.float32))


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


class ScoreCase:
    """R rows of V logits scattered over the cells of B pieces x cols columns.  A fifth of the rows is skipped (negative column, a
    piece index far outside, NaN logits).  Live row r: spread SPREADS[r % 4]; for V >= 4 and r % 3 == 0 equal logits planted below
    and above the target index (every sixth row: at the row's maximum, so the arg-max ties too); r % 7 == 3: every fourth logit is
    -inf; r % 7 == 5 (V >= 2): the target's own logit is -inf."""

    def __init__(self, V, R, seed, B=3):
        g = gen(seed)
        self.V, self.R, self.B = V, R, B
        self.ldl = V + 3
        self.cols = cols = -(-R // B) + 3
        self.ld, self.ldseq, self.ldlogp = cols + 3, cols + 2, cols + 1
        cells = torch.randperm(B * cols, generator=g)[:R]
        self.b, self.col = (cells // cols).tolist(), (cells % cols).tolist()
        self.live = [not (R >= 3 and r % 5 == 2) for r in range(R)]
        lg = torch.full((R, self.ldl), NAN)
        seq = torch.randint(1 << 40, 1 << 41, (B, cols), generator=g)              # garbage wherever no live row points
        self.rows, self.tok = [None] * R, [None] * R
        for r in range(R):
            if not self.live[r]:
                continue
            row = torch.randn(V, generator=g) * SPREADS[r % 4]
            tok = int(torch.randint(0, V, (1,), generator=g))
            if V >= 4 and r % 3 == 0:
                tok = V // 2
                row[0] = row[V - 1] = row[tok]
                if r % 6 == 0:
                    row[0] = row[V - 1] = row[tok] = row.max() + 1.0
            if r % 7 == 3 and V >= 2:
                row[(tok + 1) % V::4] = NINF
                row[tok] = 0.5
            if r % 7 == 5 and V >= 2:
                row[tok] = NINF
            lg[r, :V] = row
            seq[self.b[r], self.col[r]] = tok
            self.rows[r], self.tok[r] = row, tok
        self.lg = lg.cuda()
        self.seq = Buf(B, cols, self.ldseq, data=seq, dtype=torch.int64)
        self.row_b = torch.tensor([self.b[r] if self.live[r] else 10 ** 6 + r for r in range(R)], dtype=torch.int32).cuda()
        self.row_col = torch.tensor([self.col[r] if self.live[r] else -1 - r for r in range(R)], dtype=torch.int32).cuda()

    def launch(self, skip=(), rows=None):
        """One launch; skip: outputs passed as NULL; rows: these rows only, as an R' = len(rows) call.  -> {name: Buf}."""
        idx = (torch.arange(self.R) if rows is None else torch.as_tensor(rows)).cuda()
        outs = {name: (None if name in skip else Buf(self.B, self.cols, self.ldlogp if name == 'logp' else self.ld, dtype=dt))
                for name, dt in OUTPUTS}
        ptr = lambda name: None if outs[name] is None else outs[name].view
        call('vqcpc_prior_score', self.lg[idx].contiguous(), self.ldl, self.V, 1, 0, len(idx), self.row_b[idx].contiguous(),
             self.row_col[idx].contiguous(), self.seq.view, self.ldseq, self.B, self.cols, ptr('logp'), self.ldlogp, self.ld,
             ptr('entropy'), ptr('rank'), ptr('best'), ptr('best_logp'))
        torch.cuda.synchronize()
        self.seq.assert_untouched()
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


def _check_values(case, outs):
    """Every live row against float64 within the derived bounds; rank and best exactly.  -> the worst |error| / bound per output."""
    host = {k: v.view.cpu() for k, v in outs.items() if v is not None}
    worst = dict(logp=0.0, entropy=0.0, best_logp=0.0)
    for r in range(case.R):
        if not case.live[r]:
            continue
        row, tok, b, col = case.rows[r], case.tok[r], case.b[r], case.col[r]
        ref = PS.prior_score_ref(row.numpy(), tok)
        rank, best = PS.rank_best_fp32(row.numpy(), tok)
        label = (case.V, r, tok)
        assert int(host['rank'][b, col]) == rank == ref['rank'], label
        assert int(host['best'][b, col]) == best == ref['best'], label
        bounds = dict(logp=C.logp_bound(row, tok), best_logp=C.logp_bound(row, best), entropy=PS.entropy_bound(row.numpy()))
        for key, bound in bounds.items():
            got, want = float(host[key][b, col]), ref[key]
            if bound == 0.0 or want == NINF:
                assert got == want, (label, key, got, want)
                continue
            assert abs(got - want) <= bound, (label, key, got, want, bound)
            worst[key] = max(worst[key], abs(got - want) / bound)
        ent = float(host['entropy'][b, col])
        assert -bounds['entropy'] <= ent <= np.log(len(row)) + bounds['entropy'], label
        assert float(host['best_logp'][b, col]) >= float(host['logp'][b, col]), label
        assert (rank == 0) == (best == tok), label
        if float(row[tok]) == NINF:                                                 # a -inf target: -inf exactly, behind every finite code
            assert float(host['logp'][b, col]) == NINF and rank >= int(torch.isfinite(row).sum()), label
    return worst


@pytest.mark.parametrize('R', RS)
def test_outputs_against_float64(R):
    """Every vocabulary size, R rows each: the partial last workgroup of the single-wave form (four rows per workgroup), skipped rows,
    NaN past V, planted ties, -inf entries, a -inf target, guards, wide leading dimensions."""
    total = dict(logp=0.0, entropy=0.0, best_logp=0.0)
    for V in VS:
        case = ScoreCase(V, R, seed=7000 + 7 * R + V)
        outs = case.launch()
        case.assert_written_cells(outs)
        for key, share in _check_values(case, outs).items():
            total[key] = max(total[key], share)
    print(f'R = {R}: worst |error| / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in total.items()))


def test_each_output_may_be_null_and_two_launches_agree():
    for V in (37, 1025):
        case = ScoreCase(V, 37, seed=7100 + V)
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
        case.launch(skip=tuple(n for n, _ in OUTPUTS))                             # nothing asked for: a valid call


@pytest.mark.parametrize('V', [17, 1000, 1024, 1025, 4096])
def test_a_row_alone_equals_the_row_among_70(V):
    case = ScoreCase(V, 70, seed=7200 + V)
    full = case.launch()
    for r in (0, 1, 3, 36, 68, 69):                                  # first / last wave of a workgroup, the partial last workgroup
        assert case.live[r]
        alone = case.launch(rows=[r])
        case.assert_written_cells(alone, rows=[r])
        for name, _ in OUTPUTS:
            assert same_bits(alone[name].view[case.b[r], case.col[r]], full[name].view[case.b[r], case.col[r]]), (r, name)


@pytest.mark.parametrize('R', RS)
def test_logp_has_the_bits_of_the_constrained_sampler(R):
    """The same logits rows through vqcpc_prior_sample_constrained with the target as the constraint (at most 64 rows per sampler
    call): logp bit for bit, targets past the vocabulary (clamped by both) included."""
    for V in VS:
        g = gen(7300 + 11 * R + V)
        rows = torch.randn(R, V, generator=g) * torch.tensor(SPREADS)[torch.arange(R) % 4].view(R, 1)
        if V >= 2:
            rows[R // 2, ::2] = NINF                                                # a row with -inf entries
        lg = torch.full((R, V + 3), NAN)
        lg[:, :V] = rows
        lg = lg.cuda()
        target = torch.randint(0, V, (R,), generator=g)
        target[0] = V + 5                                                            # past the vocabulary: clamped to V - 1
        if R >= 3:
            target[2] = 2 ** 40
        want = torch.empty(R, device='cuda')
        for r0 in range(0, R, 64):
            m = min(64, R - r0)
            cons = torch.full((m, 7), -1, dtype=torch.int64)
            cons[:, 0] = target[r0:r0 + m]
            logp = Buf(m, 7, 8)
            Run('cons', lg[r0:r0 + m].contiguous(), V, 4, 1.0, 0, 1.0, _seeds(m), steps=1, cons=_cons_buf(m, cons, width=7, ld=9),
                logp=logp)
            want[r0:r0 + m] = logp.view[:, 0]
        cols = 5
        col = (torch.arange(R) * 3) % cols
        seq = Buf(R, cols, cols + 2, data=torch.full((R, cols), 1 << 40, dtype=torch.int64), dtype=torch.int64)
        seq.view[torch.arange(R), col] = target.cuda()
        seq.before = seq.full.clone()
        got = Buf(R, cols, cols + 1)
        call('vqcpc_prior_score', lg, V + 3, V, 1, 0, R, torch.arange(R, dtype=torch.int32).cuda(), col.to(torch.int32).cuda(),
             seq.view, cols + 2, R, cols, got.view, cols + 1, 0, None, None, None, None)
        torch.cuda.synchronize()
        assert same_bits(got.view[torch.arange(R), col], want), (V, R)
        exp = got.before.clone()
        exp[GR + torch.arange(R), col] = got.view[torch.arange(R), col]
        assert same_bits(exp, got.full), (V, R)                                      # one cell per row written, nothing else
        seq.assert_untouched()


@pytest.mark.parametrize('K,ncb', [(3, 4), (8, 2), (64, 2), (4096, 1)])
def test_the_stage_launches_have_the_bits_of_the_product_sampler(K, ncb):
    """ncb launches in ascending stage order on one stream against vqcpc_prior_sample_product's chain with the code forced (through
    its constraint: its `teacher` argument excludes logp): logp bit for bit, and every stage's details against float64 at the
    stage's digit.  70 rows: two sampler calls."""
    M, W = 70, 4
    g = gen(7400 + K)
    logits = torch.randn(ncb, M, K, generator=g) * 2.5
    codes = torch.randint(0, K ** ncb, (M, W), generator=g)
    codes[0, 0], codes[1, 0] = K ** ncb + 9, 2 ** 40                                # past the K^ncb codes: clamped by both
    want = torch.empty(M, device='cuda')
    for r0 in range(0, M, 64):
        m = min(64, M - r0)
        s = Step(logits[:, r0:r0 + m], K, ncb, 3, torch.arange(m, dtype=torch.int64) * 977 + 13, cons=codes[r0:r0 + m],
                 want_logp=True)
        s.position()
        torch.cuda.synchronize()
        want[r0:r0 + m] = s.logp[:, 0]
    dev_logits = logits.cuda().contiguous()
    seq = codes.cuda()
    row_b, row_col = torch.arange(M, dtype=torch.int32).cuda(), torch.zeros(M, dtype=torch.int32).cuda()
    ld = W * ncb + 2
    outs = {name: Buf(M, W if name == 'logp' else W * ncb, W + 1 if name == 'logp' else ld, dtype=dt) for name, dt in OUTPUTS}
    for j in range(ncb):
        call('vqcpc_prior_score', dev_logits[j], K, K, ncb, j, M, row_b, row_col, seq, W, M, W, outs['logp'].view, W + 1, ld,
             outs['entropy'].view, outs['rank'].view, outs['best'].view, outs['best_logp'].view)
    torch.cuda.synchronize()
    assert same_bits(outs['logp'].view[:, 0], want), (K, ncb)
    host = {k: v.view.cpu() for k, v in outs.items()}
    for b in range(M):
        for j in range(ncb):
            row = logits[j, b]
            tok = PS.target_digit(int(codes[b, 0]), K, ncb, j)
            ref = PS.prior_score_ref(row.numpy(), tok)
            assert int(host['rank'][b, j]) == ref['rank'] and int(host['best'][b, j]) == ref['best'], (b, j)
            assert abs(float(host['entropy'][b, j]) - ref['entropy']) <= PS.entropy_bound(row.numpy()), (b, j)
            assert abs(float(host['best_logp'][b, j]) - ref['best_logp']) <= C.logp_bound(row, ref['best']), (b, j)
    for name, buf in outs.items():                                                  # column 0's cells (ncb per row), nothing else
        exp = buf.before.clone()
        n = 1 if name == 'logp' else ncb
        exp[GR:GR + M, :n] = buf.view[:, :n]
        assert same_bits(exp, buf.full), name


def test_bad_arguments_are_refused_before_any_launch():
    from vqcpc_bach_amd import hip
    case = ScoreCase(13, 4, seed=7500)
    lp = Buf(case.B, case.cols, case.ldlogp)
    ent = Buf(case.B, case.cols, case.ld)

    def go(logits=case.lg, ldl=case.ldl, V=13, ncb=1, stage=0, R=4, row_b=case.row_b, row_col=case.row_col, seq=case.seq.view,
           ldseq=case.ldseq, B=case.B, cols=case.cols, ldlogp=case.ldlogp, ld=case.ld):
        call('vqcpc_prior_score', logits, ldl, V, ncb, stage, R, row_b, row_col, seq, ldseq, B, cols, lp.view, ldlogp, ld, ent.view,
             None, None, None)
    for kw in (dict(logits=None), dict(row_b=None), dict(row_col=None), dict(seq=None), dict(V=0), dict(V=4097), dict(ncb=0),
               dict(ncb=5), dict(stage=-1), dict(stage=1), dict(R=0), dict(B=0), dict(cols=0), dict(ldl=12),
               dict(ldseq=case.cols - 1), dict(ldlogp=case.cols - 1), dict(ld=case.cols - 1), dict(ncb=2, ld=2 * case.cols - 1)):
        with pytest.raises(hip.VqcpcHipError, match='prior_score'):
            go(**kw)
    torch.cuda.synchronize()
    lp.assert_untouched(), ent.assert_untouched()
    go()
    torch.cuda.synchronize()
    assert not same_bits(lp.full, lp.before) and not same_bits(ent.full, ent.before)
