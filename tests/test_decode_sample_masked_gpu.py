"""vqcpc_decode_sample_masked (csrc/decode.hip) by direct calls: bit-identity with vqcpc_decode_sample_constrained where the
two must agree (full sets; row b against the row alone with exclude = global exclusion U not-allowed; one-hot sets against
forcing), logmass against float64 within the derived bound of tests/masked_reference.py, the addressing through the device
window index, and the edges.  Conventions as in tests/test_decode_sample_constrained_gpu.py: outputs sit in sentinel-filled
allocations with guard rows and wider leading dimensions, the mask words of every column the step must not read are garbage."""
import numpy as np
import pytest
import torch

import masked_reference as MR
from test_decode_kernels_gpu import GR, Buf, _i32_words, call, gen, same_bits
from test_decode_sample_constrained_gpu import D_, SAMPLING, Case, _nan_logp, assert_same_outputs

pytestmark = pytest.mark.gpu

PLAIN = dict(temperature=1.0, top_k=0, top_p=1.0)
VS = [1, 2, 4, 5, 32, 33, 64, 65, 255, 256]        # the four-tokens-per-lane and the 32-bit word boundaries


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


def pack(bits):
    """bool (..., 256) -> int64 words (..., 8), bit i & 31 of word i >> 5."""
    b = np.ascontiguousarray(np.asarray(bits, dtype=bool))
    by = np.packbits(b.reshape(b.shape[:-1] + (32, 8)), axis=-1, bitorder='little').reshape(b.shape[:-1] + (32,))
    return np.ascontiguousarray(by).view('<u4').astype(np.int64)


def mask_buf(M, cols, ld, seed):
    """The packed-set buffer [M][ld][8] inside guards, every word garbage."""
    g = np.random.default_rng(seed)
    data = _i32_words(g.integers(0, 1 << 32, size=(M, cols * 8), dtype=np.int64))
    return Buf(M, cols * 8, ld * 8, data=data, dtype=torch.int32)


def put(buf, col, bits):
    """bits bool (M, 256) -> the words of column `col` of every row."""
    buf.view[:, col * 8:(col + 1) * 8] = _i32_words(pack(bits))
    buf.before = buf.full.clone()


def random_sets(M, V, g, density=0.5):
    """bool (M, 256): random bits everywhere (those at or past V must not matter), at least one inside [0, V)."""
    a = torch.rand(M, 256, generator=g) < density
    a[torch.arange(M), torch.randint(0, V, (M,), generator=g)] = True
    return a


def run(case, entry, rows=None, excl=None, sampling=SAMPLING, constraint=None, ldcons=0, logp=None, ldlogp=0, win=None,
        allowed=None, ldallow=0, logmass=None, ldmass=0):
    """case.steps steps of `entry` ('cons' or 'masked').  rows: these rows only, as an M' = len(rows) call on the same logits
    and seeds (the per-row arguments are the caller's).  excl: per step, the exclusion words (default: the case's)."""
    idx = torch.arange(case.M) if rows is None else torch.as_tensor(rows)
    M, T_ = len(idx), case.T
    pos = torch.full((1,), case.pos0, dtype=torch.int32, device='cuda')
    tokens = Buf(M, T_, T_ + 3, dtype=torch.int64)
    seeds = case.seeds[idx.cuda()].contiguous()
    nxt, prs = [], []
    for s in range(case.steps):
        n, p = Buf(M, D_, D_ + 3), Buf(M, 256, 256 + 4)
        lg = case.lg[s][idx.cuda()].contiguous()
        head = (lg, case.ldl, case.offs, case.nc, M, float(sampling['temperature']), int(sampling['top_k']),
                float(sampling['top_p']), case.excl if excl is None else excl[s], seeds, constraint, ldcons, logp, ldlogp, win)
        tail = (tokens.view, T_ + 3, T_, case.table, case.table_rows, D_, case.U, n.view, D_ + 3, p.view, 256 + 4, pos)
        if entry == 'cons':
            call('vqcpc_decode_sample_constrained', *head, *tail)
        else:
            call('vqcpc_decode_sample_masked', *head, allowed, ldallow, logmass, ldmass, *tail)
        torch.cuda.synchronize()
        n.assert_only(), p.assert_only()
        nxt.append(n.full.clone()), prs.append(p.full.clone())
    tokens.assert_only()
    return dict(tokens=tokens.full.clone(), tok=tokens.view.cpu().clone(), nxt=nxt, probs=prs, pos=int(pos.item()))


def excl_words(case, c, sets_row, V):
    """The exclusion words [nc * 8] of one row: the case's, with voice c's joined with the complement of the row's set -- or
    the case's alone when the set has no bit inside [0, V) (no restriction)."""
    words = case.excl.clone()
    if bool(sets_row[:V].any()):
        words[c * 8:(c + 1) * 8] |= _i32_words(pack(~sets_row.numpy()))
    return words


def check_logmass(case, lm, sets, cols, label):
    """logmass column cols[s] of step s against float64 within the derived bound; exact where the bound is 0."""
    worst = 0.0
    for s in range(case.steps):
        for b in range(case.M):
            row, a = case.rows[s][b], sets[s][b]
            got, want, bound = float(lm[b, cols[s]]), MR.logmass_ref(row, a), MR.logmass_bound(row, a)
            if want == -float('inf') or bound == 0.0:
                assert got == want, (label, s, b, got, want)
                continue
            assert abs(got - want) <= bound, (label, s, b, got, want, bound)
            worst = max(worst, abs(got - want) / bound)
    return worst


@pytest.mark.parametrize('M', [1, 16, 17, 64])
def test_masked_sampler_against_the_constrained_one(M):
    steps = 2
    worst = 0.0
    for V in VS:
        excl = {0: (1, 200) if V > 200 else (1,) if V >= 4 else (40,)}             # V < 4: a set bit past the vocabulary
        case = Case(M, (V,), steps, U=1, T_=steps + 2, seed=2000 * M + V, exclude=excl)
        T_, label = case.T, (M, V)
        g = gen(7 * M + V)
        forced = torch.randint(0, V, (M, T_), generator=g)
        mixed = torch.where(torch.rand(M, T_, generator=g) < 0.25, forced, torch.full_like(forced, -1)).cuda()
        lp0 = _nan_logp(M, T_, T_ + 2)
        cons = run(case, 'cons', constraint=mixed, ldcons=T_, logp=lp0.view, ldlogp=T_ + 2)
        assert cons['pos'] == steps

        # (a) no mask at all, and the full set in every column that is read: the constrained entry point, bit for bit
        lp = _nan_logp(M, T_, T_ + 2)
        out = run(case, 'masked', constraint=mixed, ldcons=T_, logp=lp.view, ldlogp=T_ + 2)
        assert_same_outputs(out, cons, (label, 'allowed NULL'))
        assert same_bits(lp.full, lp0.full), label
        ones = torch.ones(M, 256, dtype=torch.bool)
        al, lm, lp = mask_buf(M, T_, T_ + 1, 11 * M + V), _nan_logp(M, T_, T_ + 3), _nan_logp(M, T_, T_ + 2)
        for s in range(steps):
            put(al, s, ones)
        out = run(case, 'masked', constraint=mixed, ldcons=T_, logp=lp.view, ldlogp=T_ + 2, allowed=al.view, ldallow=T_ + 1,
                  logmass=lm.view, ldmass=T_ + 3)
        assert_same_outputs(out, cons, (label, 'full sets'))
        assert same_bits(lp.full, lp0.full), label
        exp = lm.before.clone()
        exp[GR:GR + M, :steps] = 0.0                                                # exactly +0.0f, nothing else written
        assert same_bits(exp, lm.full), label
        al.assert_untouched()

        # (b) bits at or past V only: no restriction, logmass 0.0f
        if V < 256:
            high = torch.zeros(M, 256, dtype=torch.bool)
            high[:, V:] = torch.rand(M, 256 - V, generator=g) < 0.5
            high[:, V] = True
            lm = _nan_logp(M, T_, T_ + 3)
            for s in range(steps):
                put(al, s, high)
            out = run(case, 'masked', constraint=mixed, ldcons=T_, allowed=al.view, ldallow=T_ + 1, logmass=lm.view, ldmass=T_ + 3)
            assert_same_outputs(out, cons, (label, 'bits past V'))
            assert same_bits(exp, lm.full), label

        # (c) random half-density sets per row and column; nothing forced here so that every row draws
        sets = [random_sets(M, V, g) for _ in range(steps)]
        banned = torch.zeros(256, dtype=torch.bool)
        banned[list(excl[0])] = True
        for s in range(steps):
            sets[s][~(sets[s] & ~banned)[:, :V].any(1), 0] = True                 # token 0 is never excluded: a draw is left
            put(al, s, sets[s])
        lp, lm = _nan_logp(M, T_, T_ + 2), _nan_logp(M, T_, T_ + 3)
        out = run(case, 'masked', logp=lp.view, ldlogp=T_ + 2, allowed=al.view, ldallow=T_ + 1, logmass=lm.view, ldmass=T_ + 3)
        assert out['pos'] == steps
        lp_all, lm_all = lp.view.cpu().clone(), lm.view.cpu().clone()
        for s in range(steps):
            pr = out['probs'][s][GR:GR + M, :V].cpu()
            assert bool((pr[~sets[s][:, :V]] == 0).all()), (label, s)              # no mass outside the sets
            assert bool(sets[s][torch.arange(M), out['tok'][:, s]].all()), (label, s)
        worst = max(worst, check_logmass(case, lm_all, sets, list(range(steps)), label))
        exp = lm.before.clone()
        exp[GR:GR + M, :steps] = lm.view[:, :steps]
        assert same_bits(exp, lm.full), label
        for b in range(M):       # row b alone through the CONSTRAINED entry point with exclude = global U not-allowed
            lp1 = _nan_logp(1, T_, T_ + 2)
            alone = run(case, 'cons', rows=[b], excl=[excl_words(case, 0, sets[s][b], V) for s in range(steps)], logp=lp1.view,
                        ldlogp=T_ + 2)
            assert torch.equal(alone['tok'][0], out['tok'][b]), (label, b)
            for s in range(steps):
                assert same_bits(alone['probs'][s][GR], out['probs'][s][GR + b]), (label, b, s)
                assert same_bits(alone['nxt'][s][GR], out['nxt'][s][GR + b]), (label, b, s)
            assert same_bits(lp1.view.cpu()[0], lp_all[b]), (label, b)
        for b in sorted({0, M - 1}):                                                # logmass of the row alone: M = 1
            al1, lm1 = mask_buf(1, T_, T_ + 1, 13), _nan_logp(1, T_, T_ + 3)
            for s in range(steps):
                put(al1, s, sets[s][b:b + 1])
            alone = run(case, 'masked', rows=[b], allowed=al1.view, ldallow=T_ + 1, logmass=lm1.view, ldmass=T_ + 3)
            assert torch.equal(alone['tok'][0], out['tok'][b]), (label, b)
            assert same_bits(lm1.view.cpu()[0], lm_all[b]), (label, b)

        # (d) one-hot sets are forcing; a forced token outside its set is still emitted and logmass is still the set's
        if V >= 2:
            pick = forced[:, :steps]
            hot = [torch.zeros(M, 256, dtype=torch.bool) for _ in range(steps)]
            for s in range(steps):
                hot[s][torch.arange(M), pick[:, s]] = True
                put(al, s, hot[s])
            force_all = torch.full((M, T_), -1, dtype=torch.int64)
            force_all[:, :steps] = pick
            off = [None] * steps                                                    # no exclusion: it could close a one-hot set
            want = run(case, 'cons', excl=off, constraint=force_all.cuda(), ldcons=T_)
            out = run(case, 'masked', excl=off, allowed=al.view, ldallow=T_ + 1)
            assert same_bits(out['tokens'], want['tokens']), label
            for s in range(steps):
                assert same_bits(out['nxt'][s], want['nxt'][s]), (label, s)
            other = force_all.clone()
            other[:, :steps] = (pick + 1) % V
            lm = _nan_logp(M, T_, T_ + 3)
            out = run(case, 'masked', constraint=other.cuda(), ldcons=T_, allowed=al.view, ldallow=T_ + 1, logmass=lm.view,
                      ldmass=T_ + 3)
            assert torch.equal(out['tok'][:, :steps], other[:, :steps]), label
            check_logmass(case, lm.view.cpu(), hot, list(range(steps)), (label, 'forced outside'))
    print(f'M = {M}: worst |logmass - float64| / bound = {worst:.3f}')


def test_logmass_of_wide_and_infinite_rows():
    """V = 256: a row spanning +- 80, a row whose even entries are -inf with a set inside them (-inf exactly) and a set across
    them, a row of one finite entry with a set that holds it (0 exactly: all of the mass) and one that does not (-inf)."""
    V, M = 256, 6
    case = Case(M, (V,), 1, U=1, T_=2, seed=180, scale=3.0)
    wide = torch.linspace(-80.0, 80.0, V)[torch.randperm(V, generator=gen(181))]
    holes = torch.randn(V, generator=gen(182)) * 3.0
    holes[::2] = -float('inf')
    single = torch.full((V,), -float('inf'))
    single[77] = 0.3
    for b, row in enumerate((wide, wide, holes, holes, single, single)):
        case.set_row(0, b, row)
    g = gen(183)
    sets = random_sets(M, V, g)
    sets[1] = wide < 0                                                            # the lower half of the wide row: a tiny mass
    sets[2] = False
    sets[2, 0:20:2] = True                                                        # -inf logits only
    sets[4] = False
    sets[4, 70:80] = True
    sets[5] = False
    sets[5, 0:77] = True
    al, lm = mask_buf(M, 2, 3, 184), _nan_logp(M, 2, 5)
    put(al, 0, sets)
    out = run(case, 'masked', sampling=PLAIN, allowed=al.view, ldallow=3, logmass=lm.view, ldmass=5)
    got = lm.view.cpu()
    worst = check_logmass(case, got, [sets], [0], 'wide')
    print(f'logmass wide / -inf rows: worst |error| / bound = {worst:.3f}; logmass = {got[:, 0].tolist()}')
    assert float(got[2, 0]) == -float('inf') and float(got[5, 0]) == -float('inf') and float(got[4, 0]) == 0.0
    assert -200.0 < float(got[1, 0]) < -70.0 and bool(torch.isfinite(got[[0, 1, 3, 4], 0]).all())
    assert bool(torch.isnan(got[:, 1]).all())
    assert int(out['tok'][4, 0]) == 77 and bool(sets[torch.arange(M), out['tok'][:, 0]][[0, 1, 3, 4]].all())


def test_masked_sampler_with_several_voices():
    """nc = 4 voices of widths (1, 37, 256, 60) at their own offsets, pos walked over two rounds and a step, per-voice exclusion
    words, a mixed constraint: every row equals the row alone through the constrained entry point with its voice's exclusion
    joined with the complement of its set; logmass against float64 per voice."""
    widths, M, steps = (1, 37, 256, 60), 5, 9
    excl = {1: (0, 31, 32), 2: (0, 31, 32, 255), 3: (0, 31, 32)}
    case = Case(M, widths, steps, U=8, T_=12, seed=170, exclude=excl)
    T_ = case.T
    g = gen(171)
    sets = [random_sets(M, widths[s % 4], g) for s in range(steps)]
    for s in range(steps):                                                        # something survives the exclusion
        sets[s][:, 1] = widths[s % 4] > 1
    cons = torch.full((M, T_), -1, dtype=torch.int64)
    for s in range(steps):
        pick = torch.rand(M, generator=g) < 0.3
        cons[:, s] = torch.where(pick, torch.randint(0, widths[s % 4], (M,), generator=g), cons[:, s])
    al, lm, lp = mask_buf(M, T_, T_ + 2, 172), _nan_logp(M, T_, T_ + 5), _nan_logp(M, T_, T_ + 1)
    for s in range(steps):
        put(al, s, sets[s])
    out = run(case, 'masked', constraint=cons.cuda(), ldcons=T_, logp=lp.view, ldlogp=T_ + 1, allowed=al.view, ldallow=T_ + 2,
              logmass=lm.view, ldmass=T_ + 5)
    assert out['pos'] == steps
    forced = cons[:, :steps] >= 0
    assert torch.equal(out['tok'][:, :steps][forced], cons[:, :steps][forced])
    check_logmass(case, lm.view.cpu(), sets, list(range(steps)), 'voices')
    exp = lm.before.clone()
    exp[GR:GR + M, :steps] = lm.view[:, :steps]
    assert same_bits(exp, lm.full)
    for b in range(M):
        lp1 = _nan_logp(1, T_, T_ + 1)
        words = [excl_words(case, s % 4, sets[s][b], widths[s % 4]) for s in range(steps)]
        alone = run(case, 'cons', rows=[b], excl=words, constraint=cons[b:b + 1].cuda(), ldcons=T_, logp=lp1.view, ldlogp=T_ + 1)
        assert torch.equal(alone['tok'][0], out['tok'][b]), b
        for s in range(steps):
            assert same_bits(alone['probs'][s][GR], out['probs'][s][GR + b]), (b, s)
            assert same_bits(alone['nxt'][s][GR], out['nxt'][s][GR + b]), (b, s)
        assert same_bits(lp1.view.cpu()[0], lp.view.cpu()[b]), b


@pytest.mark.parametrize('M', [3, 17])
def test_window_addressing(M):
    """win = {x, w0}: the sets are read and logmass is written at column w0 * U + pos and nowhere else -- every other column
    holds a one-hot set of ANOTHER token.  win[1] = -1: nothing masked, nothing written.  A column at or past the leading
    dimensions is free / not written."""
    V, U, S = 13, 4, 2
    T_, pos0, steps, w0, nbU = S * U, 5, 2, 3, 30
    case = Case(M, (V,), steps, U=U, T_=T_, seed=190 + M, pos0=pos0)
    plain = run(case, 'cons')
    assert plain['pos'] == pos0 + steps
    cols = [w0 * U + pos0 + s for s in range(steps)]
    want = (plain['tok'][:, pos0] + 1) % V                                            # differs from the free draw
    al = mask_buf(M, nbU, nbU + 3, 191)
    for col in range(nbU):                                                            # decoys: what any other column would force
        hot = torch.zeros(M, 256, dtype=torch.bool)
        hot[torch.arange(M), (want + 1 + col % 3) % V] = True
        put(al, col, hot)
    hot = torch.zeros(M, 256, dtype=torch.bool)
    hot[torch.arange(M), want] = True
    put(al, cols[0], hot)
    put(al, cols[1], torch.ones(M, 256, dtype=torch.bool))
    win = torch.tensor([99, w0], dtype=torch.int32).cuda()
    lm = _nan_logp(M, nbU, nbU + 2)
    out = run(case, 'masked', win=win, allowed=al.view, ldallow=nbU + 3, logmass=lm.view, ldmass=nbU + 2)
    assert out['pos'] == pos0 + steps and win.tolist() == [99, w0]
    assert torch.equal(out['tok'][:, pos0], want)
    assert torch.equal(out['tok'][:, pos0 + 1], plain['tok'][:, pos0 + 1])
    exp = lm.before.clone()
    exp[GR:GR + M, cols] = lm.view[:, cols]
    assert same_bits(exp, lm.full) and bool(torch.isfinite(lm.view[:, cols]).all())
    got = lm.view.cpu()
    assert bool((got[:, cols[1]] == 0.0).all())
    for b in range(M):
        ref, bound = MR.logmass_ref(case.rows[0][b], hot[b]), MR.logmass_bound(case.rows[0][b], hot[b])
        assert abs(float(got[b, cols[0]]) - ref) <= bound, b
    # col = pos without win: the decoy at column pos0 decides
    assert torch.equal(run(case, 'masked', allowed=al.view, ldallow=nbU + 3)['tok'][:, pos0], (want + 1 + pos0 % 3) % V)
    # no live window
    dead = torch.tensor([0, -1], dtype=torch.int32).cuda()
    lm2 = _nan_logp(M, nbU, nbU + 2)
    out = run(case, 'masked', win=dead, allowed=al.view, ldallow=nbU + 3, logmass=lm2.view, ldmass=nbU + 2)
    assert_same_outputs(out, plain, 'win[1] = -1')
    lm2.assert_untouched()
    # a window whose columns lie past the leading dimensions: free, not written (never out of bounds)
    far = torch.tensor([0, 1000], dtype=torch.int32).cuda()
    out = run(case, 'masked', win=far, allowed=al.view, ldallow=nbU + 3, logmass=lm2.view, ldmass=nbU + 2)
    assert_same_outputs(out, plain, 'window past ldallow')
    lm2.assert_untouched()
    # columns inside ldmass but past ldallow: free, and logmass says so (0.0f)
    out = run(case, 'masked', win=win, allowed=al.view, ldallow=cols[0], logmass=lm2.view, ldmass=nbU + 2)
    assert_same_outputs(out, plain, 'col >= ldallow')
    assert bool((lm2.view[:, cols] == 0.0).all())
    al.assert_untouched()


def test_nothing_happens_past_the_last_position():
    V, T_ = 13, 6
    case = Case(4, (V,), 1, U=1, T_=T_, seed=195, pos0=T_)
    cons = torch.zeros(4, T_ + 4, dtype=torch.int64).cuda()
    lp, lm, al = _nan_logp(4, T_ + 4, T_ + 6), _nan_logp(4, T_ + 4, T_ + 5), mask_buf(4, T_ + 4, T_ + 4, 196)
    pos = torch.full((1,), T_, dtype=torch.int32, device='cuda')
    tokens, n, p = Buf(4, T_, T_ + 3, dtype=torch.int64), Buf(4, D_, D_ + 3), Buf(4, 256, 260)
    for value in (T_, T_ + 3, -1):
        pos.fill_(value)
        call('vqcpc_decode_sample_masked', case.lg[0], case.ldl, case.offs, 1, 4, 1.0, 0, 1.0, None, case.seeds, cons, T_ + 4,
             lp.view, T_ + 6, None, al.view, T_ + 4, lm.view, T_ + 5, tokens.view, T_ + 3, T_, case.table, case.table_rows, D_, 1,
             n.view, D_ + 3, p.view, 260, pos)
        torch.cuda.synchronize()
        assert int(pos.item()) == value
        for buf in (tokens, n, p, lp, lm, al):
            buf.assert_untouched()


def test_bad_arguments_are_refused_before_any_launch():
    from vqcpc_bach_amd import hip
    case = Case(4, (13,), 1, U=1, T_=6, seed=197)
    T_ = case.T
    pos = torch.zeros(1, dtype=torch.int32, device='cuda')
    tokens, n = Buf(4, T_, T_, dtype=torch.int64), Buf(4, D_, D_)
    cons = torch.full((4, T_), -1, dtype=torch.int64).cuda()
    lp, lm, al = _nan_logp(4, T_, T_), _nan_logp(4, T_, T_), mask_buf(4, T_, T_, 198)
    put(al, 0, torch.ones(4, 256, dtype=torch.bool))

    def go(M=4, seeds=case.seeds, ldcons=T_, ldlogp=T_, ldallow=T_, ldmass=T_, temperature=1.0, rows=case.table_rows,
           tok=tokens.view, table=case.table, nxt=n.view, position=pos, logits=case.lg[0]):
        call('vqcpc_decode_sample_masked', logits, case.ldl, case.offs, 1, M, temperature, 0, 1.0, None, seeds, cons, ldcons,
             lp.view, ldlogp, None, al.view, ldallow, lm.view, ldmass, tok, T_, T_, table, rows, D_, 1, nxt, D_, None, 0, position)
    for kw in (dict(M=65), dict(seeds=None), dict(ldcons=T_ - 1), dict(ldlogp=T_ - 1), dict(ldallow=T_ - 1), dict(ldmass=T_ - 1),
               dict(temperature=0.0), dict(rows=12), dict(tok=None), dict(table=None), dict(nxt=None), dict(position=None),
               dict(logits=None)):
        with pytest.raises(hip.VqcpcHipError, match='decode_sample_masked'):
            go(**kw)
    torch.cuda.synchronize()
    assert int(pos.item()) == 0
    for buf in (tokens, n, lp, lm):
        buf.assert_untouched()
    go()
    torch.cuda.synchronize()
    assert int(pos.item()) == 1 and bool((lm.view[:, 0] == 0.0).all())
