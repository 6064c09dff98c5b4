"""Allowed code sets in the prior's generation (PriorRelative.generate_codes / generate / continue_tokens with `allowed`,
`return_allowed_mass`; priors/generation.py; vqcpc_prior_sample_masked, vqcpc_prior_sample_product_masked) on tiny priors: d_model
32, 2 layers, 2 heads, N = 6, num_tokens 14; merged V = 11, product 2 x 4 and 3 x 5.  The step form is pinned to 'cached' and to
'forward' in turn (the two agree to rounding only):
  (1) every emitted code lies in its set; a full `allowed` is the call without it, bit for bit; captured == eager; strides 1, 2 and
      a ragged last move; chunks == whole; the default path's launches,
  (2) greedy decoding == one forward per code with the arg-max over the allowed codes; allowed_mass == the allowed share of
      softmax(forward) on each column's window (tests/prior_masked_reference.py),
  (3) the same for product priors, digit by digit,
  (4) the refusals; continue_tokens with a fixed close; generate passes the sets through."""
import functools

import pytest
import torch

import prior_masked_reference as R
from product_codes_helpers import build_prior, prior_cfg
from test_generate_gpu import _golden_decoder
from test_generate_long_gpu import _meta_dataset
from test_prior_gpu import _golden_prior, fp32_gemms  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

NT, N = 14, 6
METHODS = ['cached', 'forward']
PRODUCT = [(4, 2), (5, 3)]                                # (K, ncb): 2 x 4 and 3 x 5


@functools.lru_cache(maxsize=None)
def tiny_prior(K, ncb, code_model, seed=3, gain=1.0):
    """gain: the heads' weights are multiplied by it -- a sharper model, whose scores depend more on the codes before (the
    particle tests need rows of a group to weigh differently)."""
    torch.manual_seed(seed)
    prior = build_prior(prior_cfg(K, ncb, p_d=32, p_H=2, p_layers=2, N=N), code_model).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in prior.named_parameters():
            if not k.startswith('encoder.') and p.dim() == 1:
                p.add_(0.05 * torch.randn(p.shape, generator=g).cuda())
        for head in prior.pre_softmaxes:
            head.weight.mul_(gain)
    return prior.eval()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def random_sets(shape, seed, share=0.4):
    """bool `shape` (..., V): every set has at least one code; about a third of the sets are full."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(shape, generator=g) < share
    a.scatter_(-1, torch.randint(0, shape[-1], shape[:-1] + (1,), generator=g), True)
    a[torch.rand(shape[:-1], generator=g) < 0.3] = True
    return a


def forced_columns(B, nt, V, seed, share=0.2):
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, V, (B, nt), generator=g)
    return torch.where(torch.rand(B, nt, generator=g) < share, codes, torch.full_like(codes, -1))


def digits_of(codes, K, ncb):
    return torch.stack([(codes // K ** j) % K for j in range(ncb)], dim=-1)          # (..., ncb)


def open_for(allowed, cons, K=None, ncb=None):
    """`allowed` with every forced code (digit) added to its own set."""
    allowed = allowed.clone()
    c = cons.clamp(min=0)
    if ncb is None:
        hit = torch.zeros_like(allowed).scatter_(2, c.unsqueeze(2), True)
    else:
        hit = torch.zeros_like(allowed).scatter_(3, digits_of(c, K, ncb).unsqueeze(3), True)
    return allowed | (hit & (cons >= 0).view(cons.shape + (1,) * (allowed.dim() - 2)))


def in_sets(codes, allowed, K=None, ncb=None):
    codes = codes.cpu()
    if ncb is None:
        return bool(allowed.gather(2, codes.unsqueeze(2)).all())
    return bool(allowed.gather(3, digits_of(codes, K, ncb).unsqueeze(3)).all())


@pytest.fixture(scope='module')
def pair_bound():
    """Twice the decoder pair's teacher-forced error measured in this run: the bound tests/test_prior_constrained_gpu.py uses for
    logp (the incremental logits differ from the forward's by at most `bound` x rms)."""
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from test_generate_gpu import _teacher_forced_error
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(0)
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=2), 5)
    return 2 * _teacher_forced_error(dec, 2, seed=11)


# ---- 1. sets in generation --------------------------------------------------------------------------------------------------
def test_the_keywords_launch_the_masked_sampler_and_the_default_path_is_unchanged(monkeypatch, fp32_gemms):  # noqa: F811
    from vqcpc_bach_amd import hip
    names, real = [], hip.call

    def recorder(entry, *args):
        names.append(entry)
        return real(entry, *args)

    def launches(fn):
        del names[:]
        with monkeypatch.context() as m:
            m.setattr(hip, 'call', recorder)
            fn()
        torch.cuda.synchronize()
        return set(n for n in names if n.startswith('vqcpc_prior_sample') or n.startswith('vqcpc_particle'))
    for (K, ncb, model), tail in (((11, 1, 'merged'), ''), ((4, 2, 'product'), '_product')):
        prior = tiny_prior(K, ncb, model)
        full = torch.ones((1, NT, K) if ncb == 1 else (1, NT, ncb, K), dtype=torch.bool)
        free = torch.full((2, NT), -1, dtype=torch.int64)
        plain = 'vqcpc_prior_sample' + tail
        cons = 'vqcpc_prior_sample_constrained' if ncb == 1 else plain
        masked = 'vqcpc_prior_sample_masked' if ncb == 1 else 'vqcpc_prior_sample_product_masked'
        for method in METHODS:
            kw = dict(num_generated_codes=2, seed=1, method=method)
            assert launches(lambda: prior.generate_codes(NT, **kw)) == {plain}
            assert launches(lambda: prior.generate_codes(NT, constraint=free, return_logp=True, **kw)) == {cons}
            assert launches(lambda: prior.generate_codes(NT, allowed=full, **kw)) == {masked}
            assert launches(lambda: prior.generate_codes(NT, return_allowed_mass=True, **kw)) == {masked}
            got = launches(lambda: prior.generate_codes(NT, particles=2, constraint=free, **kw))
            assert masked in got and 'vqcpc_particle_resample' in got and plain not in got and cons not in got


@pytest.mark.parametrize('method', METHODS)
def test_every_code_lies_in_its_set_and_a_full_set_changes_no_bit(fp32_gemms, method):  # noqa: F811
    prior = tiny_prior(11, 1, 'merged')
    B, V = 3, 11
    cons = forced_columns(B, NT, V, 31)
    allowed = open_for(random_sets((B, NT, V), 32), cons)
    filt = dict(temperature=1.3, top_p=0.9)
    for stride in ((1, 2, 3) if method == 'cached' else (1,)):                # 3: two full moves and a ragged last one of two
        kw = dict(num_generated_codes=B, seed=5, method=method, window_stride=stride, **filt)
        codes, logp, mass = prior.generate_codes(NT, constraint=cons, allowed=allowed, return_logp=True, return_allowed_mass=True,
                                                 **kw)
        assert codes.shape == (B, NT) and mass.shape == (B, NT) and mass.dtype == torch.float32 and mass.is_cuda
        assert in_sets(codes, allowed) and torch.equal(codes.cpu()[cons >= 0], cons[cons >= 0])
        assert bool(torch.isfinite(mass).all()) and bool((mass <= 0).all()) and bool(torch.isfinite(logp).all())
        assert bool((mass.cpu()[allowed.all(-1)] == 0).all()) and bool((mass.cpu()[~allowed.all(-1)] < 0).any())
        assert len(torch.unique(codes)) > 4
        eager = prior.generate_codes(NT, constraint=cons, allowed=allowed, return_logp=True, return_allowed_mass=True,
                                     use_graph=False, **kw)
        assert torch.equal(eager[0], codes) and same_bits(eager[1], logp) and same_bits(eager[2], mass)      # captured == eager
        only = prior.generate_codes(NT, constraint=cons, allowed=allowed, **kw)                               # no score asked for
        assert torch.equal(only, codes)
        # a full `allowed` is the call without it
        c0, l0 = prior.generate_codes(NT, constraint=cons, return_logp=True, **kw)
        for full in (torch.ones(B, NT, V, dtype=torch.bool), torch.ones(1, NT, V, dtype=torch.bool)):
            c1, l1, m1 = prior.generate_codes(NT, constraint=cons, allowed=full, return_logp=True, return_allowed_mass=True, **kw)
            assert torch.equal(c1, c0) and same_bits(l1, l0) and same_bits(m1, torch.zeros_like(m1))
        assert torch.equal(prior.generate_codes(NT, allowed=full, **kw), prior.generate_codes(NT, **kw))
        # one row of sets for every row
        shared = prior.generate_codes(NT, allowed=allowed[:1], return_allowed_mass=True, **kw)
        spread = prior.generate_codes(NT, allowed=allowed[:1].expand(B, NT, V), return_allowed_mass=True, **kw)
        assert torch.equal(shared[0], spread[0]) and same_bits(shared[1], spread[1])


@pytest.mark.parametrize('method', METHODS)
def test_chunks_are_the_whole_and_rows_do_not_depend_on_their_company(fp32_gemms, method):  # noqa: F811
    prior = tiny_prior(11, 1, 'merged')
    V = 11
    s70 = torch.arange(70, dtype=torch.int64) * 31 + 5                        # 70 rows run as 64 + 6
    cons = forced_columns(70, NT, V, 33)
    allowed = open_for(random_sets((70, NT, V), 34), cons)
    kw = dict(method=method, return_logp=True, return_allowed_mass=True, top_p=0.95)
    c70, l70, m70 = prior.generate_codes(NT, num_generated_codes=70, seed=s70, constraint=cons, allowed=allowed, **kw)
    assert in_sets(c70, allowed) and bool(torch.isfinite(m70).all())
    for rows in (slice(0, 3), slice(66, 67)):
        c, l, m = prior.generate_codes(NT, num_generated_codes=rows.stop - rows.start, seed=s70[rows], constraint=cons[rows],
                                       allowed=allowed[rows], **kw)
        assert torch.equal(c, c70[rows]) and same_bits(l, l70[rows]) and same_bits(m, m70[rows]), rows


# ---- 2. greedy decoding and the mass against one forward per code -------------------------------------------------------------
@pytest.mark.parametrize('method', METHODS)
def test_greedy_codes_and_mass_equal_one_forward_per_code_over_the_allowed_codes(fp32_gemms, pair_bound, method):  # noqa: F811
    """Tolerance of the mass per entry, as tests/test_prior_constrained_gpu.py::test_score_codes_is_log_softmax... has it for logp:
    the incremental logits differ from the forward's by at most `bound` x rms; a log-sum-exp moves by at most that, the mass is a
    difference of two; plus the sampler's own chain, logmass_bound."""
    prior = tiny_prior(11, 1, 'merged')
    B, V = 3, 11
    cons = forced_columns(B, NT, V, 41)
    allowed = open_for(random_sets((B, NT, V), 42), cons)
    want, gap, rms, ref_mass, rows = R.masked_greedy_loop(prior, cons, allowed)
    print(f'smallest top-two gap over the allowed codes of a free column: {gap:.3e}')
    # a precondition on the inputs, not on the code: the arg-max is defined where the forward's own gap exceeds what two
    # computations of a logit may differ by
    assert gap > 2e-5, gap
    assert in_sets(want, allowed) and torch.equal(want.cpu()[cons >= 0], cons[cons >= 0])
    for use_graph in (True, False):
        codes, mass = prior.generate_codes(NT, top_k=1, num_generated_codes=B, seed=0, method=method, use_graph=use_graph,
                                           constraint=cons, allowed=allowed, return_allowed_mass=True)
        assert torch.equal(codes, want), (method, use_graph, codes, want)
        err = (mass.cpu().double() - ref_mass).abs()
        tol = torch.tensor([[2 * pair_bound * rms + R.logmass_bound(rows[b, e], allowed[b, e]) for e in range(NT)] for b in range(B)])
        print(f'{method} (graph {use_graph}): max |allowed_mass - forward| = {float(err.max()):.2e}, smallest tolerance '
              f'{float(tol.min()):.2e}')
        assert bool((err <= tol).all()), float((err / tol).max())
        assert bool((mass.cpu()[allowed.all(-1)] == 0).all())


# ---- 3. product priors ----------------------------------------------------------------------------------------------------------
@torch.no_grad()
def product_masked_greedy_loop(prior, constraint, allowed):
    """tests/test_prior_product_gpu.py::_greedy_loop under digit sets: per code, ONE full `forward` per digit on the reference's
    window; digit j is the arg-max over ITS allowed digits of stage j's logits given the digits < j already chosen, or the
    constraint's.  allowed (B, num_tokens, ncb, K) bool.  -> (codes, smallest gap over the free digits with two allowed values,
    rms of the logits read, mass (B, num_tokens) float64: the sum over the stages of the log of the allowed share along the chosen
    digits, rows: ncb x (B, num_tokens, K) float64)."""
    prior.eval()
    N_, K, ncb = prior.num_tokens, prior.codebook_size, prior.num_codebooks
    B, nt = constraint.shape
    dev = prior.sos.device
    seq = torch.zeros(B, nt, dtype=torch.int64, device=dev)
    mass = torch.zeros(B, nt, dtype=torch.float64)
    rows = [[] for _ in range(ncb)]
    gap = float('inf')
    for e in range(nt):
        w, p = (0, e) if e < N_ else (e - N_ + 1, N_ - 1)
        f = constraint[:, e].to(dev)
        free = f < 0
        seq[:, e] = torch.where(free, torch.zeros_like(f), f)
        for j in range(ncb):
            lg = prior.forward(seq[:, w:w + N_].contiguous())['weights_per_category'][j][:, p].double()
            rows[j].append(lg.cpu())
            a = allowed[:, e, j].to(dev)
            open_lg = lg.masked_fill(~a, -float('inf'))
            mass[:, e] += (torch.logsumexp(open_lg, dim=-1) - torch.logsumexp(lg, dim=-1)).cpu()
            two = free & (a.sum(-1) >= 2)
            if bool(two.any()):
                top2 = torch.topk(open_lg[two], 2, dim=-1)[0]
                gap = min(gap, float((top2[:, 0] - top2[:, 1]).min()))
            seq[:, e] = torch.where(free, seq[:, e] + open_lg.argmax(dim=-1) * K ** j, seq[:, e])
    rows = [torch.stack(r, dim=1) for r in rows]
    return seq, gap, float(torch.stack(rows).pow(2).mean().sqrt()), mass, rows


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('K,ncb', PRODUCT)
def test_product_digits_lie_in_their_sets_and_equal_one_forward_per_digit(fp32_gemms, pair_bound, K, ncb, method):  # noqa: F811
    prior = tiny_prior(K, ncb, 'product')
    B, V = 3, K ** ncb
    cons = forced_columns(B, NT, V, 51)
    allowed = open_for(random_sets((B, NT, ncb, K), 52, share=0.5), cons, K, ncb)
    # sampling: the digits lie in their sets, captured == eager, a full set changes no bit
    for stride in ((1, 3) if method == 'cached' else (1,)):
        kw = dict(num_generated_codes=B, seed=6, method=method, window_stride=stride, temperature=1.2, top_p=0.95)
        codes, logp, mass = prior.generate_codes(NT, constraint=cons, allowed=allowed, return_logp=True, return_allowed_mass=True,
                                                 **kw)
        assert in_sets(codes, allowed, K, ncb) and torch.equal(codes.cpu()[cons >= 0], cons[cons >= 0])
        assert bool(torch.isfinite(mass).all()) and bool((mass <= 0).all())
        assert bool((mass.cpu()[allowed.all(-1).all(-1)] == 0).all())
        eager = prior.generate_codes(NT, constraint=cons, allowed=allowed, return_logp=True, return_allowed_mass=True,
                                     use_graph=False, **kw)
        assert torch.equal(eager[0], codes) and same_bits(eager[1], logp) and same_bits(eager[2], mass)
        c0, l0 = prior.generate_codes(NT, constraint=cons, return_logp=True, **kw)
        c1, l1, m1 = prior.generate_codes(NT, constraint=cons, allowed=torch.ones(1, NT, ncb, K, dtype=torch.bool), return_logp=True,
                                          return_allowed_mass=True, **kw)
        assert torch.equal(c1, c0) and same_bits(l1, l0) and same_bits(m1, torch.zeros_like(m1))
    # greedy: one forward per digit, the arg-max over the digit's set; the mass along the emitted digits
    want, gap, rms, ref_mass, rows = product_masked_greedy_loop(prior, cons, allowed)
    print(f'{ncb} x {K}: smallest top-1 / top-2 gap {gap:.2e}')
    assert gap > 2e-5, gap
    codes, mass = prior.generate_codes(NT, top_k=1, num_generated_codes=B, seed=0, method=method, constraint=cons, allowed=allowed,
                                       return_allowed_mass=True)
    assert torch.equal(codes, want)
    err = (mass.cpu().double() - ref_mass).abs()
    dig = digits_of(want.cpu(), K, ncb)
    tol = torch.tensor([[sum(2 * pair_bound * rms + R.logmass_bound(rows[j][b, e], allowed[b, e, j]) for j in range(ncb)) +
                         (ncb - 1) * 2.0 ** -24 * abs(float(ref_mass[b, e])) for e in range(NT)] for b in range(B)])
    print(f'{ncb} x {K} {method}: max |allowed_mass - forward| = {float(err.max()):.2e}, smallest tolerance {float(tol.min()):.2e}')
    assert dig.shape == (B, NT, ncb) and bool((err <= tol).all()), float((err / tol).max())


# ---- 4. refusals, continue_tokens, generate -------------------------------------------------------------------------------------
def test_the_refusals_raise(fp32_gemms):  # noqa: F811
    from vqcpc_bach_amd.priors.generation import IncrementalPrior
    from vqcpc_bach_amd.utils import STEP_LOCK
    prior = tiny_prior(11, 1, 'merged')
    full = torch.ones(2, NT, 11, dtype=torch.bool)
    empty = full.clone()
    empty[1, 4] = False
    with pytest.raises(ValueError, match=r'\(row 1, column 4\) has no allowed code'):
        prior.generate_codes(NT, num_generated_codes=2, allowed=empty)
    narrow = full.clone()
    narrow[:, 9] = False
    narrow[:, 9, 3] = True
    cons = torch.full((2, NT), -1, dtype=torch.int64)
    cons[1, 9] = 4
    with pytest.raises(ValueError, match=r'\(row 1, column 9\) is forced to code 4'):
        prior.generate_codes(NT, num_generated_codes=2, allowed=narrow, constraint=cons)
    for bad in (full.long(), full[:, :NT - 1], full[:, :, :10], full[0], torch.ones(3, NT, 11, dtype=torch.bool),
                torch.ones(2, NT, 1, 11, dtype=torch.bool)):
        with pytest.raises(ValueError, match='allowed: bool'):
            prior.generate_codes(NT, num_generated_codes=2, allowed=bad)
    prod = tiny_prior(4, 2, 'product')
    with pytest.raises(ValueError, match='allowed: bool'):
        prod.generate_codes(NT, num_generated_codes=2, allowed=torch.ones(2, NT, 16, dtype=torch.bool))
    dsets = torch.ones(1, NT, 2, 4, dtype=torch.bool)
    dsets[0, 2, 1] = False
    with pytest.raises(ValueError, match=r'\(row 0, column 2, codebook 1\) has no allowed code'):
        prod.generate_codes(NT, num_generated_codes=2, allowed=dsets)
    with STEP_LOCK, torch.no_grad():
        inc = IncrementalPrior(prior, 2)
        teacher = torch.zeros(2, N, dtype=torch.int64)
        packed = torch.zeros(2, N, 1, dtype=torch.int32)
        for kw in (dict(allowed=packed), dict(want_allowed_mass=True)):
            with pytest.raises(ValueError, match='teacher'):
                inc.start(N, seeds=0, teacher=teacher, **kw)
        with pytest.raises(ValueError, match='packed sets'):
            inc.start(NT, seeds=0, allowed=packed)


def test_continue_tokens_closes_on_a_given_code_and_generate_passes_the_sets_through(fp32_gemms):  # noqa: F811
    prior, cfg, _ = _golden_prior('v32')
    dec, dcfg, _ = _golden_decoder('decoder_tiny')
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    nc, epc, E = dec.num_channels, dec.num_events_per_code, dec.data_processor.num_events
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randint(0, v - 3, (1, 2 * epc, 1), generator=g) for v in vocab], dim=2)     # two codes of tokens
    dec.dataloader_generator = _meta_dataset(vocab)
    framed = torch.cat([torch.tensor([v - 1 for v in vocab]).view(1, 1, nc).repeat(1, E - 1, 1),
                        torch.tensor([v - 3 for v in vocab]).view(1, 1, nc), x], dim=1).cuda()
    prior.eval()
    prefix = torch.cat([prior.encode(c) for c in framed.split(E, 1)], dim=1)
    L, new = prefix.shape[1], 5
    total = L + new
    close = torch.full((1, total), -1, dtype=torch.int64)
    close[0, -2:] = torch.tensor([7, 19])                                   # the fixed close
    close[0, 1] = int(prefix[0, 1])                                          # the opening's own code may be repeated
    sets = torch.ones(1, total, 32, dtype=torch.bool)
    sets[0, L, 16:] = False                                                  # the first new code: one of the lower half
    for kw in (dict(), dict(code_particles=4)):
        codes, tokens = prior.continue_tokens(x, new, dec, num_continuations=2, seed=1, code_constraint=close, code_allowed=sets, **kw)
        assert codes.shape == (2, total) and torch.equal(codes[:, :L], prefix.expand(2, L))
        assert codes[:, -2:].tolist() == [[7, 19], [7, 19]] and bool((codes[:, L] < 16).all())
        assert tokens.shape == (2, x.shape[1] + new * epc, nc) and torch.equal(tokens[:, :x.shape[1]].cpu(), x.expand(2, -1, -1))
    wrong = close.clone()
    wrong[0, 1] = (int(prefix[0, 1]) + 1) % 32
    with pytest.raises(ValueError, match='differs from the opening'):
        prior.continue_tokens(x, new, dec, seed=1, code_constraint=wrong)
    with pytest.raises(ValueError, match='constraint'):
        prior.continue_tokens(x, new, dec, seed=1, code_constraint=close[:, :-1])
    # generate passes the sets and the particles through
    gsets = torch.ones(1, 8, 32, dtype=torch.bool)
    gsets[0, 2] = False
    gsets[0, 2, [7, 9]] = True
    kw = dict(pad=[0, 0, 0, 0], start=[1, 1, 1, 1])
    gc, gt = prior.generate(8, dec, num_generated_codes=2, seed=5, code_allowed=gsets, **kw)
    assert bool(((gc[:, 2] == 7) | (gc[:, 2] == 9)).all()) and gt.shape[0] == 2
    assert torch.equal(gc, prior.generate_codes(8, num_generated_codes=2, seed=5, allowed=gsets))
    gp, _ = prior.generate(8, dec, num_generated_codes=2, seed=5, code_allowed=gsets, code_particles=2, **kw)
    assert torch.equal(gp, prior.generate_codes(8, num_generated_codes=2, seed=5, allowed=gsets, particles=2))
