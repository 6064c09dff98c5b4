"""Given codes, code scores and the continuation of a piece (PriorRelative.generate_codes / score_codes / generate /
continue_tokens with `constraint`, `return_logp`; priors/generation.py; vqcpc_prior_sample_constrained) on the tiny priors of
tests/test_prior_gpu.py (N = 6; V = 32 and 1024), both step forms, strides 1 and 4, captured and eager:
  (1) the default path launches the plain sampler; all-free == unconstrained; forcing a run's own codes returns the run,
  (2) forcing the reference's greedy codes returns the fixture; greedy parity with one forward per code and the same forcing
      (tests/prior_constrained_reference.py),
  (3) score_codes == log_softmax of the forward on each column's window; a run's logp == score_codes of its codes, bit for bit;
      no warm-up value survives a captured run; rows are invariant across 1, 3 and 70 rows,
  (4) continue_tokens end to end with the tiny decoder."""
import pytest
import torch

import prior_constrained_reference as C
from test_generate_gpu import _golden_decoder
from test_generate_long_gpu import _meta_dataset
from test_prior_gpu import _golden_prior, fp32_gemms  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
T = torch.from_numpy

FORMS = [('auto', 1), ('cached', 1), ('forward', 1), ('cached', 4)]        # (method, window_stride)
FOREIGN_SEED = 41                                                          # test_greedy_codes_with_a_foreign_prefix...


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _half_forced(codes, seed):
    mask = torch.rand(codes.shape, generator=torch.Generator().manual_seed(seed)) < 0.5
    return torch.where(mask, codes.cpu(), torch.full_like(codes.cpu(), -1))


# ---- 1. default path and self-consistency ----------------------------------------------------------------------------
def test_the_default_path_launches_the_plain_sampler(monkeypatch, fp32_gemms):  # noqa: F811
    from vqcpc_bach_amd import hip
    prior, cfg, _ = _golden_prior('v32')
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
        return set(n for n in names if n.startswith('vqcpc_prior_sample'))
    free = torch.full((2, 15), -1, dtype=torch.int64)
    for method, stride in FORMS:
        for use_graph in (True, False):
            kw = dict(num_generated_codes=2, seed=1, method=method, window_stride=stride, use_graph=use_graph)
            assert launches(lambda: prior.generate_codes(15, **kw)) == {'vqcpc_prior_sample'}
            assert launches(lambda: prior.generate_codes(15, constraint=free, **kw)) == {'vqcpc_prior_sample_constrained'}
            assert launches(lambda: prior.generate_codes(15, return_logp=True, **kw)) == {'vqcpc_prior_sample_constrained'}


@pytest.mark.parametrize('method,stride', FORMS)
def test_all_free_is_the_unconstrained_run_and_forcing_its_own_codes_returns_it(fp32_gemms, method, stride):  # noqa: F811
    prior, cfg, _ = _golden_prior('v32')
    nt = cfg['N'] + 9                                                # stride 4: two full moves and a remainder move of one
    free = torch.full((3, nt), -1, dtype=torch.int64)
    for use_graph in (True, False):
        kw = dict(num_generated_codes=3, seed=7, method=method, window_stride=stride, use_graph=use_graph, temperature=1.2,
                  top_p=0.95)
        a = prior.generate_codes(nt, **kw)
        assert len(torch.unique(a)) > 4
        assert torch.equal(a, prior.generate_codes(nt, constraint=free, **kw))
        assert torch.equal(a, prior.generate_codes(nt, constraint=free[:1], **kw))        # one row, broadcast
        b, logp = prior.generate_codes(nt, return_logp=True, **kw)
        assert torch.equal(a, b) and logp.shape == a.shape and logp.dtype == torch.float32
        c, logp2 = prior.generate_codes(nt, constraint=_half_forced(a, 17), return_logp=True, **kw)
        assert torch.equal(a, c) and _same_bits(logp, logp2)


# ---- 2. forcing ------------------------------------------------------------------------------------------------------
def test_forcing_the_opening_of_the_greedy_fixture_returns_the_fixture(fp32_gemms):  # noqa: F811
    prior, cfg, g = _golden_prior('', 'prior_greedy_tiny')
    ref, nt, N = T(g['codes']), int(g['num_tokens']), cfg['N']
    for L in (1, N - 1, N, N + 3):
        cons = torch.full_like(ref, -1)
        cons[:, :L] = ref[:, :L]
        for method in ('auto', 'cached', 'forward'):
            codes = prior.generate_codes(nt, top_k=1, num_generated_codes=ref.shape[0], seed=0, method=method, constraint=cons)
            assert torch.equal(codes.cpu(), ref), (L, method)


def _foreign_constraint(prior, nt, seed, B=3):
    """A seeded prefix of 4 foreign codes and scattered forced columns (a quarter of the rest)."""
    g = torch.Generator().manual_seed(seed)
    V = prior.num_tokens_per_channel[0]
    codes = torch.randint(0, V, (B, nt), generator=g)
    keep = torch.rand(B, nt, generator=g) < 0.25
    keep[:, :4] = True
    return torch.where(keep, codes, torch.full_like(codes, -1))


def test_greedy_codes_with_a_foreign_prefix_equal_one_forward_per_code(fp32_gemms):  # noqa: F811
    prior, cfg, _ = _golden_prior('', 'prior_greedy_tiny')
    nt = cfg['N'] + 9
    cons = _foreign_constraint(prior, nt, FOREIGN_SEED)
    assert 0 < int((cons[:, 4:] >= 0).sum()) < cons[:, 4:].numel()
    want, gap, _, _ = C.forced_greedy_loop(prior, cons)
    print(f'smallest top-two gap at a free position: {gap:.3e}')
    assert gap > 1e-3, gap
    assert torch.equal(want.cpu()[cons >= 0], cons[cons >= 0])
    for method in ('auto', 'cached', 'forward'):
        for use_graph in (True, False):
            codes = prior.generate_codes(nt, top_k=1, num_generated_codes=3, seed=0, method=method, use_graph=use_graph,
                                         constraint=cons)
            assert torch.equal(codes, want), (method, use_graph, codes, want)


# ---- 3. logp ---------------------------------------------------------------------------------------------------------
def test_score_codes_is_log_softmax_of_the_forward_on_each_columns_window(fp32_gemms):  # noqa: F811
    """Tolerance per entry: the incremental logits differ from the forward's by at most `bound` x rms, bound = twice the decoder
    pair's teacher-forced error measured in this run (tests/test_prior_gpu.py::test_incremental_steps_equal_the_full_forward);
    logp = logit[code] - logsumexp moves by at most twice that; plus the sampler's own chain, logp_bound."""
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from test_generate_gpu import _teacher_forced_error
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=2), 5)
    bound = 2 * _teacher_forced_error(dec, 2, seed=11)
    del dec
    for tag in ('v32', 'v1024'):
        prior, cfg, _ = _golden_prior(tag)
        V, nt = prior.num_tokens_per_channel[0], cfg['N'] + 9
        codes = torch.randint(0, V, (3, nt), generator=torch.Generator().manual_seed(21))
        _, _, rms, rows = C.forced_greedy_loop(prior, codes)
        ref = torch.log_softmax(rows, dim=-1).gather(2, codes.unsqueeze(2)).squeeze(2)
        for method, stride in (('cached', 1), ('forward', 1)):
            got = prior.score_codes(codes, method=method, window_stride=stride)
            assert got.shape == (3, nt) and got.dtype == torch.float32 and got.is_cuda
            err = (got.cpu().double() - ref).abs()
            tol = torch.tensor([[2 * bound * rms + C.logp_bound(rows[b, e], int(codes[b, e])) for e in range(nt)]
                                for b in range(3)])
            print(f'{tag} {method}: max |score_codes - log_softmax(forward)| = {float(err.max()):.2e}, smallest tolerance '
                  f'{float(tol.min()):.2e} (bound {bound:.2e} of the rms {rms:.3f})')
            assert bool((err <= tol).all()), (tag, method, float((err / tol).max()))


@pytest.mark.parametrize('method,stride', FORMS)
def test_the_logp_of_a_run_is_score_codes_of_its_codes(fp32_gemms, method, stride):  # noqa: F811
    prior, cfg, _ = _golden_prior('v32')
    nt = cfg['N'] + 9
    kw = dict(method=method, window_stride=stride)
    codes, logp = prior.generate_codes(nt, num_generated_codes=3, seed=5, temperature=1.3, top_p=0.9, return_logp=True, **kw)
    assert bool(torch.isfinite(logp).all())                           # a captured run: no warm-up value, no unwritten column
    assert bool((logp <= 0).all())
    assert _same_bits(logp, prior.score_codes(codes, **kw))
    assert _same_bits(logp, prior.score_codes(codes, use_graph=False, **kw))
    eager = prior.generate_codes(nt, num_generated_codes=3, seed=5, temperature=1.3, top_p=0.9, return_logp=True, use_graph=False,
                                 **kw)
    assert torch.equal(eager[0], codes) and _same_bits(eager[1], logp)


@pytest.mark.parametrize('method', ['cached', 'forward'])
def test_rows_do_not_depend_on_the_rows_they_share_the_call_with(fp32_gemms, method):  # noqa: F811
    prior, cfg, _ = _golden_prior('v32')
    nt = 14
    s70 = torch.arange(70, dtype=torch.int64) * 31 + 5                # 70 rows run as 64 + 6
    cons = _half_forced(torch.randint(0, 32, (70, nt), generator=torch.Generator().manual_seed(9)), 10)
    kw = dict(method=method, return_logp=True)
    c70, l70 = prior.generate_codes(nt, num_generated_codes=70, seed=s70, constraint=cons, **kw)
    assert bool(torch.isfinite(l70).all()) and torch.equal(c70.cpu()[cons >= 0], cons[cons >= 0])
    c3, l3 = prior.generate_codes(nt, num_generated_codes=3, seed=s70[:3], constraint=cons[:3], **kw)
    assert torch.equal(c3, c70[:3]) and _same_bits(l3, l70[:3])
    for b in (2, 66):
        c1, l1 = prior.generate_codes(nt, num_generated_codes=1, seed=s70[b:b + 1], constraint=cons[b:b + 1], **kw)
        assert torch.equal(c1[0], c70[b]) and _same_bits(l1[0], l70[b]), b


# ---- 4. continue_tokens ----------------------------------------------------------------------------------------------
def test_continue_tokens_goes_on_from_the_opening(fp32_gemms):  # noqa: F811
    prior, cfg, _ = _golden_prior('v32')
    dec, dcfg, _ = _golden_decoder('decoder_tiny')                    # 256 merged codes >= the prior's 32, S = 3
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    nc, epc, E = dec.num_channels, dec.num_events_per_code, dec.data_processor.num_events
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randint(0, v - 3, (1, 2 * epc, 1), generator=g) for v in vocab], dim=2)     # two codes of tokens
    with pytest.raises(ValueError, match='START'):
        prior.continue_tokens(x, 4, dec, seed=1)                      # the synthetic dataset has no meta symbols
    dec.dataloader_generator = _meta_dataset(vocab)
    codes, tokens = prior.continue_tokens(x, 4, dec, num_continuations=2, seed=1)
    # the given codes: the framed opening through the prior's own encoder, in model-sized chunks
    framed = torch.cat([torch.tensor([v - 1 for v in vocab]).view(1, 1, nc).repeat(1, E - 1, 1),
                        torch.tensor([v - 3 for v in vocab]).view(1, 1, nc), x], dim=1).cuda()
    prior.eval()
    prefix = torch.cat([prior.encode(c) for c in framed.split(E, 1)], dim=1)
    L = prefix.shape[1]
    assert L == E // epc + 2
    assert codes.shape == (2, L + 4) and codes.dtype == torch.int64 and bool(((codes >= 0) & (codes < 32)).all())
    assert torch.equal(codes[:, :L], prefix.expand(2, L))
    assert tokens.shape == (2, x.shape[1] + 4 * epc, nc)
    assert torch.equal(tokens[:, :x.shape[1]].cpu(), x.expand(2, -1, -1))
    assert not torch.equal(codes[0, L:], codes[1, L:]) or not torch.equal(tokens[0], tokens[1])
    again = prior.continue_tokens(x, 4, dec, num_continuations=2, seed=1)
    assert torch.equal(again[0], codes) and torch.equal(again[1], tokens)
    c4, t4, code_logp, token_logp = prior.continue_tokens(x, 4, dec, num_continuations=2, seed=1, return_logp=True)
    assert torch.equal(c4, codes) and torch.equal(t4, tokens)
    assert code_logp.shape == codes.shape and token_logp.shape == tokens.shape
    assert bool(torch.isfinite(code_logp).all()) and bool(torch.isfinite(token_logp).all())
    assert _same_bits(code_logp, prior.score_codes(codes))
    for bad in (x[:, :2 * epc - 1], x[:, :0], x[0], x[:, :, :nc - 1]):                    # ragged, empty, wrong rank / voices
        with pytest.raises(ValueError, match='x:'):
            prior.continue_tokens(bad, 4, dec, seed=1)
    # generate passes the code constraint and the scores through
    cons = torch.full((2, 8), -1, dtype=torch.int64)
    cons[:, 2] = 7
    kw = dict(pad=[0, 0, 0, 0], start=[1, 1, 1, 1])
    gc, gt, glp = prior.generate(8, dec, num_generated_codes=2, seed=5, code_constraint=cons, return_logp=True, **kw)
    assert bool((gc[:, 2] == 7).all()) and glp.shape == (2, 8) and gt.shape[0] == 2
    assert torch.equal(gc, prior.generate_codes(8, num_generated_codes=2, seed=5, constraint=cons))
