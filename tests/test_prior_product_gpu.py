"""The prior with `code_model='product'` (priors/prior_relative.py, priors/generation.py IncrementalProductPrior,
csrc/product_codes.hip) on the tiny prior shapes of tests/test_prior_gpu.py with K = 512 x ncb = 2 (262 144 merged codes: the
merged prior cannot sample them) and K = 4 x ncb = 3:
  (1) ncb = 1: the product model IS the merged one, bit for bit (loss, logits, greedy codes);
  (2) forward / backward against the float64 restatement (product_codes_reference.prior_forward on the oracle's causal stack) at
      the tolerances of tests/test_prior_gpu.py::test_forward_backward_equal_the_reference;
  (3) teacher-forced incremental steps == the full forward, bound: twice the merged prior's error at v1024 in the same run;
  (4) generate_codes: greedy == one forward per digit with the reference's window rule, also with half of the columns given;
      logp == score_codes bit for bit and == the chained log_softmax of the forward; row / chunk / form invariance;
  (5) generate / continue_tokens through a 'product' decoder; (6) training."""
import numpy as np
import pytest
import torch

import prior_constrained_reference as C
import product_codes_reference as R
from product_codes_helpers import build_decoder, build_prior, oracle_stack, prior_cfg, tiny_cfg
from test_prior_gpu import LOSS_TOL, RMS_TOL, _golden_prior, _incremental_errors, fp32_gemms, rms_err  # noqa: F401

pytestmark = pytest.mark.gpu
SHAPES = [(512, 2), (4, 3)]


def _prior(K, ncb, seed=3, **over):
    torch.manual_seed(seed)
    prior = build_prior(prior_cfg(K, ncb, **over)).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in prior.named_parameters():
            if not k.startswith('encoder.') and p.dim() == 1:
                p.add_(0.05 * torch.randn(p.shape, generator=g).cuda())
    return prior.eval()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. one codebook: the merged prior ---------------------------------------------------------------------------------------
def test_one_codebook_is_the_merged_prior_bit_for_bit(fp32_gemms):  # noqa: F811
    merged, cfg, g = _golden_prior('v32')
    sd = {k: v.detach().clone() for k, v in merged.state_dict().items()}
    sd['embedding.weight'] = sd['embedding.weight'].unsqueeze(0)
    prod = build_prior(cfg, 'product', sd).cuda()
    assert 'digit_embeddings.weight' not in prod.state_dict() and prod.embedding.weight.shape == (1, 32, cfg['p_emb'])
    codes = torch.from_numpy(g['v32/codes']).cuda()
    merged.eval(), prod.eval()
    with torch.no_grad():
        a, b = prod.forward(codes), merged.forward(codes)
    assert _same_bits(a['loss'], b['loss']) and len(a['weights_per_category']) == 1
    assert _same_bits(a['weights_per_category'][0], b['weights_per_category'][0])
    for kw in (dict(top_k=1), dict(temperature=1.3, top_p=0.9), dict(window_stride=2), dict(method='forward')):
        ca, la = prod.generate_codes(15, num_generated_codes=3, seed=4, return_logp=True, **kw)
        cb, lb = merged.generate_codes(15, num_generated_codes=3, seed=4, return_logp=True, **kw)
        assert torch.equal(ca, cb) and _same_bits(la, lb), kw
    assert torch.equal(prod.generate_codes(15, num_generated_codes=3, seed=4), merged.generate_codes(15, num_generated_codes=3, seed=4))


# ---- 2. forward / backward against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1], ids=['f32', 'bf16x6'])
@pytest.mark.parametrize('K,ncb', SHAPES)
def test_forward_backward_equal_the_float64_reference(K, ncb, mode):
    from vqcpc_bach_amd import hip
    prior = _prior(K, ncb)
    cfg = prior_cfg(K, ncb)
    codes = torch.randint(0, K ** ncb, (cfg['B'], cfg['N']), generator=torch.Generator().manual_seed(7))
    P, stack = oracle_stack({k: v for k, v in prior.state_dict().items() if not k.startswith('encoder.')}, cfg, torch.float64)
    P = {k: v.requires_grad_(True) if v.is_floating_point() else v for k, v in P.items()}
    ref_loss, ref_logits, _ = R.prior_forward(P, codes, ncb, K, stack)
    ref_loss.backward()
    hip.set_gemm_mode(mode)
    try:
        prior.init_optimizers(lr=1e-3)
        with torch.no_grad():
            fp = prior.forward(codes.cuda())
        assert len(fp['weights_per_category']) == ncb
        errs = [rms_err(fp['weights_per_category'][j], ref_logits[j]) for j in range(ncb)]
        print(f'{ncb} x {K} mode {mode}: loss {fp["monitored_quantities"]["loss"]:.7f} (float64 {float(ref_loss):.7f}), logits '
              + ', '.join(f'{e:.2e}' for e in errs) + ' of the rms')
        assert abs(fp['monitored_quantities']['loss'] - float(ref_loss)) <= LOSS_TOL * float(ref_loss)
        for j in range(ncb):
            assert fp['weights_per_category'][j].shape == (cfg['B'], cfg['N'], K) and errs[j] <= RMS_TOL, (j, errs[j])
        loss, _ = prior.compute_loss(codes.cuda())
        prior.flat.zero_grad()
        loss.backward()
        worst = 0.0
        for k, p in prior.named_parameters():
            if k.startswith('encoder.'):
                assert p.grad is None, k
                continue
            ref = P[k].grad
            if ref is None or float(ref.abs().max()) == 0.0:
                assert float(p.grad.abs().max()) == 0.0, k
            else:
                e = rms_err(p.grad, ref)
                worst = max(worst, e)
                assert e <= RMS_TOL, (k, e)
        print(f'{ncb} x {K} mode {mode}: worst gradient error {worst:.2e} of the rms')
    finally:
        hip.set_gemm_mode(0)


# ---- 3. incremental == full forward -------------------------------------------------------------------------------------------
def _product_incremental_errors(prior, B, seed):
    """tests/test_prior_gpu._incremental_errors for the product prior: every stage's logits of every teacher-forced step against
    `forward`, max |difference| / rms(forward logits): (head cached, head forward form, stride 1, stride 4)."""
    from vqcpc_bach_amd.priors.generation import IncrementalProductPrior
    N, V, ncb = prior.num_tokens, prior.num_tokens_per_channel[0], prior.num_codebooks
    nt = N + 9
    full = torch.randint(0, V, (B, nt), generator=torch.Generator().manual_seed(seed)).cuda()
    out = []

    def fwd(w):
        ref = torch.stack(prior.forward(full[:, w:w + N])['weights_per_category'])          # (ncb, B, N, K)
        return ref, float(ref.pow(2).mean().sqrt())
    with torch.no_grad():
        inc = IncrementalProductPrior(prior, B)
        ref, rms = fwd(0)
        for form in ('step', 'step_forward'):
            inc.start(nt, seeds=1, teacher=full[:, :N])
            worst = 0.0
            for t in range(N):
                inc.step() if form == 'step' else inc.step_forward(t)
                worst = max(worst, float((inc.stage_logits - ref[:, :, t]).abs().max()))
            assert torch.equal(inc.codes_win, full[:, :N]) and int(inc.pos.item()) == N      # teacher forcing writes the given codes
            out.append(worst / rms)
        for k, windows in ((1, (1, 5, 9)), (4, (4, 8))):
            worst = 0.0
            for w in windows:
                inc.start(nt, seeds=1)
                inc.seq.copy_(full)
                inc.slide(w, N - k, advance=k)
                assert int(inc.pos.item()) == N - k and inc.win.tolist() == [w + k, w]
                inc.teacher = full[:, w:w + N].contiguous()
                ref_w, _ = fwd(w)
                for t in range(N - k, N):
                    inc.step()
                    worst = max(worst, float((inc.stage_logits - ref_w[:, :, t]).abs().max()))
                inc.commit()
                assert torch.equal(inc.seq, full)
            out.append(worst / rms)
    return out


def test_incremental_steps_equal_the_full_forward(fp32_gemms):  # noqa: F811
    """Per form (head, head forward form, stride 1, stride 4) the bound is twice the merged prior's error of the same form at its
    v1024 shape, measured in this run by tests/test_prior_gpu._incremental_errors (the yardstick is the existing code)."""
    merged = _incremental_errors(_golden_prior('v1024')[0].eval(), 3, seed=14)
    print('merged prior v1024 (head, head forward form, stride 1, stride 4): ' + ', '.join(f'{e:.2e}' for e in merged))
    for K, ncb in SHAPES:
        mine = _product_incremental_errors(_prior(K, ncb), 3, seed=14)
        print(f'product prior {ncb} x {K} (same order): ' + ', '.join(f'{e:.2e}' for e in mine))
        for e, m in zip(mine, merged):
            assert e <= 2 * m, (K, ncb, e, m)


# ---- 4. generate_codes --------------------------------------------------------------------------------------------------------
@torch.no_grad()
def _greedy_loop(prior, constraint):
    """tests/prior_constrained_reference.forced_greedy_loop digit by digit: per code, ONE full `forward` per digit on the
    reference's window; digit j is the argmax of stage j's logits given the digits < j already chosen, or the constraint's.
    -> (codes, smallest top-1 / top-2 gap over the free digits, rms of the logits read, rows: ncb x (B, num_tokens, K) float64)."""
    prior.eval()
    N, K, ncb = prior.num_tokens, prior.codebook_size, prior.num_codebooks
    B, nt = constraint.shape
    dev = prior.sos.device
    seq = torch.zeros(B, nt, dtype=torch.int64, device=dev)
    rows = [[] for _ in range(ncb)]
    gap = float('inf')
    for e in range(nt):
        w, p = (0, e) if e < N else (e - N + 1, N - 1)
        f = constraint[:, e].to(dev)
        free = f < 0
        seq[:, e] = torch.where(free, torch.zeros_like(f), f)
        for j in range(ncb):
            lg = prior.forward(seq[:, w:w + N].contiguous())['weights_per_category'][j][:, p].double()
            rows[j].append(lg.cpu())
            if bool(free.any()):
                top2 = torch.topk(lg[free], 2, dim=-1)[0]
                gap = min(gap, float((top2[:, 0] - top2[:, 1]).min()))
            seq[:, e] = torch.where(free, seq[:, e] + lg.argmax(dim=-1) * K ** j, seq[:, e])
    rows = [torch.stack(r, dim=1) for r in rows]
    return seq, gap, float(torch.stack(rows).pow(2).mean().sqrt()), rows


@pytest.mark.parametrize('K,ncb', SHAPES)
def test_greedy_codes_equal_one_forward_per_digit(fp32_gemms, K, ncb):  # noqa: F811
    prior = _prior(K, ncb)
    V, N = K ** ncb, prior.num_tokens
    nt = N + 5
    codes = prior.generate_codes(nt, num_generated_codes=3, seed=2)
    assert codes.shape == (3, nt) and codes.dtype == torch.int64 and codes.is_cuda and bool(((codes >= 0) & (codes < V)).all())
    assert len(torch.unique(codes)) > 3                                # it does sample
    free = torch.full((3, nt), -1, dtype=torch.int64)
    given = torch.randint(0, V, (3, nt), generator=torch.Generator().manual_seed(8))
    half = torch.where(torch.arange(nt) % 2 == 0, given, free)       # every other column given
    for cons in (free, half):
        ref, gap, _, _ = _greedy_loop(prior, cons)
        print(f'{ncb} x {K}: smallest top-1 / top-2 gap {gap:.2e}')
        # a precondition on the inputs, not on the code: the arg-max is only defined where the forward's own top-1 / top-2 gap
        # exceeds what the two computations of a logit may differ by (1e-6 of an rms of order 1, test 3); 2e-5 is 20 times that
        assert gap > 2e-5
        for kw in (dict(), dict(method='cached'), dict(method='forward'), dict(use_graph=False)):
            got = prior.generate_codes(nt, num_generated_codes=3, seed=0, top_k=1, constraint=cons, **kw)
            assert torch.equal(got, ref), (kw, got, ref)
        assert torch.equal(ref.cpu()[cons >= 0], cons[cons >= 0])


@pytest.fixture(scope='module')
def decoder_pair_bound():
    """Twice the teacher-forced error of the decoder pair at the DEC shape, measured in this run: the bound of
    tests/test_prior_constrained_gpu.py::test_score_codes_is_log_softmax_of_the_forward_on_each_columns_window."""
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from test_generate_gpu import _teacher_forced_error
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(0)
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=2), 5)
    return 2 * _teacher_forced_error(dec, 2, seed=11)


@pytest.mark.parametrize('K,ncb', SHAPES)
def test_logp_is_score_codes_and_the_chained_log_softmax(fp32_gemms, decoder_pair_bound, K, ncb):  # noqa: F811
    """Per stage the tolerance of tests/test_prior_constrained_gpu.py (2 bound rms for the logits + logp_bound for the sampler's
    chain), summed over the stages, plus ncb - 1 roundings of the partial sums (u |logp| each, |partial| <= |logp|: all terms
    are <= 0)."""
    prior = _prior(K, ncb)
    nt = prior.num_tokens + 5
    for kw in (dict(method='cached'), dict(method='forward'), dict(method='cached', window_stride=2)):
        codes, logp = prior.generate_codes(nt, num_generated_codes=3, seed=5, temperature=1.3, top_p=0.9, return_logp=True, **kw)
        assert bool(torch.isfinite(logp).all()) and bool((logp <= 0).all())
        assert _same_bits(logp, prior.score_codes(codes, **kw)) and _same_bits(logp, prior.score_codes(codes, use_graph=False, **kw))
    codes = torch.randint(0, K ** ncb, (3, nt), generator=torch.Generator().manual_seed(21))
    _, _, rms, rows = _greedy_loop(prior, codes)
    dig = [(codes // K ** j) % K for j in range(ncb)]
    ref = sum(torch.log_softmax(rows[j], dim=-1).gather(2, dig[j].unsqueeze(2)).squeeze(2) for j in range(ncb))
    for method in ('cached', 'forward'):
        got = prior.score_codes(codes, method=method)
        err = (got.cpu().double() - ref).abs()
        tol = torch.tensor([[sum(2 * decoder_pair_bound * rms + C.logp_bound(rows[j][b, e], int(dig[j][b, e])) for j in range(ncb))
                             + (ncb - 1) * R.U * abs(float(ref[b, e])) for e in range(nt)] for b in range(3)])
        print(f'{ncb} x {K} {method}: max |score_codes - chained log_softmax(forward)| = {float(err.max()):.2e}, smallest tolerance '
              f'{float(tol.min()):.2e}')
        assert bool((err <= tol).all()), (method, float((err / tol).max()))


@pytest.mark.parametrize('method', ['auto', 'cached', 'forward'])
def test_determinism_row_and_chunk_invariance(fp32_gemms, method):  # noqa: F811
    import functools
    prior = _prior(512, 2)
    V, N = 512 ** 2, prior.num_tokens
    gen = functools.partial(prior.generate_codes, method=method)
    a = gen(20, num_generated_codes=4, seed=7)
    assert torch.equal(a, gen(20, num_generated_codes=4, seed=7)) and torch.equal(a, gen(20, num_generated_codes=4, seed=7, use_graph=False))
    assert not torch.equal(a, gen(20, num_generated_codes=4, seed=8))
    assert a.shape == (4, 20) and bool(((a >= 0) & (a < V)).all()) and len(torch.unique(a)) > 4
    assert len(torch.unique(a % 512)) > 4 and len(torch.unique(a // 512)) > 4              # both digits are drawn
    seeds = torch.tensor([11, 22, 33, 44], dtype=torch.int64)
    assert torch.equal(gen(20, num_generated_codes=4, seed=seeds)[2], gen(20, num_generated_codes=1, seed=seeds[2:3])[0])
    s70 = torch.arange(70, dtype=torch.int64) * 31 + 5                # 70 rows run as 64 + 6
    full, lp = gen(14, num_generated_codes=70, seed=s70, return_logp=True)
    p1, l1 = gen(14, num_generated_codes=64, seed=s70[:64], return_logp=True)
    p2, l2 = gen(14, num_generated_codes=6, seed=s70[64:], return_logp=True)
    assert torch.equal(full, torch.cat([p1, p2])) and _same_bits(lp, torch.cat([l1, l2]))
    if method != 'forward':
        for stride in (2, 3, 5):
            s1 = gen(20, num_generated_codes=4, seed=7, window_stride=stride)
            assert torch.equal(s1, gen(20, num_generated_codes=4, seed=7, window_stride=stride, use_graph=False))
            assert torch.equal(s1[:, :N], a[:, :N]) and bool(((s1 >= 0) & (s1 < V)).all())


def test_the_merged_prior_still_refuses_2_x_512():
    prior = build_prior(prior_cfg(512, 2), 'merged').cuda()
    with pytest.raises(ValueError, match='4096'):
        prior.generate_codes(12)


# ---- 5. through a 'product' decoder -------------------------------------------------------------------------------------------
def test_generate_and_continue_tokens_through_a_product_decoder(fp32_gemms):  # noqa: F811
    K, ncb = 4, 3
    prior = _prior(K, ncb, vocab=[12, 12, 12, 12])
    dec = build_decoder(tiny_cfg(K, ncb), 'AC-AC', 'product', seed=5)
    nc, epc, E = dec.num_channels, dec.num_events_per_code, dec.data_processor.num_events
    codes, tokens = prior.generate(8, dec, temperature=1.0, num_generated_codes=2, seed=5)
    assert codes.shape == (2, 8) and tokens.shape == (2, 8 * epc, nc)
    assert torch.equal(codes, prior.generate_codes(8, temperature=1.0, num_generated_codes=2, seed=5))
    assert torch.equal(tokens, dec.generate_from_code_long(codes, temperature=1.0, seed=5))
    cons = torch.full((2, 8), -1, dtype=torch.int64)
    cons[:, 2] = 17
    c2, _, lp = prior.generate(8, dec, num_generated_codes=2, seed=5, code_constraint=cons, return_logp=True)
    assert bool((c2[:, 2] == 17).all()) and _same_bits(lp, prior.score_codes(c2))
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randint(0, 9, (1, 2 * epc, 1), generator=g) for _ in range(nc)], dim=2)      # two codes of tokens
    codes, tokens = prior.continue_tokens(x, 4, dec, num_continuations=2, seed=1)
    L = E // epc + 2
    assert codes.shape == (2, L + 4) and bool(((codes >= 0) & (codes < K ** ncb)).all())
    assert tokens.shape == (2, x.shape[1] + 4 * epc, nc)
    assert torch.equal(tokens[:, :x.shape[1]].cpu(), x.expand(2, -1, -1))                       # the opening comes back unchanged
    again = prior.continue_tokens(x, 4, dec, num_continuations=2, seed=1)
    assert torch.equal(again[0], codes) and torch.equal(again[1], tokens)


# ---- 6. training --------------------------------------------------------------------------------------------------------------
def _batches(cfg, n, seed, B=8):
    gen = torch.Generator().manual_seed(seed)
    return [{'x': torch.cat([torch.randint(0, v, (B, cfg['N'] * 4, 1), generator=gen) for v in cfg['vocab']], dim=2).cuda()}
            for _ in range(n)]


def test_replayed_step_is_the_eager_step():
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1)
    res = {}
    cfg = prior_cfg(512, 2)
    try:
        for graph in (False, True):
            prior = _prior(512, 2)
            prior.init_optimizers(lr=2e-3)
            prior.train()
            prior.enable_step_graph(graph)
            losses = [float(prior.train_step(b, train=True)) for b in _batches(cfg, 5, seed=9, B=4)]
            res[graph] = (losses, prior.flat.flat.detach().cpu().clone(), prior._graph.replays if prior._graph is not None else 0)
            prior.enable_step_graph(False)
    finally:
        hip.set_gemm_mode(0)
    assert res[False][2] == 0 and res[True][2] == 3
    assert np.allclose(res[False][0], res[True][0], rtol=1e-6), (res[False][0], res[True][0])
    assert float((res[False][1] - res[True][1]).abs().max()) < 1e-6 * float(res[False][1].abs().max())


def test_prior_learns_keeps_the_encoder_frozen_and_round_trips(tmp_path):
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1)
    try:
        cfg = prior_cfg(4, 3)
        prior = _prior(4, 3)
        prior.model_dir = str(tmp_path)
        enc0 = {k: v.detach().clone() for k, v in prior.encoder.state_dict().items()}
        prior.init_optimizers(lr=2e-3)
        lo, hi = prior.flat.flat.data_ptr(), prior.flat.flat.data_ptr() + 4 * prior.flat.numel
        assert lo <= prior.digit_embeddings.weight.data_ptr() < hi and lo <= prior.embedding.weight.data_ptr() < hi
        data = _batches(cfg, 1, seed=1) * 40
        first = prior.epoch(iter(data[:1]), train=False, num_batches=1)['loss']
        before = prior.digit_embeddings.weight.detach().clone()
        prior.epoch(iter(data), train=True, num_batches=40)
        last = prior.epoch(iter(data[:1]), train=False, num_batches=1)['loss']
        print(f'loss on the repeated batch: {first:.4f} -> {last:.4f}')
        assert last < 0.8 * first, (first, last)
        assert not torch.equal(before, prior.digit_embeddings.weight)
        for k, v in prior.encoder.state_dict().items():
            assert torch.equal(v, enc0[k]), k
        assert all(p.grad is None and not p.requires_grad for p in prior.encoder.parameters())
        prior.save()
        prior2 = _prior(4, 3, seed=9)
        prior2.model_dir = str(tmp_path)
        prior2.load(device='cuda')
        prior2.init_optimizers(lr=2e-3)
        assert prior2.global_step == 40 and prior2.optimizer.step_count == 40
        assert abs(prior2.epoch(iter(data[:1]), train=False, num_batches=1)['loss'] - last) < 1e-6
        for (k, p), (_, p2) in zip(prior.named_parameters(), prior2.named_parameters()):
            assert torch.equal(p, p2), k
    finally:
        hip.set_gemm_mode(0)


def test_train_model_through_the_getters(tmp_path):
    from vqcpc_bach_amd import configs, getters
    from vqcpc_bach_amd.dataloaders.synthetic_student_dataloader import SyntheticStudentDataloaderGenerator
    from vqcpc_bach_amd.priors.generation import IncrementalProductPrior  # noqa: F401
    config = configs.make_prior_config(dropout=0.0, code_model='product')
    assert config['prior_kwargs']['code_model'] == 'product' and 'code_model' not in configs.make_prior_config()['prior_kwargs']
    cfg = prior_cfg(8, 2)
    prior0 = build_prior(cfg)
    dlg = SyntheticStudentDataloaderGenerator(sequences_size=cfg['N'], subdivision=4, vocab=cfg['vocab'], seed=4, device='cuda')
    kwargs = dict(d_model=16, n_head=1, num_layers=2, dim_feedforward=32, embedding_size=4, dropout=0.0, code_model='product',
                  num_events=cfg['N'])
    prior = getters.get_prior(str(tmp_path / 'prior'), dlg, prior0.encoder, 'transformer_relative', kwargs).cuda()
    assert prior.code_model == 'product' and prior.embedding.weight.shape == (2, 8, 4)
    assert prior.digit_embeddings.weight.shape == (1, 8, 16) and [tuple(h.weight.shape) for h in prior.pre_softmaxes] == [(8, 16)] * 2
    hist = prior.train_model(batch_size=4, num_batches=4, num_epochs=1, lr=1e-3)
    assert len(hist) == 1 and np.isfinite(hist[0][0]['loss']) and np.isfinite(hist[0][1]['loss'])
    with pytest.raises(ValueError, match='code_model'):
        getters.get_prior(str(tmp_path / 'x'), dlg, prior0.encoder, 'transformer_relative', dict(kwargs, code_model='joint'))
