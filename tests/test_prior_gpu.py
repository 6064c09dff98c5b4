"""The code prior on the GPU (priors/prior_relative.py, priors/generation.py, csrc/prior.hip) against
  (1) fixtures of the reference's own PriorRelative (tests/golden/prior_*.npz: forward / backward, the window rule of its
      generate loop with arg-max, its temperature rule) and of `top_k_top_p_filtering` (generate_filter.npz),
  (2) the full forward of this package (incremental logits == `forward` logits, head and sliding regimes),
  (3) sampling statistics, determinism, batch and chunk invariance, the public `generate_codes` / `generate` surface,
  (4) the training step (learning, replayed == eager, frozen encoder, checkpoints)."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, sub_state
from test_prior_cpu import build_prior

pytestmark = pytest.mark.gpu
T = torch.from_numpy
LOSS_TOL, RMS_TOL = 5e-5, 5e-4          # the standing tolerances for reference fixtures (README "parity")


def rms_err(a, b):
    """max |a - b| / rms(b)."""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.pow(2).mean().sqrt() + 1e-300))


def _golden_prior(tag, name='prior_tiny'):
    g = load_golden(name)
    pre = f'{tag}/' if tag else ''
    cfg = json.loads(str(g[pre + 'cfg_json']))
    prior = build_prior(cfg, sub_state(g, pre + 'sd')).cuda()
    return prior, cfg, g


@pytest.fixture
def fp32_gemms():
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(0)
    yield
    hip.set_gemm_mode(0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward / backward parity with the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1], ids=['f32', 'bf16x6'])
@pytest.mark.parametrize('tag', ['v32', 'v1024'])
def test_forward_backward_equal_the_reference(tag, mode):
    from vqcpc_bach_amd import hip
    prior, cfg, g = _golden_prior(tag)
    hip.set_gemm_mode(mode)
    try:
        prior.eval()
        prior.init_optimizers(lr=1e-3)
        codes = T(g[f'{tag}/codes']).cuda()
        with torch.no_grad():
            fp = prior.forward(codes)
        ref_loss = float(g[f'{tag}/loss'])
        print(f'{tag} mode {mode}: loss {fp["monitored_quantities"]["loss"]:.7f} (reference {ref_loss:.7f}), logits '
              f'{rms_err(fp["weights_per_category"][0], g[f"{tag}/logits"]):.2e} of the rms')
        assert set(fp) == {'loss', 'weights_per_category', 'monitored_quantities'}
        assert abs(fp['monitored_quantities']['loss'] - ref_loss) <= LOSS_TOL * ref_loss
        assert fp['weights_per_category'][0].shape == g[f'{tag}/logits'].shape
        assert rms_err(fp['weights_per_category'][0], g[f'{tag}/logits']) <= RMS_TOL
        loss, _ = prior.compute_loss(codes)
        prior.flat.zero_grad()
        loss.backward()
        worst = 0.0
        for k, p in prior.named_parameters():
            if k.startswith('encoder.'):
                assert p.grad is None, k
                continue
            ref = g[f'{tag}/grad/{k}']
            if float(np.abs(ref).max()) == 0.0:
                assert float(p.grad.abs().max()) == 0.0, k
            else:
                e = rms_err(p.grad, ref)
                worst = max(worst, e)
                assert e <= RMS_TOL, (k, e)
        print(f'{tag} mode {mode}: worst gradient error {worst:.2e} of the rms')
    finally:
        hip.set_gemm_mode(0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. greedy generation: the reference's window rule
# ---------------------------------------------------------------------------------------------------------------------
def test_greedy_codes_equal_the_reference(fp32_gemms):
    prior, cfg, g = _golden_prior('', 'prior_greedy_tiny')
    ref = T(g['codes'])
    nt = int(g['num_tokens'])
    assert nt >= 3 * cfg['N'] and float(g['gaps'].min()) > 1e-3
    for method in ('auto', 'cached', 'forward'):
        for use_graph in (True, False):
            codes = prior.generate_codes(nt, top_k=1, num_generated_codes=ref.shape[0], seed=0, use_graph=use_graph,
                                         method=method)
            assert codes.dtype == torch.int64 and codes.is_cuda and codes.shape == ref.shape
            assert torch.equal(codes.cpu(), ref), (method, use_graph, codes.cpu(), ref)


# ---------------------------------------------------------------------------------------------------------------------
# 3. incremental == full forward
# ---------------------------------------------------------------------------------------------------------------------
def _pri_shape_prior(seed=31):
    cfg = dict(emb=8, vocab=[11, 12, 13, 14], d=32, H=2, layers=[1, 1], ff=64, D=8, zdim=8, up_hidden=16, Kl=2, Kr=2, K=32,
               ncb=1, p_d=512, p_H=8, p_layers=6, p_ff=1024, p_emb=32, N=24)
    torch.manual_seed(seed)
    prior = build_prior(cfg).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in prior.named_parameters():
            if not k.startswith('encoder.') and p.dim() == 1:
                p.add_(0.05 * torch.randn(p.shape, generator=g).cuda())
    return prior.eval()


def _incremental_errors(prior, B, seed):
    """max |incremental logits - forward logits| / rms(forward logits): (head regime cached, head regime forward form,
    sliding stride 1, sliding stride 4)."""
    from vqcpc_bach_amd.priors.generation import IncrementalPrior
    N, V = prior.num_tokens, prior.num_tokens_per_channel[0]
    nt = N + 9
    full = torch.randint(0, V, (B, nt), generator=torch.Generator().manual_seed(seed)).cuda()
    out = []
    with torch.no_grad():
        inc = IncrementalPrior(prior, B)
        # head: N teacher-forced steps in window 0
        ref = prior.forward(full[:, :N])['weights_per_category'][0]
        rms = float(ref.pow(2).mean().sqrt())
        inc.start(nt, seeds=1, teacher=full[:, :N])
        worst = 0.0
        for t in range(N):
            inc.step()
            worst = max(worst, float((inc.logits - ref[:, t]).abs().max()))
        assert torch.equal(inc.codes_win, full[:, :N])              # teacher forcing writes the given codes
        assert int(inc.pos.item()) == N
        out.append(worst / rms)
        # the forward form of the step IS the forward on the window: the head of one row by another kernel
        inc.start(nt, seeds=1, teacher=full[:, :N])
        worst = 0.0
        for t in range(N):
            inc.step_forward(t)
            worst = max(worst, float((inc.logits - ref[:, t]).abs().max()))
        assert torch.equal(inc.codes_win, full[:, :N]) and int(inc.pos.item()) == N
        out.append(worst / rms)
        # sliding: re-prefill + step(s) on windows further along the sequence
        for k, windows in ((1, (1, 5, 9)), (4, (4, 8))):
            worst = 0.0
            for w in windows:
                inc.start(nt, seeds=1)
                inc.seq.copy_(full)
                inc.slide(w, N - k, advance=k)
                assert int(inc.pos.item()) == N - k and inc.win.tolist() == [w + k, w]
                inc.teacher = full[:, w:w + N].contiguous()
                ref = prior.forward(full[:, w:w + N])['weights_per_category'][0]
                for t in range(N - k, N):
                    inc.step()
                    worst = max(worst, float((inc.logits - ref[:, t]).abs().max()))
                inc.commit()
                assert torch.equal(inc.seq, full)                    # the commit puts back what the window held
            out.append(worst / rms)
    return out


def test_incremental_steps_equal_the_full_forward(fp32_gemms):
    """Teacher-forced, head regime and re-prefilled windows (stride 1 and 4).  Bound: twice the error of the existing
    decoder pair (IncrementalDecoder vs Decoder.forward at the DEC shape, README: 2.4e-6 of the rms) measured in this run.
    Measured on the MI355X: decoder pair 2.49e-6 (bound 4.98e-6); prior at the PRI shape 1.30e-6 / 8.7e-7 / 9.2e-7 / 1.09e-6 (head /
    head forward form / stride 1 / stride 4), v32 5.9e-7 / 4.0e-7 / 4.0e-7 / 5.9e-7, v1024 8.1e-7 / 8.1e-7 / 1.0e-6 / 8.1e-7 (profiles/generate_prior_perf_log.md)."""
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from test_generate_gpu import _teacher_forced_error
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=2), 5)
    dec_err = _teacher_forced_error(dec, 2, seed=11)
    del dec
    bound = 2 * dec_err
    print(f'decoder pair (DEC, B = 2): {dec_err:.2e} of the rms -> bound for the prior {bound:.2e}')
    pri = _incremental_errors(_pri_shape_prior(), 2, seed=12)
    print('prior at the PRI shape (head, head forward form, stride 1, stride 4): ' + ', '.join(f'{e:.2e}' for e in pri))
    tiny = _incremental_errors(_golden_prior('v32')[0].eval(), 3, seed=13)
    print('prior v32 (head, head forward form, stride 1, stride 4): ' + ', '.join(f'{e:.2e}' for e in tiny))
    big = _incremental_errors(_golden_prior('v1024')[0].eval(), 3, seed=14)
    print('prior v1024 (head, head forward form, stride 1, stride 4): ' + ', '.join(f'{e:.2e}' for e in big))
    for e in pri + tiny + big:
        assert e <= bound, (e, bound)


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _sample(logits, temperature=1.0, top_k=0, top_p=1.0, seeds=None, N=1, steps=1, probs=True, pos0=0):
    """Direct vqcpc_prior_sample calls on rows (M, V); returns (probs of the last call, codes (M, N))."""
    from vqcpc_bach_amd import hip
    hip.load()
    M, V = logits.shape
    dev = logits.device
    pos = torch.full((1,), pos0, dtype=torch.int32, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    codes = torch.full((M, N), -1, dtype=torch.int64, device=dev)
    table = torch.arange(V + 1, dtype=torch.float32, device=dev).view(V + 1, 1).repeat(1, 4).contiguous()
    nxt = torch.zeros(M, 4, device=dev)
    pr = torch.zeros(M, V, device=dev) if probs else None
    teach = torch.zeros(M, N, dtype=torch.int64, device=dev) if seeds is None else None
    for _ in range(steps):
        hip.call('vqcpc_prior_sample', logits, V, V, M, float(temperature), int(top_k), float(top_p), seeds, teach, N, codes, N,
                 N, table, V + 1, 4, nxt, 4, pr, V, pos, ticket)
    assert int(ticket.item()) == 0
    if seeds is not None and steps >= 1 and pos0 + steps <= N:
        assert torch.equal(nxt[:, 0].long(), codes[:, pos0 + steps - 1])   # the next input row is the drawn code's table row
    return pr, codes, pos


def test_temperature_rule_equals_the_reference():
    g = load_golden('prior_temperature')
    for V in (32, 1024, 4096):
        lg = T(g[f'logits_{V}']).cuda()
        for i, temp in enumerate(g['temperature']):
            pr, _, pos = _sample(lg, temperature=float(temp))
            err = float((pr.cpu().double() - T(g[f'probs_{V}'][i])).abs().max())
            print(f'V {V} temperature {float(temp)}: max |p - reference| = {err:.2e}')
            assert err <= 1e-6, (V, temp, err)
            assert int(pos.item()) == 1
    # the opposite sense of the decoder's rule: a larger temperature sharpens
    lg = T(g['logits_32']).cuda()
    assert float(_sample(lg, temperature=2.0)[0].max()) > float(_sample(lg, temperature=0.5)[0].max())


def test_filter_equals_the_reference():
    """Keep-masks of the reference's top_k_top_p_filtering on logits / T: this kernel multiplies, so it gets 1 / T."""
    g = load_golden('generate_filter')
    logits, widths, keep = g['logits'], g['widths'], g['keep']
    for V in sorted(set(widths.tolist())):
        rows = np.nonzero(widths == V)[0]
        lg = T(logits[rows, :V].copy()).cuda()
        for a, k in enumerate(g['top_k']):
            for b, p in enumerate(g['top_p']):
                for c, temp in enumerate(g['temperature']):
                    pr, _, _ = _sample(lg, temperature=1.0 / float(temp), top_k=int(k), top_p=float(p))
                    pr = pr.cpu().double()
                    ref_keep = T(keep[rows, a, b, c, :V])
                    f = T(logits[rows, :V].copy()).double() / float(temp)
                    if p >= 1.0:
                        # documented deviation (as vqcpc_decode_sample): top_p >= 1 keeps all, where the reference can drop
                        # tail tokens whose fp32 cumulative sum rounds above 1.0 -- only mass below 1e-7
                        extra = (pr > 0) & ~ref_keep
                        assert float(torch.softmax(f, dim=-1)[extra].sum()) < 1e-7
                        ref_keep = ref_keep | extra
                    assert torch.equal(pr > 0, ref_keep), (V, k, p, temp)
                    f = f.masked_fill(~ref_keep, -float('inf'))
                    assert float((pr - torch.softmax(f, dim=-1)).abs().max()) < 1e-6, (V, k, p, temp)


def test_filter_at_large_vocabularies():
    """The fixture's rows are at most 60 wide; the radix select and the LDS sort at V = 1024 / 4096 against float64."""
    gen = np.random.default_rng(8)
    for V in (1000, 4096):
        row = (gen.standard_normal((3, V)) * 2.0).astype(np.float32)
        lg = T(row).cuda()
        pr, _, _ = _sample(lg, top_k=50)
        pr = pr.cpu()
        for r in range(3):
            assert int((pr[r] > 0).sum()) == 50
            assert set(torch.nonzero(pr[r] > 0).flatten().tolist()) == set(np.argsort(-row[r])[:50].tolist())
        pr, _, _ = _sample(lg, top_p=0.9)
        pr = pr.cpu()
        p64 = torch.softmax(T(row).double(), dim=-1)
        for r in range(3):
            order = torch.argsort(p64[r], descending=True)
            kept = pr[r][order] > 0
            n = int(kept.sum())
            assert bool(kept[:n].all()) and n >= 1               # a prefix of the sorted order
            cum = torch.cumsum(p64[r][order], dim=0)
            assert float(cum[n - 1]) > 0.9 - 1e-5                # the kept mass reaches top_p ...
            assert n == 1 or float(cum[n - 2]) <= 0.9 + 1e-5     # ... and the last kept token was needed for it
            assert abs(float(pr[r].sum()) - 1.0) < 1e-5


def test_draws_follow_the_probabilities():
    """n = 200 000 draws (64 rows x 3 125 positions, distinct (seed, position) keys) of one fixed 32-way distribution: every
    frequency within 5 sqrt(p (1 - p) / n) of its probability."""
    V, M, N, n = 32, 64, 1024, 200000
    row = (np.random.default_rng(5).standard_normal(V) * 1.5).astype(np.float32)
    lg = T(np.tile(row, (M, 1))).cuda()
    counts = torch.zeros(V, dtype=torch.float64)
    left = n // M
    pas = 0
    while left > 0:
        steps = min(N, left)
        seeds = (torch.arange(M, dtype=torch.int64) * 7919 + 1000003 * (pas + 1)).cuda()
        _, codes, pos = _sample(lg, seeds=seeds, N=N, steps=steps, probs=False)
        assert int(pos.item()) == steps
        drawn = codes[:, :steps].reshape(-1).cpu()
        assert bool(((drawn >= 0) & (drawn < V)).all()) and bool((codes[:, steps:] == -1).all())
        counts += torch.bincount(drawn, minlength=V).double()
        left -= steps
        pas += 1
    assert float(counts.sum()) == n
    p = torch.softmax(T(row).double(), dim=-1)
    dev = (counts / n - p).abs()
    lim = 5 * (p * (1 - p) / n).sqrt()
    print(f'worst deviation {float((dev / lim).max()) * 5:.2f} sigma')
    assert bool((dev <= lim).all()), (dev / lim).max()


def test_sampler_does_nothing_past_the_window():
    lg = torch.randn(2, 32, device='cuda')
    seeds = torch.tensor([3, 4], dtype=torch.int64).cuda()
    _, codes, pos = _sample(lg, seeds=seeds, N=4, steps=3, pos0=4)
    assert int(pos.item()) == 4 and bool((codes == -1).all())


# ---------------------------------------------------------------------------------------------------------------------
# 6. the public surface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['auto', 'cached', 'forward'])
def test_determinism_row_and_chunk_invariance_of_each_form(fp32_gemms, method):
    import functools
    prior, cfg, _ = _golden_prior('v32')
    gen = functools.partial(prior.generate_codes, method=method)
    a = gen(20, num_generated_codes=4, seed=7)
    assert torch.equal(a, gen(20, num_generated_codes=4, seed=7))
    assert torch.equal(a, gen(20, num_generated_codes=4, seed=7, use_graph=False))
    assert not torch.equal(a, gen(20, num_generated_codes=4, seed=8))
    assert a.shape == (4, 20) and bool(((a >= 0) & (a < 32)).all()) and len(torch.unique(a)) > 4
    seeds = torch.tensor([11, 22, 33, 44], dtype=torch.int64)
    four = gen(20, num_generated_codes=4, seed=seeds)
    one = gen(20, num_generated_codes=1, seed=seeds[2:3])
    assert torch.equal(four[2], one[0])
    s70 = torch.arange(70, dtype=torch.int64) * 31 + 5                # 70 rows run as 64 + 6
    full = gen(14, num_generated_codes=70, seed=s70)
    parts = torch.cat([gen(14, num_generated_codes=64, seed=s70[:64]), gen(14, num_generated_codes=6, seed=s70[64:])], dim=0)
    assert torch.equal(full, parts)
    with pytest.raises(ValueError, match='method'):
        prior.generate_codes(20, method='fastest')
    if method == 'forward':
        with pytest.raises(ValueError, match='window_stride'):
            gen(20, window_stride=2)


def test_determinism_row_and_chunk_invariance(fp32_gemms):
    prior, cfg, _ = _golden_prior('v32')
    N, V = cfg['N'], 32
    a = prior.generate_codes(20, num_generated_codes=4, seed=7)
    b = prior.generate_codes(20, num_generated_codes=4, seed=7)
    e = prior.generate_codes(20, num_generated_codes=4, seed=7, use_graph=False)
    assert a.shape == (4, 20) and bool(((a >= 0) & (a < V)).all())
    assert torch.equal(a, b) and torch.equal(a, e)
    assert not torch.equal(a, prior.generate_codes(20, num_generated_codes=4, seed=8))
    assert len(torch.unique(a)) > 4                                  # it does sample
    for stride in (2, 3, 5):                                          # 14 = 4 * 3 + 2: a shorter last move at stride 3
        s1 = prior.generate_codes(20, num_generated_codes=4, seed=7, window_stride=stride)
        s2 = prior.generate_codes(20, num_generated_codes=4, seed=7, window_stride=stride, use_graph=False)
        assert torch.equal(s1, s2) and torch.equal(s1[:, :N], a[:, :N]) and bool(((s1 >= 0) & (s1 < V)).all())
    seeds = torch.tensor([11, 22, 33, 44], dtype=torch.int64)
    four = prior.generate_codes(20, num_generated_codes=4, seed=seeds)
    one = prior.generate_codes(20, num_generated_codes=1, seed=seeds[2:3])
    assert torch.equal(four[2], one[0])
    # 70 rows run as 64 + 6
    s70 = torch.arange(70, dtype=torch.int64) * 31 + 5
    full = prior.generate_codes(14, num_generated_codes=70, seed=s70)
    parts = torch.cat([prior.generate_codes(14, num_generated_codes=64, seed=s70[:64]),
                       prior.generate_codes(14, num_generated_codes=6, seed=s70[64:])], dim=0)
    assert torch.equal(full, parts)
    # training mode is put back; num_tokens == N never slides
    prior.train()
    assert prior.generate_codes(N, seed=1).shape == (1, N) and prior.training
    # the larger vocabulary end to end
    big, cfg2, _ = _golden_prior('v1024')
    c = big.generate_codes(15, num_generated_codes=3, seed=2, top_p=0.95)
    assert c.shape == (3, 15) and bool(((c >= 0) & (c < 1024)).all())
    assert torch.equal(c, big.generate_codes(15, num_generated_codes=3, seed=2, top_p=0.95, use_graph=False))


def test_moving_windows_change_the_seed(fp32_gemms):
    from vqcpc_bach_amd.priors.generation import IncrementalPrior
    prior, cfg, _ = _golden_prior('v32')
    prior.eval()
    inc = IncrementalPrior(prior, 3)
    inc.start(20, seeds=torch.tensor([5, 6, 7], dtype=torch.int64))
    assert torch.equal(inc.seeds, inc.row_seeds) and inc.row_seeds.tolist() == [5, 6, 7]      # window 0: the rows' own
    seen = [inc.seeds.clone()]
    for w in (1, 2, 3):
        inc.slide(w, cfg['N'] - 1)
        seen.append(inc.seeds.clone())
    for i in range(len(seen)):
        for j in range(i):
            assert bool((seen[i] != seen[j]).all()), (i, j)
    inc.slide(2, cfg['N'] - 1)
    assert torch.equal(inc.seeds, seen[2])                            # a function of (row seed, window)


def test_generate_hands_the_codes_to_the_decoder(fp32_gemms):
    from test_generate_gpu import _golden_decoder
    prior, cfg, _ = _golden_prior('v32')
    dec, dcfg, _ = _golden_decoder('decoder_tiny')                    # 256 merged codes >= the prior's 32, S = 3
    assert dec.source_embeddings.weight.shape[0] >= 32 and dec.num_tokens_source <= 8
    kw = dict(pad=[0, 0, 0, 0], start=[1, 1, 1, 1])
    codes, tokens = prior.generate(8, dec, temperature=1.0, num_generated_codes=2, num_decodings_per_generating_code=2, seed=5,
                                   **kw)
    assert codes.shape == (2, 8) and tokens.shape == (4, 8 * dec.num_events_per_code, dec.num_channels)
    assert torch.equal(codes, prior.generate_codes(8, temperature=1.0, num_generated_codes=2, seed=5))
    direct = dec.generate_from_code_long(codes, temperature=1.0, num_decodings=2, seed=5, **kw)
    assert torch.equal(tokens, direct)
    # decoder_temperature overrides the decoder's only
    c2, t2 = prior.generate(8, dec, temperature=1.0, num_generated_codes=2, num_decodings_per_generating_code=2, seed=5,
                            decoder_temperature=0.3, **kw)
    assert torch.equal(c2, codes)
    assert torch.equal(t2, dec.generate_from_code_long(codes, temperature=0.3, num_decodings=2, seed=5, **kw))
    assert not torch.equal(t2, tokens)
    # without it the prior's temperature reaches both
    c3, t3 = prior.generate(8, dec, temperature=2.0, num_generated_codes=2, seed=5, **kw)
    assert torch.equal(t3, dec.generate_from_code_long(c3, temperature=2.0, seed=5, **kw))


def test_generate_codes_refuses_a_vocabulary_beyond_the_sampler():
    g = load_golden('prior_tiny')
    cfg = dict(json.loads(str(g['v1024/cfg_json'])), K=512, ncb=2, p_emb=4)
    prior = build_prior(cfg).cuda()
    with pytest.raises(ValueError, match='4096'):
        prior.generate_codes(12)


# ---------------------------------------------------------------------------------------------------------------------
# 7. training
# ---------------------------------------------------------------------------------------------------------------------
def _batches(cfg, n, seed, B=8):
    gen = torch.Generator().manual_seed(seed)
    events = cfg['N'] * 4                                             # N codes = N * 16 tokens = N * 4 events of 4 voices
    return [{'x': torch.cat([torch.randint(0, v, (B, events, 1), generator=gen) for v in cfg['vocab']], dim=2).cuda()}
            for _ in range(n)]


def test_prior_learns_keeps_the_encoder_frozen_and_round_trips(tmp_path):
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1)
    try:
        prior, cfg, g = _golden_prior('v32')
        prior.model_dir = str(tmp_path)
        enc0 = {k: v.detach().clone() for k, v in prior.encoder.state_dict().items()}
        prior.init_optimizers(lr=2e-3)
        data = _batches(cfg, 1, seed=1) * 40
        first = prior.epoch(iter(data[:1]), train=False, num_batches=1)['loss']
        trn = prior.epoch(iter(data), train=True, num_batches=40)
        last = prior.epoch(iter(data[:1]), train=False, num_batches=1)['loss']
        print(f'loss on the repeated batch: {first:.4f} -> {last:.4f}')
        assert set(trn) >= {'loss'} and last < 0.8 * first, (first, last)
        assert prior.training is False and not prior.encoder.training
        for k, v in prior.encoder.state_dict().items():
            assert torch.equal(v, enc0[k]), k
        assert all(p.grad is None and not p.requires_grad for p in prior.encoder.parameters())
        assert prior.global_step == 40 and prior.optimizer.step_count == 40
        prior.save()
        prior2, _, _ = _golden_prior('v32')
        prior2.model_dir = str(tmp_path)
        prior2.load(device='cuda')
        prior2.init_optimizers(lr=2e-3)
        assert prior2.global_step == 40 and prior2.optimizer.step_count == 40
        assert abs(prior2.epoch(iter(data[:1]), train=False, num_batches=1)['loss'] - last) < 1e-6
        a = prior.epoch(iter(data[:1]), train=True, num_batches=1)['loss']
        b = prior2.epoch(iter(data[:1]), train=True, num_batches=1)['loss']
        assert abs(a - b) < 1e-6
        for (k, p), (_, p2) in zip(prior.named_parameters(), prior2.named_parameters()):
            assert torch.equal(p, p2), k                      # the resumed run continues bit-identically
    finally:
        hip.set_gemm_mode(0)


def test_replayed_step_is_the_eager_step():
    """The tolerances of tests/test_graphs_gpu.py::test_decoder_step_graph: losses rtol 1e-6, parameters 1e-6 of the largest."""
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1)
    res = {}
    try:
        for graph in (False, True):
            prior, cfg, _ = _golden_prior('v32')
            prior.init_optimizers(lr=2e-3)
            prior.train()
            prior.enable_step_graph(graph)
            losses = [float(prior.train_step(b, train=True)) for b in _batches(cfg, 5, seed=9, B=4)]
            replays = prior._graph.replays if prior._graph is not None else 0
            res[graph] = (losses, prior.flat.flat.detach().cpu().clone(), replays)
            prior.enable_step_graph(False)
    finally:
        hip.set_gemm_mode(0)
    assert res[False][2] == 0 and res[True][2] == 3
    assert np.allclose(res[False][0], res[True][0], rtol=1e-6), (res[False][0], res[True][0])
    assert float((res[False][1] - res[True][1]).abs().max()) < 1e-6 * float(res[False][1].abs().max())


def test_train_model_through_the_getters(tmp_path):
    """`train_model` on the synthetic 'prior' dataloader with a tiny encoder: the reference's entry point end to end."""
    import os
    from vqcpc_bach_amd.dataloaders.synthetic_student_dataloader import SyntheticStudentDataloaderGenerator
    prior, cfg, _ = _golden_prior('v32')
    prior.model_dir = str(tmp_path / 'prior')
    prior.dataloader_generator = SyntheticStudentDataloaderGenerator(sequences_size=cfg['N'], subdivision=4, vocab=cfg['vocab'],
                                                                     seed=4, device='cuda')
    hist = prior.train_model(batch_size=4, num_batches=4, num_epochs=1, lr=1e-3)
    assert len(hist) == 1 and np.isfinite(hist[0][0]['loss']) and np.isfinite(hist[0][1]['loss'])
    assert os.path.exists(os.path.join(prior.model_dir, 'prior'))
