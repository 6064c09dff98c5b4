"""Decoder generation (decoders/generation.py, csrc/decode.hip) against
  (1) the full forward of this package (teacher-forced incremental logits == `forward` logits),
  (2) fixtures of the reference's own generate loop and `top_k_top_p_filtering` (tests/golden/generate_*.npz),
  (3) sampling statistics, determinism, batch invariance and the public `Decoder.generate*` surface."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, sub_state
from decode_reference import filter_ref as _filtered_probs
from oracle import decoder_oracle as D
from test_decoder_gpu import build_decoder, seeded_decoder

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _golden_decoder(name):
    g = load_golden(name)
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    prefix = 'sd0' if any(k.startswith('sd0/') for k in g) else 'sd'
    return build_decoder(cfg, sub_state(g, prefix)), cfg, g


def _random_inputs(dec, B, seed):
    g = torch.Generator().manual_seed(seed)
    ncodes = dec.source_embeddings.weight.shape[0]
    codes = torch.randint(0, ncodes, (B, dec.num_tokens_source), generator=g)
    x = torch.cat([torch.randint(0, v, (B, dec.num_tokens_target // dec.num_channels, 1), generator=g)
                   for v in dec.num_tokens_per_channel], dim=2)
    return codes.cuda(), x.cuda()


def _teacher_forced_error(dec, B, seed):
    """max |incremental logits - forward logits| / rms(forward logits) over every position and row."""
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.utils import flatten
    dec.eval()
    codes, x = _random_inputs(dec, B, seed)
    nc = dec.num_channels
    with torch.no_grad():
        full = dec.forward(codes, x)['weights_per_category']
        inc = IncrementalDecoder(dec, B)
        inc.prefill(codes)
        inc.start(teacher=flatten(x))
        worst, rms = 0.0, 0.0
        for t in range(dec.num_tokens_target):
            inc.step()
            c = t % nc
            mine = inc.logits[:, inc.offsets[c]:inc.offsets[c + 1]]
            ref = full[c][:, t // nc]
            worst = max(worst, float((mine - ref).abs().max()))
        rms = float(torch.cat([f.reshape(-1) for f in full]).pow(2).mean().sqrt())
        assert torch.equal(inc.tokens, flatten(x))          # teacher forcing writes the given tokens
    return worst / rms


@pytest.mark.parametrize('name', ['decoder_tiny', 'decoder_tiny_fullcross', 'DEC'])
def test_incremental_step_equals_full_forward(name):
    """Teacher-forced: the logits handed to the sampler at position t equal forward(codes, x)[t % nc][:, t // nc].
    Measured on the MI355X, max |difference| / rms(logits): 8.2e-7 (tiny), 7.6e-7 (fullCross), 2.4e-6 (DEC, B = 2)."""
    if name == 'DEC':
        dec, _ = seeded_decoder(D.make_cfg('DEC', B=2), 5)          # d 512, 8 heads of 64, 3 + 3 layers, T 384, S 24
        B = 2
    else:
        dec, _, _ = _golden_decoder(name)
        B = 3
    err = _teacher_forced_error(dec, B, seed=11)
    print(f'{name}: max |incremental - forward| / rms = {err:.2e}')
    assert err < 1e-5, err


def test_greedy_generation_equals_the_reference():
    g = load_golden('generate_greedy_tiny')
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    dec = build_decoder(cfg, sub_state(g, 'sd'))
    codes = T(g['codes']).cuda()
    for use_graph in (True, False):
        tokens = dec.generate_from_codes(codes, top_k=1, seed=0, use_graph=use_graph)
        assert torch.equal(tokens.cpu(), T(g['tokens'])), use_graph


def _sample_once(logits, V, temperature, top_k, top_p, exclude=None, teacher=True, seeds=None, T_=1, probs=True):
    """Direct vqcpc_decode_sample calls on rows (M, V) of ONE voice; returns (probs, tokens)."""
    import ctypes
    from vqcpc_bach_amd import hip
    M = logits.shape[0]
    dev = logits.device
    offs = (ctypes.c_int32 * 2)(0, V)
    pos = torch.zeros(1, dtype=torch.int32, device=dev)
    tokens = torch.zeros(M, T_, dtype=torch.int64, device=dev)
    table = torch.zeros(V + 1, 4, device=dev)
    nxt = torch.zeros(M, 4, device=dev)
    pr = torch.zeros(M, V, device=dev) if probs else None
    teach = torch.zeros(M, T_, dtype=torch.int64, device=dev) if teacher else None
    excl = None
    if exclude:
        bits = np.zeros(8, np.int64)
        for t in exclude:
            bits[t // 32] |= 1 << (t % 32)
        excl = T(np.where(bits >= 1 << 31, bits - (1 << 32), bits).astype(np.int32)).cuda()
    sd = seeds if seeds is not None else torch.arange(M, dtype=torch.int64, device=dev)
    for _ in range(T_):
        hip.call('vqcpc_decode_sample', logits, V, offs, 1, M, float(temperature), int(top_k), float(top_p), excl, sd, teach,
                 T_, tokens, T_, T_, table, V + 1, 4, 1, nxt, 4, pr, V, pos)
    assert int(pos.item()) == T_
    return pr, tokens


def test_filter_equals_the_reference():
    g = load_golden('generate_filter')
    logits, widths, keep = g['logits'], g['widths'], g['keep']
    for V in sorted(set(widths.tolist())):
        rows = np.nonzero(widths == V)[0]
        lg = T(logits[rows, :V].copy()).cuda()
        for a, k in enumerate(g['top_k']):
            for b, p in enumerate(g['top_p']):
                for c, temp in enumerate(g['temperature']):
                    pr, _ = _sample_once(lg, V, float(temp), int(k), float(p))
                    pr = pr.cpu().double()
                    ref_keep = T(keep[rows, a, b, c, :V])
                    f = T(logits[rows, :V].copy()).double() / float(temp)
                    if p >= 1.0:
                        # documented deviation: top_p >= 1 keeps all, where the reference can drop tail tokens whose fp32
                        # cumulative sum rounds above 1.0 -- only mass below 1e-7
                        extra = (pr > 0) & ~ref_keep
                        assert float(torch.softmax(f, dim=-1)[extra].sum()) < 1e-7
                        ref_keep = ref_keep | extra
                    assert torch.equal(pr > 0, ref_keep), (V, k, p, temp)
                    f = f.masked_fill(~ref_keep, -float('inf'))
                    assert float((pr - torch.softmax(f, dim=-1)).abs().max()) < 1e-6, (V, k, p, temp)


@pytest.mark.parametrize('temperature', [0.5, 1.0, 2.0])
@pytest.mark.parametrize('top_k,top_p', [(0, 1.0), (8, 1.0), (0, 0.9), (12, 0.95)])
def test_sampling_frequencies(temperature, top_k, top_p):
    """2^18 draws (64 rows x 4096 positions) from one fixed row: every token within 5 sigma of its filtered probability,
    nothing outside the keep-set, excluded tokens never."""
    V, M, steps = 40, 64, 4096
    row = np.random.default_rng(3).standard_normal(V).astype(np.float32) * 1.5
    exclude = (3, 17)
    lg = T(np.tile(row, (M, 1))).cuda()
    seeds = torch.arange(1000, 1000 + M, dtype=torch.int64).cuda() * 7919
    _, tokens = _sample_once(lg, V, temperature, top_k, top_p, exclude=exclude, teacher=False, seeds=seeds, T_=steps,
                             probs=False)
    counts = torch.bincount(tokens.reshape(-1).cpu(), minlength=V).double()
    N = float(M * steps)
    p = _filtered_probs(row, temperature, top_k, top_p, exclude)
    assert float(counts[p == 0].sum()) == 0.0
    assert float(counts[list(exclude)].sum()) == 0.0
    sigma = (N * p * (1 - p)).sqrt()
    dev = (counts - N * p).abs()
    assert bool((dev <= 5 * sigma + 1).all()), (dev / (sigma + 1e-12)).max()


def test_determinism_and_batch_invariance():
    dec, _, _ = _golden_decoder('decoder_tiny')
    codes, _ = _random_inputs(dec, 4, seed=21)
    a = dec.generate_from_codes(codes, seed=7)
    b = dec.generate_from_codes(codes, seed=7)
    e = dec.generate_from_codes(codes, seed=7, use_graph=False)
    assert torch.equal(a, b) and torch.equal(a, e)
    assert not torch.equal(a, dec.generate_from_codes(codes, seed=8))
    seeds = torch.tensor([11, 22, 33, 44], dtype=torch.int64)
    four = dec.generate_from_codes(codes, seed=seeds)
    one = dec.generate_from_codes(codes[2:3], seed=seeds[2:3])
    assert torch.equal(four[2], one[0])
    # num_decodings: rows repeated in place
    two = dec.generate_from_codes(codes[:2], num_decodings=3, seed=5)
    assert two.shape == (6, dec.num_tokens_target // dec.num_channels, dec.num_channels)
    # B = 70 runs as 64 + 6
    codes70, _ = _random_inputs(dec, 70, seed=22)
    s70 = torch.arange(70, dtype=torch.int64) * 31 + 5
    full = dec.generate_from_codes(codes70, seed=s70)
    parts = torch.cat([dec.generate_from_codes(codes70[:64], seed=s70[:64]),
                       dec.generate_from_codes(codes70[64:], seed=s70[64:])], dim=0)
    assert torch.equal(full, parts)


def test_greedy_self_consistency_at_dec_shape():
    """B = 8, 384 tokens, replayed, top_k = 1: the full forward on the generated sequence picks the generated token at
    every position, except where its own top-1 / top-2 gap is < 1e-4."""
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=8), 6)
    codes, _ = _random_inputs(dec, 8, seed=23)
    x = dec.generate_from_codes(codes, top_k=1, seed=1)
    nc = dec.num_channels
    with torch.no_grad():
        logits = dec.forward(codes, x)['weights_per_category']
    for c in range(nc):
        top2 = torch.topk(logits[c], 2, dim=-1)[0]
        gap = top2[..., 0] - top2[..., 1]
        agree = logits[c].argmax(dim=-1) == x[:, :, c]
        assert bool((agree | (gap < 1e-4)).all()), c
        assert bool((x[:, :, c] < dec.num_tokens_per_channel[c]).all())


def _api_decoder(tmp_path):
    from vqcpc_bach_amd.dataloaders.synthetic_student_dataloader import SyntheticStudentDataloaderGenerator
    dec, cfg, _ = _golden_decoder('decoder_tiny')
    dec.model_dir = str(tmp_path)
    dec.dataloader_generator = SyntheticStudentDataloaderGenerator(sequences_size=cfg['events'] // 4, subdivision=4,
                                                                   vocab=cfg['vocab'], seed=4)
    return dec, cfg


def test_generate_api(tmp_path):
    dec, cfg = _api_decoder(tmp_path)
    nc, E = len(cfg['vocab']), cfg['events']
    dec.train()
    out = dec.generate(temperature=1.0, batch_size=2, seed_set='val', seed=3)
    assert dec.training
    assert set(out) == {'original', 'generation', 'codes', 'recoding'}
    assert out['original'].shape == (2, E, nc) and out['generation'].shape == (2, E, nc)
    assert out['codes'].shape == (2, dec.num_tokens_source) and out['recoding'].shape == (3, dec.num_tokens_source)
    for c, v in enumerate(cfg['vocab']):
        assert bool((out['generation'][:, :, c] < v).all()) and bool((out['generation'] >= 0).all())
    files = glob.glob(os.path.join(str(tmp_path), 'generations', '*.txt'))
    assert len(files) == 1
    lines = open(files[0]).read().splitlines()
    assert lines == [' , '.join(str(int(v)) for v in row) for row in out['recoding'].cpu()]
    dec.eval()
    jx = dec.generate(temperature=1.0, batch_size=1, seed_set='train', code_juxtaposition=True, seed=4)
    assert not dec.training
    assert jx['generation'].shape == (1, E, nc)
    assert glob.glob(os.path.join(str(tmp_path), 'juxtapositions', '*.txt'))
    with pytest.raises(NotImplementedError):
        dec.generate(temperature=1.0, seed_set='val', plot_attentions=True)
    with pytest.raises(ValueError):
        dec.generate(temperature=1.0, seed_set='val', exclude_meta_symbols=True)
    assert dec.init_generation(E).shape == (1, E, nc)
    for name in ('generate_from_code_long', 'generate_reharmonisation', 'generate_alla_mano', 'check_duplicate', 'plot'):
        with pytest.raises(NotImplementedError):
            getattr(dec, name)()


def test_generation_leaves_training_unaffected(tmp_path):
    """Four training steps (two eager, two replayed from the step graph) with a `generate` before the last one give
    bit-identical losses and parameters to the same steps without it."""
    g = load_golden('decoder_tiny')
    batch = {'x': T(g['batch/x'])}
    results = []
    for with_generation in (False, True):
        dec, _ = _api_decoder(tmp_path)
        dec.enable_step_graph(True)
        dec.train()
        losses = []
        for i in range(4):
            if with_generation and i == 3:
                dec.generate(temperature=1.0, batch_size=2, seed_set='val', seed=9)
                assert dec.training
            losses.append(dec.train_step(batch).clone())
        assert dec._graph is not None and dec._graph.replays >= 1
        results.append((torch.stack(losses).cpu(), [p.detach().cpu().clone() for p in dec.parameters()]))
    (l0, p0), (l1, p1) = results
    assert torch.equal(l0, l1)
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
