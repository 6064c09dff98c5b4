"""Long-form generation (Decoder.generate_from_code_long, decoders/generation.py long mode, vqcpc_decode_prefill_attn /
vqcpc_decode_window) against
  (1) fixtures of the reference's own generate_from_code_long (tests/golden/generate_long_tiny_S*.npz),
  (2) the full forward of this package (re-prefill + teacher-forced steps == `forward` logits; slide consistency),
  (3) determinism, row invariance, chunking, the seed rule of moving windows and the public surface."""
import json
import types

import pytest
import torch

from conftest import load_golden, sub_state
from oracle import decoder_oracle as D
from test_decoder_gpu import build_decoder, seeded_decoder
from test_generate_gpu import _api_decoder, _golden_decoder, _random_inputs

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _meta_dataset(vocab):
    """START / END / XX as the last three ids of every voice (the stub dataset of tools/gen_golden_generate_long.py)."""
    n2i = [{'START': v - 3, 'END': v - 2, 'XX': v - 1} for v in vocab]
    return types.SimpleNamespace(dataset=types.SimpleNamespace(note2index_dicts=n2i))


def _meta_ids(dec):
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    return [v - 1 for v in vocab], [v - 3 for v in vocab]


def _random_codes(dec, B, nb, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, dec.source_embeddings.weight.shape[0], (B, nb), generator=g).cuda()


# ---- 4. greedy equality with the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['generate_long_tiny_S4', 'generate_long_tiny_S3'])
def test_greedy_long_generation_equals_the_reference(name):
    g = load_golden(name)
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    dec = build_decoder(cfg, sub_state(g, 'sd'))
    dec.dataloader_generator = types.SimpleNamespace(dataset=types.SimpleNamespace(
        note2index_dicts=[{'START': int(s), 'END': int(e), 'XX': int(p)} for s, e, p in zip(g['start'], g['end'], g['pad'])]))
    codes = T(g['codes']).cuda()
    for use_graph in (True, False):
        tokens = dec.generate_from_code_long(codes, temperature=1.0, top_k=1, num_decodings=int(g['num_decodings']),
                                             code_index_start=int(g['code_index_start']),
                                             code_index_end=int(g['code_index_end']), seed=0, use_graph=use_graph)
        assert tokens.dtype == torch.int64 and tokens.is_cuda
        assert torch.equal(tokens.cpu(), T(g['tokens'])), use_graph


# ---- 5. re-prefill equals the full forward ---------------------------------------------------------------------------
def _prefill_errors(dec, B, P, seed):
    """Prefill P tokens, teacher-force the rest: (max |logits - forward logits| / rms over the steps, max relative
    difference of the K/V cache rows [0, P) against P teacher-forced steps)."""
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.utils import flatten
    dec.eval()
    codes, x = _random_inputs(dec, B, seed)
    nc, U, Tt = dec.num_channels, dec.total_upscaling, dec.num_tokens_target
    with torch.no_grad():
        full = dec.forward(codes, x)['weights_per_category']
        rms = float(torch.cat([f.reshape(-1) for f in full]).pow(2).mean().sqrt())
        stepped = IncrementalDecoder(dec, B)
        stepped.prefill(codes)
        stepped.start(teacher=flatten(x))
        for _ in range(P):
            stepped.step()
        inc = IncrementalDecoder(dec, B)
        inc.start_long(codes, flatten(x), teacher=flatten(x))
        inc.slide(0, P // U)
        assert int(inc.pos.item()) == P
        cache = 0.0
        if P:
            assert torch.equal(inc.x, stepped.x)                              # the input row of position P
            for mine, ref in ((inc.kcache, stepped.kcache), (inc.vcache, stepped.vcache)):
                for li in range(mine.shape[0]):
                    r = ref[li, :, :P]
                    cache = max(cache, float((mine[li, :, :P] - r).abs().max() / r.pow(2).mean().sqrt()))
        worst = 0.0
        for t in range(P, Tt):
            inc.step()
            c = t % nc
            worst = max(worst, float((inc.logits[:, inc.offsets[c]:inc.offsets[c + 1]] - full[c][:, t // nc]).abs().max()))
        assert torch.equal(inc.tokens, flatten(x))
    return worst / rms, cache


@pytest.mark.parametrize('name', ['decoder_tiny', 'decoder_tiny_fullcross', 'DEC'])
def test_reprefill_equals_full_forward(name):
    """For P in {0, U, (S // 2) U, T - U}: after a re-prefill of P tokens every teacher-forced step's logits equal
    forward(codes, x) within 1e-5 of the forward logits' rms (the bound of test_incremental_step_equals_full_forward), and
    the K/V cache rows [0, P) equal those of P incremental steps within 1e-5 of their rms.
    Measured on the MI355X, max over the P (logits, caches): 8.6e-7, 9.3e-7 (tiny); 7.7e-7, 1.2e-6 (fullCross); 2.5e-6,
    2.3e-6 (DEC, B = 2)."""
    if name == 'DEC':
        dec, _ = seeded_decoder(D.make_cfg('DEC', B=2), 5)
        B = 2
    else:
        dec, _, _ = _golden_decoder(name)
        B = 3
    U, S, Tt = dec.total_upscaling, dec.num_tokens_source, dec.num_tokens_target
    for P in sorted({0, U, (S // 2) * U, Tt - U}):
        err, cache = _prefill_errors(dec, B, P, seed=11 + P)
        print(f'{name} P = {P}: logits {err:.2e}, caches {cache:.2e} (relative to rms)')
        assert cache < 1e-5, (P, cache)
        assert err < 1e-5, (P, err)


# ---- 6. slide consistency at DEC shape -------------------------------------------------------------------------------
def test_slide_consistency_at_dec_shape():
    """DEC shape, B = 2, nb = 2 S = 48 codes, greedy, every code generated (head, middle and tail): each drawn token is the
    argmax of the full forward on its window, except where that forward's own top-1 / top-2 gap is < 1e-4; the exempted
    share must stay <= 1 % of the positions.  Model seed 6 (the model of test_greedy_self_consistency_at_dec_shape):
    measured on the MI355X, 2 of 1 536 positions exempted (0.13 %)."""
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=2), 6)
    S, U, nc = dec.num_tokens_source, dec.total_upscaling, dec.num_channels
    epc = U // nc
    nb, B = 2 * S, 2
    codes = _random_codes(dec, B, nb, seed=31)
    pad, start = _meta_ids(dec)
    x = dec.generate_from_code_long(codes, temperature=1.0, top_k=1, seed=1, pad=pad, start=start)
    assert x.shape == (B, nb * epc, nc)
    exempt = total = 0
    dec.eval()
    with torch.no_grad():
        for ci in range(nb):
            tb, te, tr = dec.compute_start_end_times(ci, nb, S)
            logits = dec.forward(codes[:, tb:te], x[:, tb * epc:te * epc])['weights_per_category']
            for c in range(nc):
                lg = logits[c][:, tr * epc:(tr + 1) * epc]
                top2 = torch.topk(lg, 2, dim=-1)[0]
                close = (top2[..., 0] - top2[..., 1]) < 1e-4
                agree = lg.argmax(dim=-1) == x[:, ci * epc:(ci + 1) * epc, c]
                assert bool((agree | close).all()), (ci, c)
                exempt += int(close.sum())
                total += close.numel()
    print(f'slide consistency: {exempt} of {total} positions exempted ({100.0 * exempt / total:.3f} %)')
    assert exempt <= 0.01 * total, (exempt, total)


# ---- 7. determinism, row invariance, chunking, the seed rule -----------------------------------------------------------
def test_determinism_row_invariance_and_chunking():
    dec, _, _ = _golden_decoder('decoder_tiny')
    pad, start = _meta_ids(dec)
    kw = dict(temperature=1.0, code_index_start=1, pad=pad, start=start)
    nb = 8
    codes = _random_codes(dec, 3, nb, seed=41)
    a = dec.generate_from_code_long(codes, seed=7, **kw)
    assert torch.equal(a, dec.generate_from_code_long(codes, seed=7, **kw))
    assert torch.equal(a, dec.generate_from_code_long(codes, seed=7, use_graph=False, **kw))
    assert not torch.equal(a, dec.generate_from_code_long(codes, seed=8, **kw))
    for c, v in enumerate(dec.num_tokens_per_channel):
        assert bool((a[:, :, c] < v).all()) and bool((a >= 0).all())
    # a row alone, inside a batch of 3 and inside a batch of 70 (64 + 6)
    codes70 = _random_codes(dec, 70, nb, seed=42)
    s70 = torch.arange(70, dtype=torch.int64) * 31 + 5
    full = dec.generate_from_code_long(codes70, seed=s70, **kw)
    for r in (1, 66):
        alone = dec.generate_from_code_long(codes70[r:r + 1], seed=s70[r:r + 1], **kw)
        assert torch.equal(alone[0], full[r]), r
        three = dec.generate_from_code_long(codes70[r - 1:r + 2], seed=s70[r - 1:r + 2], **kw)
        assert torch.equal(three[1], full[r]), r
    # num_decodings: rows repeated in place, and the two decodings of one row differ
    two = dec.generate_from_code_long(codes[:1], num_decodings=2, seed=5, **kw)
    assert two.shape == (2, (nb - 1) * dec.num_events_per_code, dec.num_channels)
    assert not torch.equal(two[0], two[1])


def test_consecutive_middle_codes_draw_different_numbers():
    """Flat logits (zeroed heads), temperature 1: the token is a function of the uniform alone.  Every middle code is drawn
    at the same window positions, so unchanged seeds would repeat the same U tokens code after code."""
    dec, _, _ = _golden_decoder('decoder_tiny')
    with torch.no_grad():
        for m in dec.pre_softmaxes:
            m.weight.zero_()
            m.bias.zero_()
    pad, start = _meta_ids(dec)
    S, epc = dec.num_tokens_source, dec.num_events_per_code
    nb = 3 * S
    codes = _random_codes(dec, 4, nb, seed=43)
    for use_graph in (True, False):
        x = dec.generate_from_code_long(codes, temperature=1.0, seed=3, pad=pad, start=start, use_graph=use_graph)
        middle = [ci for ci in range(nb) if S // 2 <= ci < nb - S // 2]
        assert len(middle) >= 4
        for a, b in zip(middle[:-1], middle[1:]):
            for r in range(x.shape[0]):
                assert not torch.equal(x[r, a * epc:(a + 1) * epc], x[r, b * epc:(b + 1) * epc]), (a, b, r)


# ---- 8. nb == S: the window never moves --------------------------------------------------------------------------------
def test_single_window_equals_the_fixed_window_run():
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder, row_seeds
    dec, _, _ = _golden_decoder('decoder_tiny')
    dec.eval()
    pad, start = _meta_ids(dec)
    S, U, epc, Tt = dec.num_tokens_source, dec.total_upscaling, dec.num_events_per_code, dec.num_tokens_target
    B = 3
    codes = _random_codes(dec, B, S, seed=44)
    seeds = torch.tensor([101, 202, 303], dtype=torch.int64)
    long = dec.generate_from_code_long(codes, temperature=1.0, code_index_start=1, seed=seeds, pad=pad, start=start)
    chorale = dec.init_generation_chorale(S * epc, epc, pad=pad, start=start).reshape(1, Tt).expand(B, Tt)
    with torch.no_grad():
        inc = IncrementalDecoder(dec, B)
        inc.prefill(codes)
        inc.start(seeds=row_seeds(seeds, B), temperature=1.0, teacher=chorale)
        for _ in range(U):
            inc.step()                         # the first code teacher-forced (PAD ... START)
        inc.teacher = None
        for _ in range(Tt - U):
            inc.step()
    assert torch.equal(long.reshape(B, -1), inc.tokens[:, U:])


# ---- 9. the public surface ---------------------------------------------------------------------------------------------
def test_long_generation_api():
    dec, cfg, _ = _golden_decoder('decoder_tiny')
    vocab = cfg['vocab']
    nc, E, S = len(vocab), cfg['events'], dec.num_tokens_source
    epc = dec.num_events_per_code
    dec.dataloader_generator = _meta_dataset(vocab)
    meta = [[v - 3, v - 2, v - 1] for v in vocab]
    # generate_alla_mano: lists of codes, the body's events come back
    dec.train()
    out = dec.generate_alla_mano([1, 2], [3, 4, 5], [6, 7, 8, 9], temperature=1.0, seed=2)
    assert dec.training
    assert out.shape == (3, 4 * epc, nc) and out.dtype == torch.int64
    # exclude_meta_symbols is honoured
    ex = dec.generate_from_code_long(_random_codes(dec, 2, 2 * S, seed=45), temperature=2.0, exclude_meta_symbols=True, seed=4)
    assert ex.shape == (2, 2 * S * epc, nc)
    for c in range(nc):
        for t in meta[c]:
            assert not bool((ex[:, :, c] == t).any())
    # reharmonise_tokens on 2.5 windows of tokens: chunks START | E | E | E / 2 + END + PAD | PAD -> 5 * S codes
    g = torch.Generator().manual_seed(46)
    events = 2 * E + E // 2
    x = torch.cat([torch.randint(0, v - 3, (1, events, 1), generator=g) for v in vocab], dim=2)
    dec.eval()
    tokens, c0, c1, ncodes = dec.reharmonise_tokens(x, num_reharmonisations=2, temperature=1.0, top_k=0, top_p=0.9, seed=5,
                                                    return_bounds=True)
    assert not dec.training
    U = dec.total_upscaling
    completion = E - E // 2
    assert ncodes == 5 * S and c0 == E * nc // U and c1 == ncodes - (E + completion) * nc // U         # :937-940
    assert tokens.shape == (2, (c1 - c0) * epc, nc)
    assert dec.reharmonise_tokens(x, 1, 1.0, seed=5).shape == (1, (c1 - c0) * epc, nc)
    with pytest.raises(NotImplementedError, match='music21'):
        dec.generate_reharmonisation(2, 1.0, 0, 1.0)
    with pytest.raises(ValueError):
        dec.generate_from_code_long(_random_codes(dec, 1, S - 1, seed=1), temperature=1.0)
    dec.dataloader_generator = None
    with pytest.raises(ValueError, match='pad='):
        dec.generate_from_code_long(_random_codes(dec, 1, S, seed=1), temperature=1.0)


# ---- 10. training is left alone ----------------------------------------------------------------------------------------
def test_long_generation_leaves_training_unaffected(tmp_path):
    """Four training steps (two eager, two replayed from the step graph) with a long generation before the last one give
    bit-identical losses and parameters to the same steps without it."""
    g = load_golden('decoder_tiny')
    batch = {'x': T(g['batch/x'])}
    results = []
    for with_generation in (False, True):
        dec, _ = _api_decoder(tmp_path)
        pad, start = _meta_ids(dec)
        dec.enable_step_graph(True)
        dec.train()
        losses = []
        for i in range(4):
            if with_generation and i == 3:
                dec.generate_from_code_long(_random_codes(dec, 2, 8, seed=47), temperature=1.0, seed=9, pad=pad, start=start)
                assert dec.training
            losses.append(dec.train_step(batch).clone())
        assert dec._graph is not None and dec._graph.replays >= 1
        results.append((torch.stack(losses).cpu(), [p.detach().cpu().clone() for p in dec.parameters()]))
    (l0, p0), (l1, p1) = results
    assert torch.equal(l0, l1)
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
