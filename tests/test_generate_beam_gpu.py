"""Beam search in generation (Decoder.generate_from_codes / generate_from_code_long / generate_alla_mano / reharmonise_tokens with
`beam`, `return_beams`; decoders/generation.py `_beam`, `_beam_moves`; csrc/beam.hip) on the tiny decoders of the generation tests
(S = 3, U = 16, T = 48; long form nb = 5: head, head -> middle without a slide, middle slides, tail), captured and eager:
  G1  beam = 1 is the greedy run (top_k = 1), tokens and logp bits;
  G2  everything forced: the constraint comes back, logp has the constrained run's bits, scores[:, 0] is the fp32 sum of the logp row
      in position order, bit for bit, and the other slots are dead;
  G3  three free positions with two-token sets at W = 8: the beams are exactly the eight sequences, ranked, each score within the
      derived bound of the float64 total of a forced run of that sequence;
  G4  free voices at W = 4: every returned row's logp is bit-equal to a plain run forcing the row's own tokens (the moved caches are
      the ancestor's bits), every score is the ordered fp32 sum of its row, the recorded ancestors reproduce every row's tokens;
  G5  the long form: captured == eager, chunks of whole groups == groups alone, rules with the report recomputed from the returned
      tokens, reharmonise_tokens and generate_alla_mano pass the keywords through;
  G6  the refusals, and the default path launches nothing new."""
import numpy as np
import pytest
import torch

import beam_reference as R
from test_generate_gpu import _golden_decoder, _random_inputs
from test_generate_long_gpu import _meta_dataset, _meta_ids, _random_codes
from test_generate_masked_gpu import _random_tokens
from test_generate_particles_gpu import _own_tokens_logp, _voice0
from test_generate_rules_gpu import _assert_case_one, _exclude, _exclude_bits, _rules

pytestmark = pytest.mark.gpu

NAMES = ['decoder_tiny', 'decoder_tiny_diagonal']
NB = 5
F = np.float32


def _decoder(name):
    dec = _golden_decoder(name)[0]
    dec.eval()
    return dec


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ordered_sum(lp_rows):
    """(rows, positions) fp32 -> the fp32 running sums from 0 in position order, one add per position (the kernel's score)."""
    lp = lp_rows.detach().cpu().numpy().astype(F)
    out = np.zeros(lp.shape[0], dtype=F)
    for t in range(lp.shape[1]):
        out = (out + lp[:, t]).astype(F)
    return out


def _sum_bound(lp_rows):
    """|fp32 running sum - float64 sum| of n fp32 addends <= gamma_{n-1} sum |x_i| (Higham, Accuracy and Stability, eq. 4.4)."""
    lp = lp_rows.detach().double().cpu().numpy()
    n = lp.shape[1]
    return (n - 1) * R.U_FP32 / (1.0 - (n - 1) * R.U_FP32) * np.abs(lp).sum(axis=1)


def _long_kw(dec):
    pad, start = _meta_ids(dec)
    return dict(pad=pad, start=start, code_index_start=1, code_index_end=NB)


# ---- G1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_beam_one_is_the_greedy_run(name):
    dec = _decoder(name)
    codes, _ = _random_inputs(dec, 3, seed=401)
    long_codes = _random_codes(dec, 2, NB, seed=402)
    for use_graph in (True, False):
        tok, lp = dec.generate_from_codes(codes, top_k=1, seed=3, return_logp=True, use_graph=use_graph)
        btok, blp = dec.generate_from_codes(codes, beam=1, return_logp=True, use_graph=use_graph)
        assert torch.equal(btok, tok) and torch.equal(_bits(blp), _bits(lp))
        tok, lp = dec.generate_from_code_long(long_codes, temperature=1.0, top_k=1, seed=3, return_logp=True, use_graph=use_graph,
                                              **_long_kw(dec))
        btok, blp, info = dec.generate_from_code_long(long_codes, beam=1, return_logp=True, return_beams=True, use_graph=use_graph,
                                                      **_long_kw(dec))
        assert torch.equal(btok, tok) and torch.equal(_bits(blp), _bits(lp))
        assert np.array_equal(info['scores'].cpu().numpy()[:, 0], _ordered_sum(blp.reshape(2, -1)))
        anc = info['ancestors'].cpu()
        U = dec.total_upscaling
        assert anc.shape == (NB * U, 2) and bool((anc[:U] == -1).all()) and torch.equal(anc[U:], torch.arange(2, dtype=torch.int32).expand(4 * U, -1))


# ---- G2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_everything_forced(name):
    dec = _decoder(name)
    B, W = 2, 4
    codes, given = _random_inputs(dec, B, seed=403)
    _, lp0 = dec.generate_from_codes(codes, constraint=given, return_logp=True, seed=1)
    for use_graph in (True, False):
        tok, lp, info = dec.generate_from_codes(codes, constraint=given, beam=W, return_logp=True, return_beams=True, use_graph=use_graph)
        assert torch.equal(tok, given.repeat_interleave(W, dim=0))
        assert torch.equal(_bits(lp), _bits(lp0.repeat_interleave(W, dim=0)))
        sc = info['scores'].cpu().numpy()
        assert sc.shape == (B, W) and np.array_equal(sc[:, 0], _ordered_sum(lp0.reshape(B, -1)))
        assert np.all(sc[:, 1:] == -np.inf)
        best, blp = dec.generate_from_codes(codes, constraint=given, beam=W, return_logp=True, use_graph=use_graph)
        assert torch.equal(best, given) and torch.equal(_bits(blp), _bits(lp0))


# ---- G3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_three_free_positions_are_searched_exhaustively(name):
    dec = _decoder(name)
    B, W = 2, 8
    E, nc, vmax = dec.num_tokens_target // dec.num_channels, dec.num_channels, max(dec.num_tokens_per_channel)
    codes, given = _random_inputs(dec, B, seed=404)
    free = [(2, 1), (5, 0), (9, 3)]
    cons = given.clone()
    allowed = torch.ones(B, E, nc, vmax, dtype=torch.bool)
    pairs = {}
    for (e, c) in free:
        cons[:, e, c] = -1
        allowed[:, e, c] = False
        for b in range(B):
            a = int(given[b, e, c])
            pairs[b, e, c] = sorted((a, (a + 1 + b) % int(dec.num_tokens_per_channel[c])))
            allowed[b, e, c, pairs[b, e, c]] = True
    for use_graph in (True, False):
        tok, info = dec.generate_from_codes(codes, constraint=cons, allowed=allowed, beam=W, return_beams=True, use_graph=use_graph)
        sc = info['scores'].cpu().numpy()
        _, lp = dec.generate_from_codes(codes.repeat_interleave(W, dim=0), constraint=tok, return_logp=True, seed=0)
        total = lp.double().reshape(B * W, -1).sum(dim=1).cpu().numpy().reshape(B, W)
        bound = _sum_bound(lp.reshape(B * W, -1)).reshape(B, W)
        for b in range(B):
            want = {tuple(x) for x in np.array(np.meshgrid(*[pairs[b, e, c] for (e, c) in free], indexing='ij')).reshape(3, -1).T.tolist()}
            got = [tuple(int(tok[b * W + k, e, c]) for (e, c) in free) for k in range(W)]
            assert set(got) == want and len(set(got)) == 8, (b, got)
            rest = torch.ones(E, nc, dtype=torch.bool, device=tok.device)
            for (e, c) in free:
                rest[e, c] = False
            assert all(torch.equal(tok[b * W + k][rest], given[b][rest]) for k in range(W))
            assert np.all(np.isfinite(sc[b])) and np.all(np.abs(sc[b] - total[b]) <= bound[b]), (b, sc[b], total[b], bound[b])
            for k in range(W - 1):                                          # every adjacent pair: non-increasing, ties by token order
                assert sc[b, k] >= sc[b, k + 1], (b, k)
            assert total[b, 0] >= total[b].max() - 2 * bound[b].max(), (b, total[b])
        worst = float((np.abs(sc - total) / bound).max())
        print(f'{name} (graph {use_graph}): |score - float64 total| / bound, worst {worst:.3f}')


# ---- G4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_moved_rows_carry_their_ancestors_bits(name):
    dec = _decoder(name)
    B, W = 2, 4
    codes, given = _random_inputs(dec, B, seed=405)
    cons = _voice0(given)
    runs = {}
    for use_graph in (True, False):
        tok, lp, info = dec.generate_from_codes(codes, constraint=cons, beam=W, return_logp=True, return_beams=True, use_graph=use_graph)
        runs[use_graph] = (tok, lp, info['scores'], info['ancestors'])
        assert torch.equal(tok[:, :, 0], given.repeat_interleave(W, dim=0)[:, :, 0])
        own = _own_tokens_logp(dec, codes.repeat_interleave(W, dim=0), tok)
        assert torch.equal(_bits(lp), _bits(own))
        sc = info['scores'].cpu().numpy()
        assert np.array_equal(sc.reshape(-1), _ordered_sum(lp.reshape(B * W, -1))) and np.all(np.isfinite(sc))
        assert np.all(sc[:, :-1] >= sc[:, 1:])
        assert len({tuple(r.reshape(-1).tolist()) for r in tok[:W]}) == W              # four different hypotheses
        anc = info['ancestors'].cpu().numpy()
        moved = int((anc != np.arange(B * W)).sum())
        print(f'{name} (graph {use_graph}): {moved} of {anc.size} slots descend from another row')
        assert moved > 0 and anc.min() >= 0
        assert np.array_equal(anc // W, np.broadcast_to(np.arange(B * W) // W, anc.shape))          # inside the group
        best, blp = dec.generate_from_codes(codes, constraint=cons, beam=W, return_logp=True, use_graph=use_graph)
        assert torch.equal(best, tok[::W]) and torch.equal(_bits(blp), _bits(lp[::W]))
    for a, b in zip(runs[True], runs[False]):
        assert torch.equal(a, b)


def test_the_recorded_ancestors_reproduce_every_rows_tokens():
    """The stack itself, step by step, so that the token every slot emitted at every position is visible."""
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    dec = _decoder(NAMES[0])
    B, W = 2, 4
    codes, given = _random_inputs(dec, B, seed=406)
    cons = _voice0(given).reshape(B, -1).repeat_interleave(W, dim=0)
    outs = {}
    for in_step in (True, False):
        with STEP_LOCK, torch.no_grad():
            inc = IncrementalDecoder(dec, B * W)
            inc.beam_moves_in_step = in_step
            inc.prefill(codes.repeat_interleave(W, dim=0))
            inc.start(constraint=cons, want_logp=True, beam=W)
            by_pos = []
            for t in range(inc.T):
                inc.step()
                by_pos.append(inc.tokens[:, t].cpu().numpy().copy())         # the live column is in slot order and does not move
                inc._code_done(t + 1)
            torch.cuda.synchronize()
            hist = inc.b_hist.cpu().numpy()
            outs[in_step] = (inc.tokens.cpu().clone(), inc.logp.cpu().clone(), inc.b_score.cpu().clone(), hist)
        assert np.array_equal(R.follow_ancestors(np.array(by_pos), hist), outs[in_step][0].numpy())
    for a, b in zip(outs[True], outs[False]):                               # both placements of the moves: the same bits
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))


# ---- G5 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_long_form_captured_equals_eager_and_rows_carry_their_bits(name):
    dec = _decoder(name)
    B, W, epc = 2, 4, dec.num_events_per_code
    codes = _random_codes(dec, B, NB, seed=407)
    given = _random_tokens(dec, B, NB * epc, seed=408, reserve=3)
    cons = _voice0(given)
    long_kw = dict(temperature=1.0, **_long_kw(dec))
    runs = {}
    for use_graph in (True, False):
        tok, lp, info = dec.generate_from_code_long(codes, constraint=cons, beam=W, return_logp=True, return_beams=True,
                                                    use_graph=use_graph, **long_kw)
        runs[use_graph] = (tok, lp, info['scores'], info['ancestors'])
        assert torch.equal(tok[:, :, 0], given[:, epc:].repeat_interleave(W, dim=0)[:, :, 0])
        own = _own_tokens_logp(dec, codes.repeat_interleave(W, dim=0), tok, long_kw)
        assert torch.equal(_bits(lp), _bits(own))
        sc = info['scores'].cpu().numpy()
        assert np.array_equal(sc.reshape(-1), _ordered_sum(lp.reshape(B * W, -1))) and np.all(sc[:, :-1] >= sc[:, 1:])
        anc = info['ancestors'].cpu().numpy()
        U = dec.total_upscaling
        assert anc.shape == (NB * U, B * W) and np.all(anc[:U] == -1) and anc[U:].min() >= 0
        assert int((anc[U:] != np.arange(B * W)).sum()) > 0
    for a, b in zip(runs[True], runs[False]):
        assert torch.equal(a, b)


def test_chunks_of_whole_groups_equal_the_groups_alone():
    """B * W = 72 > 64 rows with W = 24: chunks of 48 and 24 rows, in the long form."""
    dec = _decoder(NAMES[0])
    B, W, epc = 3, 24, dec.num_events_per_code
    codes = _random_codes(dec, B, NB, seed=409)
    cons = _voice0(_random_tokens(dec, B, NB * epc, seed=410, reserve=3))
    kw = dict(beam=W, return_logp=True, return_beams=True, **_long_kw(dec))
    tok, lp, info = dec.generate_from_code_long(codes, constraint=cons, **kw)
    assert tok.shape[0] == B * W and info['scores'].shape == (B, W) and info['ancestors'].shape[1] == B * W
    for g in range(B):
        sl = slice(g * W, (g + 1) * W)
        t1, l1, i1 = dec.generate_from_code_long(codes[g:g + 1], constraint=cons[g:g + 1], **kw)
        assert torch.equal(tok[sl], t1) and torch.equal(_bits(lp[sl]), _bits(l1)), g
        assert torch.equal(_bits(info['scores'][g]), _bits(i1['scores'][0])), g
        a = i1['ancestors']
        assert torch.equal(info['ancestors'][:, sl], torch.where(a >= 0, a + g * W, a)), g


@pytest.mark.parametrize('name', NAMES)
def test_rules_and_the_report_move_with_the_hypotheses(name):
    dec = _decoder(name)
    rules, kinds = _rules(dec)
    B, W, epc = 2, 4, dec.num_events_per_code
    dec.dataloader_generator = _meta_dataset([int(v) for v in dec.num_tokens_per_channel])
    codes = _random_codes(dec, B, NB, seed=411)
    kw = dict(rules=rules, return_rule_report=True, return_allowed_mass=True, exclude_meta_symbols=True, beam=W, return_beams=True)
    outs = {}
    for use_graph in (True, False):
        tok, mass, rep, info = dec.generate_from_code_long(codes, use_graph=use_graph, **kw, **_long_kw(dec))
        outs[use_graph] = (tok, mass, rep, info['scores'])
        # the report of every returned row is the reference's for the row's own tokens: the history before the first generated
        # event is the PAD / START frame, which has no pitch
        frame = dec.init_generation_chorale(NB * epc, epc).expand(B * W, -1, -1).clone()
        frame[:, epc:] = tok
        whole = torch.full((B * W, NB * epc, dec.num_channels), -1, dtype=torch.int32)
        whole[:, epc:] = rep.cpu()
        _assert_case_one(dec, kinds, rules, frame, whole, None, None, _exclude_bits(dec), first=epc * dec.num_channels)
        assert bool((mass <= 0).all()) and bool(torch.isfinite(info['scores'][:, 0]).all())
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)
    tok, rep = dec.generate_from_codes(codes[:, :dec.num_tokens_source], rules=rules, return_rule_report=True, beam=W,
                                       exclude_tokens=_exclude(dec))
    _assert_case_one(dec, kinds, rules, tok, rep, None, None, _exclude_bits(dec))


def test_reharmonise_tokens_and_alla_mano_pass_the_keywords_through():
    dec, cfg, _ = _golden_decoder(NAMES[0])
    dec.eval()
    vocab, E = cfg['vocab'], cfg['events']
    dec.dataloader_generator = _meta_dataset(vocab)
    events = E + E // 2 - 1
    x = _random_tokens(dec, 1, events, seed=412, reserve=3).cpu()
    out = dec.reharmonise_tokens(x, 1, 1.0, keep_voices=(0,), beam=4)
    assert out.shape[0] == 1 and torch.equal(out[:, :events, 0].cpu(), x[:, :, 0])
    (tok, lp, info), c0, c1, n = dec.reharmonise_tokens(x, 1, 1.0, keep_voices=(0,), beam=4, return_beams=True, return_logp=True,
                                                        return_bounds=True)
    U = dec.total_upscaling
    assert tok.shape[0] == 4 and torch.equal(tok[:1], out) and info['scores'].shape == (1, 4)
    assert info['ancestors'].shape == (n * U, 4) and bool((info['ancestors'][c0 * U:c1 * U] >= 0).all())
    assert bool((info['ancestors'][:c0 * U] == -1).all())
    assert np.array_equal(info['scores'].cpu().numpy().reshape(-1), _ordered_sum(lp.reshape(4, -1)))
    pad, start = _meta_ids(dec)
    body = dec.generate_alla_mano([0, 1], [2], [3, 0, 1], num_decodings=1, beam=3, return_beams=True, pad=pad, start=start)
    assert body[0].shape[0] == 3 and body[1]['scores'].shape == (1, 3)
    one = dec.generate_alla_mano([0, 1], [2], [3, 0, 1], num_decodings=1, beam=3, pad=pad, start=start)
    assert torch.equal(one, body[0][:1])
    with pytest.raises(ValueError, match='num_decodings'):
        dec.generate_alla_mano([0, 1], [2], [3, 0, 1], beam=3, pad=pad, start=start)       # the default num_decodings is 3


# ---- G6 -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    dec = _decoder(NAMES[0])
    pad, start = _meta_ids(dec)
    codes, _ = _random_inputs(dec, 2, seed=413)
    long_codes = _random_codes(dec, 2, NB, seed=414)
    calls = (lambda **k: dec.generate_from_codes(codes, **k), lambda **k: dec.generate_from_code_long(long_codes, pad=pad, start=start, **k))
    for fn in calls:
        for W in (0, 65, -1, 2.5, True):
            with pytest.raises(ValueError, match='beam'):
                fn(beam=W)
        for kw, word in ((dict(particles=2), 'particles'), (dict(return_attentions=True), 'return_attentions'),
                         (dict(num_decodings=2), 'num_decodings'), (dict(temperature=0.7), 'temperature'), (dict(top_k=3), 'top_k'),
                         (dict(top_p=0.9), 'top_p')):
            with pytest.raises(ValueError, match=word):
                fn(beam=2, **kw)
        with pytest.raises(ValueError, match='return_beams'):
            fn(return_beams=True, temperature=1.0)
        assert fn(beam=2, seed=5, top_p=0.0).shape[0] == 2                       # seed accepted and unused; top_p <= 0 is no filter


@pytest.mark.parametrize('name', NAMES)
def test_the_default_path_launches_nothing_new(monkeypatch, name):
    from vqcpc_bach_amd import hip
    dec = _decoder(name)
    codes, _ = _random_inputs(dec, 2, seed=415)
    long_codes = _random_codes(dec, 2, NB, seed=416)
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
        return list(names)
    for use_graph in (True, False):
        plain = launches(lambda: dec.generate_from_codes(codes, seed=1, use_graph=use_graph))
        assert not [n for n in plain if 'beam' in n or 'permute' in n]
        beam = launches(lambda: dec.generate_from_codes(codes, beam=2, use_graph=use_graph))
        assert [n for n in beam if 'beam' not in n and 'permute' not in n] == [n for n in plain if n != 'vqcpc_decode_sample']
        plain = launches(lambda: dec.generate_from_code_long(long_codes, temperature=1.0, seed=1, use_graph=use_graph, **_long_kw(dec)))
        assert not [n for n in plain if 'beam' in n or 'permute' in n]
