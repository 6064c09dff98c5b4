"""`Decoder.score_tokens` / `score_chorale` (decoders/scoring.py, vqcpc_decode_score) on the tiny decoders of the generation tests
(S = 3, U = 16, T = 48), both cross blocks:
  (1) against the forced generation `generate_from_code_long(constraint=x, return_logp=True)`, captured and eager,
  (2) against a slow loop here: per code, `Decoder.forward` on that code's window (tests/score_reference.py's rule), float64 log_softmax,
  (3) `best` against that loop's float64 arg-max wherever its top-2 gap is decisive,
  (4) consistency of the details, allowed_mass against the generation's, (5) row chunking, (6) causality,
  (7) a continuous-latent and a product-embedding decoder, (8) score_chorale and the framing helper it shares with
  reharmonise_tokens, (9) the ValueErrors.
The statistic of (1), (2), (5), (6) is max |difference| / rms(forward logits) and its bound constrained_reference.TEACHER_FORCED_TOL,
the project's bound between the incremental step and the full forward: both sides are those two computations."""
import functools
import math

import numpy as np
import pytest
import torch

import constrained_reference as C
import score_reference as SR
from conftest import load_golden
from test_generate_gpu import _golden_decoder
from test_generate_long_gpu import _meta_dataset, _meta_ids, _random_codes

pytestmark = pytest.mark.gpu

NAMES = ['decoder_tiny', 'decoder_tiny_diagonal']
RANGES = [(7, 1, 7), (7, 0, 7), (7, 2, 5), (3, 0, 3)]              # (nb, code_index_start, code_index_end)
B = 2
TOL = C.TEACHER_FORCED_TOL


@functools.lru_cache(maxsize=None)
def _decoder(name):
    dec = _golden_decoder(name)[0]
    dec.eval()
    return dec


def _tokens(dec, rows, events, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randint(0, int(v), (rows, events, 1), generator=g) for v in dec.num_tokens_per_channel], dim=2).cuda()


@functools.lru_cache(maxsize=None)
def _reference(name, nb, c0, c1):
    """Computed once per case and shared: the inputs and the slow loop -- per code t of [c0, c1) ONE `Decoder.forward` on the window
    `start_end_times_ref(t)` of the scored chorale, the logits of t's events in float64.  -> dict with x, codes, pad, start, and per
    position of the range: lsm (B, events, nc) float64 log_softmax at the written token, best (float64 arg-max), gap (top-1 - top-2,
    inf for one token), vocab-wise entropy bound log V; rms over every forward logit read."""
    dec = _decoder(name)
    pad, start = _meta_ids(dec)
    S, epc, nc = dec.num_tokens_source, dec.num_events_per_code, dec.num_channels
    codes = _random_codes(dec, B, nb, seed=800 + nb + 10 * c0)
    x = _tokens(dec, B, nb * epc, seed=810 + nb + 10 * c0)
    chorale = dec.init_generation_chorale(nb * epc, c0 * epc, pad=pad, start=start).repeat(B, 1, 1)
    chorale[:, c0 * epc:c1 * epc] = x[:, c0 * epc:c1 * epc]
    n = (c1 - c0) * epc
    lsm = torch.zeros(B, n, nc, dtype=torch.float64)
    best = torch.zeros(B, n, nc, dtype=torch.int64)
    gap = torch.full((B, n, nc), float('inf'), dtype=torch.float64)
    sq, cnt = 0.0, 0
    with torch.no_grad():
        for t in range(c0, c1):
            tb, te, tr = SR.start_end_times_ref(t, nb, S)
            full = dec.forward(codes[:, tb:te], chorale[:, tb * epc:te * epc])['weights_per_category']
            for c, f in enumerate(full):
                f = f.double().cpu()
                sq, cnt = sq + float(f.pow(2).sum()), cnt + f.numel()
                lg = f[:, tr * epc:(tr + 1) * epc]                               # (B, epc, V_c)
                ev = slice((t - c0) * epc, (t - c0 + 1) * epc)
                tok = chorale[:, t * epc:(t + 1) * epc, c].cpu()
                lsm[:, ev, c] = torch.log_softmax(lg, dim=-1).gather(2, tok.unsqueeze(2)).squeeze(2)
                best[:, ev, c] = lg.argmax(dim=-1)
                if lg.shape[-1] >= 2:
                    top2 = torch.topk(lg, 2, dim=-1)[0]
                    gap[:, ev, c] = top2[..., 0] - top2[..., 1]
    return dict(x=x, codes=codes, pad=pad, start=start, chorale=chorale, lsm=lsm, best=best, gap=gap, rms=(sq / max(cnt, 1)) ** 0.5)


def _score(dec, ref, c0, c1, **kw):
    return dec.score_tokens(ref['x'], ref['codes'], code_index_start=c0, code_index_end=c1, pad=ref['pad'], start=ref['start'], **kw)


# ---- 1. the forced generation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb, c0, c1', RANGES)
@pytest.mark.parametrize('name', NAMES)
def test_logp_equals_the_forced_generation(name, nb, c0, c1):
    dec, ref = _decoder(name), _reference(name, nb, c0, c1)
    lp = _score(dec, ref, c0, c1)
    assert lp.dtype == torch.float32 and lp.is_cuda and bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())
    for use_graph in (True, False):
        tokens, want = dec.generate_from_code_long(ref['codes'], temperature=1.0, constraint=ref['x'], return_logp=True,
                                                   code_index_start=c0, code_index_end=c1, seed=3, pad=ref['pad'],
                                                   start=ref['start'], use_graph=use_graph)
        assert lp.shape == want.shape == tokens.shape
        assert torch.equal(tokens, ref['x'][:, c0 * dec.num_events_per_code:c1 * dec.num_events_per_code])
        err = float((lp.double() - want.double()).abs().max()) / ref['rms']
        print(f'{name} nb={nb} [{c0}, {c1}) graph={use_graph}: max |score - forced generation| / rms = {err:.2e}')
        assert err < TOL, (err, TOL)


# ---- 2. + 3. the slow loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb, c0, c1', RANGES)
@pytest.mark.parametrize('name', NAMES)
def test_logp_and_best_equal_the_forward_per_code_loop(name, nb, c0, c1):
    dec, ref = _decoder(name), _reference(name, nb, c0, c1)
    out = _score(dec, ref, c0, c1, return_details=True)
    err = float((out['logp'].double().cpu() - ref['lsm']).abs().max()) / ref['rms']
    print(f'{name} nb={nb} [{c0}, {c1}): max |score - log_softmax(forward on the code\'s window)| / rms = {err:.2e}')
    assert err < TOL, (err, TOL)
    decisive = ref['gap'] > 2 * TOL * ref['rms']
    left_out = 1.0 - float(decisive.double().mean())
    print(f'{name} nb={nb} [{c0}, {c1}): {left_out:.2%} of the positions have a top-2 gap within 2 x tolerance')
    assert left_out < 0.05, left_out
    assert torch.equal(out['best'].cpu()[decisive], ref['best'][decisive])


# ---- 4. the details ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_details_are_consistent_and_allowed_mass_is_the_generations(name):
    nb, c0, c1 = 7, 1, 7
    dec, ref = _decoder(name), _reference(name, nb, c0, c1)
    epc, nc = dec.num_events_per_code, dec.num_channels
    sizes = [int(v) for v in dec.num_tokens_per_channel]
    g = torch.Generator().manual_seed(820)
    allowed = torch.rand(B, nb * epc, nc, max(sizes), generator=g) < 0.5
    allowed[:, 0::3] = True                                                    # full sets at every third event
    allowed = allowed.cuda().scatter(3, ref['x'].unsqueeze(3), True)           # the written token is in its set
    out = _score(dec, ref, c0, c1, return_details=True, allowed=allowed)
    assert set(out) == {'logp', 'entropy', 'rank', 'best', 'best_logp', 'allowed_mass'}
    x = ref['x'][:, c0 * epc:c1 * epc]
    for key, dtype in (('logp', torch.float32), ('entropy', torch.float32), ('rank', torch.int32), ('best', torch.int64),
                       ('best_logp', torch.float32), ('allowed_mass', torch.float32)):
        assert out[key].shape == x.shape and out[key].dtype == dtype, key
    assert torch.equal(out['logp'], _score(dec, ref, c0, c1))                  # the details change nothing
    assert torch.equal(out['rank'] == 0, out['best'] == x)
    assert bool((out['best_logp'] >= out['logp']).all())
    assert torch.equal(out['best_logp'][out['rank'] == 0], out['logp'][out['rank'] == 0])
    for c, V in enumerate(sizes):
        assert bool((out['rank'][:, :, c] >= 0).all()) and bool((out['rank'][:, :, c] < V).all())
        assert bool((out['best'][:, :, c] >= 0).all()) and bool((out['best'][:, :, c] < V).all())
        slack = 1e-5 * (1.0 + math.log(V))                                     # far above score_reference.entropy_bound for any row
        ent = out['entropy'][:, :, c]
        assert bool((ent >= -slack).all()) and bool((ent <= math.log(V) + slack).all()), c
    _, lp, mass = dec.generate_from_code_long(ref['codes'], temperature=1.0, constraint=ref['x'], return_logp=True, allowed=allowed,
                                              return_allowed_mass=True, code_index_start=c0, code_index_end=c1, seed=3,
                                              pad=ref['pad'], start=ref['start'])
    err = float((out['allowed_mass'].double() - mass.double()).abs().max()) / ref['rms']
    print(f'{name}: max |allowed_mass - the generation\'s| / rms = {err:.2e}')
    assert err < TOL, err
    full = torch.stack([allowed[:, c0 * epc:c1 * epc, c, :V].all(-1) for c, V in enumerate(sizes)], dim=2)
    assert bool(full.any()) and bool((out['allowed_mass'][full] == 0.0).all())
    assert bool((out['allowed_mass'] <= 1e-6).all())
    shared = _score(dec, ref, c0, c1, return_details=True, allowed=allowed[0])      # one mask for every row
    assert torch.equal(shared['allowed_mass'][0], out['allowed_mass'][0])


# ---- 5. row chunking -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_window_rows_do_not_change_the_scores(name):
    nb, c0, c1 = 7, 0, 7
    dec, ref = _decoder(name), _reference(name, nb, c0, c1)
    want = _score(dec, ref, c0, c1, return_details=True, window_rows=32)
    for rows in (1, 2, 5):
        got = _score(dec, ref, c0, c1, return_details=True, window_rows=rows)
        for key in ('logp', 'entropy', 'best_logp'):
            err = float((got[key].double() - want[key].double()).abs().max()) / ref['rms']
            assert err < TOL, (rows, key, err)
        same = all(torch.equal(got[key], want[key]) for key in want)
        print(f'{name}: window_rows = {rows} against 32: bits {"equal" if same else "differ"}')


# ---- 6. causality --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_a_changed_token_moves_later_scores_only(name):
    nb, c0, c1 = 7, 1, 7
    dec, ref = _decoder(name), _reference(name, nb, c0, c1)
    epc, nc = dec.num_events_per_code, dec.num_channels
    e0, v0 = 3 * epc + 1, 2                                                    # a middle window's event, chorale coordinates
    x2 = ref['x'].clone()
    x2[:, e0, v0] = (x2[:, e0, v0] + 1) % int(dec.num_tokens_per_channel[v0])
    a = _score(dec, ref, c0, c1).reshape(B, -1).double()
    b = dec.score_tokens(x2, ref['codes'], code_index_start=c0, code_index_end=c1, pad=ref['pad'], start=ref['start'])
    b = b.reshape(B, -1).double()
    p = (e0 - c0 * epc) * nc + v0
    before = float((a[:, :p] - b[:, :p]).abs().max()) / ref['rms']
    after = float((a[:, p + 1:] - b[:, p + 1:]).abs().max()) / ref['rms']
    print(f'{name}: one changed token: scores before it move by {before:.2e} rms, after it by up to {after:.2e} rms')
    assert before < TOL and after > TOL, (before, after)


# ---- 7. other sources ----------------------------------------------------------------------------------------------------------
def _against_forced_generation(dec, codes, x, c0, c1, pad, start):
    lp = dec.score_tokens(x, codes, code_index_start=c0, code_index_end=c1, pad=pad, start=start)
    _, want = dec.generate_from_code_long(codes, temperature=1.0, constraint=x, return_logp=True, code_index_start=c0,
                                          code_index_end=c1, seed=3, pad=pad, start=start)
    epc, S = dec.num_events_per_code, dec.num_tokens_source
    with torch.no_grad():
        full = dec.forward(codes[:, :S], x[:, :S * epc])['weights_per_category']
    rms = float(torch.cat([f.reshape(-1) for f in full]).pow(2).mean().sqrt())
    return float((lp.double() - want.double()).abs().max()) / rms


def test_continuous_latents():
    from continuous_helpers import golden_continuous_decoder
    dec = golden_continuous_decoder('decoder_tiny_continuous_diagonal')[0]
    dec.eval()
    pad, start = _meta_ids(dec)
    nb = 6
    z = torch.randn(B, nb, dec.source_dim, generator=torch.Generator().manual_seed(830)).cuda()
    x = _tokens(dec, B, nb * dec.num_events_per_code, seed=831)
    err = _against_forced_generation(dec, z, x, 1, nb, pad, start)
    print(f'continuous latents: max |score - forced generation| / rms = {err:.2e}')
    assert err < TOL, err
    with pytest.raises(ValueError, match='latents'):
        dec.score_tokens(x, torch.zeros(B, nb, dtype=torch.int64), pad=pad, start=start)


def test_product_source_embedding():
    from product_codes_helpers import build_decoder, random_inputs, tiny_cfg
    cfg = tiny_cfg(4, 2)
    dec = build_decoder(cfg, 'AC-AC', 'product', seed=24)
    dec.eval()
    pad, start = _meta_ids(dec)
    nb = 7
    codes, _ = random_inputs(cfg, B, seed=832, num_codes=nb)
    x = _tokens(dec, B, nb * dec.num_events_per_code, seed=833)
    err = _against_forced_generation(dec, codes, x, 0, nb, pad, start)
    print(f'product source embedding: max |score - forced generation| / rms = {err:.2e}')
    assert err < TOL, err


# ---- 8. score_chorale and the framing it shares with reharmonise_tokens ----------------------------------------------------------
def _piece(dec, cfg):
    E = cfg['events']
    events = 2 * E + E // 2 - 1                                                # not a multiple of the window, nor of a code
    g = torch.Generator().manual_seed(840)
    return torch.cat([torch.randint(0, int(v) - 3, (1, events, 1), generator=g) for v in dec.num_tokens_per_channel], dim=2)


def test_score_chorale_equals_score_tokens_on_the_hand_framed_piece():
    dec, cfg, _ = _golden_decoder('decoder_tiny')
    dec.eval()
    vocab, E = cfg['vocab'], cfg['events']
    nc, epc, S = len(vocab), dec.num_events_per_code, dec.num_tokens_source
    dec.dataloader_generator = _meta_dataset(vocab)
    x = _piece(dec, cfg)
    n = x.shape[1]
    got = dec.score_chorale(x, return_details=True)
    row = lambda ids, k: torch.tensor(ids, dtype=torch.int64).view(1, 1, nc).repeat(1, k, 1)
    PAD, START, END = [v - 1 for v in vocab], [v - 3 for v in vocab], [v - 2 for v in vocab]
    fill = -n % E
    framed = torch.cat([row(PAD, E - 1), row(START, 1), x, row(END, 1), row(PAD, fill - 1), row(PAD, E)], dim=1)
    assert framed.shape[1] == 5 * E
    codes = dec.encode(framed.reshape(5, E, nc).cuda()).reshape(1, -1)
    c0, c1 = S, 5 * S - (E + fill) * nc // dec.total_upscaling
    want = dec.score_tokens(framed, codes, code_index_start=c0, code_index_end=c1, return_details=True)   # the dataset's PAD / START
    assert set(got) == set(want)
    for key in want:
        assert got[key].shape == (1, n, nc) and torch.equal(got[key], want[key][:, :n]), key
    plain = dec.score_chorale(x)
    assert torch.equal(plain, got['logp'])
    tokens, c0r, c1r, ncodes = dec.reharmonise_tokens(x, 1, 1.0, top_k=1, seed=5, return_bounds=True)
    assert (c0r, c1r, ncodes) == (c0, c1, 5 * S)
    mask = torch.ones(n, nc, max(vocab), dtype=torch.bool)
    mask[:, :, 0] = False
    masked = dec.score_chorale(x, allowed=mask, return_details=True, window_rows=3)
    assert bool((masked['allowed_mass'] < 0).all()) and masked['allowed_mass'].shape == (1, n, nc)
    with pytest.raises(ValueError, match='x: '):
        dec.score_chorale(x[0])
    bad = x.clone()
    bad[0, 5, 1] = vocab[1]
    with pytest.raises(ValueError, match=r'event 5, voice 1'):
        dec.score_chorale(bad)
    with pytest.raises(TypeError, match='pad'):
        dec.score_chorale(x, pad=PAD)
    dec.dataloader_generator = None
    with pytest.raises(ValueError, match='note2index_dicts'):
        dec.score_chorale(x)


def test_reharmonise_tokens_returns_what_it_returned_before_the_framing_moved():
    """tests/golden/reharmonise_tokens_tiny.npz: the piece of `_piece` through `reharmonise_tokens` BEFORE its framing block became
    `_frame_and_encode` (recorded on the MI355X from the parent commit's method): greedy, voice 0 kept, and a sampled call."""
    g = load_golden('reharmonise_tokens_tiny')
    dec, cfg, _ = _golden_decoder('decoder_tiny')
    dec.eval()
    dec.dataloader_generator = _meta_dataset(cfg['vocab'])
    x = _piece(dec, cfg)
    assert torch.equal(x, torch.from_numpy(g['x']))
    tokens, c0, c1, n = dec.reharmonise_tokens(x, 1, 1.0, top_k=1, seed=5, keep_voices=(0,), return_bounds=True)
    assert (c0, c1, n) == tuple(int(v) for v in g['bounds'])
    assert torch.equal(tokens.cpu(), torch.from_numpy(g['greedy']))
    sampled = dec.reharmonise_tokens(x, 2, 1.0, top_p=0.9, seed=5)
    assert torch.equal(sampled.cpu(), torch.from_numpy(g['sampled']))


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_value_errors():
    dec = _decoder('decoder_tiny')
    ref = _reference('decoder_tiny', 7, 1, 7)
    x, codes, pad, start = ref['x'], ref['codes'], ref['pad'], ref['start']
    epc, nc, S = dec.num_events_per_code, dec.num_channels, dec.num_tokens_source
    vmax = max(int(v) for v in dec.num_tokens_per_channel)
    was = dec.training
    cases = [
        (dict(x=x[:, :-1]), 'x: '), (dict(x=x[:1]), 'x: '), (dict(x=x.int()), 'x: '), (dict(x=x[..., :-1]), 'x: '),
        (dict(codes=codes[:, :S - 1], x=x[:, :(S - 1) * epc]), f'at least {S} codes'),
        (dict(codes=codes.float()), 'merged codes'), (dict(codes=codes.unsqueeze(2)), 'merged codes'),
        (dict(code_index_start=5, code_index_end=4), 'code_index_start'), (dict(code_index_end=8), 'code_index_start'),
        (dict(code_index_start=-1), 'code_index_start'),
        (dict(window_rows=0), 'window_rows'), (dict(window_rows=-3), 'window_rows'), (dict(window_rows=2.5), 'window_rows'),
        (dict(pad=pad[:-1]), 'pad'),
        (dict(allowed=torch.ones(B, 7 * epc, nc, vmax)), 'allowed'), (dict(allowed=torch.ones(7 * epc - 1, nc, vmax, dtype=torch.bool)), 'allowed'),
        (dict(allowed=torch.zeros(7 * epc, nc, vmax, dtype=torch.bool)), 'no allowed token'),
    ]
    for kw, match in cases:
        args = dict(x=x, codes=codes, pad=pad, start=start)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            dec.score_tokens(**args)
    bad = x.clone()
    bad[1, 2 * epc + 3, 1] = int(dec.num_tokens_per_channel[1])
    with pytest.raises(ValueError, match=rf'row 1, event {2 * epc + 3}, voice 1'):
        dec.score_tokens(bad, codes, pad=pad, start=start)
    bad[0, 0, 0] = -1                                                          # before the scored range: ignored
    with pytest.raises(ValueError, match=rf'row 1, event {2 * epc + 3}, voice 1'):
        dec.score_tokens(bad, codes, code_index_start=1, pad=pad, start=start)
    empty = dec.score_tokens(x, codes, code_index_start=4, code_index_end=4, pad=pad, start=start)
    assert empty.shape == (B, 0, nc)
    dec.train()
    try:
        a = dec.score_tokens(x, codes, pad=pad, start=start)
        assert dec.training                                                    # the previous mode is restored
    finally:
        dec.train(was)
    assert torch.equal(a, dec.score_tokens(x, codes, pad=pad, start=start))
