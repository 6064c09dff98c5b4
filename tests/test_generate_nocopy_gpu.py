"""The copy guard in generation (`no_copy=`, `return_copy_report=` of Decoder.generate_from_codes / generate_from_code_long /
reharmonise_tokens / generate, `Decoder.copy_index`, `Decoder.audit_copies`; decoders/generation.py `_copy_guard`; csrc/nocopy.hip) on
the tiny decoders of the generation tests (vocabularies 11..14, S = 3, U = 16, T = 48; long form nb = 5):
  (a) a memorised corpus -- the model's own greedy generations, plus random pieces: without the keyword the greedy generation IS a
      piece (the longest run is all 48 tokens), with no_copy (n = 6) every row shares at most n, no position is flagged and
      position n bans the corpus's next token;
  (b) the returned report is the reference's (tests/nocopy_reference.py), recomputed from the returned tokens, and every free token
      lies in the reference's final set;
  (c) captured == eager, chunks == whole, a row == the row alone;
  (d) the long form with n > U: contexts reach the committed chorale across a slide;
  (e) with rules the final set is the rules' set minus the ban; with particles (thresholds 0 and 1) and a beam the report is
      recomputed from every returned row;
  (f) reharmonise_tokens on a corpus piece with the soprano kept: the report is the reference's, FORCED_COPY included;
  (g) the refusals."""
import types

import numpy as np
import pytest
import torch

import nocopy_reference as N
from test_generate_gpu import _golden_decoder, _random_inputs
from test_generate_long_gpu import _meta_dataset, _meta_ids, _random_codes

pytestmark = pytest.mark.gpu

NAMES = ['decoder_tiny', 'decoder_tiny_diagonal']
NB = 5
NMAX = 6


def _decoder(name):
    dec = _golden_decoder(name)[0]
    dec.eval()
    return dec


def _vocab(dec):
    return [int(v) for v in dec.num_tokens_per_channel]


def _random_pieces(dec, ticks, seed, reserve=0):
    rng = np.random.RandomState(seed)
    return [np.stack([rng.randint(0, v - reserve, size=t) for v in _vocab(dec)], axis=1).astype(np.int64) for t in ticks]


def _device_corpus(dec, pieces, subdivision=1):
    from vqcpc_bach_amd.dataloaders.corpus import Corpus, DeviceCorpus
    tokens = np.concatenate(pieces, axis=0).astype(np.int32)
    start = np.concatenate([[0], np.cumsum([p.shape[0] for p in pieces])])
    zero = np.zeros(4, dtype=np.int64)
    return DeviceCorpus(Corpus(tokens, start, subdivision, _vocab(dec), zero, zero, zero), 'cuda')


def _memorised(dec, codes, seed, **kw):
    """(the greedy generations, the pieces: them plus random ones, the device corpus)."""
    greedy = dec.generate_from_codes(codes, temperature=1.0, top_k=1, seed=1, **kw)
    pieces = [g for g in greedy.cpu().numpy()] + _random_pieces(dec, [7, 30, 12], seed)
    return greedy, pieces, _device_corpus(dec, pieces)


def _recompute(dec, n, pieces, tokens, cons=None, static=None, exclude=None, first=0):
    rows = tokens.shape[0]
    tok = tokens.reshape(rows, -1).cpu().numpy()
    con = None if cons is None else cons.reshape(rows, -1).cpu().numpy()
    out = [N.row_report(tok[b], n, pieces, _vocab(dec), None if con is None else con[b], None if static is None else static[b],
                        exclude, first) for b in range(rows)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _assert_report(dec, n, pieces, tokens, report, cons=None, static=None, exclude=None, first=0):
    """(b): the report is the reference's and every free token lies in the final set.  -> the report as an array."""
    rows = tokens.shape[0]
    sets, want = _recompute(dec, n, pieces, tokens, cons, static, exclude, first)
    got = report.reshape(rows, -1).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got[:, first:], want[:, first:]), np.argwhere(got != want)[:5]
    tok = tokens.reshape(rows, -1).cpu().numpy()
    free = np.ones_like(tok, dtype=bool) if cons is None else cons.reshape(rows, -1).cpu().numpy() < 0
    free[:, :first] = False
    for b, col in np.argwhere(free):
        assert sets[b, col, tok[b, col]], (b, col)
    return got


def _lengths(dc, tokens, pieces=None):
    return dc.longest_common_run(tokens, pieces=pieces)['length']


# ---- (a), (b) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_a_memorised_corpus_is_not_recited(name):
    dec = _decoder(name)
    B, n, nc = 4, NMAX, dec.num_channels
    codes, _ = _random_inputs(dec, B, seed=511)
    greedy, pieces, dc = _memorised(dec, codes, seed=512)
    ix = dc.copy_index(n)
    assert _lengths(dc, greedy).tolist() == [dec.num_tokens_target] * B          # without the keyword: the whole generation
    again = dec.generate_from_codes(codes, temperature=1.0, top_k=1, seed=1)
    assert torch.equal(again, greedy)
    tokens, report = dec.generate_from_codes(codes, temperature=1.0, top_k=1, seed=1, no_copy=ix, return_copy_report=True)
    assert tokens.shape == greedy.shape and report.shape == tokens.shape and report.dtype == torch.int32
    lengths = _lengths(dc, tokens)
    rep = _assert_report(dec, n, pieces, tokens, report)
    print(f'{name}: longest runs with no_copy {lengths.tolist()}, banned tokens per row {(rep & 0x1FF).sum(axis=1).tolist()}')
    assert bool((lengths <= n).all())
    assert bool((rep >= 0).all()) and bool((rep < N.RELAXED).all())              # no position is flagged: no excuse
    assert bool((rep[:, n] >= 1).all()) and bool((rep[:, :n] == 0).all())        # position n bans the corpus's next token
    assert torch.equal(tokens.reshape(B, -1)[:, :n], greedy.reshape(B, -1)[:, :n])
    assert bool((tokens.reshape(B, -1)[:, n] != greedy.reshape(B, -1)[:, n]).all())
    # the audit: a copy map of the recited rows, nothing on the guarded ones
    audit = dec.audit_copies(torch.cat([greedy, tokens]), ix)
    assert audit.shape == (2 * B,) + tuple(greedy.shape[1:]) and audit.dtype == torch.int32
    want = np.stack([N.audit(t, n, pieces) for t in torch.cat([greedy, tokens]).reshape(2 * B, -1).cpu().numpy()])
    assert np.array_equal(audit.reshape(2 * B, -1).cpu().numpy(), want)
    assert bool((audit[:B].reshape(B, -1)[:, n:] == N.FORCED_COPY).all()) and bool((audit[B:] == 0).all())
    # a sampled run with a constraint and sets: forced and free positions, the same recomputation
    cons = torch.full_like(greedy, -1)
    cons[:, 2::3, 1] = greedy[:, 2::3, 1]
    allowed = torch.rand(B, greedy.shape[1], nc, max(_vocab(dec)), generator=torch.Generator().manual_seed(513)) < 0.6
    allowed.scatter_(3, greedy.cpu().unsqueeze(3), True)
    out = dec.generate_from_codes(codes, temperature=0.7, seed=3, constraint=cons, allowed=allowed, no_copy=ix, return_logp=True,
                                  return_allowed_mass=True, return_copy_report=True)
    assert len(out) == 4 and torch.equal(out[0][cons >= 0], cons[cons >= 0])
    static = np.zeros((B, dec.num_tokens_target, 256), dtype=bool)
    static[:, :, :allowed.shape[3]] = allowed.numpy().reshape(B, dec.num_tokens_target, -1)
    rep = _assert_report(dec, n, pieces, out[0], out[3], cons=cons, static=static)
    assert bool(torch.isfinite(out[2]).all()) and bool((out[2] <= 0).all())
    assert bool((_lengths(dc, out[0])[~((rep & (N.RELAXED | N.FORCED_COPY)) != 0).any(axis=1)] <= n).all())


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
def test_captured_equals_eager_chunks_equal_whole_and_a_row_equals_the_row_alone():
    from vqcpc_bach_amd.transformer.incremental import row_seeds
    dec = _decoder(NAMES[0])
    B, n = 33, NMAX
    codes, _ = _random_inputs(dec, B, seed=521)
    _, pieces, dc = _memorised(dec, codes[:8], seed=522)
    ix = dc.copy_index(n)
    seeds = row_seeds(17, 2 * B)
    kw = dict(temperature=1.0, top_k=1, no_copy=ix, return_logp=True, return_allowed_mass=True, return_copy_report=True)
    whole = dec.generate_from_codes(codes, num_decodings=2, seed=seeds, **kw)                # 66 rows: two chunks
    assert whole[0].shape[0] == 2 * B and bool((whole[3] >= 0).all()) and bool(((whole[3][:16] & 0x1FF) > 0).any())
    same = lambda a, b: all(torch.equal(x.view(torch.int32) if x.is_floating_point() else x, y.view(torch.int32)
                                        if y.is_floating_point() else y) for x, y in zip(a, b))
    tail = dec.generate_from_codes(codes[31:], num_decodings=2, seed=seeds[62:], **kw)
    assert same(tail, [w[62:] for w in whole])
    one = dec.generate_from_codes(codes[3:4], seed=seeds[7:8], **kw)
    assert same(one, [w[7:8] for w in whole])
    eager = dec.generate_from_codes(codes[:4], num_decodings=2, seed=seeds[:8], use_graph=False, **kw)
    assert same(eager, [w[:8] for w in whole])
    _assert_report(dec, n, pieces, whole[0][:16], whole[3][:16])
    assert bool((_lengths(dc, whole[0][:16]) <= n).all())


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_long_form_contexts_reach_the_committed_chorale_across_a_slide(name):
    dec = _decoder(name)
    dec.dataloader_generator = _meta_dataset(_vocab(dec))
    pad, start = _meta_ids(dec)
    B, nc, U = 2, dec.num_channels, dec.total_upscaling
    n = U + 4                                                           # longer than a code: every context spans a slide
    codes = _random_codes(dec, B, NB, seed=531)
    kw = dict(temperature=1.0, top_k=1, seed=2, pad=pad, start=start, code_index_start=0, exclude_meta_symbols=True)
    greedy = dec.generate_from_code_long(codes, **kw)
    assert greedy.shape == (B, NB * U // nc, nc)
    pieces = [g for g in greedy.cpu().numpy()] + _random_pieces(dec, [9, 40], seed=532, reserve=3)
    dc = _device_corpus(dec, pieces)
    ix = dc.copy_index(n)
    assert _lengths(dc, greedy).tolist() == [NB * U] * B
    tokens, report = dec.generate_from_code_long(codes, no_copy=ix, return_copy_report=True, **kw)
    excl = np.zeros((nc, 256), dtype=bool)
    for c, v in enumerate(_vocab(dec)):
        excl[c, v - 3:v] = True
    rep = _assert_report(dec, n, pieces, tokens, report, exclude=excl)
    lengths = _lengths(dc, tokens)
    print(f'{name}: long form, n = {n}: longest runs {lengths.tolist()}, positions with a ban {(rep > 0).sum(axis=1).tolist()}')
    assert bool((rep < N.RELAXED).all()) and bool((lengths <= n).all()) and bool((rep[:, n] >= 1).all())
    # the first three codes forced to the piece, n2 = 2 U + 4: column 3 U is the first one of code 3, whose window begins at
    # column 2 U, so its context [U - 4, 3 U) reaches 12 + U columns down into the committed chorale -- and bans the piece's token
    n2, first_free = 2 * U + 4, 3 * U
    cons = torch.full_like(greedy, -1)
    cons[:, :first_free // nc] = greedy[:, :first_free // nc]
    tokens2, report2 = dec.generate_from_code_long(codes, constraint=cons, no_copy=dc.copy_index(n2), return_copy_report=True, **kw)
    rep2 = _assert_report(dec, n2, pieces, tokens2, report2, cons=cons, exclude=excl)
    assert bool((rep2[:, n2:first_free] == N.FORCED_COPY).all()) and bool((rep2[:, :n2] == 0).all())
    assert bool((rep2[:, first_free] >= 1).all()) and bool((rep2[:, first_free:] < N.RELAXED).all())
    assert bool((tokens2.reshape(B, -1)[:, first_free] != greedy.reshape(B, -1)[:, first_free]).all())
    for graph in (dict(use_graph=False), dict(use_graph=True, graph_slides=False)):
        again = dec.generate_from_code_long(codes, no_copy=ix, return_copy_report=True, **kw, **graph)
        assert torch.equal(again[0], tokens) and torch.equal(again[1], report)
    # a generation that starts after a PAD / START frame: the frame is history like any token
    kw1 = dict(kw, code_index_start=1)
    tokens1, report1 = dec.generate_from_code_long(codes, no_copy=dc.copy_index(NMAX), return_copy_report=True, **kw1)
    epc = U // nc
    frame = torch.tensor(pad, dtype=torch.int64).view(1, 1, nc).repeat(B, epc, 1)
    frame[:, epc - 1] = torch.tensor(start, dtype=torch.int64)
    full = torch.cat([frame.cuda(), tokens1], dim=1)
    full_report = torch.cat([torch.full((B, epc, nc), -1, dtype=torch.int32).cuda(), report1], dim=1)
    _assert_report(dec, NMAX, pieces, full, full_report, exclude=excl, first=U)
    assert bool((_lengths(dc, tokens1) <= NMAX).all())


# ---- (e) ----------------------------------------------------------------------------------------------------------------------
def test_with_rules_the_final_set_is_the_rules_set_minus_the_ban():
    import rules_reference as R
    from test_generate_rules_gpu import _exclude, _exclude_bits, _rules
    dec = _decoder(NAMES[0])
    rules, kinds = _rules(dec)
    B, n = 4, NMAX
    codes, _ = _random_inputs(dec, B, seed=541)
    kw = dict(temperature=1.0, top_k=1, seed=4, exclude_tokens=_exclude(dec), rules=rules)
    greedy = dec.generate_from_codes(codes, **kw)
    pieces = [g for g in greedy.cpu().numpy()] + _random_pieces(dec, [20], seed=542)
    dc = _device_corpus(dec, pieces)
    ix = dc.copy_index(n)
    assert _lengths(dc, greedy).tolist() == [dec.num_tokens_target] * B
    tokens, mass, rule_report, copy_report = dec.generate_from_codes(codes, no_copy=ix, return_allowed_mass=True, return_rule_report=True,
                                                                     return_copy_report=True, **kw)
    excl = _exclude_bits(dec)
    tok = tokens.reshape(B, -1).cpu().numpy()
    rule_sets = []
    for b in range(B):
        s, r = R.row_report(tok[b], dec.num_channels, kinds, _vocab(dec), rules.max_leap.tolist(), rules.mask, None, None, excl)
        assert np.array_equal(rule_report.reshape(B, -1)[b].cpu().numpy(), r)
        rule_sets.append(s)
    rep = _assert_report(dec, n, pieces, tokens, copy_report, static=np.stack(rule_sets), exclude=excl)
    assert bool(((rep & 0x1FF) > 0).any()) and bool((mass < 0).any())
    assert bool((_lengths(dc, tokens)[(rep < N.RELAXED).all(axis=1)] <= n).all())


@pytest.mark.parametrize('name', NAMES)
def test_particles_and_the_beam_move_the_report_with_its_row(name):
    dec = _decoder(name)
    B, P, n, nc = 2, 4, NMAX, dec.num_channels
    codes, _ = _random_inputs(dec, B, seed=551)
    greedy, pieces, dc = _memorised(dec, codes, seed=552)
    ix = dc.copy_index(n)
    cons = torch.full_like(greedy, -1)
    cons[:, :, 3] = greedy[:, :, 3]                                     # the corpus's own bass: continuing by copying costs weight
    kw = dict(temperature=1.0, seed=29, constraint=cons, no_copy=ix, return_logp=True, return_allowed_mass=True,
              return_copy_report=True)
    plain = dec.generate_from_codes(codes, num_decodings=P, **kw)
    still = dec.generate_from_codes(codes, particles=P, resample_threshold=0.0, return_particles=True, **kw)
    for a, b in zip(plain, still[:4]):
        assert torch.equal(a.view(torch.int32) if a.is_floating_point() else a, b.view(torch.int32) if b.is_floating_point() else b)
    consP = cons.repeat_interleave(P, dim=0)
    _assert_report(dec, n, pieces, plain[0], plain[3], cons=consP)
    for use_graph in (True, False):
        tok, lp, mass, report, info = dec.generate_from_codes(codes, particles=P, resample_threshold=1.0, return_particles=True,
                                                              use_graph=use_graph, **kw)
        moved = int((info['ancestors'].cpu() != torch.arange(B * P, dtype=torch.int32)).sum())
        print(f'{name} (graph {use_graph}): {moved} row moves')
        assert moved > 0
        _assert_report(dec, n, pieces, tok, report, cons=consP)
    first = dec.generate_from_codes(codes, particles=P, resample_threshold=1.0, **kw)
    assert first[0].shape == greedy.shape
    _assert_report(dec, n, pieces, first[0], first[3], cons=cons)
    # the beam: all W hypotheses, in slot order, each with its own report; free search first, then around the kept bass
    for extra in (dict(), dict(constraint=cons)):
        for in_step in (True, False):
            from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
            IncrementalDecoder.beam_moves_in_step = in_step
            try:
                tok, report, info = dec.generate_from_codes(codes, beam=P, return_beams=True, no_copy=ix, return_copy_report=True, **extra)
            finally:
                IncrementalDecoder.beam_moves_in_step = True
            assert tok.shape[0] == B * P
            rep = _assert_report(dec, n, pieces, tok, report, cons=consP if extra else None)
            assert bool(((rep & 0x1FF) > 0).any())
            if not extra:
                assert bool((_lengths(dc, tok)[(rep < N.RELAXED).all(axis=1)] <= n).all())
    best, report = dec.generate_from_codes(codes, beam=P, no_copy=ix, return_copy_report=True)
    assert best.shape == greedy.shape and bool((_lengths(dc, best) <= n).all())
    # long form: the chorale rows and the report rows move together
    dec.dataloader_generator = _meta_dataset(_vocab(dec))
    pad, start = _meta_ids(dec)
    long_codes = _random_codes(dec, 1, NB, seed=553)
    lkw = dict(temperature=1.0, pad=pad, start=start, code_index_start=0, exclude_meta_symbols=True)
    lgreedy = dec.generate_from_code_long(long_codes, top_k=1, seed=2, **lkw)
    lpieces = [lgreedy[0].cpu().numpy()] + _random_pieces(dec, [15], seed=554)
    lix = _device_corpus(dec, lpieces).copy_index(n)
    lcons = torch.full_like(lgreedy, -1)
    lcons[:, :, 3] = lgreedy[:, :, 3]
    excl = np.zeros((nc, 256), dtype=bool)
    for c, v in enumerate(_vocab(dec)):
        excl[c, v - 3:v] = True
    tok, report, info = dec.generate_from_code_long(long_codes, seed=31, constraint=lcons, no_copy=lix, particles=P,
                                                    resample_threshold=1.0, return_particles=True, return_copy_report=True, **lkw)
    _assert_report(dec, n, lpieces, tok, report, cons=lcons.repeat_interleave(P, dim=0), exclude=excl)
    tok, report, info = dec.generate_from_code_long(long_codes, constraint=lcons, no_copy=lix, beam=P, return_beams=True,
                                                    return_copy_report=True, **lkw)
    _assert_report(dec, n, lpieces, tok, report, cons=lcons.repeat_interleave(P, dim=0), exclude=excl)


# ---- (f) ----------------------------------------------------------------------------------------------------------------------
def test_reharmonise_tokens_on_a_corpus_piece_reports_what_the_reference_says():
    dec, cfg, _ = _golden_decoder(NAMES[0])
    dec.eval()
    dec.dataloader_generator = _meta_dataset(cfg['vocab'])
    pad, start = _meta_ids(dec)
    n, nc, U = NMAX, dec.num_channels, dec.total_upscaling
    events = cfg['events'] + cfg['events'] // 2 - 1
    pieces = _random_pieces(dec, [events, 22], seed=561, reserve=3)
    ix = _device_corpus(dec, pieces).copy_index(n)
    x = torch.from_numpy(pieces[0]).unsqueeze(0)
    kw = dict(temperature=1.0, seed=5, keep_voices=(0,), exclude_meta_symbols=True)
    (out, report), cs, ce, nb = dec.reharmonise_tokens(x, 3, no_copy=ix, return_copy_report=True, return_bounds=True, **kw)
    assert out.shape == report.shape and out.shape[0] == 3 and report.dtype == torch.int32
    assert torch.equal(out[:, :events, 0].cpu(), x[:, :, 0].expand(3, -1))
    epc = U // nc
    frame = torch.tensor(pad, dtype=torch.int64).view(1, 1, nc).repeat(3, cs * epc, 1)
    frame[:, cs * epc - 1] = torch.tensor(start, dtype=torch.int64)
    full = torch.cat([frame.cuda(), out], dim=1)
    cons = torch.full_like(full, -1)
    cons[:, cs * epc:cs * epc + events, 0] = x[0, :, 0].cuda()
    full_report = torch.cat([torch.full(tuple(frame.shape), -1, dtype=torch.int32).cuda(), report], dim=1)
    excl = np.zeros((nc, 256), dtype=bool)
    for c, v in enumerate(_vocab(dec)):
        excl[c, v - 3:v] = True
    rep = _assert_report(dec, n, pieces, full, full_report, cons=cons, exclude=excl, first=cs * U)
    free = rep[:, cs * U:].reshape(3, -1, nc)[:, :, 1:]
    assert bool((free < N.RELAXED).all())                               # a free voice is never flagged here
    # the same piece with every voice kept IS the corpus: every position from n on says FORCED_COPY
    (same, srep), cs, ce, nb = dec.reharmonise_tokens(x, 1, no_copy=ix, return_copy_report=True, return_bounds=True,
                                                      **dict(kw, keep_voices=(0, 1, 2, 3)))
    assert torch.equal(same[:, :events].cpu(), x)
    assert bool((srep[0, :events].reshape(-1)[n:] == N.FORCED_COPY).all()) and bool((srep[0, :events].reshape(-1)[:n] == 0).all())


# ---- (g) ----------------------------------------------------------------------------------------------------------------------
def test_the_refusals_and_the_decoder_level_index(tmp_path):
    from vqcpc_bach_amd.dataloaders.corpus import CopyIndex
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    dec = _decoder(NAMES[0])
    codes, given = _random_inputs(dec, 2, seed=571)
    pieces = _random_pieces(dec, [16, 16, 16, 16, 16, 16, 16, 16], seed=572)
    dc = _device_corpus(dec, pieces, subdivision=4)
    ix = dc.copy_index(3)
    assert isinstance(ix, CopyIndex) and ix.max_copy == 3 and ix.vocab == tuple(_vocab(dec)) and ix.device.type == 'cuda'
    with pytest.raises(ValueError, match='return_copy_report'):
        dec.generate_from_codes(codes, return_copy_report=True)
    with pytest.raises(ValueError, match='no_copy'):
        dec.generate_from_codes(codes, no_copy='the corpus')
    other = [p % 5 for p in pieces]
    from vqcpc_bach_amd.dataloaders.corpus import Corpus, DeviceCorpus
    zero = np.zeros(4, dtype=np.int64)
    small = DeviceCorpus(Corpus(np.concatenate(other).astype(np.int32), np.arange(9) * 16, 4, [5] * 4, zero, zero, zero), 'cuda')
    with pytest.raises(ValueError, match='vocab'):
        dec.generate_from_codes(codes, no_copy=small.copy_index(3))
    with pytest.raises(ValueError, match='vocab'):
        dec.audit_copies(given, small.copy_index(3))
    with pytest.raises(ValueError):
        dec.audit_copies(given[0], ix)
    with pytest.raises(ValueError):
        dec.audit_copies(given, None)
    long_codes = _random_codes(dec, 1, NB, seed=573)
    with pytest.raises(ValueError, match='return_copy_report'):
        dec.generate_from_code_long(long_codes, temperature=1.0, pad=[0] * 4, start=[0] * 4, return_copy_report=True)
    inc = IncrementalDecoder(dec, 2)
    inc.prefill(codes)
    with pytest.raises(ValueError, match='teacher'):
        inc.start(seeds=1, teacher=given.reshape(2, -1), no_copy=ix)
    # without the keywords the step's launches are what they were: no buffer, the plain sampler
    inc.start(seeds=1)
    assert inc.no_copy is None and inc.copy_report is None and inc.copy_static is None and not inc.masked
    # Decoder.copy_index resolves the split as check_duplicate_all_corpus does, and needs a corpus
    with pytest.raises(ValueError, match='corpus'):
        dec.copy_index(3)
    dec.dataloader_generator = types.SimpleNamespace(device_corpus=dc, sequences_size=dec.num_tokens_target // dec.num_channels // 4)
    train = dec.copy_index(3)
    lo, hi = dc.split_pieces('train', dec.dataloader_generator.sequences_size)
    assert train.pieces == (lo, hi) and 0 < hi < len(pieces)
    assert dec.copy_index(3, split=None).pieces == (0, len(pieces))
    tokens, report = dec.generate_from_codes(codes, temperature=1.0, seed=6, no_copy=train, return_copy_report=True)
    _assert_report(dec, 3, pieces[lo:hi], tokens, report)
    assert bool((dc.longest_common_run(tokens, pieces=(lo, hi))['length'][(report.reshape(2, -1) < N.RELAXED).all(dim=1).cpu().numpy()] <= 3).all())
