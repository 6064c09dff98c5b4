"""`PriorRelative.score_codes(method='windows')` and `score_chorale` (priors/scoring.py, vqcpc_prior_score) on the tiny priors of
tests/test_prior_gpu.py (N = 6; V = 32 and 1024) and the product priors of tests/product_codes_helpers.py ((K, ncb) = (8, 2), (4, 3)):
  (1) the scores against log_softmax of one float64-read forward per window (merged, stride 1: the rows of
      prior_constrained_reference.forced_greedy_loop), against the default `score_codes`, across `window_rows`, for 70 pieces,
  (2) the details: best / rank against the float64 rows, the consistency identities, one codebook == the merged prior bit for bit,
  (3) which kernels run, every ValueError, the training mode,
  (4) `score_chorale` end to end with the tiny decoder.
The reference windows come from tests/prior_score_reference.py's own plan, not from the package's."""
import pytest
import torch

import prior_constrained_reference as C
import prior_score_reference as PS
from decode_reference import U_FP32
from product_codes_helpers import build_prior
from test_generate_gpu import _golden_decoder
from test_generate_long_gpu import _meta_dataset
from test_prior_gpu import _golden_prior, fp32_gemms  # noqa: F401  (fixture)
from test_prior_product_gpu import _prior

pytestmark = pytest.mark.gpu

PRIORS = ['v32', 'v1024', 'p8x2', 'p4x3']
CODE_SEED = {'v32': 0, 'v1024': 11, 'p8x2': 0, 'p4x3': 1}      # the codes of the details test (its preconditions are asserted)
_CACHE = {}


def _same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def _get_prior(tag):
    if tag not in _CACHE:
        if tag.startswith('v'):
            _CACHE[tag] = _golden_prior(tag)[0].eval()
        else:
            K, ncb = (int(v) for v in tag[1:].split('x'))
            _CACHE[tag] = _prior(K, ncb)
    return _CACHE[tag]


@pytest.fixture(scope='module')
def tf_bound():
    """Twice the decoder pair's teacher-forced error measured in this run, the `bound` of
    test_prior_constrained_gpu.py::test_score_codes_is_log_softmax_of_the_forward_on_each_columns_window."""
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    from test_generate_gpu import _teacher_forced_error
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(0)
    dec, _ = seeded_decoder(D.make_cfg('DEC', B=2), 5)
    bound = 2 * _teacher_forced_error(dec, 2, seed=11)
    del dec
    return bound


@torch.no_grad()
def _window_rows(prior, codes, stride):
    """One `prior.forward` per window of the REFERENCE plan, read in float64 at the window's scored positions
    -> (rows: ncb tensors (B, L, K) float64 on the host -- the logits each code's digit j is scored from --, their rms)."""
    prior.eval()
    N = prior.num_tokens
    B, L = codes.shape
    dev = prior.sos.device
    ncb = prior.num_codebooks if prior.code_model == 'product' else 1
    rows = [[None] * L for _ in range(ncb)]
    for w, lo, hi in PS.window_plan_ref(L, N, stride):
        lg = prior.forward(codes[:, w:w + N].to(dev).contiguous())['weights_per_category']
        for j in range(ncb):
            for e in range(lo, hi):
                rows[j][e] = lg[j][:, e - w].double().cpu()
    rows = [torch.stack(r, dim=1) for r in rows]
    return rows, float(torch.cat([r.reshape(-1) for r in rows]).pow(2).mean().sqrt())


def _digits(prior, codes):
    if prior.code_model != 'product':
        return [codes]
    K = prior.codebook_size
    return [(codes // K ** j) % K for j in range(prior.num_codebooks)]


def _reference(prior, codes, stride, bound):
    """(logp float64 (B, L), tolerance (B, L), rows).  Tolerance per entry and stage: the logits of two computations of a forward
    differ by at most `bound` x rms, logp = logit[code] - logsumexp moves by at most twice that, plus the kernel's own chain
    (logp_bound); a product code sums its ncb stages in fp32: ncb - 1 more roundings of at most u |logp| each."""
    rows, rms = _window_rows(prior, codes, stride)
    digs = _digits(prior, codes)
    B, L = codes.shape
    ref = sum(torch.log_softmax(r, dim=-1).gather(2, d.unsqueeze(2)).squeeze(2) for r, d in zip(rows, digs))
    tol = torch.tensor([[sum(2 * bound * rms + C.logp_bound(r[b, e], int(d[b, e])) for r, d in zip(rows, digs)) for e in range(L)]
                        for b in range(B)])
    return ref, tol + (len(rows) - 1) * U_FP32 * ref.abs(), rows


def _codes(prior, B, L, seed):
    return torch.randint(0, prior.num_tokens_per_channel[0], (B, L), generator=torch.Generator().manual_seed(seed))


# ---- 1. the scores ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('tag', PRIORS)
def test_windows_is_log_softmax_of_the_forward_on_each_columns_window(fp32_gemms, tf_bound, tag, B):  # noqa: F811
    prior = _get_prior(tag)
    N = prior.num_tokens
    worst = worst_default = 0.0
    for L in (N, N + 1, N + 9):
        codes = _codes(prior, B, L, 21 + L)
        for stride in (1, 4):
            ref, tol, rows = _reference(prior, codes, stride, tf_bound)
            if stride == 1 and prior.code_model == 'merged':           # the slow loop's rows are these rows
                _, _, _, loop_rows = C.forced_greedy_loop(prior, codes)
                assert torch.equal(loop_rows, rows[0])
            got = prior.score_codes(codes, method='windows', window_stride=stride)
            assert got.shape == (B, L) and got.dtype == torch.float32 and got.is_cuda
            err = (got.cpu().double() - ref).abs()
            worst = max(worst, float((err / tol).max()))
            assert bool((err <= tol).all()), (tag, L, stride, float((err / tol).max()))
            default = prior.score_codes(codes, window_stride=stride)
            err_d = (got.double() - default.double()).abs().cpu()
            worst_default = max(worst_default, float((err_d / (2 * tol)).max()))
            assert bool((err_d <= 2 * tol).all()), (tag, L, stride, float((err_d / (2 * tol)).max()))
    print(f'{tag} B = {B}: worst |windows - log_softmax(forward)| / tolerance = {worst:.3f}, worst |windows - default| / (2 x '
          f'tolerance) = {worst_default:.3f} (bound {tf_bound:.2e})')


@pytest.mark.parametrize('tag', PRIORS)
def test_window_rows_and_70_pieces(fp32_gemms, tf_bound, tag):  # noqa: F811
    from vqcpc_bach_amd.priors import scoring
    prior = _get_prior(tag)
    L = prior.num_tokens + 9
    codes = _codes(prior, 3, L, 5)
    for stride in (1, 4):
        ref, tol, _ = _reference(prior, codes, stride, tf_bound)
        for window_rows in (1, 5, None, scoring.WINDOW_ROWS):
            got = prior.score_codes(codes, method='windows', window_stride=stride, window_rows=window_rows)
            err = (got.cpu().double() - ref).abs()
            assert bool((err <= tol).all()), (tag, stride, window_rows, float((err / tol).max()))
    if tag == 'v32':                                                   # 70 pieces x 10 windows: several chunks of the default size
        codes = _codes(prior, 70, L, 6)
        ref, tol, _ = _reference(prior, codes, 1, tf_bound)
        got = prior.score_codes(codes, method='windows')
        assert bool(((got.cpu().double() - ref).abs() <= tol).all())
        few = prior.score_codes(codes[66:69], method='windows')
        assert bool(((few.cpu().double() - ref[66:69]).abs() <= tol[66:69]).all())


# ---- 2. the details -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', PRIORS)
def test_details_against_the_float64_rows_and_the_identities(fp32_gemms, tf_bound, tag):  # noqa: F811
    """best and rank are integer functions of comparisons: they are compared where the float64 rows decide them by more than the two
    computations of a logit differ -- asserted as preconditions on the seeded inputs, over EVERY position: the smallest top-two gap
    > 1e-3 (the existing `gap` pattern), and the given code's logit apart from every other by more than 2 x bound x rms (each of two
    logits moves by at most bound x rms, so their order holds beyond twice that)."""
    prior = _get_prior(tag)
    product = prior.code_model == 'product'
    ncb = prior.num_codebooks if product else 1
    L, B = prior.num_tokens + 9, 3
    codes = _codes(prior, B, L, CODE_SEED[tag])
    for stride in (1, 4):
        ref, tol, rows = _reference(prior, codes, stride, tf_bound)
        rms = float(torch.cat([r.reshape(-1) for r in rows]).pow(2).mean().sqrt())
        det = prior.score_codes(codes, method='windows', window_stride=stride, return_details=True)
        assert set(det) == {'logp', 'entropy', 'rank', 'best', 'best_logp'}
        shape = (B, L, ncb) if product else (B, L)
        assert det['logp'].shape == (B, L) and all(det[k].shape == shape for k in ('entropy', 'rank', 'best', 'best_logp'))
        assert det['rank'].dtype == torch.int32 and det['best'].dtype == torch.int64 and det['entropy'].dtype == torch.float32
        assert _same_bits(det['logp'], prior.score_codes(codes, method='windows', window_stride=stride))
        assert bool(((det['logp'].cpu().double() - ref).abs() <= tol).all())
        gap, sep = float('inf'), float('inf')
        for j, (r, d) in enumerate(zip(rows, _digits(prior, codes))):
            top2 = torch.topk(r, 2, dim=-1)[0]
            gap = min(gap, float((top2[..., 0] - top2[..., 1]).min()))
            xt = r.gather(2, d.unsqueeze(2))
            other = (r - xt).abs().scatter(2, d.unsqueeze(2), float('inf'))
            sep = min(sep, float(other.min()))
            pick = (lambda t: t[..., j]) if product else (lambda t: t)
            best, rank = pick(det['best']).cpu(), pick(det['rank']).cpu()
            assert torch.equal(best, r.argmax(dim=-1)), (tag, stride, j)
            assert torch.equal(rank.long(), (r > xt).sum(dim=-1)), (tag, stride, j)
            # the identities, on the kernel's own outputs
            assert torch.equal(rank == 0, best == d), (tag, stride, j)
            # entropy and best_logp: logits that move by at most delta = bound x rms move H by at most sum_i p_i |log p_i + H| delta
            # <= 2 H delta and a log-probability by at most 2 delta; plus the kernel's own chains
            ent, blp = pick(det['entropy']).cpu(), pick(det['best_logp']).cpu()
            delta = tf_bound * rms
            for b in range(B):
                for e in range(L):
                    want = PS.prior_score_ref(r[b, e].numpy(), int(d[b, e]))
                    assert abs(float(ent[b, e]) - want['entropy']) <= 2 * want['entropy'] * delta + PS.entropy_bound(r[b, e].numpy())
                    assert abs(float(blp[b, e]) - want['best_logp']) <= 2 * delta + C.logp_bound(r[b, e], want['best'])
        print(f'{tag} stride {stride}: smallest top-two gap {gap:.3e}, the given codes\' logits apart from the others by >= {sep:.3e} '
              f'(2 x bound x rms = {2 * tf_bound * rms:.3e})')
        assert gap > 1e-3, gap
        assert sep > 2 * tf_bound * rms, (sep, 2 * tf_bound * rms)
        if not product:
            assert bool((det['best_logp'] >= det['logp']).all())
        else:                                                          # per digit: the stages' best_logp sum bounds the code's logp
            assert bool((det['best_logp'].double().sum(dim=-1) >= det['logp'].double() - 1e-5).all())


def test_one_codebook_gives_the_merged_details_bit_for_bit(fp32_gemms):  # noqa: F811
    merged, cfg, _ = _golden_prior('v32')
    sd = {k: v.detach().clone() for k, v in merged.state_dict().items()}
    sd['embedding.weight'] = sd['embedding.weight'].unsqueeze(0)
    prod = build_prior(cfg, 'product', sd).cuda()
    codes = _codes(merged, 3, cfg['N'] + 9, 8)
    for stride in (1, 4):
        a = prod.score_codes(codes, method='windows', window_stride=stride, return_details=True)
        b = merged.score_codes(codes, method='windows', window_stride=stride, return_details=True)
        for k in b:
            assert _same_bits(a[k].reshape(b[k].shape), b[k]), (stride, k)
        assert a['rank'].shape == (3, cfg['N'] + 9, 1)


# ---- 3. launches, errors, mode ---------------------------------------------------------------------------------------------------
def test_which_kernels_run(monkeypatch, fp32_gemms):  # noqa: F811
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
        return [n for n in names if n.startswith('vqcpc_prior_s')]
    for tag in ('v32', 'p8x2'):
        prior = _get_prior(tag)
        ncb = prior.num_codebooks if prior.code_model == 'product' else 1
        codes = _codes(prior, 2, 15, 3)
        for method, stride in (('auto', 1), ('cached', 1), ('forward', 1), ('cached', 4)):
            ran = set(launches(lambda: prior.score_codes(codes, method=method, window_stride=stride)))
            assert ran and 'vqcpc_prior_score' not in ran, (tag, method, ran)
        ran = launches(lambda: prior.score_codes(codes, method='windows', window_rows=7))
        assert ran == ['vqcpc_prior_score'] * (3 * ncb), (tag, ran)              # 2 x 10 rows in chunks of 7: one launch per chunk and stage
        assert set(launches(lambda: prior.score_codes(codes, method='windows', use_graph=False, return_details=True))) == \
            {'vqcpc_prior_score'}


def test_value_errors_and_the_training_mode(fp32_gemms):  # noqa: F811
    prior = _get_prior('v32')
    N = prior.num_tokens
    codes = _codes(prior, 2, N + 3, 4)
    for kw, match in ((dict(method='auto', return_details=True), "method='windows'"), (dict(method='cached', window_rows=8), "method='windows'"),
                      (dict(method='forward', return_details=True), "method='windows'"), (dict(window_rows=8), "method='windows'"),
                      (dict(method='windows', window_rows=0), 'window_rows'), (dict(method='windows', window_rows=1.5), 'window_rows'),
                      (dict(method='windows', window_rows=True), 'window_rows'), (dict(method='windows', window_stride=0), 'window_stride'),
                      (dict(method='windows', window_stride=N), 'window_stride')):
        with pytest.raises(ValueError, match=match):
            prior.score_codes(codes, **kw)
    with pytest.raises(ValueError, match='at least 6 codes'):
        prior.score_codes(codes[:, :N - 1], method='windows')
    bad = codes.clone()
    bad[1, 2] = -1
    with pytest.raises(ValueError, match='negative'):
        prior.score_codes(bad, method='windows')
    bad[1, 2] = 32
    with pytest.raises(ValueError, match='outside the 32 merged codes'):
        prior.score_codes(bad, method='windows')
    with pytest.raises(ValueError, match='method'):
        prior.score_codes(codes, method='window')
    big, cfg, _ = _golden_prior('v1024')
    big.num_tokens_per_channel = [4097]                                 # the merged sampler's limit, before any launch
    with pytest.raises(ValueError, match='at most 4096'):
        big.score_codes(codes, method='windows')
    for mode in (True, False):
        prior.train(mode)
        prior.score_codes(codes, method='windows')
        assert prior.training is mode and not prior.encoder.training
    prior.eval()


# ---- 4. score_chorale ---------------------------------------------------------------------------------------------------------
def test_score_chorale_is_the_sum_of_its_halves(fp32_gemms):  # noqa: F811
    prior = _get_prior('v32')
    dec, dcfg, _ = _golden_decoder('decoder_tiny')                    # the decoder of test_prior_constrained_gpu.py's continue_tokens test
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    nc, epc, E = dec.num_channels, dec.num_events_per_code, dec.data_processor.num_events
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randint(0, v - 3, (1, 2 * epc, 1), generator=g) for v in vocab], dim=2)     # two codes of tokens
    with pytest.raises(ValueError, match='START'):
        prior.score_chorale(x, dec)                                   # the synthetic dataset has no meta symbols
    dec.dataloader_generator = _meta_dataset(vocab)
    res = prior.score_chorale(x, dec)
    assert set(res) == {'code_logp', 'token_logp', 'total_logp', 'nats_per_token'}
    want_tokens = dec.score_chorale(x)
    assert _same_bits(res['token_logp'], want_tokens) and res['token_logp'].shape == (1, 2 * epc, nc)
    # the framed codes: the framed piece through the prior's own encoder, in model-sized chunks
    n2i = dec.dataloader_generator.dataset.note2index_dicts
    _, c0, c1, chunks = dec._frame_and_encode(x, n2i)
    prior.eval()
    framed = torch.cat([prior.encode(c.unsqueeze(0)) for c in chunks], dim=1)
    assert (c0, c1) == (E // epc, E // epc + 2) and framed.shape[1] >= prior.num_tokens
    want_codes = prior.score_codes(framed, method='windows')[:, c0:c1]
    assert _same_bits(res['code_logp'], want_codes) and res['code_logp'].shape == (1, 2)
    total = float(res['code_logp'].double().sum() + res['token_logp'].double().sum())
    assert res['total_logp'] == total and res['nats_per_token'] == -total / (2 * epc * nc)
    assert total < 0 and bool(torch.isfinite(res['code_logp']).all()) and bool(torch.isfinite(res['token_logp']).all())
    det = prior.score_chorale(x, dec, return_details=True, window_rows=3, decoder_window_rows=2)
    assert set(det) == {'code_logp', 'token_logp', 'total_logp', 'nats_per_token', 'code_details', 'token_details'}
    assert det['code_details']['rank'].shape == (1, 2) and det['token_details']['rank'].shape == (1, 2 * epc, nc)
    assert _same_bits(det['code_details']['logp'], det['code_logp']) and _same_bits(det['token_details']['logp'], det['token_logp'])
    for bad in (x[0], x[:, :, :nc - 1], x[:, :0]):                    # wrong rank / voices, empty
        with pytest.raises(ValueError, match='x:'):
            prior.score_chorale(bad, dec)
