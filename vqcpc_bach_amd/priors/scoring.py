"""Scoring GIVEN codes under the prior: `PriorRelative.score_codes(method='windows')` / `score_chorale` (priors/prior_relative.py)
call into here.

`generate_codes` emits code e < N of a piece in window 0 and, at `window_stride` = k, the codes of a later window in its last k
positions (`IncrementalPrior.run`); nothing but the column decides the window.  When the codes are known, the window's input is known
too -- the start-of-sentence row, then the piece's own codes -- and since every window's row 0 is the start-of-sentence row, no window
shares a cache row with another: each is a full forward of its own.  So the windows of a piece do not wait for each other: each is one
row of a batched, teacher-forced forward through the training path's kernels (`compute_loss`'s table lookup and
`forward_rows_masked` under MASK_CAUSAL).  What the forced generation computes with N cached steps and L - N window moves, strictly one
after the other, this computes with one forward per chunk of windows.

Per chunk of `window_rows` (piece, window) rows:
  1. the window codes (rows, N) are gathered from the code sequences and shifted by one with the start-of-sentence index;
  2. the input rows are looked up (`_input_table` / `_input_tables`) and the forward gives the hidden rows (rows * N, d);
  3. only the SCORED positions' hidden rows are gathered and go through the head, the training path's GEMM: N rows of window 0, the
     last k of a later window;
  4. one vqcpc_prior_score launch (csrc/prior_score.hip) reads each row's target code from the sequence and writes log-probability,
     entropy, rank, arg-max and the arg-max's log-probability straight into (B, L) arrays in sequence coordinates.
code_model 'product': step 3 and 4 once per stage j in ascending order, on h + sum_{i<j} D_i[c_i] of the piece's own digits
(ops.ProductEmbeddingFn, as `_compute_loss_product`); the kernel adds the stages' log-probabilities in that order.
"""
import numpy as np
import torch

from .. import hip, ops
from ..utils import STEP_LOCK

WINDOW_ROWS = 512               # (piece, window) rows per forward when the caller names none: the fastest of 32 .. 512 at B = 1 / 8 / 32
                                # (profiles/prior_score_perf_log.md: 2.27 / 6.16 / 17.9 ms against 2.30 / 9.18 / 31.3 ms at 128)
MAX_SCORED_VOCAB = 4096         # vqcpc_prior_score: logits per row


def window_plan(num_tokens, N, window_stride=1):
    """[(first code of the window, first scored column, one past the last scored column)], windows ascending, columns in sequence
    coordinates: the columns `IncrementalPrior.run` scores in each window.  Window 0 scores [0, N); window i * k its last k columns;
    when (L - N) % k != 0 a last window at L - N scores the last (L - N) % k columns."""
    L, N, k = int(num_tokens), int(N), int(window_stride)
    if N < 1 or L < N:
        raise ValueError(f'score_window_plan: num_tokens >= {N} (one model window of >= 1 code) expected, got {L}')
    if isinstance(window_stride, bool) or k != window_stride or not 1 <= k < max(N, 2):
        raise ValueError(f'score_window_plan: 1 <= window_stride < {max(N, 2)} (got {window_stride!r})')
    n_full, rem = divmod(L - N, k)
    plan = [(0, 0, N)] + [(i * k, i * k + N - k, i * k + N) for i in range(1, n_full + 1)]
    if rem:
        plan.append((L - N, L - rem, L))
    return plan


def _padded_head(head):
    """The head's weight and bias with the rows padded to a multiple of 4, the GEMM's granularity (as decoders.decoder.HeadsFn)."""
    w, b = head.weight, head.bias
    pn = -w.shape[0] % 4
    if pn:
        w, b = torch.nn.functional.pad(w, (0, 0, 0, pn)), torch.nn.functional.pad(b, (0, pn))
    return w.contiguous(), b.contiguous()


def score_codes_windows(prior, codes, window_stride=1, return_details=False, window_rows=None):
    """The body of `PriorRelative.score_codes(method='windows')` (its docstring states the contract); codes (B, L) int64 on the
    device, checked by the caller to be >= 0."""
    N, V, d, dev = prior.num_tokens, prior.num_tokens_per_channel[0], prior.d_model, prior.sos.device
    product = prior.code_model == 'product'
    ncb, K = (prior.num_codebooks, prior.codebook_size) if product else (1, V)
    if window_rows is None:
        window_rows = WINDOW_ROWS
    if isinstance(window_rows, bool) or not isinstance(window_rows, (int, np.integer)) or window_rows < 1:
        raise ValueError(f'window_rows: an integer >= 1 expected, got {window_rows!r}')
    window_rows = int(window_rows)
    if not product and V > MAX_SCORED_VOCAB:
        raise ValueError(f'generate_codes: {V} merged codes, the sampling kernel (vqcpc_prior_sample) takes at most '
                         f'{MAX_SCORED_VOCAB}')
    B, L = codes.shape
    if L < N:
        raise ValueError(f'score_codes: at least {N} codes (one model window) are needed, got {L}')
    if not 1 <= int(window_stride) < max(N, 2) or int(window_stride) != window_stride:
        raise ValueError(f'score_codes: 1 <= window_stride < {N} (got {window_stride})')
    if bool((codes >= V).any()):
        raise ValueError(f'score_codes: a code is outside the {V} merged codes')
    plan = window_plan(L, N, window_stride)

    f32 = dict(dtype=torch.float32, device=dev)
    nan = float('nan')
    res = {'logp': torch.full((B, L), nan, **f32)}
    if return_details:
        res.update(entropy=torch.full((B, L * ncb), nan, **f32), rank=torch.full((B, L * ncb), -1, dtype=torch.int32, device=dev),
                   best=torch.full((B, L * ncb), -1, dtype=torch.int64, device=dev), best_logp=torch.full((B, L * ncb), nan, **f32))

    # the rows, piece-major, and per row its scored window positions: everything the chunks index with, built once on the host
    W = len(plan)
    pw = np.array([p[0] for p in plan], np.int64)
    row_piece = np.repeat(np.arange(B, dtype=np.int64), W)
    row_win = np.tile(pw, B)
    span = np.array([p[2] - p[1] for p in plan], np.int64)                       # scored positions of a window
    rel0 = np.array([p[1] - p[0] for p in plan], np.int64)                       # the first of them, window-relative
    per_row = np.tile(span, B)
    ends = np.cumsum(per_row)
    n_rows = B * W
    row_of = np.repeat(np.arange(n_rows, dtype=np.int64), per_row)               # per scored position: its row, ...
    within = np.arange(ends[-1], dtype=np.int64) - np.repeat(ends - per_row, per_row) + np.repeat(np.tile(rel0, B), per_row)
    sc_b = torch.from_numpy(row_piece[row_of].astype(np.int32)).to(dev)          # ... piece, sequence column, and window position
    sc_col = torch.from_numpy((row_win[row_of] + within).astype(np.int32)).to(dev)
    row_piece_d, row_win_d = torch.from_numpy(row_piece).to(dev), torch.from_numpy(row_win).to(dev)
    row_of_d, within_d = torch.from_numpy(row_of).to(dev), torch.from_numpy(within).to(dev)
    ar_n = torch.arange(N, device=dev)

    with STEP_LOCK, torch.no_grad():
        was_training = prior.training
        prior.eval()
        try:
            heads = [_padded_head(h) for h in prior.pre_softmaxes]
            if product:
                tables, sos = prior._input_tables().contiguous(), prior.sos.view(1, d)
                dtab = prior.digit_embeddings.weight if ncb > 1 else None
            else:
                table = prior._input_table().contiguous()
            for r0 in range(0, n_rows, window_rows):
                r1 = min(r0 + window_rows, n_rows)
                n = r1 - r0
                win = codes[row_piece_d[r0:r1].unsqueeze(1), row_win_d[r0:r1].unsqueeze(1) + ar_n]                   # (n, N)
                shifted = torch.cat([torch.full((n, 1), V, dtype=torch.int64, device=dev), win[:, :-1]], dim=1).reshape(-1)
                rows = ops.ProductEmbeddingFn.apply(tables, sos, shifted) if product else ops.EmbeddingFn.apply(table, shifted)
                out, _ = prior.transformer.forward_rows_masked(rows, n, ops.MASK_CAUSAL)
                p0, p1 = int(ends[r0] - per_row[r0]), int(ends[r1 - 1])
                gather = (row_of_d[p0:p1] - r0) * N + within_d[p0:p1]                    # hidden rows of the scored positions
                h0 = out.reshape(n * N, d).index_select(0, gather)
                low = codes[sc_b[p0:p1].long(), sc_col[p0:p1].long()] % (K ** (ncb - 1)) if ncb > 1 else None
                for j in range(ncb):
                    h = h0 if j == 0 else ops.ProductEmbeddingFn.apply(dtab, None, low, j, h0)
                    w, b = heads[j]
                    logits = ops.gemm_nt(h, w, bias=b)                                   # (p1 - p0, K padded to a multiple of 4)
                    hip.call('vqcpc_prior_score', logits, logits.shape[1], K, ncb, j, p1 - p0, sc_b[p0:], sc_col[p0:], codes, L, B,
                             L, res['logp'], L, L * ncb, res.get('entropy'), res.get('rank'), res.get('best'), res.get('best_logp'))
        finally:
            prior.train(was_training)
    if not return_details:
        return res['logp']
    if product:
        res = {k: (v if k == 'logp' else v.view(B, L, ncb)) for k, v in res.items()}
    return res


def score_chorale(prior, x, decoder, return_details=False, window_rows=None, decoder_window_rows=32):
    """The body of `PriorRelative.score_chorale` (its docstring states the contract)."""
    if decoder.continuous_source:
        raise NotImplementedError('a prior over continuous (NoQuantization) codes does not exist')
    n2i = getattr(getattr(decoder.dataloader_generator, 'dataset', None), 'note2index_dicts', None)
    if n2i is None:
        raise ValueError('score_chorale needs dataset.note2index_dicts with the START / END / XX symbols')
    nc, E, epc, U = decoder.num_channels, decoder.data_processor.num_events, decoder.num_events_per_code, decoder.total_upscaling
    if int(np.prod(prior.encoder.downscaler.downscale_factors)) != U:
        raise ValueError(f"score_chorale: the prior's encoder makes one code of "
                         f'{int(np.prod(prior.encoder.downscaler.downscale_factors))} tokens, the decoder of {U}')
    x = torch.as_tensor(x).long().cpu()
    if x.dim() != 3 or x.shape[0] != 1 or x.shape[2] != nc or x.shape[1] < 1:
        raise ValueError(f'x: (1, events, {nc}) tokens expected, got {tuple(x.shape)}')
    n = x.shape[1]
    vocab = torch.tensor([int(v) for v in decoder.num_tokens_per_channel], dtype=torch.int64)
    bad = ((x < 0) | (x >= vocab)).reshape(-1)                                            # checked before an encoder embeds x
    if bool(bad.any()):
        e, c = divmod(int(bad.to(torch.int32).argmax()), nc)
        raise ValueError(f'x: (row 0, event {e}, voice {c}) holds token {int(x[0, e, c])}, outside its voice\'s vocabulary '
                         f'[0, {int(vocab[c])})')
    # ONE framing: the decoder's half is `Decoder.score_chorale`'s own sequence of calls on it
    dec_codes, c0, c1, chunks = decoder._frame_and_encode(x, n2i)
    n2 = [n2i[c] for c in range(nc)]
    tokens = decoder.score_tokens(chunks.reshape(1, -1, nc), dec_codes, code_index_start=c0, code_index_end=c1,
                                  pad=[int(d['XX']) for d in n2], start=[int(d['START']) for d in n2],
                                  return_details=return_details, window_rows=decoder_window_rows)
    first = E - c0 * epc                                                                  # x's event 0 in the returned range
    take = lambda t: t[:, first:first + n].contiguous()
    tokens = {k: take(v) for k, v in tokens.items()} if return_details else take(tokens)
    # the prior's half: the framed code sequence, every code conditioned on everything before it, the framing chunk's codes
    # included.  In a trained pipeline the prior's frozen encoder IS the decoder's: the codes are the ones just made
    if prior.encoder is decoder.encoder:
        framed_codes = dec_codes
    else:
        was_training = prior.training
        prior.eval()
        try:
            framed_codes = torch.cat([prior.encode(c.unsqueeze(0)) for c in chunks], dim=1)                     # glued: (1, L)
        finally:
            prior.train(was_training)
        if framed_codes.shape[1] != dec_codes.shape[1]:
            raise ValueError(f"score_chorale: the prior's encoder made {framed_codes.shape[1]} codes of the framed piece, the "
                             f"decoder's {dec_codes.shape[1]}")
    codes_res = prior.score_codes(framed_codes, method='windows', return_details=return_details, window_rows=window_rows)
    cut = lambda t: t[:, c0:c1].contiguous()
    code_logp = cut(codes_res['logp'] if return_details else codes_res)
    token_logp = tokens['logp'] if return_details else tokens
    total = float(code_logp.double().sum() + token_logp.double().sum())
    out = {'code_logp': code_logp, 'token_logp': token_logp, 'total_logp': total, 'nats_per_token': -total / (n * nc)}
    if return_details:
        out['code_details'] = {k: cut(v) for k, v in codes_res.items()}
        out['token_details'] = tokens
    return out
