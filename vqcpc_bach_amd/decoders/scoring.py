"""Scoring GIVEN tokens under the decoder: `Decoder.score_tokens` / `score_chorale` (decoders/decoder.py) call into here.

`generate_from_code_long` emits code t of a piece in the model window `Decoder.compute_start_end_times(t, nb, S)` names, and
nothing but t decides that window.  When the tokens are known, the window's input is known too -- the chorale's own tokens --
so the nb - S + 1 distinct windows of a piece do not wait for each other: each is one row of a batched, teacher-forced forward
through the training path's kernels (`compute_loss`'s source rows, target rows, masks and `forward_rows`), and the logits of a
code's U positions are read off the window it would have been generated in.  What a forced generation computes with U
incremental steps per code and a K/V-cache re-prefill per window, this computes with one forward per window.

Per chunk of `window_rows` (piece, window) rows:
  1. window tokens (rows, T) and window codes (rows, S) [latents (rows, S, dz)] are gathered from the chorale and the code sequence;
  2. the forward gives the hidden rows (rows * T, d);
  3. only the SCORED positions' hidden rows go through the concatenated head (vqcpc_decode_linear with its `gather` argument, the
     arithmetic and layout of the generation's logits): U of a middle window's T rows, up to (S // 2 + 1) * U of a head / tail window;
  4. one vqcpc_decode_score launch (csrc/score.hip) reads each row's target token from the chorale and writes log-probability,
     allowed mass, entropy, rank, arg-max and the arg-max's log-probability straight into (B, nb * U) arrays in chorale coordinates.
"""
import ctypes

import numpy as np
import torch

from .. import hip, ops
from ..transformer.transformer_custom import mask_code
from ..utils import STEP_LOCK

HEAD_ROWS = 64                  # vqcpc_decode_linear's row limit: the head runs on slices of the gathered rows
DETAILS = ('logp', 'entropy', 'rank', 'best', 'best_logp')


def window_plan(num_blocks, num_blocks_model, code_index_start, code_index_end, start_end_times):
    """[(first code of the window, first scored code, one past the last scored code)], windows ascending: the distinct windows
    `start_end_times(t, num_blocks, num_blocks_model)` names for the codes t of [code_index_start, code_index_end), each with the
    codes scored in it.  A window's codes are consecutive, because the window's first code never decreases with t."""
    nb, S = int(num_blocks), int(num_blocks_model)
    if S < 1 or nb < S:
        raise ValueError(f'score_window_plan: at least {S} codes (one model window of >= 1 code) are needed, got {nb}')
    if not 0 <= code_index_start <= code_index_end <= nb:
        raise ValueError(f'0 <= code_index_start <= code_index_end <= {nb} expected, got {code_index_start}, {code_index_end}')
    plan = []
    for t in range(int(code_index_start), int(code_index_end)):
        w = int(start_end_times(t, nb, S)[0])
        if plan and plan[-1][0] == w:
            plan[-1][2] = t + 1
        else:
            plan.append([w, t, t + 1])
    return [tuple(p) for p in plan]


def _checked_tokens(dec, x, B, events, first, last):
    """x (B, events, channels) int64 -> on the device; ValueError on a wrong shape or dtype and -- one host check per call -- on a
    token of the events [first, last) outside its voice's vocabulary, naming the first (row, event, voice)."""
    x = torch.as_tensor(x)
    nc = dec.num_channels
    if tuple(x.shape) != (B, events, nc) or x.dtype != torch.int64:
        raise ValueError(f'x: ({B}, {events}, {nc}) int64 tokens over the whole code sequence expected, got {tuple(x.shape)} {x.dtype}')
    x = x.to(dec.sos.device)
    vocab = torch.tensor([int(v) for v in dec.num_tokens_per_channel], dtype=torch.int64, device=x.device)
    bad = ((x < 0) | (x >= vocab))[:, first:last].reshape(-1)
    if bad.numel():
        at = bad.to(torch.int32).argmax()
        found, at = torch.stack([bad.any().long(), at.long()]).tolist()                     # the one host check
        if found:
            b, rest = divmod(at, (last - first) * nc)
            e, c = divmod(rest, nc)
            raise ValueError(f'x: (row {b}, event {first + e}, voice {c}) holds token {int(x[b, first + e, c])}, outside its '
                             f'voice\'s vocabulary [0, {int(vocab[c])})')
    return x


def score_tokens(dec, x, codes, code_index_start=None, code_index_end=None, pad=None, start=None, allowed=None,
                 return_details=False, window_rows=32):
    """The body of `Decoder.score_tokens` (its docstring states the contract)."""
    S, U, epc, nc, T = dec.num_tokens_source, dec.total_upscaling, dec.num_events_per_code, dec.num_channels, dec.num_tokens_target
    d, dev = dec.d_model, dec.sos.device
    if isinstance(window_rows, bool) or int(window_rows) != window_rows or window_rows < 1:
        raise ValueError(f'window_rows: an integer >= 1 expected, got {window_rows!r}')
    window_rows = int(window_rows)
    codes = dec._source_on_device(codes, 'codes')
    B, nb = codes.shape[:2]
    if nb < S:
        raise ValueError(f'codes: at least {S} codes (one model window) are needed, got {nb}')
    c0 = 0 if code_index_start is None else int(code_index_start)
    c1 = nb if code_index_end is None else int(code_index_end)
    plan = window_plan(nb, S, c0, c1, dec.compute_start_end_times)
    events, width = nb * epc, nb * U
    x = _checked_tokens(dec, x, B, events, c0 * epc, c1 * epc)
    chorale = dec.init_generation_chorale(num_events=events, start_index=c0 * epc, pad=pad, start=start).repeat(B, 1, 1)
    chorale[:, c0 * epc:c1 * epc] = x[:, c0 * epc:c1 * epc]
    chorale = chorale.reshape(B, width)
    words = None
    if allowed is not None:              # the generation's validation and packing; a written token outside its set is scored all the same
        words = dec._allowed_words(allowed, B, events, c0 * epc, c1 * epc)
        words = words.expand(B, -1, -1).contiguous()

    f32 = dict(dtype=torch.float32, device=dev)
    nan = float('nan')
    res = {'logp': torch.full((B, width), nan, **f32)}
    if return_details:
        res.update(entropy=torch.full((B, width), nan, **f32), rank=torch.full((B, width), -1, dtype=torch.int32, device=dev),
                   best=torch.full((B, width), -1, dtype=torch.int64, device=dev), best_logp=torch.full((B, width), nan, **f32))
        if words is not None:
            res['allowed_mass'] = torch.full((B, width), nan, **f32)
    cut = lambda t: t.view(B, events, nc)[:, c0 * epc:c1 * epc].contiguous()
    if not plan:
        out = {k: cut(v) for k, v in res.items()}
        return out if return_details else out['logp']

    # the rows, piece-major, and per row its scored window positions: everything the chunks index with, built once on the host
    W = len(plan)
    pw = np.array([p[0] for p in plan], np.int64)
    row_piece = np.repeat(np.arange(B, dtype=np.int64), W)
    row_win = np.tile(pw, B)
    span = np.array([(p[2] - p[1]) * U for p in plan], np.int64)                 # scored positions of a window
    rel0 = np.array([(p[1] - p[0]) * U for p in plan], np.int64)                 # the first of them, window-relative
    per_row = np.tile(span, B)
    ends = np.cumsum(per_row)
    n_rows = B * W
    row_of = np.repeat(np.arange(n_rows, dtype=np.int64), per_row)               # per scored position: its row, ...
    within = np.arange(ends[-1], dtype=np.int64) - np.repeat(ends - per_row, per_row) + np.repeat(np.tile(rel0, B), per_row)
    sc_b = torch.from_numpy(row_piece[row_of].astype(np.int32)).to(dev)          # ... piece, chorale column, and window position
    sc_col = torch.from_numpy((row_win[row_of] * U + within).astype(np.int32)).to(dev)
    row_piece_d, row_win_d = torch.from_numpy(row_piece).to(dev), torch.from_numpy(row_win).to(dev)
    row_of_d, within_d = torch.from_numpy(row_of).to(dev), torch.from_numpy(within).to(dev)

    sizes = [int(n) for n in dec.num_tokens_per_channel]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    offsets_c = (ctypes.c_int32 * (nc + 1))(*offsets.tolist())
    vtot = int(offsets[-1])
    ar_t, ar_s = torch.arange(T, device=dev), torch.arange(S, device=dev)
    enc_mask = mask_code(dec.encoder_attention_type)
    memory_mask = ops.MASK_NONE if dec.cross_attention_type == 'diagonal' else mask_code(dec.cross_attention_type)
    with STEP_LOCK, torch.no_grad():
        was_training = dec.training
        dec.eval()
        try:
            head_w = torch.cat([m.weight for m in dec.pre_softmaxes], dim=0).contiguous()
            head_b = torch.cat([m.bias for m in dec.pre_softmaxes], dim=0).contiguous()
            table = dec._target_table(dev)
            for r0 in range(0, n_rows, window_rows):
                r1 = min(r0 + window_rows, n_rows)
                n = r1 - r0
                rb, rw = row_piece_d[r0:r1].unsqueeze(1), row_win_d[r0:r1].unsqueeze(1)
                tokens = chorale[rb, rw * U + ar_t].view(n, T // nc, nc)
                source = codes[rb, rw + ar_s]                                           # (n, S) or (n, S, dz)
                if dec.continuous_source:
                    src = ops.linear(source.reshape(-1, dec.source_dim), dec.source_embeddings.weight, dec.source_embeddings.bias)
                else:
                    src = dec.source_rows(source)
                tgt = dec._target_rows(dec.data_processor.checked(tokens), table=table)
                out = dec.transformer.forward_rows(src, tgt, n, enc_mask, ops.MASK_CAUSAL, memory_mask)[0].contiguous()
                p0, p1 = int(ends[r0] - per_row[r0]), int(ends[r1 - 1])
                gather = ((row_of_d[p0:p1] - r0) * T + within_d[p0:p1]).contiguous()    # hidden rows of the scored positions
                logits = torch.empty(p1 - p0, vtot, **f32)
                for g0 in range(0, p1 - p0, HEAD_ROWS):
                    m = min(HEAD_ROWS, p1 - p0 - g0)
                    hip.call('vqcpc_decode_linear', out, d, gather[g0:], head_w, head_b, None, 0, logits[g0:], vtot, m, vtot, d, 0)
                hip.call('vqcpc_decode_score', logits, vtot, offsets_c, nc, p1 - p0, sc_b[p0:], sc_col[p0:], chorale, width,
                         words, width if words is not None else 0, B, width, width, res['logp'], res.get('allowed_mass'),
                         res.get('entropy'), res.get('rank'), res.get('best'), res.get('best_logp'))
        finally:
            dec.train(was_training)
    out = {k: cut(v) for k, v in res.items()}
    return out if return_details else out['logp']
