"""Golden vectors for decoder generation (decoders/decoder.py:552-723, utils.py:101-128), produced by IMPORTING the
reference (container-only tool; reuses the stubs of tools/gen_golden.py and the decoder builders of
tools/gen_golden_decoder.py).  Fixtures hold tensors only.

  generate_filter.npz       64 tie-free logit rows of widths 11..60 and, for every (top_k, top_p, temperature) of the
                            grid, the keep-mask of the reference's own `top_k_top_p_filtering` applied to logits / T.
                            Rows whose cumulative probability lands within 1e-5 of a top_p are redrawn, so the masks do
                            not hinge on the last bits of a cumsum.
  generate_greedy_tiny.npz  the decoder_tiny configuration (T = 48, S = 3) with its state dict, merged codes for B = 3 and
                            the tokens of the reference's generate loop (:596-637: `Decoder.forward` per token, the
                            filter, np.random.choice) with top_k = 1, plus the top-1 / top-2 logit gap at every step.
                            The model seed is the first whose smallest gap is > 1e-3.

Run:  python tools/gen_golden_generate.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_decoder as gd  # noqa: E402  (stubs, the reference on sys.path, decoder builders)
from gen_golden import npy, save, sd_arrays, perturb_1d, build_encoder  # noqa: E402

from VQCPCB.utils import flatten, top_k_top_p_filtering  # noqa: E402

TOP_K = (0, 1, 3, 10)
TOP_P = (0.5, 0.9, 0.99, 1.0)
TEMPS = (0.5, 1.0, 2.0)


def _margin_ok(row):
    """True when no cumulative probability of the sorted softmax (any temperature) sits within 1e-5 of a top_p."""
    for temp in TEMPS:
        for k in TOP_K:
            lg = torch.tensor(row, dtype=torch.float64) / temp
            if k > 0:
                lg[lg < torch.topk(lg, min(k, lg.numel()))[0][-1]] = -float('inf')
            srt = torch.sort(lg, descending=True)[0]
            cum = torch.cumsum(torch.softmax(srt, dim=-1), dim=-1)
            for p in TOP_P[:-1]:
                if float((cum - p).abs().min()) < 1e-5:
                    return False
    return True


def gen_filter(name, n_rows=64, vmax=60, seed=90):
    g = np.random.default_rng(seed)
    logits = np.zeros((n_rows, vmax), np.float32)
    widths = np.zeros(n_rows, np.int64)
    keep = np.zeros((n_rows, len(TOP_K), len(TOP_P), len(TEMPS), vmax), np.bool_)
    for r in range(n_rows):
        V = int(g.integers(11, vmax + 1))
        while True:
            row = (g.standard_normal(V) * g.uniform(0.5, 4.0)).astype(np.float32)
            if len(np.unique(row)) == V and _margin_ok(row):
                break
        logits[r, :V], widths[r] = row, V
        for a, k in enumerate(TOP_K):
            for b, p in enumerate(TOP_P):
                for c, temp in enumerate(TEMPS):
                    f = top_k_top_p_filtering(torch.from_numpy(row.copy()) / temp, top_k=k, top_p=p)
                    keep[r, a, b, c, :V] = npy(f > -float('inf'))
    save(name, logits=logits, widths=widths, keep=keep, top_k=np.array(TOP_K), top_p=np.array(TOP_P, np.float32),
         temperature=np.array(TEMPS, np.float32))


def build_tiny(cfg, seed):
    """gen_golden_decoder.gen_decoder_step's model: seeded encoder + decoder, codebooks on encoder outputs."""
    torch.manual_seed(seed)
    enc = build_encoder(cfg)
    perturb_1d(enc)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        probe = torch.cat([torch.randint(0, nv, (4 * cfg['K'], 4, 1), generator=g) for nv in cfg['vocab']], dim=2)
        zp = enc.downscaler(flatten(enc.data_processor.embed(enc.data_processor.preprocess(probe)))).view(-1, cfg['D'])
        dsub = cfg['D'] // cfg['ncb']
        for c, e in enumerate(enc.quantizer.embeddings):
            e.copy_(zp[c:c + 4 * cfg['K']:4, c * dsub:(c + 1) * dsub] + 0.01 * torch.randn(cfg['K'], dsub, generator=g))
    dec = gd.build_decoder(cfg, enc)
    with torch.no_grad():
        for k, p in dec.named_parameters():
            if not k.startswith('encoder.') and p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for m in dec.pre_softmaxes:
            m.weight.mul_(4.0)          # peaked distributions: clear greedy choices
    x = torch.cat([torch.randint(0, nv, (cfg['B'], cfg['events'], 1), generator=g) for nv in cfg['vocab']], dim=2)
    dec.eval()
    with torch.no_grad():
        _, idx, _ = enc(x)
        codes = enc.merge_codes(idx.clone())
    return dec, codes


def reference_greedy(dec, codes, events, nc, vocab):
    """The loop of Decoder.generate (:596-637) with temperature 1, top_k = 1, top_p = 1, no meta-symbol exclusion."""
    B = codes.shape[0]
    x = dec.init_generation(num_events=events).repeat(B, 1, 1)
    gaps = np.zeros((B, events * nc), np.float64)
    with torch.no_grad():
        for event_index in range(events):
            for channel_index in range(nc):
                forward_pass = dec.forward(codes, x)
                logits = forward_pass['weights_per_category'][channel_index][:, event_index, :] / 1.0
                top2 = torch.topk(logits, 2, dim=-1)[0]
                gaps[:, event_index * nc + channel_index] = npy(top2[:, 0] - top2[:, 1])
                filtered = torch.stack([top_k_top_p_filtering(lg, top_k=1, top_p=1.0) for lg in logits], dim=0)
                p = npy(torch.softmax(filtered, dim=-1))
                for b in range(B):
                    x[b, event_index, channel_index] = int(np.random.choice(np.arange(vocab[channel_index]), p=p[b]))
    return x, gaps


def gen_greedy(name, cfg, first_seed=100):
    for seed in range(first_seed, first_seed + 50):
        dec, codes = build_tiny(cfg, seed)
        tokens, gaps = reference_greedy(dec, codes, cfg['events'], len(cfg['vocab']), cfg['vocab'])
        print(f'   seed {seed}: smallest top-1 / top-2 gap {gaps.min():.2e}')
        if gaps.min() > 1e-3:
            break
    assert gaps.min() > 1e-3
    arrays = sd_arrays('sd', dec)
    arrays.update(codes=npy(codes), tokens=npy(tokens), gaps=gaps, cfg_json=np.array(json.dumps(cfg)), seed=np.array(seed))
    save(name, **arrays)


if __name__ == '__main__':
    np.random.seed(0)
    gen_filter('generate_filter')
    tiny = dict(emb=8, vocab=[11, 12, 13, 14], d=32, H=2, layers=[1, 1], ff=64, D=8, K=16, ncb=2, zdim=8, up_hidden=16,
                events=12, B=3, Kl=2, Kr=2, dec_emb=8, dec_d=32, dec_H=2, dec_enc_layers=2, dec_dec_layers=2, dec_ff=64, dec_pos=4,
                enc_attn='anticausal', cross_attn='anticausal')
    gen_greedy('generate_greedy_tiny', tiny)
