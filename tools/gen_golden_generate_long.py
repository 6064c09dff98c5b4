"""Golden vectors for long-form generation (decoders/decoder.py:729-854), produced by IMPORTING the reference and driving
its own `generate_from_code_long` (container-only tool; reuses the stubs of tools/gen_golden.py and the tiny decoder
builders of tools/gen_golden_generate.py).  Fixtures hold tensors plus cfg_json only.

  generate_long_tiny_S4.npz  events 16 (T = 64, S = 4, U = 16); nb = 10 codes, code_index_start = 2, code_index_end = 8,
                             B = 2, num_decodings = 2: a prefilled first code and middle slides.
  generate_long_tiny_S3.npz  the tiny shape of generate_greedy_tiny (T = 48, S = 3, odd S: S // 2 = 1); nb = 7, codes
                             1 .. 7: middle slides and the tail.

Each holds the decoder's state dict, the merged codes (B, nb), the PAD / START ids, the initial chorale of the reference's
`init_generation_chorale`, the reference's tokens with top_k = 1 (sliced to the generated codes, as it returns them), the
(t_begin, t_end, t_relative) of every generated code and the top-1 / top-2 logit gap at every drawn position.  The dataset
is a stub (`note2index_dicts` with START / END / XX as the last three ids of every voice, `to_score` = identity).  The
model seed is the first whose smallest gap is > 1e-3, so greedy equality does not hinge on rounding.

Run:  python tools/gen_golden_generate_long.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import npy, save, sd_arrays  # noqa: E402
from gen_golden_generate import build_tiny  # noqa: E402


class StubDataset:
    def __init__(self, vocab):
        self.note2index_dicts = [{'START': v - 3, 'END': v - 2, 'XX': v - 1} for v in vocab]


class StubDataloaderGenerator:
    def __init__(self, vocab):
        self.dataset = StubDataset(vocab)

    def to_score(self, tensor_score):
        return tensor_score


def reference_long(dec, codes, cfg, start, end, num_decodings):
    """The reference's own generate_from_code_long with top_k = 1; its forward and window arithmetic are wrapped to
    record the logit gaps and the windows."""
    nc, U = len(cfg['vocab']), 16
    epc = U // nc
    calls, windows = [], []
    fwd, cset = dec.forward, dec.compute_start_end_times

    def forward(source, target):
        out = fwd(source, target)
        calls.append([w.detach().clone() for w in out['weights_per_category']])
        return out

    def times(t, num_blocks, num_blocks_model):
        r = cset(t, num_blocks=num_blocks, num_blocks_model=num_blocks_model)
        windows.append((t,) + tuple(r))
        return r

    dec.forward, dec.compute_start_end_times = forward, times
    try:
        scores = dec.generate_from_code_long(codes, temperature=1.0, top_k=1, top_p=1.0, num_decodings=num_decodings,
                                             code_index_start=start, code_index_end=end)
    finally:
        dec.forward, dec.compute_start_end_times = fwd, cset
    tokens = np.stack([np.asarray(s) for s in scores], axis=0).astype(np.int64)
    n = (end - start) * U
    assert len(calls) == n and len(windows) == n
    B = codes.shape[0] * num_decodings
    gaps = np.zeros((B, n), np.float64)
    for k, ws in enumerate(calls):
        _, _, _, t_rel = windows[k]
        ev, ch = (k % U) // nc, k % nc
        top2 = torch.topk(ws[ch][:, t_rel * epc + ev, :], 2, dim=-1)[0]
        gaps[:, k] = npy(top2[:, 0] - top2[:, 1])
    triples = np.array([windows[k * U][1:] for k in range(end - start)], np.int64)
    return tokens, gaps, triples


def gen_long(name, cfg, nb, start, end, num_decodings, first_seed):
    vocab = cfg['vocab']
    nc = len(vocab)
    for seed in range(first_seed, first_seed + 50):
        dec, _ = build_tiny(cfg, seed)
        dec.dataloader_generator = StubDataloaderGenerator(vocab)
        g = torch.Generator().manual_seed(seed + 7)
        ncodes = dec.source_embeddings.weight.shape[0]
        codes = torch.randint(0, ncodes, (cfg['B'], nb), generator=g)
        np.random.seed(seed)
        tokens, gaps, triples = reference_long(dec, codes, cfg, start, end, num_decodings)
        print(f'   seed {seed}: smallest top-1 / top-2 gap {gaps.min():.2e}')
        if gaps.min() > 1e-3:
            break
    assert gaps.min() > 1e-3
    epc = 16 // nc
    init = dec.init_generation_chorale(num_events=nb * epc, start_index=start * epc)
    n2i = dec.dataloader_generator.dataset.note2index_dicts
    arrays = sd_arrays('sd', dec)
    arrays.update(codes=npy(codes), tokens=tokens, gaps=gaps, windows=triples, init_chorale=npy(init.long()),
                  pad=np.array([d['XX'] for d in n2i], np.int64), start=np.array([d['START'] for d in n2i], np.int64),
                  end=np.array([d['END'] for d in n2i], np.int64), code_index_start=np.array(start),
                  code_index_end=np.array(end), num_decodings=np.array(num_decodings), cfg_json=np.array(json.dumps(cfg)),
                  seed=np.array(seed))
    save(name, **arrays)


if __name__ == '__main__':
    tiny = dict(emb=8, vocab=[11, 12, 13, 14], d=32, H=2, layers=[1, 1], ff=64, D=8, K=16, ncb=2, zdim=8, up_hidden=16,
                events=12, B=3, Kl=2, Kr=2, dec_emb=8, dec_d=32, dec_H=2, dec_enc_layers=2, dec_dec_layers=2, dec_ff=64, dec_pos=4,
                enc_attn='anticausal', cross_attn='anticausal')
    gen_long('generate_long_tiny_S4', dict(tiny, events=16, B=2), nb=10, start=2, end=8, num_decodings=2, first_seed=200)
    gen_long('generate_long_tiny_S3', dict(tiny, B=2), nb=7, start=1, end=7, num_decodings=1, first_seed=300)
