"""Golden vectors for the attention maps of decoder generation (decoders/decoder.py:647-667: the rows the reference's
`plot_attentions` block keeps for every emitted token), produced by IMPORTING the reference (container-only tool; reuses the
stubs of tools/gen_golden.py and `build_tiny` of tools/gen_golden_generate.py, neither of which is edited).  Fixtures hold
arrays only: the models are those of the committed greedy fixtures, rebuilt from the seed stored there, and the tests load
their state dicts from those.

  generate_attentions_tiny.npz            the model of generate_greedy_tiny.npz (T = 48, S = 3, B = 3, two layers, two heads)
  generate_attentions_tiny_diagonal.npz   the model of generate_greedy_tiny_diagonal.npz (no a_cross: the layer returns None)

Per fixture, from the reference's greedy generate loop (:596-667; the loop must reproduce the committed tokens), for EVERY
layer l where the reference's block takes its hard-coded `layer = 2`:
  self_attns_decoder  (B, layers, H, T, T)      attentions_decoder[l]['a_self_decoder'][:, :, t, :] at the step that emits t
  attns_cross         (B, layers, H, T, S)      attentions_decoder[l]['a_cross'][:, :, t, :]
  self_attns_encoder  (B, enc layers, H, T, S)  attentions_encoder[l]['a_self_encoder'][:, :, (event * nc) // U, :]
  tokens              the loop's tokens (equal to the greedy fixture's)

Run:  python tools/gen_golden_generate_attentions.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_decoder as gd  # noqa: E402,F401  (stubs, the reference on sys.path, decoder builders)
from gen_golden import OUT, npy, save  # noqa: E402
from gen_golden_generate import build_tiny  # noqa: E402

from VQCPCB.utils import top_k_top_p_filtering  # noqa: E402


def greedy_with_attentions(dec, codes, events, nc, vocab):
    """The loop of Decoder.generate (:596-667) with temperature 1, top_k = 1 and its plot_attentions block taken at every layer."""
    B = codes.shape[0]
    U = dec.total_upscaling
    x = dec.init_generation(num_events=events).repeat(B, 1, 1)
    self_dec, cross, self_enc = [], [], []
    with torch.no_grad():
        for event_index in range(events):
            for channel_index in range(nc):
                forward_pass = dec.forward(codes, x)
                logits = forward_pass['weights_per_category'][channel_index][:, event_index, :] / 1.0
                filtered = torch.stack([top_k_top_p_filtering(lg, top_k=1, top_p=1.0) for lg in logits], dim=0)
                p = npy(torch.softmax(filtered, dim=-1))
                for b in range(B):
                    x[b, event_index, channel_index] = int(np.random.choice(np.arange(vocab[channel_index]), p=p[b]))
                event_index_encoder = (event_index * nc) // U
                t = event_index * nc + channel_index
                att_enc, att_dec = forward_pass['attentions_encoder'], forward_pass['attentions_decoder']
                self_enc.append(np.stack([npy(a['a_self_encoder'][:, :, event_index_encoder, :]) for a in att_enc], axis=1))
                self_dec.append(np.stack([npy(a['a_self_decoder'][:, :, t, :]) for a in att_dec], axis=1))
                if att_dec[0]['a_cross'] is not None:
                    cross.append(np.stack([npy(a['a_cross'][:, :, t, :]) for a in att_dec], axis=1))
    # per step (B, layers, H, keys) -> (B, layers, H, T, keys)
    out = dict(self_attns_decoder=np.stack(self_dec, axis=3), self_attns_encoder=np.stack(self_enc, axis=3))
    if cross:
        out['attns_cross'] = np.stack(cross, axis=3)
    return x, {k: v.astype(np.float32) for k, v in out.items()}


def gen_attentions(name, greedy_name):
    g = np.load(os.path.join(OUT, greedy_name + '.npz'), allow_pickle=False)
    cfg = json.loads(str(g['cfg_json']))
    dec, codes = build_tiny(cfg, int(g['seed']))
    assert np.array_equal(npy(codes), g['codes']), 'the rebuilt model is not the greedy fixture\'s'
    for k, v in dec.state_dict().items():
        assert np.array_equal(npy(v), g[f'sd/{k}']), k
    tokens, maps = greedy_with_attentions(dec, codes, cfg['events'], len(cfg['vocab']), cfg['vocab'])
    assert np.array_equal(npy(tokens), g['tokens']), 'the reference\'s greedy loop does not reproduce the committed tokens'
    save(name, tokens=npy(tokens), greedy_fixture=np.array(greedy_name), **maps)
    assert os.path.getsize(os.path.join(OUT, name + '.npz')) < 512 * 1024


if __name__ == '__main__':
    np.random.seed(0)
    gen_attentions('generate_attentions_tiny', 'generate_greedy_tiny')
    gen_attentions('generate_attentions_tiny_diagonal', 'generate_greedy_tiny_diagonal')
