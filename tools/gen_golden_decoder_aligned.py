"""Golden vectors for the aligned ('diagonal') decoder block and the F-F-C decoder, produced by IMPORTING the reference
(container-only tool; reuses the stubs of tools/gen_golden.py and the builders of tools/gen_golden_decoder.py,
tools/gen_golden_generate.py and tools/gen_golden_generate_long.py, none of which is edited).  Fixtures hold tensors plus
cfg_json only.

  decoder_layer_aligned_S3_T48.npz     one TransformerAlignedDecoderLayerCustom (transformer_custom.py:389-492), n = 3: inputs,
                                       y, a_self, upstream gradient, d_tgt, d_mem, parameter gradients, state dict, and the
                                       intermediates C = cross_attn(memory rows) (S, n, d * nc) and the expanded tgt2 (T, n, d).
  decoder_tiny_diagonal.npz            gen_decoder_step with cross_attn = 'diagonal' (no a_cross: the layer returns None)
  decoder_tiny_full.npz                gen_decoder_step with enc_attn = 'full', cross_attn = 'full'
  generate_greedy_tiny_diagonal.npz    the reference's greedy generate loop on the diagonal tiny decoder
  generate_long_tiny_S3_diagonal.npz   the reference's generate_from_code_long on it (nb = 7, codes 1 .. 7)

Run:  python tools/gen_golden_decoder_aligned.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_decoder as gd  # noqa: E402  (stubs, the reference on sys.path, decoder builders)
from gen_golden import npy, save, sd_arrays, perturb_1d  # noqa: E402
from gen_golden_generate import gen_greedy  # noqa: E402
from gen_golden_generate_long import gen_long  # noqa: E402

from VQCPCB.transformer.transformer_custom import TransformerAlignedDecoderLayerCustom  # noqa: E402


def gen_decoder_layer_aligned(name, n, H, S, T, d, ff, seed, nc=4):
    torch.manual_seed(seed)
    layer = TransformerAlignedDecoderLayerCustom(d_model=d, nhead=H, attention_bias_type_self='relative_attention',
                                                 attention_bias_type_cross=None, num_channels_encoder=1, num_events_encoder=S,
                                                 num_channels_decoder=nc, num_events_decoder=T // nc, dim_feedforward=ff,
                                                 dropout=0.0)
    perturb_1d(layer)
    layer.eval()
    tgt = torch.randn(T, n, d, requires_grad=True)
    mem = torch.randn(S, n, d, requires_grad=True)
    sub = torch.triu(torch.ones(T, T)).t()
    tgt_mask = torch.zeros(T, T).masked_fill(sub == 0, float('-inf'))
    seen = {}
    h1 = layer.cross_attn.register_forward_hook(lambda m, i, o: seen.__setitem__('C', o.detach().clone()))
    h2 = layer.dropout2.register_forward_hook(lambda m, i, o: seen.__setitem__('tgt2', i[0].detach().clone()))
    y, att = layer(tgt, mem, tgt_mask=tgt_mask, memory_mask=None)
    h1.remove()
    h2.remove()
    assert att['a_cross'] is None
    g = torch.randn_like(y)
    (y * g).sum().backward()
    arrays = sd_arrays('sd', layer)
    arrays.update({f'grad/{k}': npy(p.grad) for k, p in layer.named_parameters()})
    save(name, tgt=npy(tgt), mem=npy(mem), y=npy(y), a_self=npy(att['a_self_decoder']), g=npy(g), d_tgt=npy(tgt.grad),
         d_mem=npy(mem.grad), tgt_mask=npy(tgt_mask), C=npy(seen['C']), tgt2=npy(seen['tgt2']), H=np.array(H),
         nc=np.array(nc), **arrays)


_ABSENT = object()


def gen_decoder_step_no_cross(name, cfg, seed):
    """gen_golden_decoder.gen_decoder_step as it is; the aligned layer's a_cross is None, so that one entry is left out."""
    npy0, save0 = gd.npy, gd.save
    gd.npy = lambda t: _ABSENT if t is None else npy0(t)
    gd.save = lambda nm, **arrays: save0(nm, **{k: v for k, v in arrays.items() if v is not _ABSENT})
    try:
        gd.gen_decoder_step(name, cfg, seed=seed)
    finally:
        gd.npy, gd.save = npy0, save0


if __name__ == '__main__':
    np.random.seed(0)
    gen_decoder_layer_aligned('decoder_layer_aligned_S3_T48', n=3, H=2, S=3, T=48, d=32, ff=64, seed=74)
    tiny = dict(emb=8, vocab=[11, 12, 13, 14], d=32, H=2, layers=[1, 1], ff=64, D=8, K=16, ncb=2, zdim=8, up_hidden=16,
                events=12, B=3, Kl=2, Kr=2, dec_emb=8, dec_d=32, dec_H=2, dec_enc_layers=2, dec_dec_layers=2, dec_ff=64, dec_pos=4,
                enc_attn='anticausal', cross_attn='anticausal')
    diag = dict(tiny, cross_attn='diagonal')
    gen_decoder_step_no_cross('decoder_tiny_diagonal', dict(diag, B=2), seed=83)   # B = 2 as decoder_tiny_fullcross: < 1 MiB
    gd.gen_decoder_step('decoder_tiny_full', dict(tiny, enc_attn='full', cross_attn='full'), seed=84)
    gen_greedy('generate_greedy_tiny_diagonal', diag, first_seed=400)
    gen_long('generate_long_tiny_S3_diagonal', dict(diag, B=2), nb=7, start=1, end=7, num_decodings=1, first_seed=500)
