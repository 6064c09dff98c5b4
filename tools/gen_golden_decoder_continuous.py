"""Golden vectors for the decoder on CONTINUOUS latents (a `NoQuantization` encoder without upscaler; reference
decoders/decoder.py:222-229, :327-336, :595-600), produced by IMPORTING the reference (container-only tool; reuses the stubs
of tools/gen_golden.py and the decoder / dataset builders of tools/gen_golden_decoder.py, tools/gen_golden_generate.py and
tools/gen_golden_generate_long.py, none of which is edited).  Fixtures hold tensors plus cfg_json only.

  decoder_tiny_continuous.npz                      the reference's `Decoder.epoch` (eval + one training step) on the tiny
                                                   shape of decoder_tiny, cross attention anticausal, B = 2, latents of
                                                   dimension dz = 8: state dict before / after, x, the encoder's z, losses,
                                                   per-voice logits, every parameter gradient (before clipping).
  decoder_tiny_continuous_diagonal.npz             the same with cross_attn = 'diagonal' (the reference's own pairing:
                                                   decoder_relative_AC_D_C_*_noQuantization.py)
  generate_greedy_tiny_continuous_diagonal.npz     the reference's greedy generate loop on the latents of B = 3 sequences
  generate_long_tiny_S3_continuous_diagonal.npz    the reference's generate_from_code_long on (2, 7, dz) latents, codes 1 .. 7

The reference needs no shim here: `epoch` hands z_quantized (B, S, dz) to `forward` when encoding_indices is None.  For the
two generation fixtures the model seed advances from `first_seed` until every greedy decision of the reference has a
top-1 / top-2 logit gap >= 1e-3; the fixture records the seed and the gaps.

Run:  python tools/gen_golden_decoder_continuous.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_decoder as gd  # noqa: E402  (stubs, the reference on sys.path, decoder builders)
from gen_golden import npy, save, sd_arrays, perturb_1d, build_encoder  # noqa: E402
from gen_golden_generate import reference_greedy  # noqa: E402
from gen_golden_generate_long import StubDataloaderGenerator, reference_long  # noqa: E402

from VQCPCB.quantizer.vector_quantizer import NoQuantization  # noqa: E402

GAP = 1e-3


def build_continuous(cfg, seed, logit_gain=1.0):
    """The seeded tiny model of gen_golden_decoder.gen_decoder_step / gen_golden_generate.build_tiny with the quantiser
    replaced by NoQuantization(codebook_dim = D) and no upscaler -> (decoder, generator for the inputs)."""
    torch.manual_seed(seed)
    enc = build_encoder(cfg)
    enc.quantizer = NoQuantization(codebook_dim=cfg['D'])
    enc.upscaler = None
    perturb_1d(enc)
    g = torch.Generator().manual_seed(seed + 1)
    dec = gd.build_decoder(cfg, enc)
    assert isinstance(dec.source_embeddings, torch.nn.Linear)
    with torch.no_grad():
        for k, p in dec.named_parameters():
            if not k.startswith('encoder.') and p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for m in dec.pre_softmaxes:
            m.weight.mul_(logit_gain)
    return dec, g


def random_tokens(cfg, g):
    return torch.cat([torch.randint(0, nv, (cfg['B'], cfg['events'], 1), generator=g) for nv in cfg['vocab']], dim=2)


def gen_decoder_step(name, cfg, seed, lr=1e-3):
    dec, g = build_continuous(cfg, seed)
    enc = dec.encoder
    x = random_tokens(cfg, g)
    dec.init_optimizers(lr=lr, schedule_lr=False)
    arrays = sd_arrays('sd0', dec)
    assert 'sd0/source_embeddings.bias' in arrays and arrays['sd0/source_embeddings.weight'].shape == (cfg['dec_d'], cfg['D'])
    arrays['batch/x'] = npy(x)
    enc.eval()
    with torch.no_grad():
        z, idx, _ = enc(x)
    assert idx is None
    arrays['z'] = npy(z)

    ev = dec.epoch(iter([{'x': x}]), train=False, num_batches=1)
    arrays['eval/loss'] = np.asarray(ev['loss'], dtype=np.float64)
    dec.eval()
    with torch.no_grad():
        fp = dec.forward(z, x)
    for c, w in enumerate(fp['weights_per_category']):
        arrays[f'eval_fwd/logits.{c}'] = npy(w)

    pre_clip = {}
    orig_clip = torch.nn.utils.clip_grad_norm_
    names = {id(p): n for n, p in dec.named_parameters()}

    def spy(parameters, max_norm, *a, **k):
        params = list(parameters)
        for p in params:
            if p.grad is not None:
                pre_clip[names[id(p)]] = p.grad.detach().clone()
        return orig_clip(params, max_norm, *a, **k)

    torch.nn.utils.clip_grad_norm_ = spy
    try:
        trn = dec.epoch(iter([{'x': x}]), train=True, num_batches=1)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
    arrays['train/loss'] = np.asarray(trn['loss'], dtype=np.float64)
    for k, gr in pre_clip.items():
        arrays[f'grad/{k}'] = npy(gr)
    total = torch.sqrt(sum((gr.double() ** 2).sum() for gr in pre_clip.values()))
    arrays['grad_total_norm'] = np.asarray(float(total))
    arrays.update(sd_arrays('sd1', dec))
    arrays['cfg_json'] = np.array(json.dumps(cfg))
    arrays['lr'] = np.array(lr)
    save(name, **arrays)
    print(f'   eval loss {ev["loss"]:.6f}  train loss {trn["loss"]:.6f}  grad norm {float(total):.4f}  frozen encoder grads: '
          f'{sum(k.startswith("encoder.") for k in pre_clip)}')


def gen_greedy(name, cfg, first_seed):
    for seed in range(first_seed, first_seed + 50):
        dec, g = build_continuous(cfg, seed, logit_gain=4.0)
        x = random_tokens(cfg, g)
        dec.eval()
        with torch.no_grad():
            z, _, _ = dec.encoder(x)
        tokens, gaps = reference_greedy(dec, z, cfg['events'], len(cfg['vocab']), cfg['vocab'])
        print(f'   seed {seed}: smallest top-1 / top-2 gap {gaps.min():.2e}')
        if gaps.min() >= GAP:
            break
    assert gaps.min() >= GAP
    arrays = sd_arrays('sd', dec)
    arrays.update(x=npy(x), codes=npy(z), tokens=npy(tokens), gaps=gaps, min_gap=np.array(gaps.min()),
                  cfg_json=np.array(json.dumps(cfg)), seed=np.array(seed))
    save(name, **arrays)


def gen_long(name, cfg, nb, start, end, num_decodings, first_seed):
    vocab = cfg['vocab']
    nc = len(vocab)
    for seed in range(first_seed, first_seed + 50):
        dec, _ = build_continuous(cfg, seed, logit_gain=4.0)
        dec.dataloader_generator = StubDataloaderGenerator(vocab)
        g = torch.Generator().manual_seed(seed + 7)
        # latents of nb codes: the encoder's own outputs on random tokens (16 tokens = 4 events per code)
        xs = torch.cat([torch.randint(0, nv, (cfg['B'], nb * 16 // nc, 1), generator=g) for nv in vocab], dim=2)
        dec.eval()
        with torch.no_grad():
            codes, _, _ = dec.encoder(xs)
        assert codes.shape == (cfg['B'], nb, cfg['D'])
        np.random.seed(seed)
        tokens, gaps, triples = reference_long(dec, codes, cfg, start, end, num_decodings)
        print(f'   seed {seed}: smallest top-1 / top-2 gap {gaps.min():.2e}')
        if gaps.min() >= GAP:
            break
    assert gaps.min() >= GAP
    epc = 16 // nc
    init = dec.init_generation_chorale(num_events=nb * epc, start_index=start * epc)
    n2i = dec.dataloader_generator.dataset.note2index_dicts
    arrays = sd_arrays('sd', dec)
    arrays.update(codes=npy(codes), tokens=tokens, gaps=gaps, min_gap=np.array(gaps.min()), windows=triples,
                  init_chorale=npy(init.long()), pad=np.array([d['XX'] for d in n2i], np.int64),
                  start=np.array([d['START'] for d in n2i], np.int64), end=np.array([d['END'] for d in n2i], np.int64),
                  code_index_start=np.array(start), code_index_end=np.array(end), num_decodings=np.array(num_decodings),
                  cfg_json=np.array(json.dumps(cfg)), seed=np.array(seed))
    save(name, **arrays)


if __name__ == '__main__':
    np.random.seed(0)
    tiny = dict(emb=8, vocab=[11, 12, 13, 14], d=32, H=2, layers=[1, 1], ff=64, D=8, K=16, ncb=2, zdim=8, up_hidden=16,
                events=12, B=2, Kl=2, Kr=2, dec_emb=8, dec_d=32, dec_H=2, dec_enc_layers=2, dec_dec_layers=2, dec_ff=64, dec_pos=4,
                enc_attn='anticausal', cross_attn='anticausal', quantizer=None)
    diag = dict(tiny, cross_attn='diagonal')
    gen_decoder_step('decoder_tiny_continuous', tiny, seed=85)
    gen_decoder_step('decoder_tiny_continuous_diagonal', diag, seed=86)
    gen_greedy('generate_greedy_tiny_continuous_diagonal', dict(diag, B=3), first_seed=600)
    gen_long('generate_long_tiny_S3_continuous_diagonal', diag, nb=7, start=1, end=7, num_decodings=1, first_seed=700)
