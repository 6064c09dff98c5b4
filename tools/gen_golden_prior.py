"""Golden vectors for the code prior (priors/prior_relative.py:17-353), produced by IMPORTING the reference
(container-only tool; reuses the stubs and the encoder builder of tools/gen_golden.py).  Fixtures hold tensors only.

  prior_tiny.npz            two tiny priors -- `v32/` (d 64, 4 heads, 2 layers, ff 64, N = 6, V = 1 x 32 codes) and `v1024/` (d 16,
                            1 head, 2 layers, N = 6, V = 32 ** 2 merged codes) -- each with its state dict (frozen encoder
                            included), codes (B, N), and the reference `forward`'s loss, logits and every parameter's
                            gradient in eval mode.  The model seed is the first for which no pre-ReLU activation of the
                            feed-forward layers sits within 1e-4 of zero (a ReLU that flips under fp32 rounding would move
                            whole gradient rows).
  prior_greedy_tiny.npz     the v32 model with its head scaled by 4 (peaked distributions), and the codes of the reference's
                            window rule (:327-353) driven by the reference's own `forward` with arg-max for num_tokens = 20
                            >= 3 N (head and sliding regimes), plus the top-1 / top-2 logit gap at every step.  The model
                            seed is the first whose smallest gap is > 1e-3.
  prior_temperature.npz     logit rows of widths 32, 1024 and 4096 and, for temperatures 0.5, 1 and 2, the reference's
                            exp(log(softmax + 1e-20) * temperature) renormalised (:341-347), in float64 from fp32 softmax.

Run:  python tools/gen_golden_prior.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import npy, save, sd_arrays, perturb_1d, build_encoder  # noqa: E402  (stubs, the reference on sys.path)

from VQCPCB.priors.prior_relative import PriorRelative  # noqa: E402

ENC = dict(emb=8, vocab=[11, 12, 13, 14], d=32, H=2, layers=[1, 1], ff=64, D=8, zdim=8, up_hidden=16, Kl=2, Kr=2)
V32 = dict(ENC, K=32, ncb=1, p_d=64, p_H=4, p_layers=2, p_ff=64, p_emb=8, N=6, B=3)
V1024 = dict(ENC, K=32, ncb=2, p_d=16, p_H=1, p_layers=2, p_ff=32, p_emb=4, N=6, B=3)


def build_prior(cfg, seed, head_gain=1.0):
    torch.manual_seed(seed)
    enc = build_encoder(cfg)
    perturb_1d(enc)
    prior = PriorRelative('/tmp/vqcpc_golden_prior', dataloader_generator=None, encoder=enc, d_model=cfg['p_d'],
                          num_layers=cfg['p_layers'], n_head=cfg['p_H'], dim_feedforward=cfg['p_ff'],
                          embedding_size=cfg['p_emb'], num_channels=1, num_events=cfg['N'], dropout=0.0)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in prior.named_parameters():
            if not k.startswith('encoder.') and p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        prior.pre_softmaxes[0].weight.mul_(head_gain)
    prior.eval()
    return prior, g


def gen_step(tag, cfg, first_seed):
    V = cfg['K'] ** cfg['ncb']
    for seed in range(first_seed, first_seed + 50):
        prior, g = build_prior(cfg, seed)
        codes = torch.randint(0, V, (cfg['B'], cfg['N']), generator=g)
        pre = []
        hooks = [lay.linear1.register_forward_hook(lambda m, i, o: pre.append(o.detach().abs().min().item()))
                 for lay in prior.transformer.layers]
        out = prior.forward(codes)
        for h in hooks:
            h.remove()
        print(f'   {tag} seed {seed}: smallest |pre-ReLU activation| {min(pre):.2e}')
        if min(pre) > 1e-4:
            break
    assert min(pre) > 1e-4
    out['loss'].backward()
    arrays = sd_arrays(f'{tag}/sd', prior)
    arrays.update({f'{tag}/grad/{k}': npy(p.grad) for k, p in prior.named_parameters() if not k.startswith('encoder.')})
    assert all(p.grad is None for k, p in prior.named_parameters() if k.startswith('encoder.'))
    arrays.update({f'{tag}/codes': npy(codes), f'{tag}/loss': npy(out['loss']),
                   f'{tag}/logits': npy(out['weights_per_category'][0]), f'{tag}/cfg_json': np.array(json.dumps(cfg)),
                   f'{tag}/seed': np.array(seed)})
    return arrays


def reference_greedy(prior, num_tokens, B):
    """Code e is the arg-max of the reference `forward`'s logits at row e - w of the window [w, w + N), w = max(0, e - N + 1):
    the window rule of PriorRelative.generate (:327-343) with the draw replaced by arg-max."""
    N = prior.num_tokens
    seq = torch.zeros(B, num_tokens, dtype=torch.long)
    gaps = np.zeros((B, num_tokens), np.float64)
    with torch.no_grad():
        for e in range(num_tokens):
            w = max(0, e - N + 1)
            logits = prior.forward(seq[:, w:w + N])['weights_per_category'][0][:, e - w, :]
            best = torch.topk(logits, 2, dim=-1)
            gaps[:, e] = npy(best.values[:, 0] - best.values[:, 1])
            seq[:, e] = best.indices[:, 0]
    return seq, gaps


def gen_greedy(name, cfg, num_tokens=20, B=3, first_seed=300):
    # every row of the reference's loop starts from the same all-zero sequence and arg-max is deterministic, so its rows are
    # equal: one row is computed and stored B times (the test's rows must all reproduce it)
    for seed in range(first_seed, first_seed + 50):
        prior, _ = build_prior(cfg, seed, head_gain=4.0)
        codes, gaps = reference_greedy(prior, num_tokens, 1)
        print(f'   seed {seed}: smallest top-1 / top-2 gap {gaps.min():.2e}, {len(np.unique(npy(codes)))} distinct codes')
        if gaps.min() > 1e-3 and len(np.unique(npy(codes))) >= 4:
            break
    assert gaps.min() > 1e-3
    arrays = sd_arrays('sd', prior)
    arrays.update(codes=npy(codes.repeat(B, 1)), gaps=gaps, cfg_json=np.array(json.dumps(cfg)), seed=np.array(seed),
                  num_tokens=np.array(num_tokens))
    save(name, **arrays)


def gen_temperature(name, seed=70):
    g = np.random.default_rng(seed)
    temps = np.array([0.5, 1.0, 2.0], np.float32)
    arrays = dict(temperature=temps)
    for V in (32, 1024, 4096):
        logits = (g.standard_normal((4, V)) * g.uniform(0.5, 3.0, size=(4, 1))).astype(np.float32)
        probs = np.zeros((len(temps), 4, V), np.float64)
        for i, temp in enumerate(temps):
            p = npy(torch.softmax(torch.from_numpy(logits), dim=1)).astype(np.float64)       # :341-343
            p = np.exp(np.log(p + 1e-20) * float(temp))                                      # :346
            probs[i] = p / p.sum(axis=1, keepdims=True)                                      # :347
        arrays[f'logits_{V}'] = logits
        arrays[f'probs_{V}'] = probs
    save(name, **arrays)


if __name__ == '__main__':
    np.random.seed(0)
    tiny = {}
    tiny.update(gen_step('v32', V32, first_seed=200))
    tiny.update(gen_step('v1024', V1024, first_seed=250))
    save('prior_tiny', **tiny)
    gen_greedy('prior_greedy_tiny', V32)
    gen_temperature('prior_temperature')
