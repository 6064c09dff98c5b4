"""Golden vectors of the GRU block downscaler, produced by IMPORTING the reference (container-only tool, like
tools/gen_golden.py, whose stubs and helpers it reuses; it copies no source text).

    lstm_downscaler_tiny.npz   LstmDownscaler emb 8, hidden 64, 2 layers, bidirectional, L = 16, 4 voices (unequal
                               vocabularies), D = 3 on 3 x 5 blocks: tokens, parameters, z, a cotangent, the gradients of the
                               18 downscaler tensors and of the 4 embedding tables
    lstm_downscaler_h24.npz    the same with hidden 24, 1 layer, unidirectional
    epoch_tiny_lstm.npz        VQCPCEncoderTrainer.epoch with LstmDownscaler on one seeded batch: the fields of epoch_tiny.npz
                               plus the per-window margins f_pos - max f_neg and the quantiser's top-2 distance gaps (both taken
                               from the reference's own modules while its eval epoch runs)

The epoch fixture's seed is the first one for which, on the reference alone,
  * the smallest top-2 gap is at least 1e-3 of the largest distance (10 x what a z within 5e-5 can move a distance), and
  * at most a quarter of the windows of any prediction step have |margin| < 1e-5;
both values are printed.

Run:  python tools/gen_golden_lstm.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the music21 / tensorboard stubs, puts the reference on sys.path)

from VQCPCB.data_processor.bach_cpc_data_processor import BachCPCDataProcessor  # noqa: E402
from VQCPCB.downscalers.lstm_downscaler import LstmDownscaler  # noqa: E402
from VQCPCB.encoder import Encoder  # noqa: E402
from VQCPCB.quantizer.vector_quantizer import ProductVectorQuantizer  # noqa: E402
from VQCPCB.upscalers.mlp_upscaler import MlpUpscaler  # noqa: E402

npy = G.npy
VOCAB = [5, 9, 3, 7]          # tokens per voice WITHOUT the mask token the data processor adds: tables of 6, 10, 4, 8 rows


def gen_downscaler(name, emb, hidden, layers, bidirectional, seed, R=(3, 5), L=16, D=3):
    torch.manual_seed(seed)
    dp = BachCPCDataProcessor(embedding_size=emb, num_events=R[1] * L // 4, num_channels=4, num_tokens_per_channel=VOCAB,
                              num_tokens_per_block=L)
    ds = LstmDownscaler(input_dim=emb, output_dim=D, num_channels=4, downscale_factors=[L], hidden_size=hidden,
                        num_layers=layers, dropout=0.0, bidirectional=bidirectional)
    ds.eval()
    gen = torch.Generator().manual_seed(seed + 1)
    limits = torch.tensor([v + 1 for v in VOCAB]).repeat(L // 4)                   # position p belongs to voice p % 4
    tokens = (torch.rand(R[0], R[1], L, generator=gen) * limits).long().clamp_(max=limits - 1)
    tokens[0, 0] = 0                                                                # token 0 and the last valid token of every voice
    tokens[0, 1] = limits - 1
    x = dp.embed(tokens)                                                            # (3, 5, 16, emb)
    z = ds(x.view(R[0], R[1] * L, emb))
    g_z = torch.randn(z.shape, generator=gen)
    (z * g_z).sum().backward()
    arrays = G.sd_arrays('sd', ds)
    arrays.update({f'grad/{k}': npy(p.grad) for k, p in ds.named_parameters()})
    arrays.update({f'emb/{c}': npy(e.weight) for c, e in enumerate(dp.embeddings)})
    arrays.update({f'grad_emb/{c}': npy(e.weight.grad) for c, e in enumerate(dp.embeddings)})
    cfg = dict(emb=emb, hidden=hidden, layers=layers, bidirectional=bidirectional, L=L, D=D, vocab=VOCAB)
    G.save(name, tokens=npy(tokens), z=npy(z), g_z=npy(g_z), cfg_json=np.array(json.dumps(cfg)), **arrays)


def build_lstm_encoder(cfg):
    dp = BachCPCDataProcessor(embedding_size=cfg['emb'], num_events=(cfg['Kl'] + cfg['Kr']) * 4, num_channels=4,
                              num_tokens_per_channel=cfg['vocab'], num_tokens_per_block=16)
    ds = LstmDownscaler(input_dim=cfg['emb'], output_dim=cfg['D'], num_channels=4, downscale_factors=[16],
                        hidden_size=cfg['hidden'], num_layers=cfg['layers'], dropout=0.0, bidirectional=cfg['ds_bidirectional'])
    q = ProductVectorQuantizer(codebook_size=cfg['K'], codebook_dim=cfg['D'], commitment_cost=0.25,
                               num_codebooks=cfg['ncb'], use_batch_norm=False, initialize=False, squared_l2_norm=True)
    up = MlpUpscaler(input_dim=cfg['D'], output_dim=cfg['zdim'], hidden_size=cfg['up_hidden'], dropout=0.0)
    return Encoder('/tmp/vqcpc_golden_model', dp, ds, q, up)


class _Probe:
    """Taps on the reference's own modules during the eval epoch: the scores of FksModule (calls in the order of
    VQCPCEncoderTrainer.epoch: positives, negatives; a forward hook) and the inputs of the quantiser (Encoder calls
    `quantizer.forward` directly, which no hook sees: the bound method is wrapped for the duration)."""

    def __init__(self):
        self.fks, self.zs, self.handles, self.trainer = [], [], [], None

    def attach(self, tr):
        self.trainer = tr
        self.handles = [tr.fks_module.register_forward_hook(lambda m, i, o: self.fks.append(o.detach().clone()))]
        q = tr.encoder.quantizer
        real = q.forward

        def forward(z, *a, **k):
            self.zs.append(z.detach().clone())
            return real(z, *a, **k)
        q.forward = forward

    def detach(self):
        for h in self.handles:
            h.remove()
        self.handles = []
        if self.trainer is not None:
            self.trainer.encoder.quantizer.__dict__.pop('forward', None)

    def margins(self, B, N, K):
        f_pos, f_neg = self.fks[0], self.fks[1].view(N, B, K).permute(1, 2, 0)
        return f_pos - f_neg.max(2)[0]                                              # (B, K)

    def gaps(self):
        q = self.trainer.encoder.quantizer
        gaps, dmax = [], 0.0
        for z in self.zs:
            for xc, e in zip(z.reshape(-1, z.shape[-1]).chunk(len(q.embeddings), dim=1), q.embeddings):
                d = ((xc.unsqueeze(1) - e.detach().unsqueeze(0)) ** 2).sum(2)
                top2 = torch.topk(d, 2, dim=1, largest=False)[0]
                gaps.append(top2[:, 1] - top2[:, 0])
                dmax = max(dmax, float(d.max()))
        return torch.cat(gaps), dmax


def gen_epoch(name, cfg, seeds):
    """tools/gen_golden.py's gen_encoder_and_epoch with the LSTM encoder; the first seed that meets both conditions is kept."""
    captured, probe = {}, _Probe()
    real_save, real_build, real_trainer = G.save, G.build_encoder, G.VQCPCEncoderTrainer

    def trainer_spy(*a, **k):
        tr = real_trainer(*a, **k)
        real_epoch = tr.epoch

        def epoch(loader, train, **kw):
            if not train:
                probe.attach(tr)
            try:
                return real_epoch(loader, train=train, **kw)
            finally:
                probe.detach()
        tr.epoch = epoch
        return tr

    G.save = lambda n, **arrays: captured.update(arrays)
    G.build_encoder, G.VQCPCEncoderTrainer = build_lstm_encoder, trainer_spy
    try:
        for seed in seeds:
            captured.clear()
            probe.fks, probe.zs = [], []
            G.gen_encoder_and_epoch(name, cfg, seed)
            margin = probe.margins(cfg['B'], cfg['N'], cfg['Kr'])
            gaps, dmax = probe.gaps()
            rel_gap = float(gaps.min()) / dmax
            near = float((margin.abs() < 1e-5).float().mean(0).max())
            print(f'seed {seed}: smallest top-2 gap / largest distance = {rel_gap:.3e} (need >= 1e-3), '
                  f'largest per-step fraction of |margin| < 1e-5 = {near:.3f} (need <= 0.25)')
            if rel_gap >= 1e-3 and near <= 0.25:
                break
        else:
            raise SystemExit('no seed met the conditions')
    finally:
        G.save, G.build_encoder, G.VQCPCEncoderTrainer = real_save, real_build, real_trainer
    captured.update(margin=npy(margin), top2_gap=npy(gaps), dist_max=np.array(dmax), seed=np.array(seed))
    G.save(name, **captured)


if __name__ == '__main__':
    gen_downscaler('lstm_downscaler_tiny', emb=8, hidden=64, layers=2, bidirectional=True, seed=60)
    gen_downscaler('lstm_downscaler_h24', emb=8, hidden=24, layers=1, bidirectional=False, seed=61)
    tiny = dict(emb=8, vocab=[11, 11, 11, 11], hidden=64, layers=2, ds_bidirectional=True, D=3, K=8, ncb=1, zdim=8,
                up_hidden=16, cdim=8, gru_hidden=16, B=6, N=3, Kl=2, Kr=2)
    gen_epoch('epoch_tiny_lstm', tiny, seeds=range(70, 90))
