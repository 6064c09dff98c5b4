"""Builders shared by the tests of the decoder on continuous latents (a NoQuantization encoder without upscaler)."""
import json
import types

import torch

from conftest import load_golden, sub_state
from oracle import decoder_oracle as D


def build_continuous_decoder(cfg, sd, lr=1e-3, dropout=0.0, upscaler=False):
    """tests/test_decoder_gpu.py:build_decoder with the quantiser replaced by NoQuantization(codebook_dim = D) and no upscaler
    (upscaler=True keeps one: the combination the decoder refuses)."""
    from vqcpc_bach_amd import hip
    from vqcpc_bach_amd.data_processor.bach_cpc_data_processor import BachCPCDataProcessor
    from vqcpc_bach_amd.data_processor.bach_data_processor import BachDataProcessor
    from vqcpc_bach_amd.decoders.decoder import Decoder
    from vqcpc_bach_amd.downscalers.relative_transformer_downscaler import RelativeTransformerDownscaler
    from vqcpc_bach_amd.encoder import Encoder
    from vqcpc_bach_amd.quantizer.vector_quantizer import NoQuantization
    from vqcpc_bach_amd.upscalers.mlp_upscaler import MlpUpscaler
    hip.load()
    nc = len(cfg['vocab'])
    edp = BachCPCDataProcessor(embedding_size=cfg['emb'], num_events=(cfg['Kl'] + cfg['Kr']) * 4, num_channels=nc,
                               num_tokens_per_channel=cfg['vocab'], num_tokens_per_block=16)
    ds = RelativeTransformerDownscaler(input_dim=cfg['emb'], output_dim=cfg['D'], num_channels=nc, downscale_factors=[4, 4],
                                       d_model=cfg['d'], n_head=cfg['H'], list_of_num_layers=cfg['layers'],
                                       dim_feedforward=cfg['ff'], dropout=0.0)
    up = MlpUpscaler(input_dim=cfg['D'], output_dim=cfg['zdim'], hidden_size=cfg['up_hidden'], dropout=0.0) if upscaler else None
    enc = Encoder('/tmp/vqcpc_test_decoder_continuous', edp, ds, NoQuantization(codebook_dim=cfg['D']), up)
    dp = BachDataProcessor(embedding_size=cfg['dec_emb'], num_events=cfg['events'], num_tokens_per_channel=cfg['vocab'])
    S = cfg['events'] * nc // 16
    dec = Decoder(model_dir='/tmp/vqcpc_test_decoder_continuous', dataloader_generator=None, data_processor=dp, encoder=enc,
                  transformer_type='relative', encoder_attention_type=cfg['enc_attn'],
                  cross_attention_type=cfg['cross_attn'], d_model=cfg['dec_d'], num_encoder_layers=cfg['dec_enc_layers'],
                  num_decoder_layers=cfg['dec_dec_layers'], n_head=cfg['dec_H'], dim_feedforward=cfg['dec_ff'],
                  positional_embedding_size=cfg['dec_pos'], num_channels_encoder=1, num_events_encoder=S,
                  num_channels_decoder=nc, num_events_decoder=cfg['events'], dropout=dropout)
    if sd is not None:
        assert set(dec.state_dict()) == set(sd), 'state_dict keys must be the reference\'s'
        dec.load_state_dict(sd, strict=True)
    dec.cuda()
    dec.init_optimizers(lr=lr, schedule_lr=False)
    assert dec.flat.check_views()
    return dec


def golden_continuous_decoder(name, **kw):
    g = load_golden(name)
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    prefix = 'sd0' if any(k.startswith('sd0/') for k in g) else 'sd'
    return build_continuous_decoder(cfg, sub_state(g, prefix), **kw), cfg, g


def stub_dataset(g):
    return types.SimpleNamespace(dataset=types.SimpleNamespace(
        note2index_dicts=[{'START': int(s), 'END': int(e), 'XX': int(p)} for s, e, p in zip(g['start'], g['end'], g['pad'])]))


def random_inputs(dec, B, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, dec.num_tokens_source, dec.source_dim, generator=g)
    x = torch.cat([torch.randint(0, v, (B, dec.num_tokens_target // dec.num_channels, 1), generator=g)
                   for v in dec.num_tokens_per_channel], dim=2)
    return z.cuda(), x.cuda()
