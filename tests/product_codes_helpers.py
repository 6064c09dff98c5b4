"""Tiny product-quantised encoders with a decoder or a prior on top, for the product-code tests
(tests/test_product_codes_reference_cpu.py, tests/test_decoder_product_gpu.py, tests/test_prior_product_gpu.py): the models of
tests/test_decoder_gpu.build_decoder with a choice of decoder type and of `source_embedding`, the merged twin of a 'product'
decoder, the priors of tests/test_prior_cpu.build_prior with a choice of `code_model`, and the oracle's causal stack for the
prior's float64 reference."""
import types

import torch

from oracle import decoder_oracle as D

KINDS = {'AC-AC': ('anticausal', 'anticausal'), 'AC-F': ('anticausal', 'full'), 'F-F': ('full', 'full'),
         'AC-D': ('anticausal', 'diagonal')}


def tiny_cfg(K, ncb, **over):
    """16 events x 4 voices = 64 target tokens = 4 codes of `ncb` digits of `K` values."""
    cfg = dict(vocab=[12, 12, 12, 12], emb=16, d=32, H=2, layers=[1, 1], ff=64, D=4 * ncb, K=K, ncb=ncb, zdim=8, up_hidden=16,
               Kl=2, Kr=2, events=16, B=3, dec_emb=16, dec_d=64, dec_H=2, dec_enc_layers=1, dec_dec_layers=2, dec_ff=128)
    cfg.update(over)
    return D.make_cfg(**cfg)


def build_encoder(cfg, quantizer=None, model_dir='/tmp/vqcpc_test_product'):
    from vqcpc_bach_amd.data_processor.bach_cpc_data_processor import BachCPCDataProcessor
    from vqcpc_bach_amd.downscalers.relative_transformer_downscaler import RelativeTransformerDownscaler
    from vqcpc_bach_amd.encoder import Encoder
    from vqcpc_bach_amd.quantizer.vector_quantizer import ProductVectorQuantizer
    from vqcpc_bach_amd.upscalers.mlp_upscaler import MlpUpscaler
    nc = len(cfg['vocab'])
    edp = BachCPCDataProcessor(embedding_size=cfg['emb'], num_events=(cfg['Kl'] + cfg['Kr']) * 4, num_channels=nc,
                               num_tokens_per_channel=cfg['vocab'], num_tokens_per_block=16)
    ds = RelativeTransformerDownscaler(input_dim=cfg['emb'], output_dim=cfg['D'], num_channels=nc, downscale_factors=[4, 4],
                                       d_model=cfg['d'], n_head=cfg['H'], list_of_num_layers=cfg['layers'],
                                       dim_feedforward=cfg['ff'], dropout=0.0)
    q = quantizer or ProductVectorQuantizer(codebook_size=cfg['K'], codebook_dim=cfg['D'], commitment_cost=0.25,
                                            num_codebooks=cfg['ncb'], use_batch_norm=False, initialize=False, squared_l2_norm=True)
    up = None if quantizer is not None else MlpUpscaler(input_dim=cfg['D'], output_dim=cfg['zdim'], hidden_size=cfg['up_hidden'],
                                                        dropout=0.0)
    return Encoder(model_dir, edp, ds, q, up)


def build_decoder(cfg, kind='AC-AC', source_embedding='product', device='cuda', lr=1e-3, quantizer=None, seed=None):
    """device=None: construction only, on the host (no HIP call)."""
    from vqcpc_bach_amd.data_processor.bach_data_processor import BachDataProcessor
    from vqcpc_bach_amd.decoders.decoder import Decoder
    if seed is not None:
        torch.manual_seed(seed)
    enc = build_encoder(cfg, quantizer)
    nc = len(cfg['vocab'])
    dp = BachDataProcessor(embedding_size=cfg['dec_emb'], num_events=cfg['events'], num_tokens_per_channel=cfg['vocab'])
    dec = Decoder(model_dir='/tmp/vqcpc_test_product', dataloader_generator=None, data_processor=dp, encoder=enc,
                  transformer_type='relative', encoder_attention_type=KINDS[kind][0], cross_attention_type=KINDS[kind][1],
                  d_model=cfg['dec_d'], num_encoder_layers=cfg['dec_enc_layers'], num_decoder_layers=cfg['dec_dec_layers'],
                  n_head=cfg['dec_H'], dim_feedforward=cfg['dec_ff'], positional_embedding_size=cfg['dec_pos'],
                  num_channels_encoder=1, num_events_encoder=cfg['events'] * nc // 16, num_channels_decoder=nc,
                  num_events_decoder=cfg['events'], dropout=0.0, source_embedding=source_embedding)
    # START / END / XX as the last three ids of every voice (the stub dataset of tests/test_generate_long_gpu.py)
    n2i = [{'START': v - 3, 'END': v - 2, 'XX': v - 1} for v in cfg['vocab']]
    dec.dataloader_generator = types.SimpleNamespace(dataset=types.SimpleNamespace(note2index_dicts=n2i))
    if device is not None:
        from vqcpc_bach_amd import hip
        hip.load()
        dec.to(device)
        dec.init_optimizers(lr=lr, schedule_lr=False)
        assert dec.flat.check_views()
    return dec


def merged_twin(cfg, kind, dec, lr=1e-3):
    """The 'merged' decoder that computes what the 'product' decoder `dec` computes: its source table is dec's
    `merged_table()`, every other parameter (the frozen encoder's included) is copied."""
    twin = build_decoder(cfg, kind, 'merged', lr=lr)
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    sd['source_embeddings.weight'] = dec.source_embeddings.merged_table()
    twin.load_state_dict(sd, strict=True)
    assert twin.flat.check_views()
    return twin


def random_inputs(cfg, B, seed, num_codes=None):
    """(merged codes (B, num_codes or S), tokens (B, events, voices)) on the device."""
    g = torch.Generator().manual_seed(seed)
    nc = len(cfg['vocab'])
    S = num_codes or cfg['events'] * nc // 16
    codes = torch.randint(0, cfg['K'] ** cfg['ncb'], (B, S), generator=g)
    x = torch.stack([torch.randint(0, nv - 3, (B, cfg['events']), generator=g) for nv in cfg['vocab']], dim=2)
    return codes.cuda(), x.cuda()


def build_prior(cfg, code_model='product', sd=None, model_dir='/tmp/vqcpc_test_product_prior', dropout=0.0):
    """tests/test_prior_cpu.build_prior with a choice of `code_model` (cfg: the keys of the prior fixtures' cfg_json)."""
    from vqcpc_bach_amd.priors.prior_relative import PriorRelative
    enc = build_encoder(cfg, model_dir=model_dir)
    prior = PriorRelative(model_dir, dataloader_generator=None, encoder=enc, d_model=cfg['p_d'], num_layers=cfg['p_layers'],
                          n_head=cfg['p_H'], dim_feedforward=cfg['p_ff'], embedding_size=cfg['p_emb'], num_channels=1,
                          num_events=cfg['N'], dropout=dropout, code_model=code_model)
    if sd is not None:
        prior.load_state_dict(sd, strict=True)
    return prior


def prior_cfg(K, ncb, **over):
    """The tiny prior shapes of tests/golden/prior_tiny.npz (v1024) on ncb codebooks of K codewords."""
    cfg = dict(emb=8, vocab=[11, 12, 13, 14], d=32, H=2, layers=[1, 1], ff=64, D=4 * ncb, zdim=8, up_hidden=16, Kl=2, Kr=2, K=K,
               ncb=ncb, p_d=16, p_H=1, p_layers=2, p_ff=32, p_emb=4, N=6, B=3)
    cfg.update(over)
    return cfg


def oracle_stack(P, cfg, dtype):
    """The prior's causal stack on oracle/decoder_oracle.source_layer (TransformerEncoderLayerCustom with the causal mask), on
    the tensors of the state dict P cast to `dtype`."""
    Q = {k: v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu() for k, v in P.items()}

    def stack(x):
        for l in range(cfg['p_layers']):
            x, _ = D.source_layer(x, Q, f'transformer.layers.{l}.', cfg['p_H'], D.CAUSAL)
        return x
    return Q, stack
