"""The code prior without a GPU: construction through the getters and configs, state-dict keys against the reference's
fixture, the C ABI of the two new entry points (declared, bound, argument validation before any HIP call) and the
host-side argument checks of `generate_codes`."""
import ctypes
import json
import os

import pytest
import torch

from conftest import load_golden, sub_state


def build_prior(cfg, sd=None, model_dir='/tmp/vqcpc_test_prior', dropout=0.0):
    """The fixtures' model (tools/gen_golden_prior.py: build_encoder + PriorRelative) from this package's classes."""
    from vqcpc_bach_amd.data_processor.bach_cpc_data_processor import BachCPCDataProcessor
    from vqcpc_bach_amd.downscalers.relative_transformer_downscaler import RelativeTransformerDownscaler
    from vqcpc_bach_amd.encoder import Encoder
    from vqcpc_bach_amd.priors.prior_relative import PriorRelative
    from vqcpc_bach_amd.quantizer.vector_quantizer import ProductVectorQuantizer
    from vqcpc_bach_amd.upscalers.mlp_upscaler import MlpUpscaler
    nc = len(cfg['vocab'])
    edp = BachCPCDataProcessor(embedding_size=cfg['emb'], num_events=(cfg['Kl'] + cfg['Kr']) * 4, num_channels=nc,
                               num_tokens_per_channel=cfg['vocab'], num_tokens_per_block=16)
    ds = RelativeTransformerDownscaler(input_dim=cfg['emb'], output_dim=cfg['D'], num_channels=nc, downscale_factors=[4, 4],
                                       d_model=cfg['d'], n_head=cfg['H'], list_of_num_layers=cfg['layers'],
                                       dim_feedforward=cfg['ff'], dropout=0.0)
    q = ProductVectorQuantizer(codebook_size=cfg['K'], codebook_dim=cfg['D'], commitment_cost=0.25,
                               num_codebooks=cfg['ncb'], use_batch_norm=False, initialize=False, squared_l2_norm=True)
    up = MlpUpscaler(input_dim=cfg['D'], output_dim=cfg['zdim'], hidden_size=cfg['up_hidden'], dropout=0.0)
    enc = Encoder(model_dir, edp, ds, q, up)
    prior = PriorRelative(model_dir, dataloader_generator=None, encoder=enc, d_model=cfg['p_d'], num_layers=cfg['p_layers'],
                          n_head=cfg['p_H'], dim_feedforward=cfg['p_ff'], embedding_size=cfg['p_emb'], num_channels=1,
                          num_events=cfg['N'], dropout=dropout)
    if sd is not None:
        prior.load_state_dict(sd, strict=True)
    return prior


@pytest.fixture(scope='module')
def lib():
    import torch  # noqa: F401  (loads the process-wide libamdhip64.so.7 first)
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    return hip.load()


@pytest.mark.parametrize('tag', ['v32', 'v1024'])
def test_state_dict_keys_are_the_references(tag):
    g = load_golden('prior_tiny')
    cfg = json.loads(str(g[f'{tag}/cfg_json']))
    sd = sub_state(g, f'{tag}/sd')
    prior = build_prior(cfg)
    assert set(prior.state_dict()) == set(sd)
    prior.load_state_dict(sd, strict=True)
    assert prior.num_tokens_per_channel == [cfg['K'] ** cfg['ncb']] and prior.num_tokens == cfg['N']
    for k in ('embedding.weight', 'linear.weight', 'linear.bias', 'sos', 'pre_softmaxes.0.weight', 'pre_softmaxes.0.bias',
              'transformer.layers.0.self_attn.in_proj_weight', 'transformer.layers.1.norm2.bias'):
        assert k in sd, k
    assert all(not p.requires_grad for p in prior.encoder.parameters())
    named = {k for k, p in prior.named_parameters() if not k.startswith('encoder.')}
    assert named == {k[len(tag) + 6:] for k in g if k.startswith(f'{tag}/grad/')}
    assert repr(prior) == 'PriorRelative'


def test_prior_config_builds_through_the_getters():
    from vqcpc_bach_amd import configs, getters
    from vqcpc_bach_amd.priors.prior_relative import PriorRelative
    assert configs.make_config('PRI')['prior_kwargs'] == dict(configs.make_prior_config()['prior_kwargs'], dropout=0.1)
    config = configs.make_prior_config()
    assert config['prior_kwargs'] == dict(d_model=512, n_head=8, num_layers=6, dim_feedforward=1024, embedding_size=32,
                                          dropout=0.2)
    assert config['training_method'] == 'prior' and config['prior_type'] == 'transformer_relative'
    dlg = getters.get_dataloader_generator('bach', 'prior', dict(config['dataloader_generator_kwargs'], seed=3))
    batch = next(dlg.dataloaders(batch_size=2)[0])
    assert set(batch) == {'x'} and batch['x'].shape == (2, 96, 4)
    enc_cfg = config['config_encoder']
    enc_dlg = getters.get_dataloader_generator(enc_cfg['dataset'], enc_cfg['training_method'],
                                               dict(enc_cfg['dataloader_generator_kwargs'], seed=3))
    encoder = getters.get_encoder('/tmp/vqcpc_test_prior_cfg', enc_dlg, enc_cfg)
    prior = getters.get_prior('/tmp/vqcpc_test_prior_cfg', dlg, encoder, config['prior_type'], config['prior_kwargs'])
    assert isinstance(prior, PriorRelative)
    assert prior.num_tokens == 24 and prior.num_tokens_per_channel == [32] and prior.d_model == 512
    assert len(prior.transformer.layers) == 6 and prior.embedding.weight.shape == (32, 32)
    assert prior.transformer.layers[0].self_attn.attn_bias.e1.shape[0] == 8 * 24
    with pytest.raises(NotImplementedError):
        getters.get_prior('/tmp/x', dlg, encoder, 'lstm', config['prior_kwargs'])


def test_install_as_vqcpcb_exposes_the_prior():
    import sys
    import vqcpc_bach_amd
    vqcpc_bach_amd.install_as_vqcpcb()
    from vqcpc_bach_amd.priors import prior_relative
    assert sys.modules['VQCPCB.priors.prior_relative'] is prior_relative
    assert sys.modules['VQCPCB.getters'].get_prior is vqcpc_bach_amd.getters.get_prior


def test_new_symbols_are_declared_bound_and_exported(lib):
    from test_abi import header_symbols
    from vqcpc_bach_amd import hip
    for s in ('vqcpc_prior_sample', 'vqcpc_prior_window'):
        assert s in header_symbols() and s in hip.SIGNATURES and hasattr(lib, s)
    assert lib.vqcpc_abi_version() == 2


def test_prior_entry_points_validate_arguments_without_gpu(lib):
    """Bad arguments are rejected before any HIP call, with a message (as test_abi.test_argument_validation_without_gpu)."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value                       # a non-null pointer that is never dereferenced

    def sample(V=32, M=1, logits=p, ticket=p, temperature=1.0):
        return lib.vqcpc_prior_sample(logits, V, V, M, temperature, 0, 1.0, p, None, 0, p, 8, 8, p, V + 1, 16, p, 16, None, 0, p,
                                      ticket, None)
    assert sample(V=4097) == -1 and b'prior_sample' in lib.vqcpc_last_error() and b'4096' in lib.vqcpc_last_error()
    assert sample(V=0) == -1
    assert sample(M=65) == -1 and b'64' in lib.vqcpc_last_error()
    assert sample(logits=None) == -1 and b'null' in lib.vqcpc_last_error()
    assert sample(ticket=None) == -1
    assert sample(temperature=0.0) == -1 and b'temperature' in lib.vqcpc_last_error()

    def window(M=1, seq=p, P=0, N=8):
        return lib.vqcpc_prior_window(seq, 20, 20, p, 1, p, N, P, p, p, 33, 16, p, 16, p, p, p, M, None)
    assert window(M=65) == -1 and b'prior_window' in lib.vqcpc_last_error() and b'64' in lib.vqcpc_last_error()
    assert window(seq=None) == -1 and b'null' in lib.vqcpc_last_error()
    assert window(P=8) == -1 and b'P < N' in lib.vqcpc_last_error()
    assert window(N=21) == -1


def test_generate_codes_refuses_what_the_sampler_cannot_take():
    """V = 2 x 512 = 262 144 merged codes: the model builds (training is limited only by the existing kernels), sampling
    raises a ValueError that names the limit -- before anything touches the device."""
    g = load_golden('prior_tiny')
    cfg = dict(json.loads(str(g['v1024/cfg_json'])), K=512, ncb=2, p_emb=4)
    prior = build_prior(cfg)
    assert prior.num_tokens_per_channel == [262144]
    with pytest.raises(ValueError, match='4096'):
        prior.generate_codes(12)
    small = build_prior(json.loads(str(g['v32/cfg_json'])))
    with pytest.raises(ValueError, match='num_tokens'):
        small.generate_codes(5)                                       # fewer than one model window (N = 6)
    with pytest.raises(ValueError, match='window_stride'):
        small.generate_codes(12, window_stride=6)
    with pytest.raises(ValueError, match='temperature'):
        small.generate_codes(12, temperature=0.0)
    with pytest.raises(NotImplementedError):
        small.plot()
    assert torch.equal(small._generate_square_subsequent_mask(3) == 0, torch.tril(torch.ones(3, 3)) == 1)
