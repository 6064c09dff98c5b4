"""The GRU block downscaler ('lstm_downscaler') through the factories, without a GPU: construction, the reference's
state_dict names and shapes (tests/golden/lstm_downscaler_*.npz hold the reference module's own tensors) and the SAMESEQ
configuration."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden


def _kwargs(cfg):
    return dict(input_dim=cfg['emb'], output_dim=cfg['D'], num_channels=4, num_tokens=64, downscale_factors=[cfg['L']],
                hidden_size=cfg['hidden'], num_layers=cfg['layers'], dropout=0.1, bidirectional=cfg['bidirectional'])


@pytest.mark.parametrize('name', ['lstm_downscaler_tiny', 'lstm_downscaler_h24'])      # bidirectional True / False
def test_get_downscaler_builds_the_reference_state_dict(name):
    from vqcpc_bach_amd import getters
    from vqcpc_bach_amd.downscalers.lstm_downscaler import LstmDownscaler
    g = load_golden(name)
    cfg = json.loads(str(g['cfg_json']))
    ds = getters.get_downscaler('lstm_downscaler', _kwargs(cfg))
    assert isinstance(ds, LstmDownscaler)
    assert ds.sequence_length == cfg['L'] and ds.downscale_factors == [cfg['L']]
    assert (ds.g_enc_bwd is not None) == cfg['bidirectional']
    ref = {k[3:]: tuple(v.shape) for k, v in g.items() if k.startswith('sd/')}
    assert {k: tuple(v.shape) for k, v in ds.state_dict().items()} == ref
    assert list(ds.state_dict().keys()) == [k[3:] for k in g if k.startswith('sd/')], 'same order as the reference'
    ds.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}, strict=True)


def test_mlp_downscaler_still_raises():
    from vqcpc_bach_amd import getters
    with pytest.raises(NotImplementedError):
        getters.get_downscaler('mlp_downscaler', {})


def test_sameseq_config_goes_through_get_encoder():
    from vqcpc_bach_amd import configs, getters
    from vqcpc_bach_amd.downscalers.lstm_downscaler import LstmDownscaler
    config = configs.make_config('SAMESEQ')
    assert config['downscaler_type'] == 'lstm_downscaler' and config['batch_size'] == 16
    assert config['auxiliary_networks_kwargs']['quantization_weighting'] == 1.0
    dlg = getters.get_dataloader_generator('bach', 'vqcpc', config['dataloader_generator_kwargs'])
    assert (dlg.num_blocks_left, dlg.num_blocks_right) == (6, 6)
    enc = getters.get_encoder('/tmp/vqcpc_test_model', dlg, config)
    ds = enc.downscaler
    assert isinstance(ds, LstmDownscaler) and ds.g_enc_bwd is not None
    assert ds.g_enc_fwd.weight_ih_l0.shape == (3 * 512, 32) and ds.g_enc_fwd.num_layers == 2
    assert ds.output_linear.weight.shape == (3, 1024)
    assert enc.quantizer.codebook_size == 32 and enc.upscaler is not None
    tr = getters.get_encoder_trainer('/tmp/vqcpc_test_model', dlg, 'vqcpc', enc, config['auxiliary_networks_kwargs'])
    assert tr.c_module.g_ar_fwd.hidden_size == 512
