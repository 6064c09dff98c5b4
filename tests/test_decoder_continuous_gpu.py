"""The decoder on continuous latents (a NoQuantization encoder without upscaler; `source_embeddings` an nn.Linear) against
fixtures produced by the reference's own `Decoder.epoch` (tests/golden/decoder_tiny_continuous.npz,
decoder_tiny_continuous_diagonal.npz; tools/gen_golden_decoder_continuous.py), at the tolerances of tests/test_decoder_gpu.py
and tests/test_decoder_aligned_gpu.py: forward within 5e-5, gradients within 5e-4 of their maximum."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, sub_state
from continuous_helpers import build_continuous_decoder, golden_continuous_decoder

pytestmark = pytest.mark.gpu
T = torch.from_numpy
FWD_TOL, GRAD_TOL = 5e-5, 5e-4
FIXTURES = ['decoder_tiny_continuous', 'decoder_tiny_continuous_diagonal']


@pytest.fixture(params=['f32', 'bf16x6'])
def gemm_mode(request):
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1 if request.param == 'bf16x6' else 0)
    yield request.param
    hip.set_gemm_mode(0)


@pytest.mark.parametrize('name', FIXTURES)
def test_decoder_epoch_golden(name, gemm_mode):
    from vqcpc_bach_amd import ops
    dec, cfg, g = golden_continuous_decoder(name, lr=float(load_golden(name)['lr']))      # strict load of the reference's keys
    sd0 = sub_state(g, 'sd0')
    assert 'source_embeddings.bias' in sd0 and tuple(sd0['source_embeddings.weight'].shape) == (cfg['dec_d'], cfg['D'])
    assert dec.continuous_source and dec.source_dim == cfg['D'] and isinstance(dec.source_embeddings, torch.nn.Linear)
    assert repr(dec) == ('Decoder-relative-AC-D' if cfg['cross_attn'] == 'diagonal' else 'Decoder-relative-AC-AC')
    batch = {'x': T(g['batch/x'])}
    nc = len(cfg['vocab'])
    dec.eval()
    z = dec.encode(batch['x'])
    assert z.dtype == torch.float32 and tuple(z.shape) == g['z'].shape and not z.requires_grad
    assert rel_err(z.cpu(), g['z']) < FWD_TOL
    dec.train()
    assert rel_err(dec.encode(batch['x']).cpu(), g['z']) < FWD_TOL and dec.training         # eval-mode latents, mode put back
    dec.eval()
    with torch.no_grad():
        fp = dec.forward(z, batch['x'])
    assert abs(fp['monitored_quantities']['loss'] - float(g['eval/loss'])) < FWD_TOL * float(g['eval/loss'])
    for c in range(nc):
        assert rel_err(fp['weights_per_category'][c].cpu(), g[f'eval_fwd/logits.{c}']) < FWD_TOL
    ev = dec.epoch(iter([batch]), train=False, num_batches=1)
    assert set(ev) == {'loss'} and abs(ev['loss'] - float(g['eval/loss'])) < FWD_TOL * float(g['eval/loss'])

    golden_grads = {k[5:]: v for k, v in g.items() if k.startswith('grad/')}
    named = {k: p for k, p in dec.named_parameters() if not k.startswith('encoder.')}
    assert set(named) == set(golden_grads)
    assert float(np.abs(golden_grads['source_embeddings.weight']).max()) > 0
    for direct in (False, True):
        dec.train()
        loss, _, _, _ = dec.compute_loss(z, dec.data_processor.preprocess(batch['x']))
        dec.flat.zero_grad()
        if direct:
            with ops.direct_weight_gradients(dec.flat):
                loss.backward()
        else:
            loss.backward()
        assert dec.flat.check_views()
        for k in ('source_embeddings.weight', 'source_embeddings.bias'):
            assert rel_err(named[k].grad.cpu(), golden_grads[k]) < GRAD_TOL, (k, direct)
        for k, p in named.items():
            ref = golden_grads[k]
            if float(np.abs(ref).max()) == 0.0:
                assert float(p.grad.abs().max()) == 0.0, k
            else:
                assert rel_err(p.grad.cpu(), ref) < GRAD_TOL, (k, direct)
    assert all(p.grad is None for k, p in dec.named_parameters() if k.startswith('encoder.'))
    trn = dec.epoch(iter([batch]), train=True, num_batches=1)
    assert abs(trn['loss'] - float(g['train/loss'])) < FWD_TOL * float(g['train/loss'])
    gn = float(g['grad_total_norm'])
    assert abs(dec.optimizer.grad_norm() - gn) < 2e-4 * gn


def _steps(dec, batches, graph):
    dec.train()
    dec.enable_step_graph(graph)
    losses = [dec.train_step({'x': x}).clone() for x in batches]
    replays = dec._graph.replays if dec._graph is not None else 0
    dec.enable_step_graph(False)
    return torch.stack(losses).cpu(), dec.flat.flat.detach().cpu().clone(), replays


@pytest.mark.parametrize('name', FIXTURES)
def test_replayed_step_is_the_eager_step_bit_for_bit(name):
    """train_model()'s defaults (bf16x6 GEMMs, f16x3 gradient products, step-graph replay), dropout 0: three steps eager and
    with the step graph give the same losses and parameters, bit for bit; the step is ONE graph replay."""
    from vqcpc_bach_amd import hip, ops
    from oracle import decoder_oracle as D
    import json
    g = load_golden(name)
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    gen = torch.Generator().manual_seed(9)
    batches = [torch.stack([torch.randint(0, nv, (cfg['B'], cfg['events']), generator=gen) for nv in cfg['vocab']], dim=2).cuda()
               for _ in range(3)]
    mode, arith = hip.gemm_mode_state(), ops.gradient_arithmetic_state()
    res = {}
    try:
        for graph in (False, True):
            dec = build_continuous_decoder(cfg, sub_state(g, 'sd0'), lr=float(g['lr']))
            dec.use_training_defaults()
            res[graph] = _steps(dec, batches, graph)
    finally:
        hip.restore_gemm_mode_state(mode)
        ops.restore_gradient_arithmetic_state(arith)
    assert res[False][2] == 0 and res[True][2] >= 1, 'the step must have been replayed'
    assert torch.equal(res[False][0], res[True][0])
    assert torch.equal(res[False][1], res[True][1])


def _getter_decoder(decoder_type, enc_cfg=None):
    from vqcpc_bach_amd import configs, getters
    config = configs.make_decoder_config(dropout=0.0, decoder_type=decoder_type)
    config['dataloader_generator_kwargs'] = dict(sequences_size=4)                       # 16 ticks = 64 target tokens, 4 codes
    config['decoder_kwargs'].update(d_model=64, n_head=2, num_encoder_layers=1, num_decoder_layers=2, dim_feedforward=128)
    if enc_cfg is None:
        enc_cfg = config['config_encoder']
        enc_cfg['downscaler_kwargs'].update(d_model=64, n_head=2, list_of_num_layers=[1, 1], dim_feedforward=128, dropout=0.0)
        enc_cfg.update(quantizer_type=None, quantizer_kwargs=dict(codebook_dim=32), upscaler_type=None)
    dlg = getters.get_dataloader_generator(config['dataset'], config['training_method'],
                                           dict(config['dataloader_generator_kwargs'], seed=7, device='cuda'))
    enc_dlg = getters.get_dataloader_generator(enc_cfg['dataset'], enc_cfg['training_method'],
                                               dict(enc_cfg['dataloader_generator_kwargs'], seed=7, device='cuda'))
    encoder = getters.get_encoder('/tmp/vqcpc_test_decoder_continuous', enc_dlg, enc_cfg)
    dp = getters.get_data_processor(dlg, config['data_processor_type'], config['data_processor_kwargs'])
    dec = getters.get_decoder('/tmp/vqcpc_test_decoder_continuous', dlg, dp, encoder, config['decoder_type'],
                              config['decoder_kwargs'])
    dec.cuda()
    dec.init_optimizers(lr=1e-3, schedule_lr=False)
    return dec, dlg


def _trains_one_step(dec, dlg):
    assert dec.continuous_source and dec.source_dim == 32 and tuple(dec.source_embeddings.weight.shape) == (64, 32)
    lo, hi = dec.flat.flat.data_ptr(), dec.flat.flat.data_ptr() + 4 * dec.flat.numel
    for p in dec.source_embeddings.parameters():
        assert lo <= p.data_ptr() < hi
    x = next(dlg.dataloaders(batch_size=2)[0])['x']
    dec.train()
    loss = float(dec.train_step({'x': x}))
    assert np.isfinite(loss) and dec.flat.check_views()
    for p in dec.source_embeddings.parameters():
        assert float(p.grad.abs().max()) > 0
    assert all(p.grad is None for p in dec.encoder.parameters())


@pytest.mark.parametrize('decoder_type', ['transformer_relative_diagonal', 'transformer_relative'])
def test_no_quantisation_chain_through_the_getters(decoder_type):
    torch.manual_seed(3)
    _trains_one_step(*_getter_decoder(decoder_type))


def test_sameseq_noq_config_builds():
    from vqcpc_bach_amd import configs
    enc_cfg = configs.make_config('SAMESEQ_NOQ', dropout=0.0)
    assert enc_cfg['quantizer_type'] is None and enc_cfg['quantizer_kwargs'] == dict(codebook_dim=32)
    assert enc_cfg['upscaler_type'] is None and enc_cfg['downscaler_type'] == 'lstm_downscaler'
    assert enc_cfg == configs.make_sameseq_config(dropout=0.0, quantizer_type=None)
    same = configs.make_config('SAMESEQ')
    assert same['quantizer_type'] == 'commitment' and same['upscaler_type'] == 'mlp_upscaler' and \
        same['quantizer_kwargs']['codebook_dim'] == 3 and same['auxiliary_networks_kwargs']['quantization_weighting'] == 1.0
    enc_cfg['downscaler_kwargs'].update(hidden_size=32)
    torch.manual_seed(4)
    dec, dlg = _getter_decoder('transformer_relative_diagonal', enc_cfg=enc_cfg)
    assert type(dec.encoder.quantizer).__name__ == 'NoQuantization' and dec.encoder.upscaler is None
    _trains_one_step(dec, dlg)


def test_rejections():
    from vqcpc_bach_amd.priors.prior_relative import PriorRelative  # noqa: F401
    dec, cfg, g = golden_continuous_decoder('decoder_tiny_continuous_diagonal')
    with pytest.raises(NotImplementedError, match='upscaler'):
        build_continuous_decoder(cfg, None, upscaler=True)
    S, dz = dec.num_tokens_source, dec.source_dim
    codes = torch.zeros(2, S, dtype=torch.int64, device='cuda')
    x = T(g['batch/x']).cuda()
    for bad in (codes, torch.zeros(2, S, dz + 4, device='cuda'), torch.zeros(2, S + 1, dz, device='cuda'),
                torch.zeros(2, S, dz, dtype=torch.int64, device='cuda')):
        with pytest.raises(ValueError):
            dec.generate_from_codes(bad, top_k=1, seed=0)
    with pytest.raises(ValueError):
        dec.forward(codes, x)
    with pytest.raises(ValueError):
        dec.generate_from_code_long(torch.zeros(1, S + 2, dtype=torch.int64), temperature=1.0, pad=[0] * 4, start=[0] * 4)
    # the reverse: latents handed to a code decoder
    from test_generate_gpu import _golden_decoder
    code_dec = _golden_decoder('decoder_tiny_diagonal')[0]
    assert not code_dec.continuous_source and code_dec.source_dim is None
    with pytest.raises(ValueError):
        code_dec.generate_from_codes(torch.zeros(2, S, dz, device='cuda'), top_k=1, seed=0)
    with pytest.raises(ValueError):
        code_dec.generate_from_code_long(torch.zeros(1, S + 2, dz), temperature=1.0, pad=[0] * 4, start=[0] * 4)
    with pytest.raises(ValueError):
        code_dec.forward(torch.zeros(2, S, dz, device='cuda'), x)
