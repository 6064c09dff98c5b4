"""The aligned ('diagonal') decoder and the F-F-C decoder (decoder_type 'transformer_relative_diagonal' /
'transformer_relative_full') against fixtures produced by the reference's own TransformerAlignedDecoderLayerCustom and Decoder
(tests/golden/decoder_layer_aligned_S3_T48.npz, decoder_tiny_diagonal.npz, decoder_tiny_full.npz; tools/
gen_golden_decoder_aligned.py), at the tolerances of tests/test_decoder_gpu.py: forward within 5e-5, gradients within 5e-4
(relative to max |ref|), codes bit-exact; plus the step graph, dropout and the locality of the aligned block."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, sub_state
from oracle import decoder_oracle as D
from test_decoder_gpu import FWD_TOL, GRAD_TOL, build_decoder

pytestmark = pytest.mark.gpu
T = torch.from_numpy


@pytest.fixture(params=['f32', 'bf16x6'])
def gemm_mode(request):
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1 if request.param == 'bf16x6' else 0)
    yield request.param
    hip.set_gemm_mode(0)


def _aligned_layer(g, dropout=0.0):
    from vqcpc_bach_amd.transformer.transformer_custom import TransformerAlignedDecoderLayerCustom
    Tn, n, d = g['tgt'].shape
    S, nc = g['mem'].shape[0], int(g['nc'])
    layer = TransformerAlignedDecoderLayerCustom(d_model=d, nhead=int(g['H']), attention_bias_type_self='relative_attention',
                                                 attention_bias_type_cross=None, num_channels_encoder=1, num_events_encoder=S,
                                                 num_channels_decoder=nc, num_events_decoder=Tn // nc,
                                                 dim_feedforward=g['sd/linear1.weight'].shape[0], dropout=dropout)
    sd = sub_state(g, 'sd')
    assert set(layer.state_dict()) == set(sd), 'state_dict keys must be the reference\'s'
    assert not any(k.startswith('multihead_attn') for k in sd) and 'cross_attn.0.weight' in sd and 'cross_attn.2.bias' in sd
    layer.load_state_dict(sd, strict=True)
    return layer.cuda()


def test_aligned_layer_golden(gemm_mode):
    g = load_golden('decoder_layer_aligned_S3_T48')
    layer = _aligned_layer(g).eval()
    tgt = T(g['tgt']).cuda().requires_grad_(True)
    mem = T(g['mem']).cuda().requires_grad_(True)
    y, att = layer(tgt, mem, tgt_mask=T(g['tgt_mask']).cuda(), memory_mask=None)     # API path, time-first, the additive mask
    assert att['a_cross'] is None
    assert rel_err(y.cpu(), g['y']) < FWD_TOL
    assert rel_err(att['a_self_decoder'].cpu(), g['a_self']) < FWD_TOL
    (y * T(g['g']).cuda()).sum().backward()
    assert rel_err(tgt.grad.cpu(), g['d_tgt']) < GRAD_TOL
    assert rel_err(mem.grad.cpu(), g['d_mem']) < GRAD_TOL
    for k, p in layer.named_parameters():
        ref = g['grad/' + k]
        if float(np.abs(ref).max()) == 0.0:
            assert float(p.grad.abs().max()) == 0.0, k
        else:
            assert rel_err(p.grad.cpu(), ref) < GRAD_TOL, k
    # the intermediates: C = cross_attn(memory rows) and its expansion
    from vqcpc_bach_amd import ops
    S, n, w = g['C'].shape
    Tn, nc = g['tgt'].shape[0], int(g['nc'])
    with torch.no_grad():
        C = layer.cross_rows(mem.detach().transpose(0, 1).reshape(n * S, -1))
        assert rel_err(C.view(n, S, w).transpose(0, 1).cpu(), g['C']) < FWD_TOL
        tgt2 = ops.AlignedExpandFn.apply(T(g['C']).transpose(0, 1).reshape(n * S, w).contiguous().cuda(), n, S, Tn // S, nc)
        assert torch.equal(tgt2.view(n, Tn, -1).transpose(0, 1).cpu(), T(g['tgt2']))            # a copy: exact


@pytest.mark.parametrize('name', ['decoder_tiny_diagonal', 'decoder_tiny_full'])
def test_decoder_epoch_golden(name, gemm_mode):
    g = load_golden(name)
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    diagonal = cfg['cross_attn'] == 'diagonal'
    lr = float(g['lr'])
    sd0 = sub_state(g, 'sd0')
    dec = build_decoder(cfg, sd0, lr=lr)                  # checks the state_dict keys and loads strictly
    assert repr(dec) == ('Decoder-relative-AC-D' if diagonal else 'Decoder-relative-F-F')
    assert any('cross_attn.2.weight' in k for k in sd0) == diagonal and any('multihead_attn' in k for k in sd0) != diagonal
    batch = {'x': T(g['batch/x'])}
    nc = len(cfg['vocab'])
    dec.eval()
    codes = dec.encode(batch['x'])
    assert torch.equal(codes.cpu(), T(g['codes'])), 'codes must be bit-exact'
    with torch.no_grad():
        fp = dec.forward(codes, batch['x'])
    assert abs(fp['monitored_quantities']['loss'] - float(g['eval/loss'])) < FWD_TOL * float(g['eval/loss'])
    for c in range(nc):
        assert rel_err(fp['weights_per_category'][c].cpu(), g[f'eval_fwd/logits.{c}']) < FWD_TOL
    if diagonal:
        assert 'eval_fwd/a_cross_last' not in g and all(a['a_cross'] is None for a in fp['attentions_decoder'])
    else:
        assert rel_err(fp['attentions_decoder'][-1]['a_cross'].cpu(), g['eval_fwd/a_cross_last']) < FWD_TOL
    assert rel_err(fp['attentions_decoder'][-1]['a_self_decoder'].cpu(), g['eval_fwd/a_self_last']) < FWD_TOL
    assert rel_err(fp['attentions_encoder'][-1]['a_self_encoder'].cpu(), g['eval_fwd/a_enc_last']) < FWD_TOL
    ev = dec.epoch(iter([batch]), train=False, num_batches=1)
    assert set(ev) == {'loss'} and abs(ev['loss'] - float(g['eval/loss'])) < FWD_TOL * float(g['eval/loss'])

    from vqcpc_bach_amd import ops
    golden_grads = {k[5:]: v for k, v in g.items() if k.startswith('grad/')}
    named = {k: p for k, p in dec.named_parameters() if not k.startswith('encoder.')}
    assert set(named) == set(golden_grads)
    for direct in (False, True):
        dec.train()
        loss, _, _, _ = dec.compute_loss(codes, dec.data_processor.preprocess(batch['x']))
        dec.flat.zero_grad()
        if direct:
            with ops.direct_weight_gradients():
                loss.backward()
        else:
            loss.backward()
        assert dec.flat.check_views()
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
    sd1 = sub_state(g, 'sd1')
    now = dec.state_dict()
    for k, v in sd1.items():
        if k.startswith('encoder.'):
            assert torch.equal(now[k].cpu(), sd0[k]), k                 # frozen
            continue
        gr = T(golden_grads[k]).abs()
        solid = gr > 1e-4 * gr.max() if float(gr.max()) > 0 else torch.zeros_like(gr, dtype=torch.bool)
        mine, ref = now[k].cpu() - sd0[k], v - sd0[k]
        if bool(solid.any()):
            assert rel_err(mine[solid], ref[solid]) < 2e-2, k
        assert float((mine - ref).abs().max()) <= 2.0001 * lr, k       # noise-sign elements move by at most lr each way


def _getter_decoder(decoder_type, dropout=0.0):
    """A small decoder through configs.make_decoder_config(decoder_type=...) and the getters, as the tools build it."""
    from vqcpc_bach_amd import configs, getters
    config = configs.make_decoder_config(dropout=dropout, decoder_type=decoder_type)
    assert config['decoder_type'] == decoder_type
    config['dataloader_generator_kwargs'] = dict(sequences_size=4)                       # 16 ticks = 64 target tokens, 4 codes
    config['decoder_kwargs'].update(d_model=64, n_head=2, num_encoder_layers=1, num_decoder_layers=2, dim_feedforward=128)
    enc_cfg = config['config_encoder']
    enc_cfg['downscaler_kwargs'].update(d_model=64, n_head=2, list_of_num_layers=[1, 1], dim_feedforward=128, dropout=0.0)
    dlg = getters.get_dataloader_generator(config['dataset'], config['training_method'],
                                           dict(config['dataloader_generator_kwargs'], seed=7, device='cuda'))
    enc_dlg = getters.get_dataloader_generator(enc_cfg['dataset'], enc_cfg['training_method'],
                                               dict(enc_cfg['dataloader_generator_kwargs'], seed=7, device='cuda'))
    encoder = getters.get_encoder('/tmp/vqcpc_test_decoder_aligned', enc_dlg, enc_cfg)
    dp = getters.get_data_processor(dlg, config['data_processor_type'], config['data_processor_kwargs'])
    dec = getters.get_decoder('/tmp/vqcpc_test_decoder_aligned', dlg, dp, encoder, config['decoder_type'], config['decoder_kwargs'])
    dec.cuda()
    dec.init_optimizers(lr=1e-3, schedule_lr=False)
    return dec, dlg


@pytest.mark.parametrize('decoder_type,name,layer', [('transformer_relative_diagonal', 'Decoder-relative-AC-D', 'Aligned'),
                                                     ('transformer_relative_full', 'Decoder-relative-F-F', '')])
def test_new_decoder_types_through_the_getters(decoder_type, name, layer):
    from vqcpc_bach_amd import configs
    assert configs.make_decoder_config()['decoder_type'] == 'transformer_relative'      # the default is unchanged
    torch.manual_seed(3)
    dec, dlg = _getter_decoder(decoder_type)
    assert repr(dec) == name
    assert all(type(l).__name__ == f'Transformer{layer}DecoderLayerCustom' for l in dec.transformer.decoder.layers)
    # the flat parameter / gradient buffers (one all-reduce bucket on the multi-rank path) hold the new parameters
    assert dec.flat.check_views()
    lo, hi = dec.flat.flat.data_ptr(), dec.flat.flat.data_ptr() + 4 * dec.flat.numel
    for k, p in dec.named_parameters():
        if not k.startswith('encoder.'):
            assert lo <= p.data_ptr() < hi and p.grad is not None, k
    x = next(dlg.dataloaders(batch_size=2)[0])['x']
    dec.train()
    a = float(dec.train_step({'x': x}))
    assert np.isfinite(a) and dec.flat.check_views()
    if layer:
        for l in dec.transformer.decoder.layers:
            for p in l.cross_attn.parameters():
                assert float(p.grad.abs().max()) > 0                                      # ... and their gradients land there
    with pytest.raises(NotImplementedError):
        from vqcpc_bach_amd import getters
        getters.get_decoder('/tmp/x', dlg, dec.data_processor, dec.encoder, 'transformer', {})


def _steps(dec, batches, graph):
    dec.train()
    dec.enable_step_graph(graph)
    losses = [dec.train_step({'x': x}).clone() for x in batches]
    replays = dec._graph.replays if dec._graph is not None else 0
    dec.enable_step_graph(False)
    return torch.stack(losses).cpu(), dec.flat.flat.detach().cpu().clone(), replays


def test_replayed_step_is_the_eager_step_bit_for_bit():
    """train_model()'s defaults (bf16x6 GEMMs, f16x3 gradient products, step-graph replay), dropout 0: the same five steps
    eager and with the step graph give the same losses and parameters, bit for bit."""
    from vqcpc_bach_amd import hip, ops
    g = load_golden('decoder_tiny_diagonal')
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    gen = torch.Generator().manual_seed(9)
    batches = [torch.stack([torch.randint(0, nv, (cfg['B'], cfg['events']), generator=gen) for nv in cfg['vocab']], dim=2).cuda()
               for _ in range(5)]
    mode, arith = hip.gemm_mode_state(), ops.gradient_arithmetic_state()
    res = {}
    try:
        for graph in (False, True):
            dec = build_decoder(cfg, sub_state(g, 'sd0'), lr=float(g['lr']))
            dec.use_training_defaults()
            res[graph] = _steps(dec, batches, graph)
    finally:
        hip.restore_gemm_mode_state(mode)
        ops.restore_gradient_arithmetic_state(arith)
    assert res[False][2] == 0 and res[True][2] >= 1, 'the step must have been replayed'
    print('eager vs replayed: max |d loss|', float((res[False][0] - res[True][0]).abs().max()), 'max |d param|',
          float((res[False][1] - res[True][1]).abs().max()))
    assert torch.equal(res[False][0], res[True][0])
    assert torch.equal(res[False][1], res[True][1])


def test_dropout_step():
    from vqcpc_bach_amd.utils import SEEDS
    g = load_golden('decoder_tiny_diagonal')
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    x = T(g['batch/x']).cuda()
    res = []
    for _ in range(2):
        SEEDS.manual_seed(1234)
        dec = build_decoder(cfg, sub_state(g, 'sd0'), lr=float(g['lr']), dropout=0.2)
        dec.train()
        losses = [dec.train_step({'x': x}).clone() for _ in range(2)]
        assert all(bool(torch.isfinite(l)) for l in losses)
        assert bool(torch.isfinite(dec.flat.flat_grad).all()) and float(dec.flat.flat_grad.abs().max()) > 0
        res.append((torch.stack(losses).cpu(), dec.flat.flat_grad.cpu().clone(), dec.flat.flat.detach().cpu().clone()))
    assert float(res[0][0][0]) != float(g['train/loss'])                   # dropout was on
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_a_code_reaches_only_its_own_target_rows():
    """Layer level, memory held fixed apart from ONE row (sequence 1, code s): of tgt2 only that code's U rows change; of the
    layer output nothing of the other sequences and nothing before the code's first token (causal self-attention)."""
    from vqcpc_bach_amd import ops
    g = load_golden('decoder_layer_aligned_S3_T48')
    layer = _aligned_layer(g, dropout=0.2).eval()
    Tn, n, d = g['tgt'].shape
    S, nc = g['mem'].shape[0], int(g['nc'])
    U = Tn // S
    tgt = T(g['tgt']).transpose(0, 1).reshape(n * Tn, d).contiguous().cuda()
    mem = T(g['mem']).transpose(0, 1).reshape(n * S, d).contiguous().cuda()
    with torch.no_grad():
        base2 = ops.AlignedExpandFn.apply(layer.cross_rows(mem), n, S, U, nc).view(n, Tn, d)
        base = layer.forward_rows(tgt, mem, n, ops.MASK_CAUSAL)[0].view(n, Tn, d)
        for s in range(S):
            mem2 = mem.clone()
            mem2[1 * S + s] += 1.0
            new2 = ops.AlignedExpandFn.apply(layer.cross_rows(mem2), n, S, U, nc).view(n, Tn, d)
            changed = (new2 != base2).any(dim=2)
            want = torch.zeros(n, Tn, dtype=torch.bool, device='cuda')
            want[1, s * U:(s + 1) * U] = True
            assert torch.equal(changed, want), s
            new = layer.forward_rows(tgt, mem2, n, ops.MASK_CAUSAL)[0].view(n, Tn, d)
            assert torch.equal(new[[0, 2]], base[[0, 2]]) and torch.equal(new[1, :s * U], base[1, :s * U])
            assert not torch.equal(new[1, s * U:(s + 1) * U], base[1, s * U:(s + 1) * U])
