"""LstmDownscaler (vqcpc_bach_amd/downscalers/lstm_downscaler.py) against the reference's own module and trainer step:
tests/golden/lstm_downscaler_tiny.npz, lstm_downscaler_h24.npz and epoch_tiny_lstm.npz (tools/gen_golden_lstm.py).
Forward quantities within 5e-5, gradients within 5e-4 (FWD_TOL / GRAD_TOL of tests/test_trainer_gpu.py, relative to
max |ref|), under both GEMM modes; code indices bit-exact."""
import json

import numpy as np
import pytest
import torch

import train_reference as TR
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
T = torch.from_numpy
FWD_TOL, GRAD_TOL = 5e-5, 5e-4
INF = 10 ** 9


@pytest.fixture(params=['f32', 'bf16x6'], autouse=True)
def gemm_mode(request):
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1 if request.param == 'bf16x6' else 0)
    yield request.param
    hip.set_gemm_mode(0)


@pytest.fixture
def table_ratio():
    """Sets LstmDownscaler.table_lookup_min_ratio (0: table path forced on, INF: forced off) and restores it."""
    from vqcpc_bach_amd.downscalers.lstm_downscaler import LstmDownscaler as D
    old = D.table_lookup_min_ratio

    def set_(value):
        D.table_lookup_min_ratio = value
    yield set_
    D.table_lookup_min_ratio = old


def _modules(g, dropout=0.0):
    from vqcpc_bach_amd.data_processor.bach_cpc_data_processor import BachCPCDataProcessor
    from vqcpc_bach_amd.downscalers.lstm_downscaler import LstmDownscaler
    cfg = json.loads(str(g['cfg_json']))
    dp = BachCPCDataProcessor(embedding_size=cfg['emb'], num_events=20, num_channels=4, num_tokens_per_channel=cfg['vocab'],
                              num_tokens_per_block=cfg['L'])
    ds = LstmDownscaler(input_dim=cfg['emb'], output_dim=cfg['D'], num_channels=4, downscale_factors=[cfg['L']],
                        hidden_size=cfg['hidden'], num_layers=cfg['layers'], dropout=dropout, bidirectional=cfg['bidirectional'])
    sd = {k[3:]: T(np.array(v)) for k, v in g.items() if k.startswith('sd/')}
    ds.load_state_dict(sd, strict=True)                              # the reference's tensors, names and shapes as they are
    for c, e in enumerate(dp.embeddings):
        with torch.no_grad():
            e.weight.copy_(T(g[f'emb/{c}']))
    return cfg, dp.cuda(), ds.cuda()


def _run(path, g, dp, ds, set_ratio):
    """z and the gradients of every downscaler tensor and embedding table under the fixture's cotangent."""
    for p in list(ds.parameters()) + list(dp.parameters()):
        p.grad = None
    tokens = T(g['tokens']).cuda()
    if path == 'embedded':
        x = dp.embed(tokens)                                         # (3, 5, 16, emb)
        z = ds(x.reshape(x.shape[0], -1, x.shape[-1]))
    else:
        set_ratio(0 if path == 'table' else INF)
        z = ds.forward_tokens(tokens, dp)
    (z * T(g['g_z']).cuda()).sum().backward()
    grads = {k: p.grad.detach().cpu() for k, p in ds.named_parameters()}
    grads.update({f'emb{c}': e.weight.grad.detach().cpu() for c, e in enumerate(dp.embeddings)})
    return z.detach().cpu(), grads


@pytest.mark.parametrize('name', ['lstm_downscaler_tiny', 'lstm_downscaler_h24'])
def test_downscaler_golden(name, table_ratio):
    g = load_golden(name)
    cfg, dp, ds = _modules(g)
    ds.eval()
    assert len(ds.state_dict()) == (18 if cfg['bidirectional'] else 6) and ds.sequence_length == cfg['L']
    res = {path: _run(path, g, dp, ds, table_ratio) for path in ('table', 'plain', 'embedded')}
    for path, (z, grads) in res.items():
        e = rel_err(z, g['z'])
        print(f'{name} {path}: z {e:.2e}')
        assert e < FWD_TOL, (path, e)
        for k, gr in grads.items():
            ref = g['grad_emb/' + k[3:]] if k.startswith('emb') else g['grad/' + k]
            e = rel_err(gr, ref)
            print(f'{name} {path}: d {k} {e:.2e}')
            assert e < GRAD_TOL, (path, k, e)
    zt, gt = res['table']
    zp, gp = res['plain']
    assert rel_err(zt, zp) < FWD_TOL
    for k in gt:
        assert rel_err(gt[k], gp[k]) < GRAD_TOL, k


def _gru_layer64(x, w_ih, w_hh, b_ih, b_hh):
    """x (T, R, in) float64 -> all steps (T, R, H): nn.GRU's layer with h0 = 0, gate order r | z | n."""
    H = w_hh.shape[1]
    h = torch.zeros(x.shape[1], H, dtype=torch.float64)
    out = []
    for t in range(x.shape[0]):
        gi, gh = x[t] @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        u = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - u) * n + u * h
        out.append(h)
    return torch.stack(out)


def test_train_mode_dropout_is_reproducible_and_matches_float64(table_ratio):
    """Dropout 0.5 between the two layers of both stacks: two calls from the same SEEDS state give the same bits, and the
    gradients match a float64 evaluation that applies the masks train_reference computes for the same seeds (the first layer's
    output of stack s, time-major in STEP order, element index = row * H + column, seed = the s-th SEEDS.next())."""
    from vqcpc_bach_amd.utils import SEEDS
    g = load_golden('lstm_downscaler_tiny')
    cfg, dp, ds = _modules(g, dropout=0.5)
    ds.train()
    SEEDS.manual_seed(123)
    seeds = [SEEDS.next(), SEEDS.next()]
    runs = []
    for _ in range(2):
        SEEDS.manual_seed(123)
        runs.append(_run('table', g, dp, ds, table_ratio))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    # float64 evaluation
    L, H = cfg['L'], cfg['hidden']
    tokens = T(g['tokens']).reshape(-1, L)
    R = tokens.shape[0]
    P = {k[3:]: T(np.array(v)).double().requires_grad_(True) for k, v in g.items() if k.startswith('sd/')}
    E = [T(g[f'emb/{c}']).double().requires_grad_(True) for c in range(4)]
    x = torch.stack([E[p % 4][tokens[:, p]] for p in range(L)])                   # (L, R, emb)
    lasts = []
    for s, (stack, rev) in enumerate((('g_enc_fwd', False), ('g_enc_bwd', True))):
        xs = x.flip(dims=[0]) if rev else x
        y = _gru_layer64(xs, *(P[f'{stack}.{n}_l0'] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')))
        y = y * TR.dropout_scale(seeds[s], (L * R, H), 0.5).reshape(L, R, H)
        y = _gru_layer64(y, *(P[f'{stack}.{n}_l1'] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')))
        lasts.append(y[-1])
    z = torch.cat(lasts, 1) @ P['output_linear.weight'].t() + P['output_linear.bias']
    (z.reshape(g['g_z'].shape) * T(g['g_z']).double()).sum().backward()
    assert rel_err(runs[0][0], z.reshape(g['z'].shape)) < FWD_TOL
    for k, gr in runs[0][1].items():
        ref = E[int(k[3:])].grad if k.startswith('emb') else P[k].grad
        assert rel_err(gr, ref) < GRAD_TOL, k


# ---- the reference's VQCPCEncoderTrainer.epoch with LstmDownscaler -------------------------------------------------------
def _build_trainer(cfg, sd, lr):
    from vqcpc_bach_amd.data_processor.bach_cpc_data_processor import BachCPCDataProcessor
    from vqcpc_bach_amd.dataloaders.synthetic_cpc_dataloader import SyntheticCPCDataloaderGenerator
    from vqcpc_bach_amd.downscalers.lstm_downscaler import LstmDownscaler
    from vqcpc_bach_amd.encoder import Encoder
    from vqcpc_bach_amd.quantizer.vector_quantizer import ProductVectorQuantizer
    from vqcpc_bach_amd.upscalers.mlp_upscaler import MlpUpscaler
    from vqcpc_bach_amd.vqcpc_encoder_trainer import VQCPCEncoderTrainer
    dlg = SyntheticCPCDataloaderGenerator(num_blocks_left=cfg['Kl'], num_blocks_right=cfg['Kr'], num_negative_samples=cfg['N'],
                                          vocab=cfg['vocab'])
    dp = BachCPCDataProcessor(embedding_size=cfg['emb'], num_events=(cfg['Kl'] + cfg['Kr']) * 4, num_channels=4,
                              num_tokens_per_channel=cfg['vocab'], num_tokens_per_block=16)
    ds = LstmDownscaler(input_dim=cfg['emb'], output_dim=cfg['D'], num_channels=4, downscale_factors=[16],
                        hidden_size=cfg['hidden'], num_layers=cfg['layers'], dropout=0.0, bidirectional=cfg['ds_bidirectional'])
    q = ProductVectorQuantizer(codebook_size=cfg['K'], codebook_dim=cfg['D'], commitment_cost=0.25, num_codebooks=cfg['ncb'],
                               use_batch_norm=False, initialize=False, squared_l2_norm=True)
    up = MlpUpscaler(input_dim=cfg['D'], output_dim=cfg['zdim'], hidden_size=cfg['up_hidden'], dropout=0.0)
    enc = Encoder('/tmp/vqcpc_test_model', dp, ds, q, up)
    tr = VQCPCEncoderTrainer('/tmp/vqcpc_test_model', dlg, enc,
                             c_net_kwargs=dict(output_dim=cfg['cdim'], hidden_size=cfg['gru_hidden'], num_layers=2, dropout=0.0,
                                               bidirectional=False), quantization_weighting=cfg.get('qw', 0.5))
    for name in ('encoder', 'c_module', 'fks_module'):
        getattr(tr, name).load_state_dict({k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + '.')}, strict=True)
    tr.to('cuda')
    tr.init_optimizers(lr=lr, schedule_lr=False)
    assert tr.flat.check_views()
    return tr


def _epoch_fixture():
    g = load_golden('epoch_tiny_lstm')
    cfg = json.loads(str(g['cfg_json']))
    sd = {}
    for k, v in g.items():
        if k.startswith('sd0/'):
            mod, rest = k[4:].split('/', 1)
            sd[mod + '.' + rest] = T(np.array(v))
    batch = {k.split('/', 1)[1]: T(v) for k, v in g.items() if k.startswith('batch/')}
    return g, cfg, sd, batch


@pytest.mark.parametrize('path', ['table', 'plain'])
def test_epoch_golden_lstm(path, table_ratio):
    """epoch(train=False), then one training step, against the reference's VQCPCEncoderTrainer.epoch (the rules of
    tests/test_trainer_gpu.py::test_epoch_golden).  The fixture's seed was chosen, on the reference alone, so that the smallest
    top-2 distance gap is >= 1e-3 of the largest distance (no code can flip under a z within 5e-5) and at most a quarter of the
    windows of a prediction step have |margin| < 1e-5: accuracy may differ by exactly those windows."""
    table_ratio(0 if path == 'table' else INF)
    g, cfg, sd, batch = _epoch_fixture()
    assert float(g['top2_gap'].min()) >= 1e-3 * float(g['dist_max'])
    lr = float(g['lr'])
    tr = _build_trainer(cfg, sd, lr)
    tr.eval()
    with torch.no_grad():
        z_up, idx, ql = tr.encoder(batch['x_left'])
    assert torch.equal(idx.cpu(), T(g['fwd_idx'])), 'code indices must be bit-exact'
    assert rel_err(z_up.cpu(), g['fwd_zup']) < FWD_TOL
    ev = tr.epoch(iter([batch]), train=False, num_batches=1, corrupt_labels=False)
    for k in ('loss', 'loss_quantize', 'loss_contrastive'):
        assert abs(ev[k] - float(g[f'eval/{k}'])) < FWD_TOL * max(1.0, abs(float(g[f'eval/{k}']))), k
    assert ev['num_codewords'] == float(g['eval/num_codewords'])
    assert ev['num_codewords_negative'] == float(g['eval/num_codewords_negative'])
    slack = (np.abs(g['margin']) < 1e-5).astype(np.float64).mean(0)
    assert np.all(slack <= 0.25)
    assert np.all(np.abs(np.asarray(ev['accuracy']) - g['eval/accuracy']) <= slack + 1e-6), (ev['accuracy'], slack)
    # pre-clip gradients of one training step
    tr.train()
    loss, out = tr.compute_losses(batch)
    tr.flat.zero_grad()
    loss.backward()
    names = {id(p): n for n, p in tr.named_parameters()}
    for p in tr.flat.params:
        ref = g.get('grad/' + names[id(p)])
        if ref is None:
            assert float(p.grad.abs().max()) == 0.0, names[id(p)]
            continue
        e = rel_err(p.grad.cpu(), ref)
        assert e < GRAD_TOL, (names[id(p)], e)
    tr.optimizer.step(lr=lr)
    assert abs(tr.optimizer.grad_norm() - float(g['grad_total_norm'])) < 2e-4 * float(g['grad_total_norm'])
    coef = min(1.0, 5.0 / (float(g['grad_total_norm']) + 1e-6))
    after = dict(tr.named_parameters())
    for k, v in g.items():
        if not k.startswith('sd1/'):
            continue
        mod, rest = k[4:].split('/', 1)
        pname = mod + '.' + rest
        got, ref = after[pname].detach().cpu(), T(np.array(v))
        gref = g.get('grad/' + pname)
        if gref is None:
            assert torch.equal(got, ref), pname
            continue
        assert float((got - ref).abs().max()) <= 1.01 * lr + 1e-7, pname
        sig = T(np.abs(gref) * coef > 1e-4)
        if sig.any():
            assert float((got - ref)[sig].abs().max()) < 2e-2 * lr + 1e-7, pname


def test_three_eager_and_three_replayed_steps_are_bit_identical(table_ratio, gemm_mode):
    """The step with this downscaler captures and replays as a HIP graph: from the same state, three eager steps and three
    replayed ones end with bit-identical parameters (table path, the product's path at training sizes)."""
    table_ratio(0)
    g, cfg, sd, batch = _epoch_fixture()
    dev_batch = {k: v.cuda() for k, v in batch.items()}
    ends = []
    for graph in (False, True):
        tr = _build_trainer(cfg, sd, 1e-3)
        tr.train()
        tr.enable_step_graph(graph)
        try:
            for _ in range(tr.graph_warmup_steps):                   # eager in both runs: the capture follows the warm-up steps
                tr.train_step(dev_batch, train=True)
            start = tr.flat.flat.detach().clone()
            for _ in range(3):
                tr.train_step(dev_batch, train=True)
            replays = tr._graph.replays if tr._graph is not None else 0
        finally:
            tr.enable_step_graph(False)
        assert replays == (3 if graph else 0), replays
        ends.append((start.cpu(), tr.flat.flat.detach().cpu().clone()))
    assert torch.equal(ends[0][0], ends[1][0]), 'the two runs must start from the same state'
    assert not torch.equal(ends[0][0], ends[0][1])
    diff = (ends[0][1] - ends[1][1]).abs().max()
    print(f'eager vs replayed after 3 steps: max |difference| {float(diff):.3e}')
    assert torch.equal(ends[0][1], ends[1][1])
