"""Decoder with `source_embedding='product'` (decoders/decoder.py, quantizer/product_embedding.py, csrc/product_codes.hip) on tiny
decoders of every type, K = 4 x ncb = 2 and K = 3 x ncb = 3.

A merged twin is built from `merged_table()` with every other parameter copied.  Everything downstream of the source rows runs
the same kernels on the same bits, so loss, logits, greedy generations (one window and long form with a middle slide) and
log-probabilities are compared for EQUALITY, and so is every gradient but the source embedding's.  That one is a different sum:

  d source_embeddings[j][k] = fp32 sum, in ascending m, of g[m] over the n rows m whose code has digit j = k        (product)
  reference                 = float64 sum over the codes v with digit j = k of the twin's fp32 d_table[v]

With A = sum |g[m]| over those rows (per element): the product's sum is within n u A of the exact sum
(product_codes_reference.sum_bound, the bound of tests/vq_ema_reference.py), and so is the reference, whose rows v carry
n_v u A_v each with sum_v n_v A_v <= n A.  Bound: 2 n u A."""
import numpy as np
import pytest
import torch

import product_codes_reference as R
from product_codes_helpers import build_decoder, merged_twin, random_inputs, tiny_cfg

pytestmark = pytest.mark.gpu

CASES = [('AC-AC', 4, 2), ('AC-F', 3, 3), ('F-F', 4, 2), ('AC-D', 3, 3)]


@pytest.fixture(autouse=True)
def fp32_gemms():
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(0)
    yield
    hip.set_gemm_mode(0)


def _loss_and_grads(dec, codes, x):
    """One forward + backward in train mode (dropout 0); returns (loss, logits, gradient of the source rows)."""
    seen = {}
    rows = type(dec).source_rows

    def hooked(c):
        out = rows(dec, c)
        out.register_hook(lambda g: seen.setdefault('g', g.detach().clone()))
        return out
    dec.source_rows = hooked
    try:
        dec.train()
        loss, logits, _, _ = dec.compute_loss(codes, dec.data_processor.preprocess(x))
        dec.flat.zero_grad()
        loss.backward()
    finally:
        del dec.source_rows
    return loss.detach(), [lg.detach() for lg in logits], seen['g']


@pytest.mark.parametrize('kind,K,ncb', CASES)
def test_product_decoder_equals_its_merged_twin(kind, K, ncb):
    cfg = tiny_cfg(K, ncb)
    dec = build_decoder(cfg, kind, 'product', seed=20 + K)
    twin = merged_twin(cfg, kind, dec)
    assert dec.source_embeddings.weight.shape == (ncb, K, cfg['dec_d'])
    assert twin.source_embeddings.weight.shape == (K ** ncb, cfg['dec_d'])
    B = cfg['B']
    codes, x = random_inputs(cfg, B, seed=5)
    codes[0, 0], codes[0, 1] = 0, K ** ncb - 1

    # forward of the public entry: loss and logits
    dec.eval(), twin.eval()
    with torch.no_grad():
        a, b = dec.forward(codes, x), twin.forward(codes, x)
    assert torch.equal(a['loss'], b['loss'])
    for la, lb in zip(a['weights_per_category'], b['weights_per_category']):
        assert torch.equal(la, lb)

    # gradients
    loss_a, logits_a, g_a = _loss_and_grads(dec, codes, x)
    loss_b, logits_b, g_b = _loss_and_grads(twin, codes, x)
    assert torch.equal(loss_a, loss_b) and all(torch.equal(p, q) for p, q in zip(logits_a, logits_b))
    assert torch.equal(g_a, g_b)
    named_a = {k: p for k, p in dec.named_parameters() if not k.startswith('encoder.')}
    named_b = {k: p for k, p in twin.named_parameters() if not k.startswith('encoder.')}
    assert set(named_a) == set(named_b)
    for k, p in named_a.items():
        if k != 'source_embeddings.weight':
            assert torch.equal(p.grad, named_b[k].grad), k
    mine = named_a['source_embeddings.weight'].grad.cpu().double().numpy()
    d_table = named_b['source_embeddings.weight'].grad.cpu().double().numpy()
    flat = codes.reshape(-1).cpu().numpy()
    _, _, (n, A), _ = R.segment_sums(g_a.cpu().numpy(), flat, ncb, K)
    dig = R.digits(np.arange(K ** ncb), ncb, K)
    ref = np.stack([np.stack([d_table[dig[j] == k].sum(0) for k in range(K)]) for j in range(ncb)])
    bound = 2 * R.sum_bound(n, A)
    err = np.abs(mine - ref)
    print(f'{kind} {ncb} x {K}: d source_embeddings max error {err.max():.3e}, smallest slack {(bound - err).min():.3e}')
    assert (err <= bound).all()
    assert (mine[n == 0] == 0).all()                                   # rows no code of the batch refers to: exactly 0
    assert all(p.grad is None for k, p in dec.named_parameters() if k.startswith('encoder.'))

    # greedy generation from one window of codes, with the emitted tokens' log-probabilities
    ta, pa = dec.generate_from_codes(codes, top_k=1, seed=3, return_logp=True)
    tb, pb = twin.generate_from_codes(codes, top_k=1, seed=3, return_logp=True)
    assert torch.equal(ta, tb) and torch.equal(pa, pb)

    # long form: S + 3 codes, so windows at the head, in the middle and at the tail
    S = dec.num_tokens_source
    long_codes, _ = random_inputs(cfg, 2, seed=6, num_codes=S + 3)
    for use_graph in (True, False):
        la, qa = dec.generate_from_code_long(long_codes, temperature=1.0, top_k=1, seed=4, use_graph=use_graph, return_logp=True)
        lb, qb = twin.generate_from_code_long(long_codes, temperature=1.0, top_k=1, seed=4, use_graph=use_graph, return_logp=True)
        assert la.shape[1] == (S + 3) * dec.num_events_per_code
        assert torch.equal(la, lb) and torch.equal(qa, qb), use_graph


def _steps(dec, batches, graph):
    dec.train()
    dec.enable_step_graph(graph)
    losses = [float(dec.train_step({'x': x}, train=True)) for x in batches]
    replays = dec._graph.replays if dec._graph is not None else 0
    dec.enable_step_graph(False)
    return losses, dec.flat.flat.detach().cpu().clone(), replays


def test_training_replay_equals_eager_learns_and_round_trips(tmp_path):
    from vqcpc_bach_amd import hip
    cfg = tiny_cfg(4, 2, B=4)
    gen = torch.Generator().manual_seed(9)
    batches = [torch.stack([torch.randint(0, nv - 3, (cfg['B'], cfg['events']), generator=gen) for nv in cfg['vocab']], dim=2).cuda()
               for _ in range(5)]
    hip.set_gemm_mode(1)                                               # the training default
    res = {}
    for graph in (False, True):
        dec = build_decoder(cfg, 'AC-AC', 'product', lr=2e-3, seed=31)
        res[graph] = _steps(dec, batches, graph)
    assert res[False][2] == 0 and res[True][2] > 0
    assert np.allclose(res[False][0], res[True][0], rtol=1e-6, atol=0), (res[False][0], res[True][0])
    assert float((res[False][1] - res[True][1]).abs().max()) < 1e-6 * float(res[False][1].abs().max())

    dec = build_decoder(cfg, 'AC-AC', 'product', lr=2e-3, seed=32)
    dec.model_dir = str(tmp_path)
    data = [{'x': batches[0]}] * 40
    first = dec.epoch(iter(data[:1]), train=False, num_batches=1)['loss']
    before = dec.source_embeddings.weight.detach().clone()
    dec.epoch(iter(data), train=True, num_batches=40)
    last = dec.epoch(iter(data[:1]), train=False, num_batches=1)['loss']
    assert last < 0.8 * first, (first, last)                           # memorises one batch
    assert not torch.equal(before, dec.source_embeddings.weight)      # the per-codebook rows are trained
    dec.save(early_stopped=False)
    saved = torch.load(f'{tmp_path}/overfitted/decoder')
    assert saved['source_embeddings.weight'].shape == (2, 4, cfg['dec_d'])
    dec2 = build_decoder(cfg, 'AC-AC', 'product', lr=2e-3, seed=33)
    dec2.model_dir = str(tmp_path)
    dec2.load(early_stopped=False, device='cuda')
    dec2.init_optimizers(lr=2e-3, schedule_lr=False)
    assert dec2.global_step == dec.global_step == 40
    assert abs(dec2.epoch(iter(data[:1]), train=False, num_batches=1)['loss'] - last) < 1e-6
    for (k, p), (_, p2) in zip(dec.named_parameters(), dec2.named_parameters()):
        assert torch.equal(p, p2), k


def test_flat_buffer_at_2_x_512_is_smaller_by_the_merged_table():
    """Construction only: at K = 512, ncb = 2, d_model = 512 the merged source table has 262 144 rows (512 MB), the product one
    1 024.  The flat parameter buffers differ by exactly (V - ncb K) d_model floats."""
    K, ncb, d = 512, 2, 512
    cfg = tiny_cfg(K, ncb, dec_d=d, dec_H=2, dec_enc_layers=1, dec_dec_layers=1, dec_ff=64)
    prod = build_decoder(cfg, 'AC-AC', 'product', seed=1)
    n_prod = prod.flat.numel
    assert prod.source_embeddings.weight.shape == (ncb, K, d)
    lo, hi = prod.flat.flat.data_ptr(), prod.flat.flat.data_ptr() + 4 * n_prod
    assert lo <= prod.source_embeddings.weight.data_ptr() < hi
    del prod
    merged = build_decoder(cfg, 'AC-AC', 'merged', seed=1)
    assert merged.flat.numel - n_prod == (K ** ncb - ncb * K) * d
