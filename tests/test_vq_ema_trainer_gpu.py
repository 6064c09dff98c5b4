"""EMA codebooks end to end (quantizer_type 'ema'): EMAProductVectorQuantizer against the float64 reference, and
VQCPCEncoderTrainer with it -- buffers after every step against the float64 update of the recorded quantiser inputs, parameter
accounting, graph replay, checkpoints, the frozen-encoder consumer -- on a C0-sized configuration (two codebooks) without
dropout.  Bounds: tests/vq_ema_reference.py."""
import numpy as np
import pytest
import torch

import train_reference as T
import vq_ema_reference as E

pytestmark = pytest.mark.gpu
U = E.U
C_DZ = 4.0                     # as tests/test_vq_ema_kernels_gpu.py


@pytest.fixture(scope='module', autouse=True)
def _mode():
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1)
    yield
    hip.set_gemm_mode(0)


def build(qtype, model_dir, initialize=True, seed=11, lr=1e-3):
    from vqcpc_bach_amd import configs, getters
    torch.manual_seed(seed)
    config = configs.make_config('C0', dropout=0.0, quantizer_type=qtype)
    config['quantizer_kwargs'].update(num_codebooks=2, initialize=initialize)
    dlg = getters.get_dataloader_generator('bach', 'vqcpc', dict(config['dataloader_generator_kwargs'], device='cuda'))
    enc = getters.get_encoder(str(model_dir), dlg, config)
    tr = getters.get_encoder_trainer(str(model_dir), dlg, 'vqcpc', enc, config['auxiliary_networks_kwargs'])
    tr.to('cuda')
    tr.init_optimizers(lr=lr, schedule_lr=False)
    return tr, dlg


def batches(dlg, n, batch_size=8):
    gen = dlg.dataloaders(batch_size=batch_size)[0]
    out = []
    for b in gen:
        out.append({k: v.clone() for k, v in b.items()})
        if len(out) == n:
            break
    return out


def buffers(q):
    return [t.detach().clone() for t in q.ema_buffers()]


def same(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


# =====================================================================================================================
def loss_bound(z, q, squared):
    """|fp32 loss - float64 loss| per row for l = sum_t v_t^2 (v = q - z, or (q - z) + 1e-5) and its square root, times beta =
    0.25 (a power of two: exact).  d = fl(q - z): |err| <= u |d|.  v = fl(d + 1e-5): |err| <= u |d| + u |v| (squared: v = d).
    v^2: 2 |v| err_v + u v^2.  The sum of D terms adds (D - 1) u sum v^2.  sqrt: err / (2 l) + u l."""
    d = (q - z).abs()
    v = d if squared else ((q - z) + E.LOSS_EPS).abs()
    ev = U * d if squared else U * d + U * v
    D = z.shape[1]
    es = (2 * v * ev + U * v * v).sum(1) + (D - 1) * U * (v * v).sum(1)
    if squared:
        return 0.25 * es * 1.01
    l = torch.sqrt((v * v).sum(1))
    return 0.25 * (es / (2 * l) + U * l) * 1.01


@pytest.mark.parametrize('squared', [True, False])
def test_module_against_the_float64_reference(squared):
    from vqcpc_bach_amd import ops
    from vqcpc_bach_amd.quantizer.vector_quantizer import EMAProductVectorQuantizer
    R, ncb, K, dsub = 300, 2, 8, 8
    g = torch.Generator().manual_seed(5)
    q = EMAProductVectorQuantizer(codebook_size=K, codebook_dim=ncb * dsub, commitment_cost=0.25, num_codebooks=ncb,
                                  initialize=False, squared_l2_norm=squared).cuda()
    assert list(q.parameters()) == []
    q.embeddings.copy_(torch.randn(ncb, K, dsub, generator=g))
    q.reset_ema()
    z = torch.randn(R, ncb * dsub, generator=g)
    g_zq, g_loss = torch.randn(R, ncb * dsub, generator=g), torch.randn(R, generator=g)
    zd = z.cuda().requires_grad_(True)
    q.train()
    before = buffers(q)
    zq, idx, loss = q(zd)
    ((zq * g_zq.cuda()).sum() + (loss * g_loss.cuda()).sum()).backward()
    torch.cuda.synchronize()
    assert same(before, buffers(q)), 'forward / backward alone never move the buffers'
    cb = q.embeddings.cpu()
    assert torch.equal(idx, ops.vq_assign(zd.detach(), q.embeddings)) and torch.equal(idx.cpu(), E.nearest(z, cb))
    zq64, loss64 = E.forward(z, cb, idx, 0.25, squared)
    qq = E.lookup(cb, idx)
    assert bool(((zq.detach().cpu().double() - zq64).abs() <= 2 * U * ((qq - z.double()).abs() + zq64.abs())).all())
    lerr = (loss.detach().cpu().double() - loss64).abs()
    assert bool((lerr <= loss_bound(z.double(), qq, squared)).all()), float(lerr.max())
    ref = E.d_z(z, cb, idx, g_zq, g_loss, 0.25, squared)
    plain = E.d_z(z, cb, idx, g_zq, g_loss, 0.25, squared, dtype=torch.float32)
    ek, ep = float(T.row_err(zd.grad.cpu(), ref).max()), float(T.row_err(plain, ref).max())
    print(f'MODULE DZ sq{int(squared)}: kernel {ek:.3e} plain {ep:.3e} ratio {ek / ep:.2f}')
    assert ek <= C_DZ * ep
    # the statistics of the training forward, and the update they feed
    n, s, a = E.stats(z, idx, K)
    st = q.stats.cpu().double()
    assert torch.equal(st[..., 0], n) and bool(((st[..., 1:] - s).abs() <= E.sum_bound(n, a)).all())
    q.apply_update()
    torch.cuda.synchronize()
    gc, hc, eps = E.constants(q.decay, q.epsilon)
    check_update(before, buffers(q), q.stats, z, idx, K, (gc, hc, eps))


def check_update(before, after, stats_dev, z, idx, K, consts):
    """after == float64 update of (before, statistics of (z, idx)) within the bounds; counts exact."""
    g, h, eps = consts
    e0, N0, m0 = (t.cpu() for t in before)
    n, s, a = E.stats(z, idx, K)
    st = stats_dev.cpu().double()
    assert torch.equal(st[..., 0], n), 'counts must be exact'
    s_err = E.sum_bound(n, a)
    rN, rm, re = E.update(N0, m0, n, s, g, h, eps)
    bN, bm, be = E.ema_bounds(N0, m0, n, s, g, h, eps, s_err=s_err)
    e1, N1, m1 = (t.cpu().double() for t in after)
    for name, got, ref, bound in (('N', N1, rN, bN), ('m', m1, rm, bm), ('e', e1, re, be)):
        err = (got - ref).abs()
        assert bool((err <= bound).all()), (name, float((err - bound).max()))


def test_eval_and_no_grad_leave_every_buffer_unchanged():
    from vqcpc_bach_amd.quantizer.vector_quantizer import EMAProductVectorQuantizer
    q = EMAProductVectorQuantizer(codebook_size=8, codebook_dim=8, commitment_cost=0.25, num_codebooks=2, initialize=False,
                                  squared_l2_norm=True).cuda()
    q.stats.fill_(7.0)
    before = buffers(q) + [q.stats.clone()]
    z = torch.randn(64, 8, device='cuda')
    q.eval()
    q(z)
    q.train()
    with torch.no_grad():
        q(z, corrupt_labels=True)
    torch.cuda.synchronize()
    assert same(before, buffers(q) + [q.stats])


# =====================================================================================================================
def test_three_training_steps_follow_the_float64_update(tmp_path):
    """A forward hook records the quantiser's input and the buffers as the forward left them (after the data-dependent
    initialisation of step 1, before the update); after each step N, m and e equal the float64 update within the bounds."""
    from vqcpc_bach_amd import ops
    tr, dlg = build('ema', tmp_path / 'a')
    q = tr.encoder.quantizer
    assert q.initialize and list(q.parameters()) == []
    rec = {}

    def hook(mod, args, output):
        rec['z'] = args[0].detach().reshape(-1, mod.codebook_dim).clone()
        rec['before'] = buffers(mod)

    handle = q.register_forward_hook(hook)
    tr.train()
    consts = E.constants(q.decay, q.epsilon)
    try:
        for i, b in enumerate(batches(dlg, 3)):
            out = tr.train_step(b, train=True)
            torch.cuda.synchronize()
            if i == 0:
                assert not q.initialize and torch.equal(rec['before'][0], rec['before'][2]), 'after the data init m = e'
                assert bool((rec['before'][1] == 1).all()), 'after the data init N = 1'
            idx = ops.vq_assign(rec['z'], rec['before'][0])
            K = q.codebook_size
            check_update(rec['before'], buffers(q), q.stats, rec['z'].cpu(), idx.cpu(), K, consts)
            assert float(q.stats[..., 0].sum()) == rec['z'].shape[0] * q.num_codebooks
            assert np.isfinite(float(out['loss']))
            assert not torch.equal(rec['before'][0], q.embeddings), 'the codebooks moved'
    finally:
        handle.remove()
    # evaluation steps move nothing
    before = buffers(q) + [q.stats.clone()]
    tr.eval()
    tr.train_step(batches(dlg, 1)[0], train=False)
    tr.train()
    tr.train_step(batches(dlg, 1)[0], train=False)
    torch.cuda.synchronize()
    assert same(before, buffers(q) + [q.stats])


def test_codebooks_are_outside_the_flat_parameter_buffer(tmp_path):
    from vqcpc_bach_amd.quantizer.vector_quantizer import EMAProductVectorQuantizer, ProductVectorQuantizer
    ema, _ = build('ema', tmp_path / 'a', initialize=False)
    com, _ = build('commitment', tmp_path / 'b', initialize=False)
    qe, qc = ema.encoder.quantizer, com.encoder.quantizer
    assert isinstance(qe, EMAProductVectorQuantizer) and isinstance(qc, ProductVectorQuantizer)
    cells = qe.num_codebooks * qe.codebook_size * (qe.codebook_dim // qe.num_codebooks)
    count = lambda tr: sum(p.numel() for p in tr.flat.params)
    assert count(ema) == count(com) - cells and ema.flat.numel == com.flat.numel - cells
    lo, hi = ema.flat.flat.data_ptr(), ema.flat.flat.data_ptr() + 4 * ema.flat.numel
    assert all(not (lo <= t.data_ptr() < hi) for t in qe.ema_buffers())
    # regression guard: the commitment quantiser's codebooks are parameters inside the flat buffer, as before
    lo, hi = com.flat.flat.data_ptr(), com.flat.flat.data_ptr() + 4 * com.flat.numel
    assert len(list(qc.parameters())) == qc.num_codebooks and all(lo <= p.data_ptr() < hi for p in qc.parameters())
    assert com.flat.check_views() and ema.flat.check_views()


def test_replayed_steps_are_the_eager_steps_bit_for_bit(tmp_path):
    """Each replayed step against an eager twin that starts the step from the SAME state (parameters, Adam moments and count, EMA
    buffers copied over before the step): the loss and the three buffers after the step are bit-identical.  (Whole trajectories are
    compared per step, not end to end: the captured Adam takes its bias corrections from pow() on the device, an ulp apart from the
    host's, which is the documented difference of tests/test_graphs_gpu.py and none of this quantiser's.)"""
    tr, dlg = build('ema', tmp_path / 'a')
    twin, _ = build('ema', tmp_path / 'b')
    tr.train(), twin.train()
    tr.enable_step_graph(True)
    bs = batches(dlg, 6)
    try:
        for i, b in enumerate(bs):
            if i >= 1:          # step 0: each trainer's own data-dependent initialisation
                twin.flat.flat.copy_(tr.flat.flat)
                twin.optimizer.m.copy_(tr.optimizer.m)
                twin.optimizer.v.copy_(tr.optimizer.v)
                twin.optimizer.step_count = tr.optimizer.step_count
                for dst, src in zip(twin.encoder.quantizer.ema_buffers(), tr.encoder.quantizer.ema_buffers()):
                    dst.copy_(src)
            la = tr.train_step(b, train=True)['loss'].clone()
            lb = twin.train_step(b, train=True)['loss'].clone()
            torch.cuda.synchronize()
            if i >= 1:
                assert same([la], [lb]), (i, float(la), float(lb))
                assert same(buffers(tr.encoder.quantizer), buffers(twin.encoder.quantizer)), i
        assert tr._graph is not None and tr._graph.replays == len(bs) - tr.graph_warmup_steps - 1      # step 0 (init) is not a warm-up step
        assert len(tr._graph.stages) == 1, 'one graph per step on one rank'
    finally:
        tr.enable_step_graph(False)


def test_checkpoints_round_trip_and_a_commitment_checkpoint_loads(tmp_path):
    tr, dlg = build('ema', tmp_path / 'a')
    tr.train()
    for b in batches(dlg, 2):
        tr.train_step(b, train=True)
    tr.save(early_stopped=False)
    other, _ = build('ema', tmp_path / 'a', seed=12)
    assert not same(buffers(tr.encoder.quantizer), buffers(other.encoder.quantizer))
    other.load(early_stopped=False, device='cuda')
    assert same(buffers(tr.encoder.quantizer), buffers(other.encoder.quantizer)) and not other.encoder.quantizer.initialize
    com, _ = build('commitment', tmp_path / 'c', initialize=False)
    com.save(early_stopped=False)
    cont, _ = build('ema', tmp_path / 'c', seed=13)
    cont.load(early_stopped=False, device='cuda')
    e, N, m = cont.encoder.quantizer.ema_buffers()
    want = torch.stack([p.detach() for p in com.encoder.quantizer.embeddings])
    assert torch.equal(e, want) and torch.equal(m, want) and bool((N == 1).all())
    cont.init_optimizers(lr=1e-3, schedule_lr=False)        # as train_model() does after load(): the resume state is applied
    cont.train()
    out = cont.train_step(batches(dlg, 1)[0], train=True)
    assert np.isfinite(float(out['loss'])) and not torch.equal(cont.encoder.quantizer.embeddings, want)


def test_frozen_encoder_consumers_read_the_buffers(tmp_path):
    from vqcpc_bach_amd import ops
    tr, dlg = build('ema', tmp_path / 'a')
    tr.train()
    b = batches(dlg, 1)[0]
    tr.train_step(b, train=True)
    enc = tr.encoder
    enc.eval()
    x = b['x_left']
    idx = enc.encode_indices(x)
    rec = {}
    h = enc.quantizer.register_forward_hook(lambda mod, args, out: rec.update(z=args[0].detach().reshape(-1, mod.codebook_dim)))
    with torch.no_grad():
        _, idx_fwd, _ = enc(x)
    h.remove()
    want = ops.vq_assign(rec['z'], enc.quantizer.embeddings).view(idx.shape)
    assert torch.equal(idx, want) and torch.equal(idx, idx_fwd)
    merged = enc.encode_indices(x, merged=True)
    assert torch.equal(merged, idx[..., 0] + idx[..., 1] * enc.quantizer.codebook_size)
    m = tr.epoch(iter([b]), train=False, num_batches=1, corrupt_labels=False)
    assert 1 <= m['num_codewords'] <= enc.quantizer.codebook_size ** 2


def test_label_corruption_keeps_the_statistics_of_the_nearest_codes(tmp_path):
    from vqcpc_bach_amd import ops
    tr, dlg = build('ema', tmp_path / 'a', initialize=False)
    q = tr.encoder.quantizer
    rec = {}
    h = q.register_forward_hook(lambda mod, args, out: rec.update(z=args[0].detach().reshape(-1, mod.codebook_dim).clone(),
                                                                  idx=out[1].reshape(-1, mod.num_codebooks).clone()))
    tr.train()
    before = buffers(q)
    tr.train_step(batches(dlg, 1)[0], train=True, corrupt_labels=True)
    torch.cuda.synchronize()
    h.remove()
    near = ops.vq_assign(rec['z'], before[0])
    assert not torch.equal(near, rec['idx']), 'some labels were corrupted'
    n = E.stats(rec['z'].cpu(), near.cpu(), q.codebook_size)[0]
    assert torch.equal(q.stats[..., 0].cpu().double(), n)
