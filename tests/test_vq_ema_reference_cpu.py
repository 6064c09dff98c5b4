"""Pins of tests/vq_ema_reference.py (no GPU): the closed-form loss and d_z against torch float64 autograd for both `squared`
forms, the vectorised update against a plain loop over k, the statistics against a row loop, the bounds against an fp32
emulation of the update in numpy -- plus the host-side pieces of the EMA quantiser that need no device (module buffers, checkpoint
conversion, argument refusals of the new entry points, the student trainer's refusal)."""
import numpy as np
import pytest
import torch

import vq_ema_reference as E

F64 = torch.float64


def _case(seed, R=37, ncb=2, K=5, dsub=3):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(R, ncb * dsub, generator=g)
    cb = torch.randn(ncb, K, dsub, generator=g)
    idx = torch.randint(0, K, (R, ncb), generator=g)
    return z, cb, idx


@pytest.mark.parametrize('squared', [True, False])
def test_loss_and_dz_against_float64_autograd(squared):
    z, cb, idx = _case(1)
    beta = 0.25
    g = torch.Generator().manual_seed(2)
    g_zq, g_loss = torch.randn(z.shape, generator=g).double(), torch.randn(z.shape[0], generator=g).double()
    zz = z.double().requires_grad_(True)
    q = E.lookup(cb, idx)
    out = zz + (q - zz).detach()                                  # straight-through
    if squared:
        l = ((q - zz) ** 2).sum(1)
    else:
        l = torch.linalg.vector_norm((q - zz) + E.LOSS_EPS, dim=1)
    loss = beta * l
    (out * g_zq).sum().add((loss * g_loss).sum()).backward()
    out_ref, loss_ref = E.forward(z, cb, idx, beta, squared)
    assert torch.equal(out_ref, out.detach())
    assert torch.allclose(loss_ref, loss.detach(), rtol=1e-14, atol=0)
    dz = E.d_z(z, cb, idx, g_zq, g_loss, beta, squared)
    assert torch.allclose(dz, zz.grad, rtol=1e-12, atol=1e-14)


def test_statistics_against_a_row_loop():
    z, cb, idx = _case(3, R=41, ncb=3, K=4, dsub=2)
    idx[5, 1] = -1                                                # skipped rows
    idx[6, 0] = 4
    n, s, a = E.stats(z, idx, 4)
    n2, s2 = np.zeros((3, 4)), np.zeros((3, 4, 2))
    for r in range(41):
        for c in range(3):
            k = int(idx[r, c])
            if 0 <= k < 4:
                n2[c, k] += 1
                s2[c, k] += z[r, c * 2:(c + 1) * 2].double().numpy()
    assert np.array_equal(n.numpy(), n2) and np.allclose(s.numpy(), s2, rtol=1e-14, atol=1e-15)
    assert float(n.sum()) == 41 * 3 - 2
    assert bool((a >= s.abs() - 1e-15).all())


def _update_case(seed, ncb, K, dsub):
    g = torch.Generator().manual_seed(seed)
    N = (torch.rand(ncb, K, generator=g) * 3).float()
    m = torch.randn(ncb, K, dsub, generator=g).float()
    n = torch.randint(0, 9, (ncb, K), generator=g).float()
    s = (torch.randn(ncb, K, dsub, generator=g) * n.unsqueeze(-1)).float()
    return N, m, n, s


@pytest.mark.parametrize('K', [1, 3, 17])
def test_update_against_a_plain_loop(K):
    N, m, n, s = _update_case(4, 2, K, 3)
    g, h, eps = E.constants()
    a, b = E.update(N, m, n, s, g, h, eps), E.update_loop(N, m, n, s, g, h, eps)
    for x, y in zip(a, b):
        assert torch.allclose(x, y, rtol=1e-13, atol=1e-300)


def test_constants_are_rounded_on_the_host():
    g, h, eps = E.constants(0.99, 1e-5)
    assert g == float(np.float32(0.99)) and h == float(np.float32(1.0 - 0.99)) and eps == float(np.float32(1e-5))
    assert h != float(np.float32(1.0) - np.float32(0.99))         # NOT 1.0f - g


@pytest.mark.parametrize('K', [1, 3, 512])
def test_bounds_hold_for_an_fp32_evaluation_in_another_order(K):
    """numpy fp32 with a SEQUENTIAL T (another order than the kernel's tree): the bounds are order-free and must hold."""
    N, m, n, s = _update_case(5, 2, K, 4)
    g, h, eps = E.constants()
    f = np.float32
    N1 = f(g) * N.numpy() + f(h) * n.numpy()
    m1 = f(g) * m.numpy() + f(h) * s.numpy()
    T = np.zeros(2, dtype=f)
    for k in range(K):
        T = T + N1[:, k]
    Nt = (N1 + f(eps)) / (T[:, None] + f(K) * f(eps)) * T[:, None]
    e = m1 / Nt[:, :, None]
    rN, rm, re = E.update(N, m, n, s, g, h, eps)
    bN, bm, be = E.ema_bounds(N, m, n, s, g, h, eps)
    assert bool(((torch.from_numpy(N1).double() - rN).abs() <= bN).all())
    assert bool(((torch.from_numpy(m1).double() - rm).abs() <= bm).all())
    assert bool(((torch.from_numpy(e).double() - re).abs() <= be).all())
    assert E.e_constant(K) == 2 * K + 13


def test_initial_state_is_a_fixed_point_in_exact_arithmetic():
    """N = 1, m = e: Nt = 1 and e = m / Nt exactly; an update with n = 0, s = 0 keeps e (N and m both shrink by g)."""
    g, h, eps = E.constants()
    e0 = torch.randn(2, 7, 3).float()
    N1, m1, e1 = E.update(torch.ones(2, 7), e0, torch.zeros(2, 7), torch.zeros(2, 7, 3), g, h, eps)
    assert torch.allclose(e1, e0.double(), rtol=1e-14, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# host-side pieces
def test_ema_quantizer_has_buffers_only_and_converts_a_commitment_checkpoint():
    from vqcpc_bach_amd.quantizer.vector_quantizer import EMAProductVectorQuantizer, ProductVectorQuantizer
    q = EMAProductVectorQuantizer(codebook_size=6, codebook_dim=8, commitment_cost=0.25, num_codebooks=2, initialize=False,
                                  squared_l2_norm=True)
    assert list(q.parameters()) == []
    assert sorted(q.state_dict()) == ['ema_cluster_size', 'ema_sum', 'embeddings']          # `stats` is not persistent
    assert q.decay == 0.99 and q.epsilon == 1e-5
    assert [tuple(e.shape) for e in q.embeddings] == [(6, 4), (6, 4)]
    assert torch.equal(q.ema_sum, q.embeddings) and bool((q.ema_cluster_size == 1).all())
    p = ProductVectorQuantizer(codebook_size=6, codebook_dim=8, commitment_cost=0.25, num_codebooks=2, use_batch_norm=False,
                               initialize=False, squared_l2_norm=True)
    q.ema_cluster_size.fill_(3.0)
    q.load_state_dict(p.state_dict())
    want = torch.stack([e.detach() for e in p.embeddings])
    assert torch.equal(q.embeddings, want) and torch.equal(q.ema_sum, want) and bool((q.ema_cluster_size == 1).all())
    q2 = EMAProductVectorQuantizer(codebook_size=6, codebook_dim=8, commitment_cost=0.25, num_codebooks=2, initialize=False,
                                   squared_l2_norm=True)
    q.ema_cluster_size.mul_(0.5)
    q2.load_state_dict(q.state_dict())
    for a, b in zip(q.ema_buffers(), q2.ema_buffers()):
        assert torch.equal(a, b)


def test_getters_build_the_ema_quantizer_and_the_student_trainer_refuses_it():
    from vqcpc_bach_amd import configs, getters
    from vqcpc_bach_amd.quantizer.vector_quantizer import EMAProductVectorQuantizer, ProductVectorQuantizer
    cfg = configs.make_config('C0', dropout=0.0, quantizer_type='ema')
    cfg['quantizer_kwargs'].update(ema_decay=0.9, ema_epsilon=1e-4)
    dlg = getters.get_dataloader_generator('bach', 'vqcpc', cfg['dataloader_generator_kwargs'])
    enc = getters.get_encoder('/tmp/vqcpc_ema_cpu', dlg, cfg)
    assert isinstance(enc.quantizer, EMAProductVectorQuantizer) and enc.quantizer.decay == 0.9 and enc.quantizer.epsilon == 1e-4
    cfg = configs.make_config('C0', dropout=0.0)
    assert isinstance(getters.get_encoder('/tmp/vqcpc_ema_cpu', dlg, cfg).quantizer, ProductVectorQuantizer)
    from vqcpc_bach_amd.student_encoder_trainer import StudentEncoderTrainer
    with pytest.raises(NotImplementedError, match='ema'):
        StudentEncoderTrainer('/tmp/vqcpc_ema_cpu', dlg, enc, num_events_masked=4, teacher=None, auxiliary_decoder=None,
                              quantization_weighting=0.1)


def test_new_entry_points_refuse_bad_shapes_on_the_host():
    """Refusals happen before any HIP call: observable without a GPU (the pointers are never dereferenced)."""
    import torch  # noqa: F401
    from vqcpc_bach_amd import hip
    lib = hip.load()
    assert lib.vqcpc_vq_ema_stats_workspace(34816, 2, 512, 16) == 136 * 2 * 512 * 17 * 4
    p = 4096                                                      # a non-null placeholder
    big = 1 << 40
    assert lib.vqcpc_vq_ema_stats(p, p, 10, 1, 4, 256, p, p, big, None) == -1 and b'vq_ema_stats' in lib.vqcpc_last_error()
    assert lib.vqcpc_vq_ema_stats(p, p, 10, 1, 4096, 16, p, p, big, None) == -1 and b'LDS' in lib.vqcpc_last_error()
    assert lib.vqcpc_vq_ema_stats(p, p, 1 << 24, 1, 4, 4, p, p, big, None) == -1 and b'2^24' in lib.vqcpc_last_error()
    assert lib.vqcpc_vq_ema_stats(p, p, 10, 1, 4, 4, p, p, 16, None) != 0 and b'workspace' in lib.vqcpc_last_error()
    assert lib.vqcpc_vq_ema_stats(None, p, 10, 1, 4, 4, p, p, big, None) == -1
    assert lib.vqcpc_vq_commit_bwd(None, p, p, p, p, 10, 1, 4, 4, 0.25, 1, p, None) == -1
    assert b'vq_commit_bwd' in lib.vqcpc_last_error()
    assert lib.vqcpc_vq_ema_update(p, p, p, p, 1, 0, 4, 0.99, 0.01, 1e-5, None) == -1 and b'vq_ema_update' in lib.vqcpc_last_error()
