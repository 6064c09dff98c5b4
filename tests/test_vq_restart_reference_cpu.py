"""Dead-code restarts without a GPU: the numpy reference (tests/vq_restart_reference.py) checked on its own -- the hash against
Python integers, the candidates as a function of their arguments, the rank split, the coverage of the rows, the restart rule --
and the host side of the option (constructor, getters, configs, state_dict keys, host-side refusals of the entry points)."""
import numpy as np
import pytest
import torch

import vq_restart_reference as Rr


def z_of(R, D, seed):
    return np.random.RandomState(seed).randn(R, D).astype(np.float32)


def test_hash_on_arrays_equals_the_hash_on_python_integers():
    vals = [0, 1, Rr.GOLDEN, Rr.M64, 1234567890123456789]
    got = Rr.mix(np.array(vals, dtype=np.uint64))
    assert [int(v) for v in got] == [Rr.mix(v) for v in vals]
    # draws() is the two-level formula of the header, spelt out on Python integers
    seed, step, ncb, K = 7, 41, 2, 5
    key = Rr.mix((seed + (step + 1) * Rr.GOLDEN) & Rr.M64)
    want = [[Rr.mix((key + (c * K + k + 1) * Rr.GOLDEN) & Rr.M64) for k in range(K)] for c in range(ncb)]
    assert Rr.draws(seed, step, ncb, K).tolist() == want
    # seeds near 2^64 wrap
    assert Rr.draws(Rr.M64, 3, 1, 4).tolist() == Rr.draws(-1 & Rr.M64, 3, 1, 4).tolist()


def test_candidates_are_a_pure_function_of_their_arguments():
    z = z_of(37, 8, 0)
    a = Rr.candidates([z], 5, 9, 2, 6)[0]
    b = Rr.candidates([z.copy()], 5, 9, 2, 6)[0]
    assert a.tobytes() == b.tobytes() and a.shape == (2, 6, 4) and a.dtype == np.float32
    assert Rr.candidates([z], 5, 10, 2, 6)[0].tobytes() != a.tobytes(), 'another step draws other rows'
    assert Rr.candidates([z], 6, 9, 2, 6)[0].tobytes() != a.tobytes(), 'another seed draws other rows'
    # each candidate IS sub-vector c of the drawn row
    r = Rr.rows(5, 9, 2, 6, 37)
    for c in range(2):
        for k in range(6):
            assert np.array_equal(a[c, k], z[r[c, k], c * 4:(c + 1) * 4])


@pytest.mark.parametrize('world', [1, 2, 3])
def test_rank_candidates_have_disjoint_supports_and_sum_to_the_one_rank_result(world):
    R, ncb, K, dsub = 23, 2, 64, 3
    zs = [np.abs(z_of(R, ncb * dsub, 10 + w)) + 1.0 for w in range(world)]          # no zero element: support = ownership
    per_rank = Rr.candidates(zs, 3, 17, ncb, K)
    one = Rr.candidates([np.concatenate(zs)], 3, 17, ncb, K)[0]
    support = sum((c != 0).astype(np.int64) for c in per_rank)
    assert int(support.max()) == 1 and int(support.min()) == 1, 'exactly one rank holds each element'
    total = per_rank[0].copy()
    for c in per_rank[1:]:
        total = total + c
    assert total.tobytes() == one.tobytes()
    if world > 1:
        assert all((c != 0).any() for c in per_rank), 'every rank owns some rows at this size'


def test_every_row_index_is_drawn():
    total, K = 1000, 256
    seen = np.zeros(total, dtype=bool)
    for step in range(256):                                   # 256 steps x 256 codes = 2^16 (step, code) pairs
        seen[Rr.rows(0, step, 1, K, total).ravel()] = True
    assert bool(seen.all()), int((~seen).sum())


def test_restart_rule_is_strict_and_a_zero_threshold_changes_nothing():
    rng = np.random.RandomState(3)
    ncb, K, dsub = 2, 7, 3
    N = rng.rand(ncb, K).astype(np.float32) + 0.6
    N[0, 1], N[0, 2], N[0, 3], N[1, 0] = 0.25, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.0
    m, e, cand = (rng.randn(ncb, K, dsub).astype(np.float32) for _ in range(3))
    N1, m1, e1, cnt = Rr.restart(cand, N, m, e, 0.5)
    dead = np.zeros((ncb, K), dtype=bool)
    dead[0, 1] = dead[0, 3] = dead[1, 0] = True               # N == thr (0, 2) is left alone
    assert cnt.tolist() == [2, 1]
    assert np.array_equal(e1[dead], cand[dead]) and np.array_equal(m1[dead], cand[dead]) and bool((N1[dead] == 1).all())
    for new, old in ((N1, N), (m1, m), (e1, e)):
        assert new[~dead].tobytes() == old[~dead].tobytes()
    N0, m0, e0, cnt0 = Rr.restart(cand, N, m, e, 0.0)
    assert cnt0.tolist() == [0, 0] and N0.tobytes() == N.tobytes() and m0.tobytes() == m.tobytes() and e0.tobytes() == e.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# host-side pieces
def quantizer(**kw):
    from vqcpc_bach_amd.quantizer.vector_quantizer import EMAProductVectorQuantizer
    return EMAProductVectorQuantizer(codebook_size=6, codebook_dim=8, commitment_cost=0.25, num_codebooks=2, initialize=False,
                                     squared_l2_norm=True, **kw)


def test_constructor_defaults_are_off_and_a_negative_threshold_raises():
    q = quantizer()
    assert q.restart_threshold == 0.0 and q.restart_seed == 0 and not q.restarting
    assert not hasattr(q, 'restart_rows') and not hasattr(q, 'restarts'), 'no buffer changes with the option absent'
    for off in (None, 0, 0.0):
        assert not quantizer(restart_threshold=off).restarting
    on = quantizer(restart_threshold=0.5, restart_seed=9)
    assert on.restarting and on.restart_threshold == 0.5 and on.restart_seed == 9
    assert tuple(on.restart_rows.shape) == (2, 6, 4) and on.restart_rows.dtype == torch.float32
    assert tuple(on.restarts.shape) == (2,) and on.restarts.dtype == torch.int32
    assert quantizer(restart_threshold=1.5).restarting, 'a threshold of 1 or more is accepted (the docstring warns)'
    for bad in (-0.5, -1e-9, float('nan')):
        with pytest.raises(ValueError, match='restart_threshold'):
            quantizer(restart_threshold=bad)


def test_state_dict_keys_are_unchanged_and_checkpoints_are_interchangeable():
    off, on = quantizer(), quantizer(restart_threshold=0.5)
    assert sorted(on.state_dict()) == sorted(off.state_dict()) == ['ema_cluster_size', 'ema_sum', 'embeddings']
    on.ema_cluster_size.mul_(0.25)
    off.load_state_dict(on.state_dict(), strict=True)
    for a, b in zip(on.ema_buffers(), off.ema_buffers()):
        assert torch.equal(a, b)
    off.embeddings.add_(1.0)
    on.load_state_dict(off.state_dict(), strict=True)
    assert torch.equal(on.embeddings, off.embeddings)


def test_getters_and_configs_pass_the_option_on_and_commitment_refuses_it():
    from vqcpc_bach_amd import configs, getters
    from vqcpc_bach_amd.quantizer.vector_quantizer import ProductVectorQuantizer
    cfg = configs.make_config('C0', dropout=0.0, quantizer_type='ema')
    assert 'ema_restart_threshold' not in cfg['quantizer_kwargs'] and 'ema_restart_seed' not in cfg['quantizer_kwargs']
    dlg = getters.get_dataloader_generator('bach', 'vqcpc', cfg['dataloader_generator_kwargs'])
    q = getters.get_encoder('/tmp/vqcpc_restart_cpu', dlg, cfg).quantizer
    assert not q.restarting and q.restart_seed == 0
    for name in ('C0', 'SAMESEQ'):
        cfg = configs.make_config(name, dropout=0.0, quantizer_type='ema', ema_restart_threshold=0.5, ema_restart_seed=7)
        assert 'ema_restart_threshold' not in cfg and 'ema_restart_seed' not in cfg
        assert cfg['quantizer_kwargs']['ema_restart_threshold'] == 0.5 and cfg['quantizer_kwargs']['ema_restart_seed'] == 7
    cfg = configs.make_config('C0', dropout=0.0, quantizer_type='ema', ema_restart_threshold=0.5, ema_restart_seed=7)
    q = getters.get_encoder('/tmp/vqcpc_restart_cpu', dlg, cfg).quantizer
    assert q.restarting and q.restart_threshold == 0.5 and q.restart_seed == 7
    cfg['quantizer_kwargs']['ema_restart_threshold'] = -1.0
    with pytest.raises(ValueError, match='restart_threshold'):
        getters.get_encoder('/tmp/vqcpc_restart_cpu', dlg, cfg)
    cfg = configs.make_config('C0', dropout=0.0, ema_restart_threshold=0.5)
    with pytest.raises(ValueError, match='ema_restart_threshold'):
        getters.get_encoder('/tmp/vqcpc_restart_cpu', dlg, cfg)
    cfg['quantizer_kwargs']['ema_restart_threshold'] = 0          # present and zero: the commitment quantiser as always
    assert isinstance(getters.get_encoder('/tmp/vqcpc_restart_cpu', dlg, cfg).quantizer, ProductVectorQuantizer)
    with pytest.raises(TypeError):
        ProductVectorQuantizer(codebook_size=6, codebook_dim=8, commitment_cost=0.25, num_codebooks=2, use_batch_norm=False,
                               initialize=False, squared_l2_norm=True, restart_threshold=0.5)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Refusals happen before any HIP call: observable without a GPU (the pointers are never dereferenced)."""
    from vqcpc_bach_amd import hip
    lib = hip.load()
    p = 4096                                                      # a non-null placeholder
    cand = lib.vqcpc_vq_restart_candidates
    for rank, world in ((0, 0), (0, -1), (-1, 1), (1, 1), (3, 3)):
        assert cand(p, 10, 1, 4, 4, 0, 1, None, rank, world, p, None) == -1 and b'rank' in lib.vqcpc_last_error(), (rank, world)
    assert cand(p, 1 << 31, 1, 4, 4, 0, 1, None, 0, 1, p, None) == -1 and b'2^31' in lib.vqcpc_last_error()
    assert cand(p, 1 << 30, 1, 4, 4, 0, 1, None, 1, 2, p, None) == -1 and b'2^31' in lib.vqcpc_last_error()
    assert cand(p, 0, 1, 4, 4, 0, 1, None, 0, 1, p, None) == -1 and cand(None, 10, 1, 4, 4, 0, 1, None, 0, 1, p, None) == -1
    assert b'vq_restart_candidates' in lib.vqcpc_last_error()
    res = lib.vqcpc_vq_ema_restart
    assert res(p, p, p, p, 1, 0, 4, 0.5, p, None) == -1 and b'vq_ema_restart' in lib.vqcpc_last_error()
    assert res(p, p, p, p, 1, 4, 4, -0.5, p, None) == -1 and b'negative' in lib.vqcpc_last_error()
    assert res(p, p, p, p, 1, 4, 4, 0.5, None, None) == -1
