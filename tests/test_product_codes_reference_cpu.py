"""Product codes without a GPU: the restatements of tests/product_codes_reference.py pinned on torch float64 autograd over sums of
nn.Embedding lookups, the host-side refusals (limits, 'product' on a continuous encoder, unknown key values), state-dict shapes
with a strict round trip, the config keys through the getters, and the C ABI of the new entry points (declared, bound, argument
validation before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import product_codes_reference as R
from product_codes_helpers import build_decoder, tiny_cfg


def _torch_tables(tables):
    embs = [torch.nn.Embedding(tables.shape[1], tables.shape[2]).double() for _ in range(tables.shape[0])]
    for e, t in zip(embs, tables):
        e.weight.data.copy_(torch.from_numpy(np.asarray(t, dtype=np.float64)))
    return embs


@pytest.mark.parametrize('ncb,K,C,M,nj,n_extra', [(1, 5, 4, 9, 1, 0), (2, 3, 8, 40, 2, 2), (3, 4, 12, 70, 2, 1), (4, 8, 4, 33, 4, 0)])
def test_float64_restatements_equal_torch_autograd(ncb, K, C, M, nj, n_extra):
    rng = np.random.default_rng(ncb * 100 + K)
    tables = rng.standard_normal((ncb, K, C)).astype(np.float32)
    extra = rng.standard_normal((n_extra, C)).astype(np.float32) if n_extra else None
    V = K ** ncb
    idx = rng.integers(0, V + n_extra, M)
    idx[0] = V - 1
    g = rng.standard_normal((M, C)).astype(np.float32)
    embs = _torch_tables(tables)
    ex = torch.from_numpy(extra).double().requires_grad_(True) if n_extra else None
    code = torch.from_numpy(idx < V)
    safe = torch.from_numpy(np.where(idx < V, idx, 0))
    out = sum(embs[j]((safe // K ** j) % K) for j in range(nj))
    if n_extra:
        out = torch.where(code[:, None], out, ex[torch.from_numpy(np.where(idx < V, 0, idx - V))])
    mine = R.gather(tables, idx, nj=nj, extra=extra, dtype=np.float64)
    assert np.abs(mine - out.detach().numpy()).max() < 1e-14
    out.backward(torch.from_numpy(g).double())
    d_t, d_e, (n_t, a_t), (n_e, a_e) = R.segment_sums(g, idx, ncb, K, nj=nj, n_extra=n_extra)
    for j in range(ncb):
        ref = embs[j].weight.grad.numpy() if j < nj else np.zeros((K, C))
        assert np.abs(d_t[j] - ref).max() < 1e-13, j
    if n_extra:
        assert np.abs(d_e - ex.grad.numpy()).max() < 1e-13
        assert n_e.sum() == (idx >= V).sum()
    assert n_t[:nj].sum() == nj * (idx < V).sum() and (n_t[nj:] == 0).all()
    # the fp32 chain is the float64 chain to rounding, its first link exact, and the digits merge back
    f32 = R.gather(tables, idx, nj=nj, extra=extra)
    # (each of the nj - 1 adds rounds a partial sum of at most nj max|t|)
    assert f32.dtype == np.float32 and np.abs(f32 - mine).max() <= (nj - 1) * R.U * nj * np.abs(tables).max()
    assert np.array_equal(R.gather(tables, idx[idx < V], nj=1), tables[0][idx[idx < V] % K])
    assert np.array_equal(R.merge(R.digits(idx[idx < V], ncb, K), K), idx[idx < V])


def test_residual_chain_and_bound():
    rng = np.random.default_rng(3)
    tables = rng.standard_normal((3, 4, 8)).astype(np.float32)
    idx = rng.integers(0, 64, 20)
    res = rng.standard_normal((20, 8)).astype(np.float32)
    dig = R.digits(idx, 3, 4)
    want = (res + tables[0][dig[0]]) + tables[1][dig[1]]
    assert np.array_equal(R.gather(tables, idx, nj=2, res=res), want)
    g = rng.standard_normal((20, 8)).astype(np.float32)
    d_t, _, (n, a), _ = R.segment_sums(g, np.zeros(20, dtype=np.int64), 3, 4)          # all equal: the longest segment
    acc = np.zeros(8, dtype=np.float32)
    for m in range(20):
        acc = acc + g[m]
    assert n[0, 0] == 20 and (np.abs(acc - d_t[0, 0]) <= R.sum_bound(n, a)[0, 0]).all()


# ---- host-side refusals ----------------------------------------------------------------------------------------------------
def test_limits_are_refused_on_the_host():
    from vqcpc_bach_amd import ops
    from vqcpc_bach_amd.quantizer.product_embedding import ProductEmbedding
    assert ops.check_product_shape(2, 512) == 262144 and ops.check_product_shape(4, 181) == 181 ** 4
    assert ops.check_product_shape(1, 1) == 1 and ops.check_product_shape(2, 4096, 1) == 4096 ** 2
    for ncb, K, n_extra in ((0, 4, 0), (5, 2, 0), (2, 0, 0), (2, 4097, 0), (3, 4096, 0), (4, 216, 0), (1, 4, -1)):
        with pytest.raises(ValueError):
            ops.check_product_shape(ncb, K, n_extra)
    assert 215 ** 4 < 2 ** 31 <= 216 ** 4
    with pytest.raises(ValueError):
        ProductEmbedding(5, 4, 8)
    emb = ProductEmbedding(3, 4, 8)
    assert emb.weight.shape == (3, 4, 8) and emb.num_codes == 64 and list(emb.state_dict()) == ['weight']


def test_decoder_refusals_and_state_dict_shapes():
    from vqcpc_bach_amd.quantizer.vector_quantizer import NoQuantization
    cfg = tiny_cfg(4, 2)
    with pytest.raises(ValueError, match='source_embedding'):
        build_decoder(cfg, 'AC-AC', 'factorised', device=None)
    with pytest.raises(ValueError, match='quantised encoder'):
        build_decoder(tiny_cfg(4, 2, D=8), 'AC-AC', 'product', device=None, quantizer=NoQuantization(codebook_dim=8))
    with pytest.raises(ValueError):
        build_decoder(tiny_cfg(4, 5), 'AC-AC', 'product', device=None)   # five codebooks: one more than the kernels take
    merged = build_decoder(cfg, 'AC-AC', 'merged', device=None)
    assert merged.source_embeddings.weight.shape == (16, cfg['dec_d']) and merged.source_embedding == 'merged'
    for kind in ('AC-AC', 'AC-F', 'F-F', 'AC-D'):
        dec = build_decoder(cfg, kind, 'product', device=None, seed=1)
        sd = dec.state_dict()
        assert sd['source_embeddings.weight'].shape == (2, 4, cfg['dec_d'])
        assert set(sd) == set(build_decoder(cfg, kind, 'merged', device=None).state_dict())
        other = build_decoder(cfg, kind, 'product', device=None, seed=2)
        other.load_state_dict(sd, strict=True)
        assert all(torch.equal(v, other.state_dict()[k]) for k, v in sd.items())
    with pytest.raises(RuntimeError):                                  # the two formats do not load into each other
        merged.load_state_dict(build_decoder(cfg, 'AC-AC', 'product', device=None).state_dict(), strict=True)


def test_config_key_reaches_the_decoder_through_the_getters():
    from vqcpc_bach_amd import configs, getters
    assert 'source_embedding' not in configs.make_decoder_config()['decoder_kwargs']      # the default config is unchanged
    enc = configs.make_config('C1', dropout=0.0)
    enc['downscaler_kwargs'].update(d_model=32, n_head=2, list_of_num_layers=[1, 1], dim_feedforward=64)
    enc['quantizer_kwargs'].update(num_codebooks=2, codebook_size=8, codebook_dim=8, initialize=False)
    for value, shape in (('product', (2, 8, 64)), (None, (64, 64))):
        config = configs.make_decoder_config(dropout=0.0, source_embedding=value, config_encoder=enc)
        assert config['decoder_kwargs'].get('source_embedding') == value
        config['dataloader_generator_kwargs'] = dict(sequences_size=4)
        config['decoder_kwargs'].update(d_model=64, n_head=2, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=128)
        dlg = getters.get_dataloader_generator(config['dataset'], config['training_method'],
                                               dict(config['dataloader_generator_kwargs'], seed=7))
        enc_dlg = getters.get_dataloader_generator(enc['dataset'], enc['training_method'], dict(enc['dataloader_generator_kwargs'], seed=7))
        encoder = getters.get_encoder('/tmp/vqcpc_test_product_cfg', enc_dlg, enc)
        dp = getters.get_data_processor(dlg, config['data_processor_type'], config['data_processor_kwargs'])
        dec = getters.get_decoder('/tmp/vqcpc_test_product_cfg', dlg, dp, encoder, config['decoder_type'], config['decoder_kwargs'])
        assert dec.source_embeddings.weight.shape == shape
    with pytest.raises(ValueError, match='source_embedding'):
        getters.get_decoder('/tmp/vqcpc_test_product_cfg', dlg, dp, encoder, config['decoder_type'],
                            dict(config['decoder_kwargs'], source_embedding='sum'))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    return hip.load()


def test_new_symbols_are_declared_bound_and_validate_before_any_hip_call(lib):
    from test_abi import header_symbols
    from vqcpc_bach_amd import hip
    p = ctypes.c_void_p(16)
    for s in ('vqcpc_product_gather', 'vqcpc_product_gather_bwd'):
        assert s in header_symbols() and s in hip.SIGNATURES and hasattr(lib, s)

    def gather(ncb=2, K=4, nj=2, C=8, res=None, extra=None, n_extra=0, ldo=8, M=3):
        return lib.vqcpc_product_gather(p, p, res, 8, extra, n_extra, p, ldo, M, ncb, K, nj, C, None)
    for bad in (dict(ncb=0), dict(ncb=5), dict(K=0), dict(K=4097), dict(ncb=3, K=4096), dict(nj=0), dict(nj=3), dict(C=6), dict(C=0),
                dict(ldo=4), dict(ldo=9), dict(res=p, extra=p, n_extra=1), dict(extra=p), dict(n_extra=1), dict(M=-1),
                dict(ncb=4, K=215, extra=p, n_extra=2 ** 31 - 215 ** 4)):
        assert gather(**bad) == -1 and b'product_gather' in lib.vqcpc_last_error(), bad
    assert gather(M=0) == 0                                            # nothing to do: no launch

    def bwd(ncb=2, K=4, C=8, d_extra=None, n_extra=0, ldg=8, M=3, S=6, d_tables=p):
        return lib.vqcpc_product_gather_bwd(p, ldg, p, p, d_tables, d_extra, M, S, ncb, K, n_extra, C, None)
    for bad in (dict(ncb=5), dict(K=4097), dict(C=0), dict(d_tables=None), dict(d_extra=p), dict(n_extra=1), dict(M=-1), dict(S=-1)):
        assert bwd(**bad) == -1 and b'product_gather_bwd' in lib.vqcpc_last_error(), bad


# ---- the prior over product codes --------------------------------------------------------------------------------------------
def test_prior_restatement_equals_embedding_and_linear_sums_in_float64():
    """`prior_forward` with the identity in place of the stack, against nn.Embedding / nn.Linear modules and F.cross_entropy."""
    from torch import nn
    ncb, K, emb, d, B, N = 3, 4, 8, 12, 2, 5
    torch.manual_seed(1)
    E = [nn.Embedding(K, emb).double() for _ in range(ncb)]
    Dg = [nn.Embedding(K, d).double() for _ in range(ncb - 1)]
    lin = nn.Linear(emb, d).double()
    heads = [nn.Linear(d, K).double() for _ in range(ncb)]
    sos = torch.randn(1, 1, d, dtype=torch.float64)
    codes = torch.randint(0, K ** ncb, (B, N))
    dig = [(codes // K ** j) % K for j in range(ncb)]
    x = torch.cat([sos.expand(B, 1, d), lin(sum(E[j](dig[j]) for j in range(ncb)))[:, :-1]], dim=1)
    want_loss, want_logp = 0.0, 0.0
    for j in range(ncb):
        lg = heads[j](x + sum(Dg[i](dig[i]) for i in range(j)))
        want_loss = want_loss + nn.functional.cross_entropy(lg.reshape(-1, K), dig[j].reshape(-1))
        want_logp = want_logp - nn.functional.cross_entropy(lg.reshape(-1, K), dig[j].reshape(-1), reduction='none').view(B, N)
    P = {'embedding.weight': torch.stack([e.weight for e in E]), 'linear.weight': lin.weight, 'linear.bias': lin.bias, 'sos': sos,
         'digit_embeddings.weight': torch.stack([e.weight for e in Dg])}
    for j, h in enumerate(heads):
        P[f'pre_softmaxes.{j}.weight'], P[f'pre_softmaxes.{j}.bias'] = h.weight, h.bias
    loss, logits, logp = R.prior_forward(P, codes, ncb, K, lambda rows: rows)
    assert abs(float(loss - want_loss)) < 1e-13 and float((logp - want_logp).abs().max()) < 1e-13
    assert len(logits) == ncb and logits[0].shape == (B, N, K)
    assert abs(float(loss) + float(logp.mean())) < 1e-13             # the loss is minus the mean log-probability per code


def test_prior_refusals_and_state_dict_shapes():
    from product_codes_helpers import build_prior, prior_cfg
    with pytest.raises(ValueError, match='code_model'):
        build_prior(prior_cfg(4, 2), 'joint')
    with pytest.raises(ValueError):
        build_prior(prior_cfg(4, 5))                                   # five codebooks
    with pytest.raises(ValueError):
        build_prior(prior_cfg(216, 4))                                 # 216^4 >= 2^31
    cfg = prior_cfg(512, 2)
    prior = build_prior(cfg)
    sd = {k: v for k, v in prior.state_dict().items() if not k.startswith('encoder.')}
    assert sd['embedding.weight'].shape == (2, 512, cfg['p_emb']) and sd['digit_embeddings.weight'].shape == (1, 512, cfg['p_d'])
    assert [sd[f'pre_softmaxes.{j}.weight'].shape for j in range(2)] == [(512, cfg['p_d'])] * 2 and 'pre_softmaxes.2.weight' not in sd
    assert max(v.numel() for v in sd.values()) < 512 ** 2              # no tensor of K**ncb rows
    merged = build_prior(cfg, 'merged')
    assert merged.embedding.weight.shape == (512 ** 2, cfg['p_emb']) and merged.code_model == 'merged'
    assert set(prior.state_dict()) - set(merged.state_dict()) == {'pre_softmaxes.1.weight', 'pre_softmaxes.1.bias',
                                                                   'digit_embeddings.weight'}
    other = build_prior(cfg)
    other.load_state_dict(prior.state_dict(), strict=True)
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in prior.state_dict().items())
    one = build_prior(prior_cfg(32, 1))
    assert 'digit_embeddings.weight' not in one.state_dict() and one.embedding.weight.shape == (1, 32, 4)
    with pytest.raises(ValueError, match='4096'):                      # the host-side check comes before any device work
        merged.generate_codes(12)


def test_prior_symbols_validate_before_any_hip_call(lib):
    from vqcpc_bach_amd import hip
    p = ctypes.c_void_p(16)
    for s in ('vqcpc_prior_sample_product', 'vqcpc_prior_window_product'):
        assert s in hip.SIGNATURES and hasattr(lib, s)

    def sample(K=8, ncb=2, stage=0, M=3, temperature=1.0, teacher=None, cons=None, logp=None, digits=p, acc=p, h=p, dtab=p, hn=p,
               codes=p, tables=p, nxt=p, N=6, d=16, ldl=8):
        return lib.vqcpc_prior_sample_product(p, ldl, K, ncb, stage, M, temperature, 0, 1.0, p, teacher, N, cons, N, logp, N, None,
                                              digits, acc, h, d, dtab, hn, d, codes, N, N, tables, d, nxt, d, None, K, p, p, None)
    for bad in (dict(ncb=5), dict(K=4097), dict(stage=2), dict(stage=-1), dict(M=65), dict(M=0), dict(temperature=0.0),
                dict(teacher=p, cons=p), dict(teacher=p, logp=p), dict(digits=None), dict(logp=p, acc=None), dict(h=None),
                dict(dtab=None), dict(hn=None), dict(stage=1, codes=None), dict(stage=1, tables=None), dict(stage=1, nxt=None),
                dict(ldl=7), dict(N=0), dict(d=0)):
        assert sample(**bad) == -1 and b'prior_sample_product' in lib.vqcpc_last_error(), bad

    def window(K=8, ncb=2, M=3, N=6, P=2, nt=9, sos=p, prefix=p):
        return lib.vqcpc_prior_window_product(p, nt, nt, p, 1, p, N, P, prefix, p, ncb, K, sos, 16, p, 16, p, p, p, M, None)
    for bad in (dict(ncb=0), dict(K=0), dict(M=65), dict(P=6), dict(nt=5), dict(sos=None), dict(prefix=None)):
        assert window(**bad) == -1 and b'prior_window_product' in lib.vqcpc_last_error(), bad
