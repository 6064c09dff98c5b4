"""The float64 references of tests/aligned_reference.py, pinned on what the reference's own aligned layer computed
(tests/golden/decoder_layer_aligned_S3_T48.npz: C = cross_attn(memory rows) from a forward hook and the expanded tgt2 that
enters dropout2) and on torch's ELU; reduce must be the exact adjoint of expand."""
import numpy as np
import pytest
import torch

import aligned_reference as A
from conftest import load_golden

SHAPES = [(1, 1, 1, 1, 4), (3, 3, 4, 4, 32), (2, 3, 3, 2, 5), (3, 1, 1, 4, 8), (1, 3, 4, 1, 12)]      # n, S, nc, epc, d


def _rows(x):
    """time-first (L, n, w) -> batch-major rows (n * L, w)"""
    return np.ascontiguousarray(np.transpose(x, (1, 0, 2))).reshape(-1, x.shape[2])


def test_expand_reproduces_the_reference_layer():
    g = load_golden('decoder_layer_aligned_S3_T48')
    nc = int(g['nc'])
    S, n, w = g['C'].shape
    T, _, d = g['tgt2'].shape
    assert w == nc * d and T % S == 0
    out = A.expand(_rows(g['C']), n, S, T, T // S, nc, dtype=np.float32)
    assert out.dtype == np.float32 and np.array_equal(out, _rows(g['tgt2']))
    for pos in (0, 1, T // S - 1, T // S, T - 1):
        h = np.zeros((n, d), np.float32)
        assert np.array_equal(A.step_add(h, _rows(g['C']), pos, S, T // S, nc, dtype=np.float32), out.reshape(n, T, d)[:, pos])


@pytest.mark.parametrize('n,S,nc,epc,d', SHAPES)
def test_partial_prefix_is_the_head_of_the_full_expand(n, S, nc, epc, d):
    U = nc * epc
    C = np.random.default_rng(1).standard_normal((n * S, nc * d))
    full = A.expand(C, n, S, S * U, U, nc).reshape(n, S * U, d)
    for P in sorted({0, 1, U - 1, min(U + 1, S * U), S * U}):
        assert np.array_equal(A.expand(C, n, S, P, U, nc).reshape(n, P, d), full[:, :P])


@pytest.mark.parametrize('n,S,nc,epc,d', SHAPES)
def test_reduce_is_the_adjoint_of_expand(n, S, nc, epc, d):
    """<expand(C), G> == <C, reduce(G)>: integer-valued float64 data, so both sides are exact."""
    U = nc * epc
    r = np.random.default_rng(2)
    C = r.integers(-8, 9, (n * S, nc * d)).astype(np.float64)
    G = r.integers(-8, 9, (n * S * U, d)).astype(np.float64)
    assert float((A.expand(C, n, S, S * U, U, nc) * G).sum()) == float((C * A.reduce(G, n, S, U, nc)).sum())
    assert np.array_equal(A.reduce_abs(G, n, S, U, nc), A.reduce(np.abs(G), n, S, U, nc))


def test_elu_matches_torch_in_float64():
    x = torch.cat([torch.tensor([0.0, -0.0, 1e-40, -1e-40, -88.0, 88.0, -1e-7, 1e-7], dtype=torch.float64),
                   torch.randn(1000, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 4]).requires_grad_()
    g = torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    y = torch.nn.functional.elu(x)
    y.backward(g)
    assert np.allclose(A.elu(x.detach().numpy()), y.detach().numpy(), rtol=1e-14, atol=0)
    assert np.allclose(A.elu_grad(x.detach().numpy(), g.numpy()), x.grad.numpy(), rtol=1e-14, atol=0)
