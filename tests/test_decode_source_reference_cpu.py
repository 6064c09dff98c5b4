"""tests/decode_source_reference.py (the float64 restatement of vqcpc_decode_source_rows) against
torch.nn.functional.linear in float64 on the sliced window."""
import numpy as np
import pytest
import torch

from decode_source_reference import error_bound, source_rows, source_rows_fast


@pytest.mark.parametrize('M,nb,S,dz,N,w0', [(1, 3, 3, 4, 4, 0), (2, 7, 3, 8, 5, 4), (3, 5, 1, 12, 9, 2), (2, 6, 6, 36, 7, 0)])
@pytest.mark.parametrize('with_bias', [True, False])
def test_reference_equals_linear_on_the_window(M, nb, S, dz, N, w0, with_bias):
    g = np.random.default_rng(M * 100 + nb * 10 + dz)
    z = g.standard_normal((M, nb, dz)).astype(np.float32)
    w = g.standard_normal((N, dz)).astype(np.float32)
    b = g.standard_normal(N).astype(np.float32) if with_bias else None
    want = torch.nn.functional.linear(torch.from_numpy(z[:, w0:w0 + S]).double(), torch.from_numpy(w).double(),
                                      torch.from_numpy(b).double() if with_bias else None).reshape(M * S, N).numpy()
    got = source_rows(z, w, b, S, w0)
    assert got.shape == (M * S, N) and np.abs(got - want).max() < 1e-13
    assert np.abs(source_rows_fast(z, w, b, S, w0) - want).max() < 1e-13
    bound = error_bound(z, w, b, S, w0)
    assert bound.shape == got.shape and (bound >= 0).all()
    # an fp32 evaluation of the same rows sits inside the bound
    f32 = torch.nn.functional.linear(torch.from_numpy(z[:, w0:w0 + S]), torch.from_numpy(w),
                                     torch.from_numpy(b) if with_bias else None).reshape(M * S, N).numpy()
    assert (np.abs(f32 - want) <= bound + 1e-300).all()


def test_window_that_does_not_fit_gives_nothing():
    z, w = np.zeros((1, 4, 4), np.float32), np.zeros((2, 4), np.float32)
    assert source_rows(z, w, None, 3, w0=2) is None and source_rows(z, w, None, 3, w0=-1) is None
    assert source_rows_fast(z, w, None, 3, w0=2) is None and source_rows(z, w, None, 3, w0=1) is not None


def test_rows_do_not_depend_on_the_other_rows_or_the_offset():
    g = np.random.default_rng(5)
    z = g.standard_normal((3, 9, 8)).astype(np.float32)
    w, b = g.standard_normal((6, 8)).astype(np.float32), g.standard_normal(6).astype(np.float32)
    a = source_rows(z, w, b, 4, w0=3)
    one = source_rows(z[1:2, 3:7], w, b, 4, w0=0)
    assert np.array_equal(a[4:8], one)
