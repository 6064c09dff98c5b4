"""vqcpc_decode_source_rows (csrc/decode.hip), called directly through ctypes, against the float64 restatement of
tests/decode_source_reference.py.

Bound (derived, not tuned): an output element is a length-dz fp32 dot product accumulated by FMA (dz roundings) plus the bias
addition (one more); with gamma_n <= n u / (1 - n u) and u = 2^-24 the error is at most
(dz + 2) * 2^-24 * (sum_k |z_k w_nk| + |bias_n|), the +1 covering the second-order terms."""
import numpy as np
import pytest
import torch

from decode_source_reference import error_bound, source_rows_fast

pytestmark = pytest.mark.gpu
SENTINEL = -777.25


def _lib():
    from vqcpc_bach_amd import hip
    return hip.load()


def _run(z_full, w, bias, S, N, win=None, lds=None, M=None):
    """z_full (M, nb, dz) device, w (N, dz), bias (N,) -> the whole src buffer (M * S * lds + 8,) prefilled with SENTINEL."""
    from vqcpc_bach_amd import hip
    M = z_full.shape[0] if M is None else M
    nb, dz = z_full.shape[1], z_full.shape[2]
    lds = N + 3 if lds is None else lds
    src = torch.full((M * S * lds + 8,), SENTINEL, dtype=torch.float32, device='cuda')
    hip.call('vqcpc_decode_source_rows', z_full, nb, dz, win, w, bias, src, lds, M, S, N)
    return src


def _win(w0):
    return torch.tensor([w0 + 1, w0], dtype=torch.int32, device='cuda')


@pytest.mark.parametrize('dz', [4, 8, 32, 36, 256])
def test_grid_against_float64(dz):
    """dz x N {4, 32, 512, 516} x S {1, 3, 24} x M {1, 2, 64} x nb {S, S + 4} x w0 {NULL, 0, nb - S}: the componentwise bound,
    NaN rows outside the window never read, guard columns (lds = N + 3) and the tail past the last row untouched."""
    g = np.random.default_rng(1000 + dz)
    w_all = g.standard_normal((516, dz)).astype(np.float32)
    b_all = g.standard_normal(516).astype(np.float32)
    worst = 0.0
    for S in (1, 3, 24):
        for M in (1, 2, 64):
            for nb in (S, S + 4):
                z = g.standard_normal((M, nb, dz)).astype(np.float32)
                for w0 in (None, 0, nb - S):
                    off = 0 if w0 is None else w0
                    zp = np.full_like(z, np.nan)                         # poison everything outside the window
                    zp[:, off:off + S] = z[:, off:off + S]
                    zd = torch.from_numpy(zp).cuda()
                    for N in (4, 32, 512, 516):
                        w, b = w_all[:N], b_all[:N]
                        lds = N + 3
                        buf = _run(zd, torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda(), S, N,
                                   win=None if w0 is None else _win(w0)).cpu().numpy()
                        body = buf[:M * S * lds].reshape(M * S, lds)
                        got = body[:, :N].astype(np.float64)
                        assert np.isfinite(got).all(), (dz, N, S, M, nb, w0)
                        assert (body[:, N:] == SENTINEL).all() and (buf[M * S * lds:] == SENTINEL).all(), 'guards were written'
                        want = source_rows_fast(z, w, b, S, off)
                        bound = error_bound(z, w, b, S, off)
                        ratio = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
                        worst = max(worst, ratio)
                        assert ratio <= 1.0, (dz, N, S, M, nb, w0, ratio)
    print(f'dz = {dz}: worst |err| / bound = {worst:.3f}')


@pytest.mark.parametrize('dz,N,S', [(4, 4, 1), (32, 512, 24), (36, 516, 3), (256, 32, 24)])
def test_a_row_is_bit_identical_across_M_b_and_w0(dz, N, S):
    g = np.random.default_rng(7 + dz)
    L = g.standard_normal((S, dz)).astype(np.float32)
    w = torch.from_numpy(g.standard_normal((N, dz)).astype(np.float32)).cuda()
    b = torch.from_numpy(g.standard_normal(N).astype(np.float32)).cuda()
    alone = _run(torch.from_numpy(L[None]).cuda(), w, b, S, N, lds=N)[:S * N].view(S, N)
    for M, nb, w0 in ((64, S + 4, 4), (2, S + 4, 0), (2, S, None), (64, S + 4, 1)):
        z = g.standard_normal((M, nb, dz)).astype(np.float32)
        off = 0 if w0 is None else w0
        z[:, off:off + S] = L
        out = _run(torch.from_numpy(z).cuda(), w, b, S, N, win=None if w0 is None else _win(w0), lds=N)[:M * S * N].view(M, S, N)
        for bi in range(M):
            assert torch.equal(out[bi], alone), (M, nb, w0, bi)
    # a row among DIFFERENT rows: sequence 1 of a random batch equals the sequence alone
    z = g.standard_normal((3, S + 4, dz)).astype(np.float32)
    out = _run(torch.from_numpy(z).cuda(), w, b, S, N, win=_win(2), lds=N)[:3 * S * N].view(3, S, N)
    one = _run(torch.from_numpy(z[1:2, 2:2 + S].copy()).cuda(), w, b, S, N, lds=N)[:S * N].view(S, N)
    assert torch.equal(out[1], one)


def test_a_window_that_does_not_fit_leaves_src_untouched():
    S, nb, dz, N, M = 3, 7, 8, 32, 2
    z = torch.randn(M, nb, dz, device='cuda')
    w, b = torch.randn(N, dz, device='cuda'), torch.randn(N, device='cuda')
    for w0 in (-1, nb - S + 1, nb):
        buf = _run(z, w, b, S, N, win=_win(w0))
        assert bool((buf == SENTINEL).all()), w0
    buf = _run(z, w, b, S, N, win=_win(nb - S))
    assert not bool((buf[:N] == SENTINEL).any())
    # bias == NULL is accepted: the plain product
    a = _run(z, w, None, S, N, lds=N)[:M * S * N].view(M * S, N)
    ref = torch.from_numpy(source_rows_fast(z.cpu().numpy(), w.cpu().numpy(), None, S, 0))
    assert float((a.cpu().double() - ref).abs().max()) < 1e-4


def test_bad_arguments_are_rejected_without_a_launch():
    from vqcpc_bach_amd import hip
    lib = _lib()
    st = hip._stream()
    z = torch.zeros(65 * 4 * 260, device='cuda')
    w = torch.zeros(8 * 260, device='cuda')
    src = torch.full((65 * 4 * 8,), SENTINEL, device='cuda')
    f = lib.vqcpc_decode_source_rows
    EINVAL = -1
    assert f(z.data_ptr(), 4, 6, None, w.data_ptr(), None, src.data_ptr(), 8, 2, 4, 8, st) == EINVAL      # dz % 4
    assert b'decode_source_rows' in lib.vqcpc_last_error()
    assert f(z.data_ptr(), 4, 8, None, w.data_ptr(), None, src.data_ptr(), 8, 65, 4, 8, st) == EINVAL     # M = 65
    assert f(z.data_ptr(), 4, 260, None, w.data_ptr(), None, src.data_ptr(), 8, 2, 4, 8, st) == EINVAL    # dz = 260
    assert f(z.data_ptr(), 3, 8, None, w.data_ptr(), None, src.data_ptr(), 8, 2, 4, 8, st) == EINVAL      # nb < S
    assert f(z.data_ptr(), 4, 8, None, w.data_ptr(), None, src.data_ptr(), 7, 2, 4, 8, st) == EINVAL      # lds < N
    assert f(z.data_ptr(), 4, 8, None, w.data_ptr(), None, src.data_ptr(), 8, 2, 1025, 8, st) == EINVAL   # S > 1024
    assert f(z.data_ptr(), 4, 8, None, w.data_ptr(), None, src.data_ptr(), 4097, 2, 4, 4097, st) == EINVAL  # N > 4096
    torch.cuda.synchronize()
    assert bool((src == SENTINEL).all())
    assert f(z.data_ptr(), 4, 8, None, w.data_ptr(), None, src.data_ptr(), 8, 2, 4, 8, st) == 0
