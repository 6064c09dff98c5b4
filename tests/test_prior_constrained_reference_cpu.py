"""The float64 reference of the prior's constrained sampler (tests/prior_constrained_reference.py) against plain definitions,
the new entry point's host-side argument checks (no GPU: the checks fail before any HIP call) and the host-side checks of
`generate_codes(constraint=...)`."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import decode_reference as R
import prior_constrained_reference as C

SETTINGS = [(1.0, 0, 1.0), (0.7, 5, 1.0), (1.5, 0, 0.9), (2.0, 4, 0.8)]


def _rows(M, V, seed):
    return torch.randn(M, V, generator=torch.Generator().manual_seed(seed)) * 2.0


@pytest.mark.parametrize('V', [3, 17, 1000])
def test_all_free_is_the_filter_and_the_inverse_cdf_draw(V):
    M = 4
    lg = _rows(M, V, 100 + V)
    seeds = torch.arange(M, dtype=torch.int64) * 1000003 + 17
    for temperature, top_k, top_p in SETTINGS:
        for pos in (0, 7):
            for cons in (None, torch.full((M,), -1, dtype=torch.int64)):
                code, pr, _ = C.prior_constrained_step_ref(lg, temperature, top_k, top_p, seeds, pos, cons)
                for b in range(M):
                    want = R.filter_ref(lg[b], temperature, top_k, top_p, multiply=True)     # the prior multiplies
                    assert torch.equal(pr[b], want)
                    u = (float(R.rng_u24_ref(int(seeds[b]), pos)) + 0.5) / 2.0 ** 24
                    cum = torch.cumsum(want, dim=0)
                    t = int(code[b])
                    assert float(want[t]) > 0
                    assert float(cum[t]) - float(want[t]) <= u * float(cum[-1]) + 1e-15 and u * float(cum[-1]) < float(cum[t]) + 1e-15


def test_forcing_some_rows_leaves_the_draws_of_the_others():
    lg = _rows(4, 17, 7)
    seeds = torch.tensor([5, 6, 7, 8], dtype=torch.int64)
    free, _, _ = C.prior_constrained_step_ref(lg, 1.0, 0, 1.0, seeds, 3, None)
    mixed, pr, _ = C.prior_constrained_step_ref(lg, 1.0, 0, 1.0, seeds, 3, torch.tensor([4, -1, 2 ** 40, -5]))
    assert mixed.tolist() == [4, int(free[1]), 16, int(free[3])]                    # 2^40 is clamped to V - 1
    assert torch.equal(pr[0], R.filter_ref(lg[0], 1.0, 0, 1.0, multiply=True))      # probs stay the filtered ones


@pytest.mark.parametrize('V', [1, 2, 17, 4096])
def test_logp_is_log_softmax_of_the_unfiltered_row(V):
    M = 4
    lg = _rows(M, V, 300 + V)
    if V > 1:
        lg[1] = torch.linspace(-80.0, 80.0, V)[torch.randperm(V, generator=torch.Generator().manual_seed(1))]
    if V > 2:
        lg[2, ::2] = -float('inf')
    cons = torch.tensor([0, V - 1, min(1, V - 1), -1], dtype=torch.int64)
    seeds = torch.tensor([1, 2, 3, 4], dtype=torch.int64)
    for temperature, top_k, top_p in SETTINGS:
        code, _, lp = C.prior_constrained_step_ref(lg, temperature, top_k, top_p, seeds, 2, cons)
        want = torch.log_softmax(lg.double(), dim=-1).gather(1, code.view(-1, 1)).view(-1)
        assert torch.allclose(lp, want, rtol=0, atol=1e-12), (lp, want)              # filters and temperature do not enter
        if V > 2:
            assert float(lp[2]) > -float('inf') and float(C.logp_ref(lg[2], 0)) == -float('inf')


def test_logp_bound_is_positive_and_of_order_1e_6():
    """On a +-40 row of each width the bound is positive and of order 1e-6 (|logp| <= 80 costs 80 u = 5e-6 alone), zero for a
    forced -inf code, and it covers the same chain in fp32 numpy with the kernel's order of additions."""
    g = torch.Generator().manual_seed(9)
    for V in (17, 1000, 4096):
        row = (torch.rand(V, generator=g) * 80.0 - 40.0).float()
        r = row.numpy()
        d = (r - r.max()).astype(np.float32)
        e = np.zeros(4096, dtype=np.float32)
        e[:V] = np.exp(d).astype(np.float32)
        t = np.zeros(256, dtype=np.float32)
        for k in range(16):                                                # thread t: its 16 codes in ascending order
            t = (t + e.reshape(256, 16)[:, k]).astype(np.float32)
        w = t.reshape(4, 64)
        for o in (32, 16, 8, 4, 2, 1):                                     # the wave butterfly
            w = (w + w[:, np.arange(64) ^ o]).astype(np.float32)
        s = np.float32(np.float32(w[0, 0] + w[1, 0]) + np.float32(w[2, 0] + w[3, 0]))
        for code in (0, V - 1, int(r.argmax()), int(r.argmin())):
            got = float(np.float32(d[code] - np.log(s, dtype=np.float32)))
            b = C.logp_bound(row, code)
            assert 1e-7 < b < 2e-5, b
            assert abs(got - C.logp_ref(row, code)) <= b, (V, code, got, b)
    row = torch.tensor([0.5, -float('inf'), 1.0])
    assert C.logp_bound(row, 1) == 0.0 and C.logp_bound(row, 0) > 0


class _Window:
    """A stand-in prior for the slow loop: the logits of position p favour (sum of the window's codes before p + p) % V."""
    num_tokens, V = 4, 7
    sos = torch.zeros(1)

    def eval(self):
        return self

    def forward(self, x):
        B, N = x.shape
        assert N == self.num_tokens
        lg = torch.zeros(B, N, self.V)
        for p in range(N):
            lg[torch.arange(B), p, (x[:, :p].sum(dim=1) + p) % self.V] = 2.0
        return {'weights_per_category': [lg]}


def test_the_slow_loop_follows_the_references_window_rule():
    cons = torch.full((2, 9), -1, dtype=torch.int64)
    cons[1, 2], cons[1, 6] = 5, 0
    seq, gap, rms, rows = C.forced_greedy_loop(_Window(), cons)
    for b in range(2):
        for e in range(9):
            w, p = (0, e) if e < 4 else (e - 3, 3)
            want = int(cons[b, e]) if int(cons[b, e]) >= 0 else (int(seq[b, w:w + p].sum()) + p) % 7
            assert int(seq[b, e]) == want, (b, e)
    assert gap == 2.0 and rows.shape == (2, 9, 7) and rms > 0


@pytest.fixture(scope='module')
def lib():
    import torch  # noqa: F401  (loads the process-wide libamdhip64.so.7 first)
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    return hip.load()


def test_new_symbol_is_declared_bound_and_exported(lib):
    from test_abi import header_symbols
    from vqcpc_bach_amd import hip
    s = 'vqcpc_prior_sample_constrained'
    assert s in header_symbols() and s in hip.SIGNATURES and hasattr(lib, s)
    assert lib.vqcpc_abi_version() == 2


def test_constrained_entry_point_rejects_bad_arguments(lib):
    """Bad arguments are rejected before any HIP call, with the entry point's name in the message (the pattern of
    tests/test_prior_cpu.py)."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value                       # a non-null pointer that is never dereferenced

    def sample(V=32, M=1, seeds=p, cons=p, ldcons=8, logp=p, ldlogp=8, logits=p, temperature=1.0):
        return lib.vqcpc_prior_sample_constrained(logits, V, V, M, temperature, 0, 1.0, seeds, cons, ldcons, logp, ldlogp, None,
                                                  p, 8, 8, p, V + 1, 16, p, 16, None, 0, p, p, None)
    for kw, word in ((dict(V=4097), b'4096'), (dict(M=65), b'64'), (dict(seeds=None), b'seeds'), (dict(ldcons=7), b'ldcons'),
                     (dict(ldlogp=7), b'ldlogp'), (dict(V=0), b''), (dict(logits=None), b'null'),
                     (dict(temperature=0.0), b'temperature')):
        assert sample(**kw) == -1, kw
        err = lib.vqcpc_last_error()
        assert b'prior_sample_constrained' in err and word in err, (kw, err)


def test_generate_codes_checks_the_constraint_on_the_host():
    from conftest import load_golden
    from test_prior_cpu import build_prior
    g = load_golden('prior_tiny')
    prior = build_prior(json.loads(str(g['v32/cfg_json'])))
    free = torch.full((2, 12), -1, dtype=torch.int64)
    for bad in (free[:, :11], free[:1].expand(3, 12), free.int(), free.view(2, 12, 1)):
        with pytest.raises(ValueError, match='constraint'):
            prior.generate_codes(12, num_generated_codes=2, constraint=bad)
    over = free.clone()
    over[1, 3] = 32
    with pytest.raises(ValueError, match='32 merged codes'):
        prior.generate_codes(12, num_generated_codes=2, constraint=over)
    with pytest.raises(ValueError, match='negative'):
        prior.score_codes(free)
