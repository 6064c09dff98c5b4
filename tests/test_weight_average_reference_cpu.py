"""Weight averaging without a GPU: the numpy float32 restatement of the rule against its float64 closed form, the C ABI of
vqcpc_weight_average (declared, bound, exported, every refusal before any HIP call) and the launches ops.FlatAdam.step()
issues with and without an average, with the kernel library replaced by a recorder."""
import ctypes
import os

import numpy as np
import pytest
import torch

import weight_average_reference as R

EPS = 2.0 ** -24          # half an ulp of 1: the relative rounding error of one float32 operation


@pytest.fixture(scope='module')
def lib():
    import torch  # noqa: F401  (loads the process-wide libamdhip64.so.7 first)
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    return hip.load()


# ---- the restatement against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize('decay', [0.9, 0.999])
def test_constant_parameters_are_the_fixed_point(decay):
    """p constant: the average converges to p.  In float32 it stops moving once w * (p - avg) falls below half an ulp of avg,
    i.e. within 1 / (2 w) ulps of p (5 for decay 0.9, 500 for 0.999); one more ulp for the last rounding."""
    rng = np.random.default_rng(1)
    p = rng.standard_normal(257).astype(np.float32)
    avg0 = rng.standard_normal(257).astype(np.float32)
    n = 400 if decay == 0.9 else 40000
    if decay == 0.999:                          # the long run on a handful of elements: the chain is elementwise
        p, avg0 = p[:8], avg0[:8]
    avg = avg0
    for u in range(1, n + 1):
        avg = R.update_f32(avg, p, decay, u)
    w = 1.0 - float(np.float32(decay))
    assert np.all(np.abs(avg.astype(np.float64) - p) <= (0.5 / w + 1.0) * np.spacing(np.abs(p)))
    # and a constant p that the average already equals is left exactly alone
    assert np.array_equal(R.update_f32(p, p, decay, 7), p)


@pytest.mark.parametrize('decay', [0.5, 0.9, 0.999])
def test_weight_left_on_the_initial_average_is_the_product_of_the_decays(decay):
    """p = 0: after n updates avg_n / avg_0 = prod d_u.  Per step the float32 chain deviates from avg * d_u by at most
    eps (2 + 1.5 / d_u) relatively: d_u's own division (eps), w = 1 - d_u (2^-25 absolute, exact for d_u >= 1/2), the
    product w * avg (eps w) and the final subtraction (eps), all relative to d_u >= 2 / 11."""
    n = 40 if decay == 0.5 else 200
    avg0 = np.array([1.0, -3.5, 1e-3, 12345.678], dtype=np.float32)
    zeros = np.zeros_like(avg0)
    got = R.average_f32(avg0, [zeros] * n, decay, u0=1)
    want = R.average_f64(avg0, [zeros] * n, decay, u0=1)
    ds = np.array([R.decay_f64(decay, u) for u in range(1, n + 1)])
    assert np.allclose(want, avg0.astype(np.float64) * np.prod(ds), rtol=1e-14, atol=0.0)
    bound = 1.01 * EPS * float(np.sum(2.0 + 1.5 / ds))
    assert np.all(np.abs(want) >= 2.0 ** -100)  # far inside the float32 normal range: the relative bound applies
    assert np.all(np.abs(got.astype(np.float64) - want) <= bound * np.abs(want)), (got, want, bound)


def test_random_trajectory_against_the_closed_form():
    """A recorded trajectory: per step the float32 chain adds at most 7 eps M of absolute error (M bounds |avg| and |p|: the
    difference, 2 M, and the product are rounded once each, the sum once, w carries 2^-24), and later steps only shrink it."""
    rng = np.random.default_rng(2)
    n, M = 120, 4.0
    traj = [np.clip(rng.standard_normal(64), -M, M).astype(np.float32) for _ in range(n)]
    avg0 = traj[0].copy()
    for decay in (0.0, 0.9, 0.9999):
        got = R.average_f32(avg0, traj, decay, u0=1)
        want = R.average_f64(avg0, traj, decay, u0=1)
        assert np.max(np.abs(got - want)) <= 7 * n * EPS * M


def test_crossover_for_decay_0_9():
    """Updates 79, 80, 81: the warm-up term acts at 79 (80 / 89 < 0.9), ties at 80 (81 / 90 rounds to float32(0.9)), and decay
    alone acts from there on."""
    d = np.float32(0.9)
    assert R.crossover(0.9) == 80
    assert R.decay_f32(0.9, 79) == np.float32(np.float32(80) / np.float32(89)) < d
    assert R.decay_f32(0.9, 80) == d and np.float32(np.float32(81) / np.float32(90)) == d
    assert R.decay_f32(0.9, 81) == d and np.float32(np.float32(82) / np.float32(91)) > d
    assert R.decay_f32(0.9, 10 ** 6) == d
    # the first update of a run from scratch keeps 2 / 11 of the initial weights, whatever the decay
    assert R.decay_f32(0.9999, 1) == np.float32(np.float32(2) / np.float32(11))
    # the counts are converted exactly as integers first: 10 + (2**24 + 1) is not a float32 and rounds to even
    assert R.decay_f32(0.99999994, 2 ** 24 + 1) == np.float32(np.float32(2 ** 24 + 2) / np.float32(2 ** 24 + 12))


def test_decay_zero_is_not_a_special_case():
    """decay = 0: d_u = 0, w = 1, avg + 1 * (p - avg) -- which is NOT p when the difference rounds."""
    a = np.array([1.0, 1e8, -2.5, 0.0], dtype=np.float32)
    p = np.array([1e-8, 1.0, 2.5, 1e-40], dtype=np.float32)
    got = R.update_f32(a, p, 0.0, 5)
    assert np.array_equal(got, (a + (p - a).astype(np.float32)).astype(np.float32))
    assert got[0] == 0.0 != p[0] and got[1] == 0.0 != p[1] and got[2] == p[2] and got[3] == p[3]


# ---- the C ABI ---------------------------------------------------------------------------------------------------
def test_new_symbol_is_declared_bound_and_exported(lib):
    from test_abi import header_symbols
    from vqcpc_bach_amd import hip
    s = 'vqcpc_weight_average'
    assert s in header_symbols() and s in hip.SIGNATURES and hasattr(lib, s)
    assert len(hip.SIGNATURES[s][1]) == 8
    assert lib.vqcpc_abi_version() == 2


def test_weight_average_refuses_bad_arguments_before_any_hip_call(lib):
    """This machine has no GPU: a call that reached the HIP runtime would fail with a launch error, not with -1 and a message."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value                       # non-null, 16-byte-agnostic, never dereferenced
    p -= p % 4

    def avg(a=p, q=p, n=8, decay=0.9, u=1, step_dev=None, t0=0):
        return lib.vqcpc_weight_average(a, q, n, decay, u, step_dev, t0, None)
    assert avg(a=None) == -1 and b'weight_average' in lib.vqcpc_last_error() and b'null' in lib.vqcpc_last_error()
    assert avg(q=None) == -1 and b'null' in lib.vqcpc_last_error()
    assert avg(n=-1) == -1 and b'n < 0' in lib.vqcpc_last_error()
    for bad in (1.0, 1.5, -0.001, float('nan'), float('inf')):
        assert avg(decay=bad) == -1 and b'decay' in lib.vqcpc_last_error(), bad
    assert avg(decay=float(np.nextafter(np.float32(1.0), np.float32(2.0)))) == -1
    assert avg(decay=0.99999999) == -1          # rounds to 1.0f: "as a float"
    assert avg(u=0) == -1 and b'u = 1' in lib.vqcpc_last_error()
    # n == 0: nothing is launched, valid arguments otherwise (both forms)
    assert avg(n=0) == 0
    assert avg(n=0, decay=0.0, u=2 ** 40) == 0
    assert avg(n=0, u=0, step_dev=p, t0=3) == 0
    # ... but n == 0 does not excuse a bad argument
    assert avg(n=0, a=None) == -1 and avg(n=0, decay=1.0) == -1 and avg(n=0, u=0) == -1


# ---- ops.FlatAdam: the launches of a step ----------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    from vqcpc_bach_amd import hip
    calls = []
    monkeypatch.setattr(hip, 'call', lambda name, *args: calls.append((name, args)) or 0)
    monkeypatch.setattr(hip, 'query', lambda name, *args: 1)
    monkeypatch.setattr(hip, 'workspace', lambda n, dev: torch.empty(16, dtype=torch.uint8), raising=False)
    return calls


def test_flat_adam_step_launches_with_and_without_the_average(rec, monkeypatch):
    from vqcpc_bach_amd import ops
    flat, grad = torch.arange(12, dtype=torch.float32), torch.ones(12)
    opt = ops.FlatAdam(flat[4:11], grad[4:11], lr=1e-3)
    assert opt.avg is None
    before = ops._PARAM_STEPS
    opt.step()
    assert [c[0] for c in rec] == ['vqcpc_sumsq', 'vqcpc_adam_step']
    assert ops._PARAM_STEPS == before + 1
    del rec[:]

    opt.enable_average(0.9)
    assert opt.avg_t0 == 1 and opt.avg.data_ptr() != opt.p.data_ptr() and torch.equal(opt.avg, flat[4:11])
    opt.step()
    opt.step(lr=5e-4)
    assert [c[0] for c in rec] == ['vqcpc_sumsq', 'vqcpc_adam_step', 'vqcpc_weight_average'] * 2
    for k, (name, args) in enumerate(c for c in rec if c[0] == 'vqcpc_weight_average'):
        avg, p, n, decay, u, step_dev, t0 = args
        assert avg is opt.avg and p is opt.p and n == 7 and decay == 0.9
        assert (u, step_dev, t0) == (k + 1, None, 0)                   # host form: u = step_count - t0, counting this update
    del rec[:]

    # being recorded into a step graph: the device form, exactly where Adam takes its own device form
    lr_dev, step_dev = torch.zeros(1), torch.zeros(1, dtype=torch.int64)
    opt.use_device_scalars(lr_dev, step_dev)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    opt.step()
    assert [c[0] for c in rec] == ['vqcpc_sumsq', 'vqcpc_adam_step_dev', 'vqcpc_weight_average']
    avg, p, n, decay, u, sd, t0 = rec[-1][1]
    assert sd is step_dev and sd is rec[1][1][9] and t0 == 1 and avg is opt.avg and n == 7
    del rec[:]
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
    opt.step()                                  # a graph owns the scalars, but this step is eager: host form
    assert [c[0] for c in rec] == ['vqcpc_sumsq', 'vqcpc_adam_step', 'vqcpc_weight_average']
    assert rec[-1][1][4:] == (opt.step_count - 1, None, 0)
    del rec[:]

    opt.disable_average()
    opt.step()
    assert [c[0] for c in rec] == ['vqcpc_sumsq', 'vqcpc_adam_step'] and opt.avg is None


def test_flat_adam_enable_average_arguments(rec):
    from vqcpc_bach_amd import ops
    opt = ops.FlatAdam(torch.zeros(8), torch.zeros(8), lr=1e-3)
    for bad in (1.0, -0.1, 2.0, float('nan')):
        with pytest.raises(ValueError, match='decay'):
            opt.enable_average(bad)
    assert opt.avg is None
    mine = torch.full((8,), 3.0)
    opt.step_count = 5
    opt.enable_average(0.0, avg=mine, t0=2)
    assert opt.avg is mine and opt.avg_t0 == 2 and opt.avg_decay == 0.0
    opt.step()
    assert rec[-1][0] == 'vqcpc_weight_average' and rec[-1][1][4] == 4
