"""vqcpc_weight_average on the GPU against the numpy float32 restatement (tests/weight_average_reference.py), as BITS: every
size x every pair of pointer offsets x every decay x every update count, NaN guards on both sides of every `avg`, the device
form against the host form, and determinism.

All (size, offset, offset) cases of one (decay, u) live in ONE pair of device buffers -- slot after slot, each data range
between NaN-filled guards -- so a case costs one launch and the whole grid one copy each way."""
import numpy as np
import pytest
import torch

import weight_average_reference as R

pytestmark = pytest.mark.gpu

# The launcher (csrc/util.hip) starts at most kWeightAverageBlocks = 2048 blocks of 256 threads; a thread takes one float4 per
# pass of its grid-stride loop where both pointers permit it and one float where they do not.  One full pass is therefore
# 2048 * 256 * 4 = 2**21 elements on the float4 path (2**19 on the scalar path): 2**21 + 5 is just past it on either.
ONE_PASS = 2048 * 256 * 4
SIZES = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
OFFSETS = [(a, p) for a in range(4) for p in range(4)]
DECAYS = [0.0, 0.9, 0.999, 0.9999]
UPDATES = [1, 2, 79, 80, 81, 8989, 8990, 2 ** 24 + 1]
GUARD = 8                                       # NaN elements before and after every data range (a multiple of 4)


def _values(rng, n):
    """Gaussian values with a few exact zeros (both signs) and denormals sprinkled in."""
    x = rng.standard_normal(n).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -3e-42, 1.4e-45, 1.1754942e-38], dtype=np.float32)
    k = max(1, n // 16)
    x[rng.integers(0, n, size=k)] = special[rng.integers(0, len(special), size=k)]
    return x


def _layout(cases):
    """cases: [(n, off_avg, off_p)] -> (total elements, [(start_avg, start_p, n)]): every slot starts 16-byte aligned, its data
    GUARD + offset elements in, and ends with at least GUARD more NaN elements."""
    slots, total = [], 0
    for n, oa, op in cases:
        slots.append((total + GUARD + oa, total + GUARD + op, n))
        total += (GUARD + 3 + n + GUARD + 3) // 4 * 4
    return total, slots


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _run_grid(cases, decay, updates, seed, device_form=None):
    """Fills the buffers, launches every case once per update count in `updates` (consecutively: the average of one is the
    input of the next), and returns (got avg buffer, expected avg buffer, p buffer after, p buffer before)."""
    from vqcpc_bach_amd import hip
    rng = np.random.default_rng(seed)
    total, slots = _layout(cases)
    avg = np.full(total, np.nan, dtype=np.float32)
    p = np.full(total, np.nan, dtype=np.float32)
    for sa, sp, n in slots:
        avg[sa:sa + n] = _values(rng, n)
        p[sp:sp + n] = _values(rng, n)
    want = avg.copy()
    d_avg, d_p = torch.from_numpy(avg).cuda(), torch.from_numpy(p).cuda()
    assert d_avg.data_ptr() % 16 == 0 and d_p.data_ptr() % 16 == 0
    step_dev = torch.zeros(1, dtype=torch.int64, device='cuda') if device_form is not None else None
    for u in updates:
        if step_dev is not None:
            step_dev.fill_(device_form + u)
        for sa, sp, n in slots:
            if step_dev is not None:
                hip.call('vqcpc_weight_average', d_avg[sa:sa + n], d_p[sp:sp + n], n, decay, 0, step_dev, device_form)
            else:
                hip.call('vqcpc_weight_average', d_avg[sa:sa + n], d_p[sp:sp + n], n, decay, u, None, 0)
        for sa, sp, n in slots:
            want[sa:sa + n] = R.update_f32(want[sa:sa + n], p[sp:sp + n], decay, u)
    torch.cuda.synchronize()
    return d_avg.cpu().numpy(), want, d_p.cpu().numpy(), p


GRID = [(n, oa, op) for n in SIZES for oa, op in OFFSETS]


@pytest.mark.parametrize('decay', DECAYS)
def test_every_size_offset_and_update_count_bit_for_bit(decay):
    """17 sizes x 16 offset pairs, each of the 8 update counts applied in turn to the running average.  The whole buffer is
    compared: the NaN guards on both sides of every `avg` are part of the expectation."""
    got, want, p_after, p_before = _run_grid(GRID, decay, UPDATES, seed=11)
    assert np.isnan(want).sum() > 2 * GUARD * len(GRID)                 # the guards are there ...
    _, slots = _layout(GRID)
    assert not any(np.isnan(want[sa:sa + n]).any() for sa, _, n in slots)   # ... and no data is
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (decay, bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.array_equal(_bits(p_after), _bits(p_before))              # p is only read


@pytest.mark.parametrize('u', UPDATES)
def test_each_update_count_on_its_own(u):
    """One update from fresh inputs per count (the chained test feeds each count the previous average): the ratio
    float(1 + u) / float(10 + u), 2**24 + 1 included, for every decay."""
    cases = [(257, 1, 3), (1025, 0, 0), (64, 2, 2)]
    for decay in DECAYS:
        got, want, _, _ = _run_grid(cases, decay, [u], seed=100 + u % 97)
        assert np.array_equal(_bits(got), _bits(want)), (decay, u)
    w = np.float32(1.0) - R.decay_f32(0.9999, u)
    assert w > 0                                 # the update moves the average at every count tested


@pytest.mark.parametrize('offsets', [(0, 0), (1, 1), (1, 2), (3, 0)])
def test_just_past_one_pass_of_the_grid_stride_loop(offsets):
    """n = ONE_PASS + 5 (see ONE_PASS above): equal offsets take the float4 path with a scalar head and tail, unequal ones
    the scalar path, four passes deep."""
    got, want, p_after, p_before = _run_grid([(ONE_PASS + 5, *offsets)], 0.999, [81], seed=5)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (bad[:8], bad.size)
    assert np.array_equal(_bits(p_after), _bits(p_before))


def test_device_form_is_the_host_form():
    """step_dev[0] - t0 = u: the same bits as the host form with that u, for every size and offset pair and a t0 beyond
    2**32; step_dev[0] <= t0 leaves avg untouched."""
    from vqcpc_bach_amd import hip
    t0 = 2 ** 33 + 7
    for decay, updates in ((0.9, [79, 80, 81]), (0.9999, [1, 2 ** 24 + 1])):
        host, want, _, _ = _run_grid(GRID, decay, updates, seed=3)
        dev, want_dev, _, _ = _run_grid(GRID, decay, updates, seed=3, device_form=t0)
        assert np.array_equal(_bits(want), _bits(want_dev))
        assert np.array_equal(_bits(dev), _bits(host)) and np.array_equal(_bits(host), _bits(want))
    rng = np.random.default_rng(4)
    a0, p = _values(rng, 4097), _values(rng, 4097)
    avg, d_p = torch.from_numpy(a0).cuda(), torch.from_numpy(p).cuda()
    step_dev = torch.zeros(1, dtype=torch.int64, device='cuda')
    for t in (t0, t0 - 1, 0):
        step_dev.fill_(t)
        hip.call('vqcpc_weight_average', avg, d_p, 4097, 0.9, 0, step_dev, t0)
        assert np.array_equal(_bits(avg.cpu().numpy()), _bits(a0)), t
    step_dev.fill_(t0 + 1)
    hip.call('vqcpc_weight_average', avg, d_p, 4097, 0.9, 0, step_dev, t0)
    assert np.array_equal(_bits(avg.cpu().numpy()), _bits(R.update_f32(a0, p, 0.9, 1)))


def test_two_launches_from_equal_inputs_give_equal_bits():
    cases = [(ONE_PASS + 5, 0, 0), (4097, 1, 2), (4097, 3, 3)]
    a = _run_grid(cases, 0.999, [2, 8990], seed=9)[0]
    b = _run_grid(cases, 0.999, [2, 8990], seed=9)[0]
    assert np.array_equal(_bits(a), _bits(b))


def test_n_zero_launches_nothing_and_bad_arguments_raise():
    from vqcpc_bach_amd import hip
    avg = torch.full((8,), float('nan'), device='cuda')
    hip.call('vqcpc_weight_average', avg, avg, 0, 0.9, 1, None, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(avg).all())
    with pytest.raises(hip.VqcpcHipError, match='decay'):
        hip.call('vqcpc_weight_average', avg, avg, 8, 1.0, 1, None, 0)
    with pytest.raises(hip.VqcpcHipError, match='u = 1'):
        hip.call('vqcpc_weight_average', avg, avg, 8, 0.5, 0, None, 0)
