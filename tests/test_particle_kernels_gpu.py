"""vqcpc_particle_resample and vqcpc_particle_permute_{i64,f32,cache} (csrc/particles.hip) by direct calls on the cases of
tests/particles_cases.py, against tests/particles_reference.py:
  resample: lw bit-exact (sequential fp32 adds); wn, ess and the evidence against float64 within the bounds derived in the
  reference file (worst ratio printed); the decision, the ANCESTORS and the flag exactly the reference's function of the wn and
  ess the kernel itself stored and of u -- every case, no near-tie exemption; lw reset exactly where the group resampled;
  histories written at row c only; every output inside sentinel-filled allocations with guard rows, inputs the kernel must not
  read are NaN;
  permute: equal to numpy's gather bit for bit on [0, bound), everything else -- rows at and beyond pos, other planes' padding,
  guard cells -- keeps its bits; identity maps touch nothing (early exit on the flag, also with a poisoned ancestor buffer)."""
import numpy as np
import pytest
import torch

import particles_cases as K
import particles_reference as R
from test_decode_kernels_gpu import GR, Buf, call, same_bits

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    return hip


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).cuda().contiguous()


def vec(n, data=None, dtype=torch.float32):
    """A vector of n elements as a one-row Buf: guard rows around it and three guard elements behind it."""
    return Buf(1, n, n + 3, data=None if data is None else torch.as_tensor(data, dtype=dtype).reshape(1, n), dtype=dtype)


def launch_resample(x, hist_rows=None):
    M, G, P, c = x['M'], x['G'], x['P'], x['c']
    H = c + 2 if hist_rows is None else hist_rows
    o = dict(lw=vec(M, x['lw']), evidence=vec(G, x['evidence']), pending=vec(G), anc=vec(M, dtype=torch.int32), wn=vec(M),
             ess=vec(G), flag=vec(1, dtype=torch.int32))
    ld = x['ld']
    pos = torch.tensor([x['pos']], dtype=torch.int32, device='cuda')
    win = dev(x['win'])
    hist_anc = torch.full((H, M), -7, dtype=torch.int32, device='cuda')
    hist_wn = torch.full((H, M), 77.0, dtype=torch.float32, device='cuda')
    hist_ess = torch.full((H, G), 77.0, dtype=torch.float32, device='cuda')
    call('vqcpc_particle_resample', o['lw'].view, o['evidence'].view, o['pending'].view, dev(x['seeds']), dev(x['constraint']), ld,
         dev(x['logp']), ld, dev(x['logmass']), ld, pos, win, x['U'], float(x['threshold']), int(x['force']), o['anc'].view,
         o['wn'].view, o['ess'].view, o['flag'].view, hist_anc, hist_wn, hist_ess, H, M, P)
    torch.cuda.synchronize()
    for k in ('lw', 'evidence', 'pending', 'anc', 'wn', 'ess', 'flag'):
        o[k].assert_only()                                    # guard rows and guard elements keep their bits
    out = {k: o[k].view.reshape(-1).cpu().numpy() for k in ('lw', 'evidence', 'pending', 'anc', 'wn', 'ess', 'flag')}
    out.update(hist_anc=hist_anc.cpu().numpy(), hist_wn=hist_wn.cpu().numpy(), hist_ess=hist_ess.cpu().numpy())
    assert int(pos.item()) == x['pos']
    return out


@pytest.mark.parametrize('name', sorted(K.RESAMPLE_CASES))
def test_resample_against_the_reference(name):
    x = K.resample_inputs(name)
    M, G, P, c, U = x['M'], x['G'], x['P'], x['c'], x['U']
    got = launch_resample(x)
    ref = R.resample(x['lw'], x['evidence'], x['seeds'], c, U, P, x['threshold'], x['force'], x['constraint'], x['logp'],
                     x['logmass'], wn=got['wn'], ess=got['ess'])
    worst = dict(wn=0.0, ess=0.0, evidence=0.0)
    for g in range(G):
        rows = slice(g * P, (g + 1) * P)
        lw1 = ref['lw_updated'][rows]
        wn64, ess64, inc64, dmax = R.group_weights64(lw1)
        worst['wn'] = max(worst['wn'], float((np.abs(got['wn'][rows] - wn64) / R.wn_bound(wn64, dmax, P)).max()))
        worst['ess'] = max(worst['ess'], abs(float(got['ess'][g]) - ess64) / R.ess_bound(ess64, dmax, P))
        assert got['ess'][g] == R.ess_of(got['wn'][rows])                             # ess is its own chain on the stored wn
        if np.isinf(inc64):
            assert got['pending'][g] == -np.inf and got['evidence'][g] == -np.inf
            assert (got['wn'][rows] == F(1.0) / F(P)).all() and not ref['resampled'][g]
            continue
        b_inc = R.inc_bound(float(lw1.max()), inc64, dmax, P)
        worst['evidence'] = max(worst['evidence'], abs(float(got['pending'][g]) - inc64) / b_inc)
        if ref['resampled'][g]:
            want = float(x['evidence'][g]) + inc64
            worst['evidence'] = max(worst['evidence'], abs(float(got['evidence'][g]) - want) / (b_inc + R.EPS * abs(want)))
            assert got['evidence'][g] == F(x['evidence'][g] + got['pending'][g])      # one fp32 add of the stored increment
        else:
            assert got['evidence'][g] == x['evidence'][g]
    print(f'{name}: worst error / bound: wn {worst["wn"]:.3f}, ess {worst["ess"]:.3f}, evidence {worst["evidence"]:.3f}')
    assert max(worst.values()) <= 1.0, worst
    # exact: the decision and the ancestors as functions of the stored wn / ess and u; the reset; the flag
    assert np.array_equal(got['anc'], ref['ancestors']), (got['anc'], ref['ancestors'])
    assert same_bits(torch.from_numpy(got['lw']), torch.from_numpy(ref['lw']))
    assert (got['lw'][np.repeat(ref['resampled'], P)] == 0).all()
    assert int(got['flag'][0]) == ref['flag'] and int(got['flag'][0]) in (0, 1)
    # the histories: row c holds this launch, every other row keeps its filler
    assert np.array_equal(got['hist_anc'][c], got['anc']) and (np.delete(got['hist_anc'], c, axis=0) == -7).all()
    assert same_bits(torch.from_numpy(got['hist_wn'][c]), torch.from_numpy(got['wn']))
    assert same_bits(torch.from_numpy(got['hist_ess'][c]), torch.from_numpy(got['ess']))
    assert (np.delete(got['hist_wn'], c, axis=0) == 77.0).all() and (np.delete(got['hist_ess'], c, axis=0) == 77.0).all()
    for g, kind in enumerate(x['kinds']):
        if kind == 'dominant' and ref['resampled'][g]:
            assert (got['anc'][g * P:(g + 1) * P] == g * P + x['dominant'][g]).all()
        if kind == 'uniform':
            assert (got['anc'][g * P:(g + 1) * P] == np.arange(g * P, (g + 1) * P)).all()


def test_resample_without_a_finished_code_or_history_row():
    """pos < U, or no live window: the identity map, flag 0, nothing else written.  A code past the histories' rows is
    processed, its history row is not written."""
    x = K.resample_inputs('p8_threshold1')
    for change in (dict(pos=x['U'] - 1), dict(win=np.array([0, -1], dtype=np.int32))):
        y = dict(x, **change)
        got = launch_resample(y)
        assert np.array_equal(got['anc'], np.arange(x['M'])) and got['flag'][0] == 0
        assert same_bits(torch.from_numpy(got['lw']), torch.from_numpy(x['lw']))
        assert same_bits(torch.from_numpy(got['evidence']), torch.from_numpy(x['evidence']))
        assert (got['hist_anc'] == -7).all() and (got['hist_wn'] == 77.0).all()
    full = launch_resample(x)
    short = launch_resample(x, hist_rows=x['c'])                      # rows [0, c): row c does not exist
    assert np.array_equal(short['anc'], full['anc']) and same_bits(torch.from_numpy(short['wn']), torch.from_numpy(full['wn']))
    assert (short['hist_anc'] == -7).all() and full['flag'][0] == 1


# ---- permute ---------------------------------------------------------------------------------------------------------
def _padded(shape, dtype, seed, pad=64):
    """A dense tensor of `shape` inside a flat allocation with `pad` guard elements on both sides (16-byte aligned for fp32)."""
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        flat = torch.randn(n + 2 * pad, generator=g)
        flat[::97] = float('nan')                                   # bits, not values, are compared
    else:
        flat = torch.randint(-2 ** 62, 2 ** 62, (n + 2 * pad,), generator=g, dtype=torch.int64)
    flat = flat.cuda()
    return flat, flat[pad:pad + n].view(shape)


def _bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize('name', sorted(K.PERMUTE_CASES))
def test_permute_equals_the_gather_and_leaves_the_rest(name):
    x = K.permute_inputs(name)
    P, M, L, W, d, p = x['P'], x['M'], x['layers'], x['W'], x['d'], x['pos']
    anc_h = x['ancestors']
    anc = torch.from_numpy(anc_h).cuda()
    moved = bool((anc_h != np.arange(M)).any())
    flag = torch.tensor([int(moved)], dtype=torch.int32, device='cuda')
    pos = torch.tensor([p], dtype=torch.int32, device='cuda')
    # the cache (layers, M, W, d): positions [0, pos) of every layer move
    flat, cache = _padded((L, M, W, d), torch.float32, 1)
    before = _bits(flat)
    call('vqcpc_particle_permute_cache', cache, L, W, d, pos, anc, flag, M, P)
    torch.cuda.synchronize()
    want = R.permute_rows(before[64:-64].reshape(L, M, W * d), anc_h, p * d)
    assert np.array_equal(_bits(flat)[64:-64].reshape(L, M, W * d), want)
    assert np.array_equal(_bits(flat)[:64], before[:64]) and np.array_equal(_bits(flat)[-64:], before[-64:])
    # rows: int64 with the bound read from pos and ld > width; fp32 with the whole width (the vector path: width % 4 == 0 and
    # the scalar one: odd width), and fp32 with the bound from pos
    for dtype, entry, width, ld, bound in ((torch.int64, 'vqcpc_particle_permute_i64', W, W + 3, pos),
                                           (torch.int64, 'vqcpc_particle_permute_i64', W + 1, W + 1, None),
                                           (torch.float32, 'vqcpc_particle_permute_f32', d, d + 4, None),
                                           (torch.float32, 'vqcpc_particle_permute_f32', d + 1, d + 2, None),
                                           (torch.float32, 'vqcpc_particle_permute_f32', W, W + 4, pos)):
        buf = Buf(M, width, ld, dtype=dtype)
        g = torch.Generator().manual_seed(width)
        data = torch.randint(-2 ** 62, 2 ** 62, (M, width), generator=g) if dtype == torch.int64 else \
            torch.randn(M, width, generator=g)
        buf.view.copy_(data)
        buf.before = buf.full.clone()
        start = _bits(buf.view)
        call(entry, buf.view, ld, width, bound, anc, flag, M, P)
        torch.cuda.synchronize()
        cols = width if bound is None else min(p, width)
        assert np.array_equal(_bits(buf.view), R.permute_rows(start, anc_h, cols)), (entry, width, ld)
        buf.assert_only()                                            # guard rows and the columns [width, ld) keep their bits
    if not moved:                                                     # the early exit: the flag alone decides, the map is not read
        junk = torch.full((M,), 10 ** 6, dtype=torch.int32, device='cuda')
        call('vqcpc_particle_permute_cache', cache, L, W, d, pos, junk, flag, M, P)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(flat), before)


def test_permute_ignores_an_ancestor_outside_the_group():
    """A garbage map (a row of another group, a negative or a huge index) with the flag set moves nothing for that row and
    reads nothing outside the buffer."""
    P, M, W, d = 4, 8, 8, 16
    anc_h = np.array([1, 0, 6, -1, 4, 10 ** 6, 3, 7], dtype=np.int32)
    safe = np.array([1, 0, 2, 3, 4, 5, 6, 7], dtype=np.int32)
    flat, cache = _padded((1, M, W, d), torch.float32, 5)
    before = _bits(flat)
    call('vqcpc_particle_permute_cache', cache, 1, W, d, torch.tensor([W], dtype=torch.int32, device='cuda'),
         torch.from_numpy(anc_h).cuda(), torch.ones(1, dtype=torch.int32, device='cuda'), M, P)
    torch.cuda.synchronize()
    want = R.permute_rows(before[64:-64].reshape(1, M, W * d), safe, W * d)
    assert np.array_equal(_bits(flat)[64:-64].reshape(1, M, W * d), want)


def test_refusals():
    from vqcpc_bach_amd import hip
    a = torch.zeros(8, dtype=torch.int32, device='cuda')
    f = torch.zeros(8, dtype=torch.float32, device='cuda')
    i = torch.zeros(8, 4, dtype=torch.int64, device='cuda')
    for P, M in ((1, 8), (65, 65), (3, 8)):
        with pytest.raises(hip.VqcpcHipError):
            call('vqcpc_particle_permute_i64', i, 4, 4, None, a, a, M, P)
    with pytest.raises(hip.VqcpcHipError):
        call('vqcpc_particle_permute_i64', i, 3, 4, None, a, a, 8, 2)                     # ld < width
    with pytest.raises(hip.VqcpcHipError):
        call('vqcpc_particle_permute_cache', f, 1, 1, 6, a, a, a, 2, 2)                   # d % 4
    with pytest.raises(hip.VqcpcHipError):
        call('vqcpc_particle_resample', f, f, f, i, None, 0, None, 0, None, 0, a, None, 4, 1.5, 0, a, f, f, a, None, None, None, 0,
             8, 2)                                                                        # threshold > 1
