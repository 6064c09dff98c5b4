"""The token-indirection GRU kernels (csrc/gru.hip: vqcpc_gru_tok_cell_fwd / _bwd, vqcpc_gru_tok_step_fwd / _bwd) and the
table gradient vqcpc_gru_tok_segsum, by direct calls in the conventions of tests/test_train_kernels_gpu.py (sentinel-filled
outputs with guard elements, NaN in everything a result must not depend on, fixed seeds).

Every tok kernel is checked twice:
  * bit for bit against the row-pointer entry point fed with gi = gi_table[key] gathered on the host, key[b] =
    (p % n_voices) * vmax + tokens[b, p] -- only the address of gi differs, so no tolerance applies;
  * against the float64 cell / step of tests/train_reference.py under the yardstick that file's GRU tests use (`judge`, C = 4).
Table rows that no (voice, token) pair can reach hold NaN: reading one poisons an output.  The kernels see the block
position p only; the forward stack passes p = t and the flipped stack p = L - 1 - t, so p in {0, 1, L - 1} covers both.

Table gradient: against a float64 segment sum under the fp32 summation bound of test_upscale (Higham, lemma 3.1: n u sum|terms|)
with n = the longest segment + the number of row chunks + L (terms of a row, chunk partials, steps of a voice); two runs give
the same bits; rows nobody refers to are exactly 0.
"""
import math

import pytest
import torch

import train_reference as T
from test_train_kernels_gpu import F32, NAN, U, Guard, call, gen, judge, query, same_bits

pytestmark = pytest.mark.gpu

SEED = 0x2468ACE000000005
# (L, per-voice number of valid token ids): 4 voices with unequal vocabularies (vmax 9), and 2 voices
SETUPS = [(16, [5, 9, 3, 7]), (4, [4, 6])]
ROWS = [1, 33, 70]              # one row, one row past a 32-row tile, a ragged third tile


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    yield hip


def _table_and_tokens(R, H, L, limits, seed):
    """gi_table (nv * vmax, 3H) with NaN in the unreachable rows; tokens (R, L) that include token 0 and the last valid token
    of every voice at every position parity."""
    g = gen(seed)
    nv, vmax = len(limits), max(limits)
    table = torch.full((nv * vmax, 3 * H), NAN)
    for c, n in enumerate(limits):
        table[c * vmax:c * vmax + n] = torch.randn(n, 3 * H, generator=g)
    lim = torch.tensor([limits[p % nv] for p in range(L)])
    tokens = (torch.rand(R, L, generator=g) * lim).long().clamp_(max=lim - 1)
    even = (torch.arange(L) // nv) % 2 == 0
    tokens[0] = torch.where(even, torch.zeros(L, dtype=torch.long), lim - 1)
    if R > 1:
        tokens[R - 1] = torch.where(even, lim - 1, torch.zeros(L, dtype=torch.long))
    return table, tokens, nv, vmax


def _gathered(table, tokens, p, nv, vmax):
    gi = table[(p % nv) * vmax + tokens[:, p]]
    assert bool(torch.isfinite(gi).all()), 'the test data must reach valid table rows only'
    return gi


def _positions(L):
    return (0, 1, L - 1)


@pytest.mark.parametrize('R', ROWS)
def test_tok_cell_kernels(R):
    H = 24                                                           # not a multiple of 64: the cell kernels only
    for L, limits in SETUPS:
        table, tokens, nv, vmax = _table_and_tokens(R, H, L, limits, 1000 + R + L)
        td, kd = table.cuda(), tokens.cuda()
        g = gen(R * 31 + L)
        gh, hp = torch.randn(R, 3 * H, generator=g), torch.randn(R, H, generator=g)
        d_y, d_h = torch.randn(R, H, generator=g), torch.randn(R, H, generator=g)
        ghd = gh.cuda()
        for p in _positions(L):
            gi = _gathered(table, tokens, p, nv, vmax)
            gid = gi.cuda()
            for hp_given, drop, base in ((False, 0.0, 0), (True, 0.25, 4321), (False, 0.25, 1 << 33)):
                lab = f'R{R} L{L} p{p} hprev{int(hp_given)} drop{drop}'
                hp_, hpd = (hp, hp.cuda()) if hp_given else (None, None)
                scale = T.dropout_scale(SEED, (R, H), drop, idx_base=base)
                o, o2 = [Guard((R, H)), Guard((R, H))], [Guard((R, H)), Guard((R, H))]
                call('vqcpc_gru_tok_cell_fwd', td, kd, L, p, nv, vmax, ghd, hpd, o[0].view, o[1].view, R, H, drop, SEED, base)
                call('vqcpc_gru_cell_fwd', gid, ghd, hpd, o2[0].view, o2[1].view, R, H, drop, SEED, base)
                torch.cuda.synchronize()
                ref, pl = T.gru_cell_fwd(gi, gh, hp_, scale), T.gru_cell_fwd(gi, gh, hp_, scale, dtype=F32)
                for name, a, b, c, r in zip(('h', 'y'), o, o2, pl, ref):
                    assert same_bits(a.check().cpu(), b.check().cpu()), f'tok cell {name} {lab}'
                    judge('GRU', f'tok cell {name} {lab}', a.cpu(), c, r)
                for dy_, dh_ in ((d_y, None), (d_y, d_h)):
                    o, o2 = ([Guard((R, 3 * H)), Guard((R, 3 * H)), Guard((R, H))] for _ in range(2))
                    dyd, dhd = dy_.cuda(), (None if dh_ is None else dh_.cuda())
                    call('vqcpc_gru_tok_cell_bwd', td, kd, L, p, nv, vmax, ghd, hpd, dyd, dhd, o[0].view, o[1].view, o[2].view, R, H,
                         drop, SEED, base)
                    call('vqcpc_gru_cell_bwd', gid, ghd, hpd, dyd, dhd, o2[0].view, o2[1].view, o2[2].view, R, H, drop, SEED, base)
                    torch.cuda.synchronize()
                    rb = T.gru_cell_bwd(gi, gh, hp_, dy_, dh_, scale)
                    pb = T.gru_cell_bwd(gi, gh, hp_, dy_, dh_, scale, dtype=F32)
                    for name, a, b, c, r in zip(('d_gi', 'd_gh', 'd_hprev'), o, o2, pb, rb):
                        assert same_bits(a.check().cpu(), b.check().cpu()), f'tok cell {name} {lab}'
                        judge('GRU', f'tok cell {name} {lab} dh{int(dh_ is not None)}', a.cpu(), c, r)


@pytest.mark.parametrize('H', [64, 128])
@pytest.mark.parametrize('R', ROWS)
def test_tok_step_kernels(R, H):
    """h_prev / dgh_next carry NaN rows past R: the 32-row tile must not read them into a result."""
    assert query('vqcpc_gru_step_supported', R, H) == 1
    for L, limits in SETUPS:
        table, tokens, nv, vmax = _table_and_tokens(R, H, L, limits, 2000 + R + L + H)
        td, kd = table.cuda(), tokens.cuda()
        g = gen(7 * R + H + L)
        w = torch.randn(3 * H, H, generator=g) / math.sqrt(H)
        b = torch.randn(3 * H, generator=g)
        hp = torch.randn(R, H, generator=g)
        dgh, dhp, d_y = torch.randn(R, 3 * H, generator=g), torch.randn(R, H, generator=g), torch.randn(R, H, generator=g)
        wd, bd, wtd = w.cuda(), b.cuda(), w.t().contiguous().cuda()
        hpd_full = torch.cat([hp, torch.full((3, H), NAN)]).cuda()
        dghd = torch.cat([dgh, torch.full((3, 3 * H), NAN)]).cuda()
        for p in _positions(L):
            gi = _gathered(table, tokens, p, nv, vmax)
            gid = gi.cuda()
            for hp_given, drop, base in ((True, 0.0, 0), (True, 0.25, 99), (False, 0.25, 1 << 33)):
                lab = f'R{R} H{H} L{L} p{p} hprev{int(hp_given)} drop{drop}'
                hp_, hpd = (hp, hpd_full) if hp_given else (None, None)
                scale = T.dropout_scale(SEED, (R, H), drop, idx_base=base)
                o, o2 = ([Guard((R, 3 * H)), Guard((R, H)), Guard((R, H))] for _ in range(2))
                call('vqcpc_gru_tok_step_fwd', td, kd, L, p, nv, vmax, wd, bd, hpd, o[0].view, o[1].view, o[2].view, R, H, drop, SEED,
                     base)
                call('vqcpc_gru_step_fwd', gid, wd, bd, hpd, o2[0].view, o2[1].view, o2[2].view, R, H, drop, SEED, base)
                torch.cuda.synchronize()
                ref = T.gru_step_fwd(gi, w, b, hp_, scale)
                pl = T.gru_step_fwd(gi, w, b, hp_, scale, dtype=F32)
                for name, a, a2, c, r in zip(('gh', 'h', 'y'), o, o2, pl, ref):
                    assert same_bits(a.check().cpu(), a2.check().cpu()), f'tok step {name} {lab}'
                    judge('GRU', f'tok step {name} {lab}', a.cpu(), c, r)
            gh = T.gru_step_fwd(gi, w, b, hp)[0].float()
            ghd = gh.cuda()
            for dy_given, hp_given, drop, base in ((False, True, 0.0, 0), (True, True, 0.25, 99), (True, False, 0.25, 7)):
                lab = f'R{R} H{H} L{L} p{p} dy{int(dy_given)} hprev{int(hp_given)} drop{drop}'
                hp_, hpd = (hp, hpd_full) if hp_given else (None, None)
                dy_ = d_y if dy_given else None
                dyd = None if dy_ is None else dy_.cuda()
                scale = T.dropout_scale(SEED, (R, H), drop, idx_base=base)
                o, o2 = ([Guard((R, 3 * H)), Guard((R, 3 * H)), Guard((R, H), data=dhp)] for _ in range(2))
                call('vqcpc_gru_tok_step_bwd', dghd, wtd, o[2].view, td, kd, L, p, nv, vmax, ghd, hpd, dyd, o[0].view, o[1].view, R, H,
                     drop, SEED, base)
                call('vqcpc_gru_step_bwd', dghd, wtd, o2[2].view, gid, ghd, hpd, dyd, o2[0].view, o2[1].view, R, H, drop, SEED, base)
                torch.cuda.synchronize()
                ref = T.gru_step_bwd(dgh, w.t(), dhp, gi, gh, hp_, dy_, scale)
                pl = T.gru_step_bwd(dgh, w.t(), dhp, gi, gh, hp_, dy_, scale, dtype=F32)
                for name, a, a2, c, r in zip(('d_gi', 'd_gh', 'dhp'), o, o2, pl, ref):
                    assert same_bits(a.check().cpu(), a2.check().cpu()), f'tok step {name} {lab}'
                    judge('GRU', f'tok step {name} {lab}', a.cpu(), c, r)


SEG_CHUNK_ROWS, SEG_MAX_CHUNKS = 128, 64          # kTokSegChunkRows / kTokSegMaxChunks of csrc/gru.hip


@pytest.mark.parametrize('C', [72, 384])           # 3H of H = 24; one full column tile of 256 and a partial one
@pytest.mark.parametrize('R', ROWS + [1000])       # 1000 rows: 8 row chunks
def test_tok_segsum(R, C):
    for L, limits in SETUPS:
        nv, vmax = len(limits), max(limits)
        _, tokens, _, _ = _table_and_tokens(R, 1, L, limits, 3000 + R + L)
        kd = tokens.cuda()
        g = gen(R + C + L)
        dgi = [torch.randn(R, C, generator=g) for _ in range(L)]
        wsb = query('vqcpc_gru_tok_segsum_workspace', R, vmax, C)
        nchunks = min(SEG_MAX_CHUNKS, -(-R // SEG_CHUNK_ROWS))
        assert wsb == nchunks * vmax * C * 4
        runs = []
        for _ in range(2):
            out, ws = Guard((nv * vmax, C)), Guard(wsb // 4)
            seen = set()
            for p in range(L - 1, -1, -1):                           # the order of the backward pass: first visit of a voice writes
                call('vqcpc_gru_tok_segsum', dgi[p].cuda(), kd, L, p, nv, vmax, out.view, R, C, 1 if p % nv in seen else 0, ws.view,
                     wsb)
                seen.add(p % nv)
            torch.cuda.synchronize()
            ws.check(written=None)
            runs.append(out.check().cpu())
        assert same_bits(runs[0], runs[1]), 'two runs must give the same bits'
        ref = torch.zeros(nv * vmax, C, dtype=torch.float64)
        mag = torch.zeros(nv * vmax, C, dtype=torch.float64)
        count = torch.zeros(nv * vmax, dtype=torch.long)
        for p in range(L):
            key = (p % nv) * vmax + tokens[:, p]
            ref.index_add_(0, key, dgi[p].double())
            mag.index_add_(0, key, dgi[p].double().abs())
            count.index_add_(0, key, torch.ones(R, dtype=torch.long))
        unreached = count == 0
        assert bool(unreached.any()) and bool((runs[0][unreached] == 0).all()), 'rows nobody refers to are exactly 0'
        n = int(count.max()) + nchunks + L
        err = (runs[0].double() - ref).abs()
        print(f'TOKSEG R{R} C{C} L{L}: longest segment {int(count.max())}, max err / bound {float((err / (n * U * mag + 2.0 ** -149)).max()):.3f}')
        assert bool((err <= n * U * mag + 2.0 ** -149).all())
