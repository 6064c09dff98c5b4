"""The kernels that index by token or code, one by one, by direct calls, against the float64 references of
tests/table_reference.py: vqcpc_vq_fwd, vqcpc_vq_bwd (csrc/vq.hip), vqcpc_embed_pos_fwd / _bwd, vqcpc_block_table_gather /
_segsum / _segsum_b16 and vqcpc_embedding_bwd (csrc/embed_ln.hip), at the sizes where their LDS accumulators, chunked partial
sums and v_readlane hand-outs change path.  The case tables and what each case is for are in tests/table_reference.py;
tests/test_table_reference_cpu.py verifies on the CPU that every id these tests pass is in range and that every planted tie and
unreferenced cell is what it claims to be.

Conventions (those of tests/test_train_kernels_gpu.py, whose Guard / strided / same_bits are used):
  * every output sits in a sentinel-filled allocation with guard elements on both sides, which must be bit-unchanged afterwards;
  * every workspace is exactly the *_workspace(..) size inside such a guard and holds NaN bit patterns before the call: a NaN in
    an output is a read of a partial sum nobody wrote;
  * gap columns of a strided input are NaN; every launch is made twice and must give the same bits; seeds are fixed.

Statistic.  Segment sums (d_codebooks, d_table, d_chan, d_event, the block table's and the embedding's d_table): per ELEMENT,
|out - out64| / ||its summands||_2 (table_reference.seg_err); an element nothing is summed into must be +0.0, bit for bit.  d_z and
the loss of the non-squared form: per row, max |out - out64| / rms(out64 of the row) (train_reference.row_err).  Never a
tensor-wide denominator.

Tolerance.  The yardstick of the project: the SAME formula in plain fp32 torch on the CPU (index_add_ in fp32 for the sums)
against float64; a group passes when max err(kernel) <= 4 max err(plain fp32); where plain fp32 is exact the bound is 4 ulp of
each output, and outputs ALL within 4 ulp pass in any case.  One group per output is formed over ALL calls of one test, so that no
maximum rests on a single entry (the reason tests/test_relattn_x_kernels_gpu.py gives); where one test holds sums of a few terms and
sums of thousands, the two kinds are judged apart (`size_class`), so that the long chains' error is not the bound of the short.  Every group prints
`<family> <label>: kernel .. plain .. ratio ..`; a SUMMARY line per family ends the module; the figures are in
profiles/table_kernel_tests_log.md.

Derived bounds (u = 2^-24, gamma_n = n u / (1 - n u); inputs are fp32 values, so the float64 reference is exact to 1e-16):
  * vq_fwd argmin.  The kernel's distance is the chain d = fl(d + fl(fl(z_t - e_t)^2)), t ascending from d = 0: term t = 0 meets
    one rounding in the subtraction (squared: two factors 1 + u), one in the product and dsub - 1 in the additions, later terms
    fewer, all terms are >= 0, so d^ = d (1 + theta), |theta| <= gamma_{dsub + 2}.  The kernel takes the smallest d^, hence for the
    chosen code c and the float64 minimum m:  d_c (1 - gamma) <= d^_c <= d^_m <= d_m (1 + gamma), i.e.
    d_c <= d_m (1 + gamma_{dsub + 2}) / (1 - gamma_{dsub + 2}).
  * squared loss.  lsum is ONE sequential fp32 chain over the D squares fl(fl(q - z)^2): D + 1 roundings at most for a term as
    above (two of them from the squared difference), then fl(beta l) and the final addition: |loss - loss64| <= gamma_{D + 4} loss64.
  * squared d_z = fl(g - fl(fl(gl beta) 2 fl(q - z))): the subtracted term T carries three roundings, the difference one more:
    |d_z - d_z64| <= u |g_zq| + gamma_4 |T|, componentwise.
Exact: idx (bit for bit vqcpc_oracle.vq_assign, the header's contract), zq = fl(z + fl(q - z)), the gather, the embedding forward,
the bf16 segment sum against the fp32 one on the upcast values, vqcpc_embedding_bwd against the host replay of the order the
header fixes, d_z of the squared form against vqcpc_vq_commit_bwd.

Finding.  vqcpc_vq_bwd's shape check used to admit dsub <= 256, but its LDS holds the K x dsub accumulator AND the 256 x dsub staged
rows: (K + 256) dsub + 256 floats must fit 160 KiB, so dsub >= 159 is refused for every K (dsub = 200, 256: -1, "do not fit the
LDS"; the dead range left the shape check, the message and include/vqcpc.h name the limit).  The refusals are asserted below; dsub = 150 and 158 (the largest that
runs) are the kgroups = 1 cases."""
import math

import pytest
import torch

import table_reference as R
import train_reference as T
from oracle import vqcpc_oracle as O
from test_train_kernels_gpu import F32, NAN, Guard, bits, call, gen, query, same_bits, strided, ulp32

pytestmark = pytest.mark.gpu

C_FAMILY = {'vq_fwd': 4.0, 'vq_bwd': 4.0, 'segsum': 4.0, 'embed_pos': 4.0, 'embedding': 4.0}
RATIOS = {}
I64 = torch.int64
BETA = 0.25
TINY = 1e-30


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from vqcpc_bach_amd import hip
    hip.load()
    yield hip
    for fam, rs in sorted(RATIOS.items()):
        r = sorted(x for _, x, _, _ in rs if math.isfinite(x))
        if r:
            print(f'SUMMARY {fam}: {len(rs)} groups, median ratio {r[len(r) // 2]:.2f}, max {r[-1]:.2f}, max kernel '
                  f'{max(k for _, _, k, _ in rs):.3e}, max plain {max(p for _, _, _, p in rs):.3e}, C = {C_FAMILY[fam]:g}; above 2: '
                  + ', '.join(f'{lab} {x:.2f}' for lab, x, _, _ in rs if x > 2.0))


# =====================================================================================================================
# the yardstick
class Judge:
    """Collects the calls of one test into one group per output; finish() prints every group's line and fails with all that
    missed."""

    def __init__(self, fam, name):
        self.fam, self.name, self.groups = fam, name, {}

    def _add(self, out, label, kernel, ref, ek, ep):
        k, ref = torch.as_tensor(kernel).detach().cpu().double(), torch.as_tensor(ref).double()
        w4 = bool(((k.reshape(ref.shape) - ref).abs() <= 4.0 * ulp32(ref)).all())
        self.groups.setdefault(out, []).append((label, ek, ep, w4))

    def seg(self, out, label, kernel, plain, ref64, nrm):
        """A segment sum: per element against the norm of its summands; elements without summands must be +0.0."""
        kernel = torch.as_tensor(kernel).detach().cpu()
        assert bool(torch.isfinite(kernel).all()), f'{self.fam} {label}: non-finite {out} (a stale partial sum or a wrong read)'
        dead = (nrm == 0).reshape(kernel.shape)
        assert R.is_pos_zero(kernel[dead]), f'{self.fam} {label}: an element of {out} that nothing is summed into is not +0.0'
        self._add(out, label, kernel, ref64, R.seg_err(kernel, ref64, nrm), R.seg_err(plain, ref64, nrm))

    def rows(self, out, label, kernel, plain, ref64):
        kernel = torch.as_tensor(kernel).detach().cpu()
        assert bool(torch.isfinite(kernel).all()), f'{self.fam} {label}: non-finite {out}'
        self._add(out, label, kernel, ref64, T.row_err(kernel, ref64), T.row_err(plain, ref64))

    def finish(self):
        bad = []
        for out, items in self.groups.items():
            Ek = max([float(i[1].max()) for i in items if i[1].numel()] or [0.0])
            Ep = max([float(i[2].max()) for i in items if i[2].numel()] or [0.0])
            w4 = all(i[3] for i in items)
            label = f'{self.name} {out} ({len(items)} calls)'
            if Ep == 0.0:
                ok, ratio = w4, (0.0 if Ek == 0.0 else float('inf'))
            else:
                ratio = Ek / Ep
                ok = ratio <= C_FAMILY[self.fam] or w4
            print(f'{self.fam} {label}: kernel {Ek:.3e} plain {Ep:.3e} ratio {ratio:.2f}')
            RATIOS.setdefault(self.fam, []).append((label, ratio, Ek, Ep))
            if not ok:
                worst = max(items, key=lambda i: float(i[1].max()) if i[1].numel() else 0.0)
                bad.append((self.fam, label, Ek, Ep, ratio, 'worst call: ' + worst[0]))
        self.groups = {}
        assert not bad, bad


def size_class(n, long_from):
    """Calls with long sums and calls with short ones are judged apart: the plain-fp32 error of a chain of tens of thousands of terms
    would otherwise be the yardstick of a sum of three."""
    return 'long sums' if n >= long_from else 'short sums'


def nan_ws(nbytes):
    """A workspace of exactly `nbytes` inside a guard, NaN everywhere."""
    assert nbytes % 4 == 0 and nbytes > 0
    return Guard(nbytes // 4, data=torch.full((nbytes // 4,), NAN))


def twice(fn, label):
    """Two launches on fresh buffers: the same bits."""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert (x is None and y is None) or same_bits(x, y), f'{label}: two launches differ'
    return a


def refused(lib, rc, message, fn, untouched):
    with pytest.raises(lib.VqcpcHipError, match=rf'failed \({rc}\): {message}'):
        fn()
    torch.cuda.synchronize()
    for g in untouched:
        g.check(written=False)


# =====================================================================================================================
# vq_fwd
def vq_fwd_launch(zd, cbd, Rr, ncb, K, dsub, squared, assign=1, idx_given=None, index_only=False):
    idx = Guard((Rr, ncb), I64, data=idx_given)
    zq, loss = (None, None) if index_only else (Guard((Rr, ncb * dsub)), Guard(Rr))
    call('vqcpc_vq_fwd', zd, cbd, Rr, ncb, K, dsub, BETA, squared, assign, idx.view, None if index_only else zq.view,
         None if index_only else loss.view)
    torch.cuda.synchronize()
    idx.check(written=True if assign else False)
    if index_only:
        return idx.cpu(), None, None
    return idx.cpu(), zq.check().cpu(), loss.check().cpu()


def vq_fwd_check(J, label, z, cb, idx, zq, loss, squared):
    D = z.shape[1]
    assert same_bits(zq, R.vq_zq_bits(z, cb, idx)), f'{label}: zq is not fl(z + fl(q - z))'
    _, loss64 = R.vq_fwd(z, cb, idx, BETA, squared)
    if squared:
        err = (loss.double() - loss64).abs()
        assert bool((err <= R.gamma(D + 4) * loss64 + TINY).all()), (label, float((err / loss64.clamp_min(TINY)).max()), R.gamma(D + 4))
    else:
        J.rows('loss l2', label, loss, R.vq_fwd(z, cb, idx, BETA, squared, dtype=F32)[1], loss64)


VQ_FWD_GROUPS = {'dsub': R.VQ_FWD_DSUB, 'K': R.VQ_FWD_K, 'big': R.VQ_FWD_BIG}


@pytest.mark.parametrize('group', list(VQ_FWD_GROUPS))
def test_vq_fwd(group):
    J = Judge('vq_fwd', group)
    for ci, (label, Rr, ncb, K, dsub) in enumerate(VQ_FWD_GROUPS[group]):
        label = f'{label} dsub{dsub} K{K} ncb{ncb} R{Rr}'
        z, cb, plan, given = R.vq_fwd_inputs(VQ_FWD_GROUPS[group][ci])
        zd, cbd = z.cuda(), cb.cuda()
        want = O.vq_assign(z, list(cb))
        d64 = R.vq_distances(z, cb)
        gm = R.gamma(dsub + 2)
        for squared in (1, 0):
            idx, zq, loss = twice(lambda: vq_fwd_launch(zd, cbd, Rr, ncb, K, dsub, squared), label)
            assert torch.equal(idx, want), f'{label}: idx differs from vqcpc_oracle.vq_assign in {int((idx != want).sum())} places'
            chosen = torch.gather(d64, 2, idx.unsqueeze(-1)).squeeze(-1)
            assert bool((chosen <= d64.min(-1)[0] * (1 + gm) / (1 - gm) + TINY).all()), f'{label}: a chosen code is too far'
            vq_fwd_check(J, f'{label} sq{squared}', z, cb, idx, zq, loss, squared)
        for c, p in enumerate(plan):                                           # the planted rows did what they were planted for
            if p['dup'] is not None:
                assert bool((idx[p['tie_rows'], c] == p['dup'][0]).all()), f'{label}: a tie did not go to the first index'
            for r in p['on_rows']:
                assert float(chosen[r, c]) == 0.0
        # index-only mode: the same idx, nothing else exists to be written
        only = twice(lambda: vq_fwd_launch(zd, cbd, Rr, ncb, K, dsub, 1, index_only=True), label)[0]
        assert torch.equal(only, want), f'{label}: index-only mode'
        # assign = 0: idx is an input and stays bit-unchanged; zq and the loss follow the GIVEN codes
        for squared in (1, 0):
            idx0, zq0, loss0 = twice(lambda: vq_fwd_launch(zd, cbd, Rr, ncb, K, dsub, squared, assign=0, idx_given=given), label)
            assert torch.equal(bits(idx0), bits(given))
            vq_fwd_check(J, f'{label} given sq{squared}', z, cb, given, zq0, loss0, squared)
    J.finish()


def test_vq_fwd_refuses_a_codebook_over_144_kib(_lib):
    K, dsub = 36 * 1024 + 1, 1
    z, cb = torch.zeros(4, dsub, device='cuda'), torch.zeros(1, K, dsub, device='cuda')
    idx, zq, loss = Guard((4, 1), I64), Guard((4, dsub)), Guard(4)
    refused(_lib, -1, 'vq_fwd: codebook of 36865 x 1 floats does not fit the LDS',
            lambda: call('vqcpc_vq_fwd', z, cb, 4, 1, K, dsub, BETA, 1, 1, idx.view, zq.view, loss.view), (idx, zq, loss))


# =====================================================================================================================
# vq_bwd
def vq_bwd_launch(dev, Rr, ncb, K, dsub, squared):
    d_z, d_cb = Guard((Rr, ncb * dsub)), Guard((ncb, K, dsub))
    nbytes = query('vqcpc_vq_bwd_workspace', Rr, ncb, K, dsub)
    assert nbytes == -(-Rr // 256) * ncb * K * dsub * 4
    ws = nan_ws(nbytes)
    call('vqcpc_vq_bwd', *dev, Rr, ncb, K, dsub, BETA, squared, d_z.view, d_cb.view, ws.view, nbytes)
    torch.cuda.synchronize()
    ws.check(written=None)
    return d_z.check().cpu(), d_cb.check().cpu()


def vq_bwd_run(J, cases):
    for case in cases:
        label, Rr, ncb, K, dsub, pat = case
        data = R.vq_bwd_inputs(case)
        z, cb, idx, g_zq, g_loss = data
        dev = [t.cuda() for t in data]
        for squared in (1, 0):
            lab = f'{label} ncb{ncb} sq{squared}'
            d_z, d_cb = twice(lambda: vq_bwd_launch(dev, Rr, ncb, K, dsub, squared), lab)
            rz, rcb, nrm, Tm = R.vq_bwd(z, cb, idx, g_zq, g_loss, BETA, squared)
            pz, pcb, _, _ = R.vq_bwd(z, cb, idx, g_zq, g_loss, BETA, squared, dtype=F32)
            assert bool(torch.isfinite(d_z).all()), lab
            if squared:
                bound = R.U * g_zq.double().abs() + R.gamma(4) * Tm.abs() + TINY
                assert bool(((d_z.double() - rz).abs() <= bound).all()), (lab, float(((d_z.double() - rz).abs() / bound).max()))
                commit = Guard((Rr, ncb * dsub))
                call('vqcpc_vq_commit_bwd', *dev, Rr, ncb, K, dsub, BETA, squared, commit.view)
                torch.cuda.synchronize()
                assert same_bits(commit.check().cpu(), d_z), f'{lab}: d_z differs from vqcpc_vq_commit_bwd'
            else:
                J.rows('d_z l2', lab, d_z, pz, rz)
            J.seg('d_codebooks sq' if squared else 'd_codebooks l2', lab, d_cb, pcb, rcb, nrm)
            chosen = torch.zeros(ncb, K, dtype=torch.bool)
            for c in range(ncb):
                chosen[c, idx[:, c]] = True
            assert R.is_pos_zero(d_cb[~chosen]), f'{lab}: the gradient of a code no row chose is not +0.0'


@pytest.mark.parametrize('dsub', R.VQ_BWD_DSUBS)
def test_vq_bwd(dsub):
    J = Judge('vq_bwd', f'dsub{dsub}')
    vq_bwd_run(J, R.vq_bwd_cases(dsub))
    J.finish()


def test_vq_bwd_2048_codes():
    """K x dsub = 2048 x 16: 148 480 bytes of LDS (hipFuncSetAttribute); R = 513 rows each on a code of its own."""
    J = Judge('vq_bwd', '2048x16')
    vq_bwd_run(J, R.VQ_BWD_BIG)
    J.finish()


@pytest.mark.parametrize('dsub,K', R.VQ_BWD_REFUSED)
def test_vq_bwd_refuses_what_does_not_fit_the_lds(_lib, dsub, K):
    Rr = 3
    data = R.vq_bwd_case(Rr, 1, K, dsub, 'one', 5)
    dev = [t.cuda() for t in data]
    d_z, d_cb = Guard((Rr, dsub)), Guard((1, K, dsub))
    nbytes = query('vqcpc_vq_bwd_workspace', Rr, 1, K, dsub)
    ws = nan_ws(nbytes)
    refused(_lib, -1, f'vq_bwd: {K} codes \\+ 256 staged rows of {dsub} floats do not fit the LDS',
            lambda: call('vqcpc_vq_bwd', *dev, Rr, 1, K, dsub, BETA, 1, d_z.view, d_cb.view, ws.view, nbytes), (d_z, d_cb, ws))


def test_vq_bwd_refuses_a_short_workspace(_lib):
    Rr, ncb, K, dsub = 257, 2, 7, 5
    dev = [t.cuda() for t in R.vq_bwd_case(Rr, ncb, K, dsub, 'random', 5)]
    d_z, d_cb = Guard((Rr, ncb * dsub)), Guard((ncb, K, dsub))
    nbytes = query('vqcpc_vq_bwd_workspace', Rr, ncb, K, dsub)
    ws = nan_ws(nbytes)
    refused(_lib, -3, 'vq_bwd: workspace too small',
            lambda: call('vqcpc_vq_bwd', *dev, Rr, ncb, K, dsub, BETA, 1, d_z.view, d_cb.view, ws.view, nbytes - 1), (d_z, d_cb, ws))


# =====================================================================================================================
# block table
def segsum_launch(entry, gd, tokd, M, L, vmax, C):
    out = Guard((vmax * L, C))
    nbytes = query('vqcpc_block_table_segsum_workspace', M, L, vmax, C)
    ws = nan_ws(nbytes)
    call(entry, gd, tokd, out.view, M, L, vmax, C, ws.view, nbytes)
    torch.cuda.synchronize()
    ws.check(written=None)
    return (out.check().cpu(),)


def gather_launch(td, tokd, M, L, vmax, C):
    out = Guard((M, C))
    call('vqcpc_block_table_gather', td, tokd, out.view, M, L, vmax, C)
    torch.cuda.synchronize()
    return (out.check().cpu(),)


def seg_dead_check(label, out, L, dead, dead_cells):
    for t in dead:
        assert R.is_pos_zero(out[t * L:(t + 1) * L]), f'{label}: token {t} never occurs, its rows are not +0.0'
    for t, p in dead_cells:
        assert R.is_pos_zero(out[t * L + p]), f'{label}: cell ({t}, {p}) is never referred to and is not +0.0'


def test_block_table_fp32():
    J = Judge('segsum', 'fp32')
    for i, (L, vmax, C, nb, dist) in enumerate(R.SEG_F32):
        label = f'L{L} vmax{vmax} C{C} nb{nb} {dist}'
        tokens, g, dead, dead_cells = R.seg_case(L, vmax, C, nb, dist, i)
        M = nb * L
        tokd = tokens.cuda()
        if C % 4 == 0:
            table = torch.randn(vmax * L, C, generator=gen(500 + i))
            out, = twice(lambda: gather_launch(table.cuda(), tokd, M, L, vmax, C), label)
            assert same_bits(out, R.block_gather(table, tokens, L)), f'{label}: gather'
        gd = g.cuda()
        out, = twice(lambda: segsum_launch('vqcpc_block_table_segsum', gd, tokd, M, L, vmax, C), label)
        ref, nrm = R.block_segsum(g, tokens, L, vmax)
        J.seg(f'd_table {size_class(nb, 500)}', label, out, R.block_segsum(g, tokens, L, vmax, dtype=F32)[0], ref, nrm)
        seg_dead_check(label, out, L, dead, dead_cells)
    J.finish()


def test_block_table_bf16():
    J = Judge('segsum', 'bf16')
    for i, (L, vmax, C, nb, dist) in enumerate(R.SEG_B16):
        label = f'b16 L{L} vmax{vmax} C{C} nb{nb} {dist}'
        tokens, g, dead, dead_cells = R.seg_case(L, vmax, C, nb, dist, len(R.SEG_F32) + i)
        g, gb = R.bf16_trunc_values(g)
        M = nb * L
        tokd = tokens.cuda()
        out, = twice(lambda: segsum_launch('vqcpc_block_table_segsum_b16', gb.cuda(), tokd, M, L, vmax, C), label)
        out32, = twice(lambda: segsum_launch('vqcpc_block_table_segsum', g.cuda(), tokd, M, L, vmax, C), label)
        assert same_bits(out, out32), f'{label}: the bf16 form differs from the fp32 form on the upcast values'
        ref, nrm = R.block_segsum(g, tokens, L, vmax)
        J.seg(f'd_table {size_class(nb, 500)}', label, out, R.block_segsum(g, tokens, L, vmax, dtype=F32)[0], ref, nrm)
        seg_dead_check(label, out, L, dead, dead_cells)
    J.finish()


@pytest.mark.parametrize('entry,vmax,C', [('vqcpc_block_table_segsum', 161, 4), ('vqcpc_block_table_segsum_b16', 81, 4)])
def test_block_table_segsum_refuses_a_vocabulary_over_the_lds(_lib, entry, vmax, C):
    L, nb = 4, 33
    tokens = torch.randint(0, vmax, (nb * L,), generator=gen(1)).cuda()
    g = torch.zeros(nb * L, C, dtype=torch.int16 if entry.endswith('b16') else F32, device='cuda')
    out = Guard((vmax * L, C))
    nbytes = query('vqcpc_block_table_segsum_workspace', nb * L, L, vmax, C)
    ws = nan_ws(nbytes)
    refused(_lib, -1, f'block_table_segsum: vocabulary of {vmax} tokens does not fit the LDS accumulator',
            lambda: call(entry, g, tokens, out.view, nb * L, L, vmax, C, ws.view, nbytes), (out, ws))


@pytest.mark.parametrize('entry', ['vqcpc_block_table_segsum', 'vqcpc_block_table_segsum_b16'])
def test_block_table_segsum_refuses_a_workspace_one_byte_short(_lib, entry):
    L, nb, vmax, C = 4, 513, 57, 6
    tokens = torch.randint(0, vmax, (nb * L,), generator=gen(1)).cuda()
    g = torch.zeros(nb * L, C, dtype=torch.int16 if entry.endswith('b16') else F32, device='cuda')
    out = Guard((vmax * L, C))
    nbytes = query('vqcpc_block_table_segsum_workspace', nb * L, L, vmax, C)
    assert nbytes == 2 * vmax * L * C * 4                                              # 513 blocks: two chunks
    ws = nan_ws(nbytes)
    refused(_lib, -3, 'block_table_segsum: workspace too small',
            lambda: call(entry, g, tokens, out.view, nb * L, L, vmax, C, ws.view, nbytes - 1), (out, ws))


def test_block_table_segsum_workspace_follows_the_chunk_thresholds():
    per = 57 * 4 * 8 * 4
    for nb, chunks in ((1, 1), (255, 1), (511, 1), (512, 2), (513, 2), (8191, 31), (8192, 32), (8193, 32), (100000, 32)):
        assert query('vqcpc_block_table_segsum_workspace', nb * 4, 4, 57, 8) == chunks * per, nb


# =====================================================================================================================
# embed_pos
def embed_fwd_launch(tokd, n_rows, tpb, nv, td, vmax, dlin, cd, ed, pos, d):
    out = Guard((n_rows, d))
    call('vqcpc_embed_pos_fwd', tokd, n_rows, tpb, nv, td, vmax, dlin, cd, ed, pos, out.view)
    torch.cuda.synchronize()
    return (out.check().cpu(),)


def embed_bwd_launch(tokd, n_rows, tpb, nv, vmax, dlin, pos, gd, has_ev):
    d_table, d_chan = Guard((nv, vmax, dlin)), Guard((nv, pos))
    d_event = Guard((tpb // nv, pos)) if has_ev else None
    nbytes = query('vqcpc_embed_pos_bwd_workspace', n_rows, tpb, nv, vmax, dlin, pos)
    ws = nan_ws(nbytes)
    call('vqcpc_embed_pos_bwd', tokd, n_rows, tpb, nv, vmax, dlin, pos, gd, d_table.view, d_chan.view, d_event.view if has_ev else None,
         ws.view, nbytes)
    torch.cuda.synchronize()
    ws.check(written=None)
    return d_table.check().cpu(), d_chan.check().cpu(), d_event.check().cpu() if has_ev else None


def emb_chunks(n_rows, tpb):
    """The number of chunks the header's workspace formula implies for a table of one float per voice: (chunks + 1) nv per."""
    per = 1 * 4 + 4 + (tpb // 1) * 4
    return query('vqcpc_embed_pos_bwd_workspace', n_rows, tpb, 1, 1, 4, 4) // (per * 4) - 1


def test_embed_pos_chunking_is_what_the_cases_assume():
    assert [emb_chunks(16 * n, 16) for n in (1, 47, 48, 49)] == [1, 47, 48, 25]         # 49 blocks: chunks of two, the last ragged
    assert emb_chunks(65536 - 16, 16) == 48 and emb_chunks(65536, 16) == 32 and emb_chunks(65536 + 16, 16) == 33
    assert emb_chunks(3 * 2048, 2048) == 3 and emb_chunks(2048, 2048) == 1


def test_embed_pos():
    J = Judge('embed_pos', 'all')
    vmax = R.EMB_VMAX
    for i, (label, tpb, nv, pos, dlin, has_ev, n_rows) in enumerate(R.EMB_CASES):
        tokens, table, chan, event, g, dead = R.emb_case(tpb, nv, pos, dlin, has_ev, n_rows, i)
        d = g.shape[1]
        tokd = tokens.cuda()
        out, = twice(lambda: embed_fwd_launch(tokd, n_rows, tpb, nv, table.cuda(), vmax, dlin, chan.cuda(), event.cuda() if has_ev else None,
                                              pos, d), label)
        assert same_bits(out, R.embed_pos_fwd(tokens, tpb, nv, table, chan, event)), f'{label}: forward'
        gd = g.cuda()
        d_table, d_chan, d_event = twice(lambda: embed_bwd_launch(tokd, n_rows, tpb, nv, vmax, dlin, pos, gd, has_ev), label)
        ref = R.embed_pos_bwd(tokens, tpb, nv, vmax, dlin, pos, g, has_ev)
        pl = R.embed_pos_bwd(tokens, tpb, nv, vmax, dlin, pos, g, has_ev, dtype=F32)
        sz = size_class(n_rows, 4096)
        J.seg(f'd_table {sz}', label, d_table, pl['d_table'], ref['d_table'], ref['n_table'])
        J.seg(f'd_chan {sz}', label, d_chan, pl['d_chan'], ref['d_chan'], ref['n_chan'])
        if has_ev:
            J.seg(f'd_event {sz}', label, d_event, pl['d_event'], ref['d_event'], ref['n_event'])
        for v in range(nv):
            assert R.is_pos_zero(d_table[v, dead[v]]), f'{label}: the table rows of ids voice {v} never sees are not +0.0'
    J.finish()


# =====================================================================================================================
# embedding_bwd
def embg_launch(gd, ldg, sd, pd, M, V, C):
    out = Guard((V, C))
    call('vqcpc_embedding_bwd', gd, ldg, sd, pd, out.view, M, V, C)
    torch.cuda.synchronize()
    return (out.check().cpu(),)


def test_embedding_bwd():
    J = Judge('embedding', 'all')
    for i, (M, C, gap, V, pat) in enumerate(R.EMBG_CASES):
        label = f'M{M} C{C} ldg{C + gap} V{V} {pat}'
        g, idx, runs = R.embg_case(M, C, gap, V, pat, i)
        sidx, perm = torch.sort(idx, stable=True)
        gd, sd, pd = (strided(g, C + gap), sidx.cuda(), perm.cuda()) if M else (None, None, None)
        out, = twice(lambda: embg_launch(gd, C + gap, sd, pd, M, V, C), label)
        assert same_bits(out, R.embedding_bwd_replay(g, idx, V)), f'{label}: not the sums in ascending m'
        ref, nrm = R.embedding_bwd(g, idx, V)
        J.seg(f'd_table {size_class(M, 1000)}', label, out, R.embedding_bwd(g, idx, V, dtype=F32)[0], ref, nrm)
        unref = torch.ones(V, dtype=torch.bool)
        unref[idx] = False
        assert R.is_pos_zero(out[unref]), f'{label}: a row no index refers to is not +0.0'
    J.finish()
