"""The five kernels of csrc/relattn_x.hip (forward, dq, dkv, de, de_split) by direct calls of vqcpc_relattn_x_fwd,
vqcpc_relattn_x_bwd_workspace and vqcpc_relattn_x_bwd, against the float64 reference of tests/attention_reference.py, at the
shapes where the index arithmetic changes: ragged last key tile and query strip, one wave against four (Lk 96 / 97), r > 1 with
the clamped band rows of the last strip, every mask branch of the tile skips, the largest supported Lk, the chunked dE reduction.

Conventions of every case (those of tests/test_train_kernels_gpu.py, whose Guard / strided / same_bits are used):
  * outputs (ctx, probs, dq, dk, dv, d_e1, d_e2) live in sentinel-filled allocations with guard elements on both sides; where
    the ABI has a stride some case uses ld > width, inputs with NaN in the gap columns, outputs with the sentinel still in the
    gap columns afterwards;
  * q, k, v come as three tensors with three strides ('sep'), as q and one k | v buffer ('q|kv'), and as one (M, 3d) buffer
    ('qkv'); dq, dk, dv likewise;
  * the workspace is exactly vqcpc_relattn_x_bwd_workspace(..) bytes inside a guard and holds NaN bit patterns before the
    call: a NaN in an output is a wrong read of a masked dS entry or of a stale partial sum;
  * the backward's `probs` input is the float64 forward's, rounded to fp32 (masked entries exactly 0, as the forward leaves
    them), so the backward kernels are judged on their own;
  * every launch is made twice and must give the same bits ("deterministic (no atomics)"); seeds are fixed.

Statistic.  ctx, dq, dk, dv: per (row, head), max |out - out64| / rms(out64 of those hd elements) (train_reference.row_err);
probs: per row, max |out - out64| (rows sum to 1); d_e1 / d_e2: per element, |out - out64| / ||its summands||_2
(attention_reference.de_err).  Never a tensor-wide denominator.  A row or element whose reference is structurally zero must be
exactly zero (its error is inf otherwise).

Tolerance.  None is a fixed number.  The yardstick is the SAME formula in plain fp32 torch on the CPU against float64: a group
passes when max err(kernel) <= C * max err(plain fp32); where plain fp32 is exact the bound is 4 ulp of each output, and outputs
ALL within 4 ulp pass in any case.  Every group prints `<family> <label>: kernel .. plain .. ratio ..`; medians, maxima and the
groups above 2 are in profiles/relattn_x_kernel_tests_log.md.

Groups.  One group per output and per instantiation is formed over ALL calls of one test: the calls that launch <HD, 1> (fewer
than four key tiles, Lk <= 96) and those that launch <HD, 4>.  The reason is the shape of the backward's error, not a
measurement: dS = P (dP - rowsum) is a difference, so the fp32 error of one dS entry relative to that entry is
u |dP| / |dP - rowsum|, which has a 1 / x tail.  Outputs that are sums of one or two dS entries (dk of the last key under the
causal mask, dq of the first queries, the corner rows of d_e1 / d_e2) inherit it, the maximum of a call is then set by ONE
entry, and the kernel's and plain fp32's roundings at that entry are independent: the ratio of the two maxima of a single
call is the ratio of two unrelated numbers.  Pooling the calls of a test puts several such entries into both maxima (the
remedy profiles/decode_kernel_tests_log.md records for the same statistic).  The Lk <= 3 calls are part of the <HD, 1> group.

C (`C_FAMILY`) = 4, the project's constant, for ctx, probs, dv and dk; 8 for dq and de: doubled once, because one group of dq
(4.28) and two of de (4.34, 7.49) exceeded 4 and the cause is named and replayed.  Cause: the strips' sequential fp32 chains.
The dq kernel forms dP = dO . V^T as chains of hd products per entry (v_mfma_f32_32x32x2_f32 rounds after each product; the
CPU's blocked dot product keeps several partial sums) and dP - rowsum cancels (dq 4.28, de 7.49: one ill-conditioned dS entry
each); the de kernel sums every element of dErel as ONE chain over all queries of all its sequences (de 4.34: 2 x 1552 terms).
`replay_dS` evaluates dP, the row sums and dS in fp32 in the kernel's order on the host, `replay_de` the dErel chains; dq and dk
follow from the replayed dS through float64 sums.  The replays give the kernel's own error to three or four digits (7.658e-04,
5.633e-05, 4.158e-06 for the three groups).  Whenever a dq / de group exceeds 4 the test replays the call that set the maximum,
prints `REPLAY ..: the host replay of the kernel's order gives X of the kernel's Y` and requires X >= Y / 2 ("most of it"): an
excess over 4 that the chains do not explain fails whatever C is.

What these tests changed in the kernel.  With ONE dP chain per entry, test_largest_lk[128-0.0-1] (Lq = Lk = 1024, hd = 128,
causal) missed C = 4 in dk: kernel 3.169e-05, plain 3.519e-06, ratio 9.00.  The maximum was row 1023 of dk, the last key, which
under the causal mask only query 1023 sees: dk[1023] = dS[1023][1023] qs_1023, one entry (P = 9.57e-4, dP = -1.1373, rowsum =
-0.8515), and the host replay of the 128 sequential roundings reproduced the figure.  relattn_x_bwd_dq_kernel now keeps two
accumulators (even / odd steps) for dP at hd >= 64, so no chain is longer than 32 steps: same registers and occupancy, the
group is at 3.20 (kernel 1.128e-05), and `replay_dS` follows the new order.  The bound was not moved.
"""
import math

import pytest
import torch

import attention_reference as A
import train_reference as T
from test_train_kernels_gpu import F32, NAN, SENT_I32, Guard, bits, call, gen, query, same_bits, strided, ulp32

pytestmark = pytest.mark.gpu

C_START = 4.0
C_FAMILY = {'ctx': 4.0, 'probs': 4.0, 'dq': 8.0, 'dk': 4.0, 'dv': 4.0, 'de': 8.0}      # dq, de: doubled once (module docstring)
RATIOS = {}
SEED = 0x5EED0A7700000000 + 4242
PACKS = ('sep', 'q|kv', 'qkv')


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
def stat(fam, out, ref, hd=None, norm=None):
    """The error vector of the module docstring: one entry per (row, head), per probs row, per d_e element."""
    out, ref = torch.as_tensor(out).detach().cpu().double(), torch.as_tensor(ref).detach().double()
    assert out.shape == ref.shape, (fam, out.shape, ref.shape)
    if fam == 'de':
        return A.de_err(out, ref, norm).reshape(-1)
    if fam == 'probs':
        return (out - ref).abs().reshape(-1, ref.shape[-1]).max(1)[0]
    return T.row_err(out.reshape(-1, hd), ref.reshape(-1, hd))


class Judge:
    """Collects the calls of one test into groups (family, instantiation); finish() prints every group's line and fails with all
    groups that missed."""

    def __init__(self, name):
        self.name, self.groups = name, {}

    def add(self, fam, group, label, kernel, plain, ref64, hd=None, norm=None, replay=None):
        """replay: None, or a callable -> the error vector (same statistic) of the host replay of this call's kernel order."""
        k = torch.as_tensor(kernel).detach().cpu().double()
        ref = torch.as_tensor(ref64).detach().double()
        assert bool(torch.isfinite(k).all()), f'{fam} {label}: non-finite output (a wrong read: NaN gap, masked dS, stale workspace)'
        ek, ep = stat(fam, k, ref, hd, norm), stat(fam, plain, ref, hd, norm)
        w4 = bool(((k - ref).abs() <= 4.0 * ulp32(ref)).all())
        self.groups.setdefault((fam, group), []).append((label, ek, ep, w4, replay))

    def finish(self):
        bad = []
        for (fam, group), items in self.groups.items():
            Ek, Ep = max(float(i[1].max()) for i in items), max(float(i[2].max()) for i in items)
            w4 = all(i[3] for i in items)
            label = f'{self.name} {group} ({len(items)} calls)'
            if Ep == 0.0:
                ok, ratio = w4, (0.0 if Ek == 0.0 else float('inf'))
            else:
                ratio = Ek / Ep
                ok = ratio <= C_FAMILY[fam] or w4
            print(f'{fam} {label}: kernel {Ek:.3e} plain {Ep:.3e} ratio {ratio:.2f}')
            RATIOS.setdefault(fam, []).append((label, ratio, Ek, Ep))
            if ok and not w4 and ratio > C_START:                      # only a doubled family gets here: the replay must explain it
                worst = max(items, key=lambda i: float(i[1].max()))
                Er = float(worst[4]().max())
                print(f"REPLAY {fam} {worst[0]}: the host replay of the kernel's order gives {Er:.3e} of the kernel's {float(worst[1].max()):.3e}")
                ok = Er >= 0.5 * float(worst[1].max())
            if not ok:
                bad.append((fam, label, Ek, Ep, ratio))
        self.groups = {}
        assert not bad, bad


def replay_dS(go, v, pin, scale, n, Lq, Lk, H, hd, mask):
    """dS of relattn_x_bwd_dq_kernel in fp32 in the kernel's order, on the host -> (n, H, Lq, Lk) float32 tensor.
      dP[i][j]: one chain over s = 0 .. hd/2 - 1 (hd >= 64: two chains, over the even and the odd s, and their sum), each step
                adding the products of head elements s and hd/2 + s (the two lane halves of v_mfma_f32_32x32x2_f32), rounded
                after each; times the keep-scale;
      rowsum:   lane j % 32 of wave w adds dP P of its key tiles jt0 + w, jt0 + w + NW, .. in turn (fma), the 32 lanes are
                combined by the xor butterfly 16, 8, 4, 2, 1, the NW waves in wave order;
      dS:       P * (dP - rowsum), both operations rounded.
    Entries outside the visible tiles have P = 0 and add exact zeros, so only the tile-to-wave assignment (jt0) matters."""
    import numpy as np
    f4, f8 = np.float32, np.float64
    r, KH = Lq // Lk, hd // 2
    QT, KT = (Lq + 31) // 32, (Lk + 31) // 32
    NW = 4 if KT >= 4 else 1
    do = A.heads(torch.as_tensor(go).float(), n, Lq, H).numpy()
    vh = A.heads(torch.as_tensor(v).float(), n, Lk, H).numpy()
    na = 2 if KH > 16 else 1
    accs = [np.zeros((n, H, Lq, Lk), f4) for _ in range(na)]
    for s in range(KH):
        for c in (s, KH + s):
            accs[s % na] = (accs[s % na].astype(f8) + do[..., c:c + 1].astype(f8) * vh[..., None, :, c].astype(f8)).astype(f4)
    acc = accs[0] if na == 1 else (accs[0] + accs[1]).astype(f4)
    dp = acc if scale is None else (acc * torch.as_tensor(scale).float().numpy()).astype(f4)
    P = np.zeros((n, H, 32 * QT, 32 * KT), f4)
    P[:, :, :Lq, :Lk] = torch.as_tensor(pin).float().numpy()
    dpp = np.zeros_like(P)
    dpp[:, :, :Lq, :Lk] = dp
    rd = np.zeros((n, H, 32 * QT), f4)
    lanes = np.arange(32)
    for t in range(QT):
        i0 = 32 * t
        jt0 = (i0 // r) // 32 if mask == 2 else 0
        KTe = min(KT, ((i0 + 31) // r) // 32 + 1) if mask == 1 else KT
        tot = None
        for w in range(NW):
            part = np.zeros((n, H, 32, 32), f4)
            for jt in range(jt0 + w, KTe, NW):
                sl = (slice(None), slice(None), slice(i0, i0 + 32), slice(32 * jt, 32 * jt + 32))
                part = (part.astype(f8) + dpp[sl].astype(f8) * P[sl].astype(f8)).astype(f4)
            for o in (16, 8, 4, 2, 1):
                part = (part + part[..., lanes ^ o]).astype(f4)
            tot = part[..., 0] if tot is None else (tot + part[..., 0]).astype(f4)
        rd[:, :, i0:i0 + 32] = tot
    dS = (P * (dpp - rd[..., None]).astype(f4)).astype(f4)
    return torch.from_numpy(dS[:, :, :Lq, :Lk].copy())


def replay_de(dS, q, n, Lq, Lk, H, hd):
    """d_e1 | d_e2 of relattn_x_bwd_de_kernel from a given fp32 dS, in fp32 in the kernel's order: every element of dErel is ONE
    chain over the sequences of its chunk and, per sequence, over the queries in the order the MFMA steps take them (per query
    tile: rows u and 16 + u of each half tile), rounded after each product; the chunk sums are then added in chunk order.
    Masked and out-of-range terms are exact zeros in the kernel as well, so no mask enters here."""
    import numpy as np
    f4, f8 = np.float32, np.float64
    r, QT = Lq // Lk, (Lq + 31) // 32
    _, spc, _ = x_chunks(n, Lk, H)
    dSn = torch.as_tensor(dS).float().numpy()
    qs = (A.heads(torch.as_tensor(q).float(), n, Lq, H).numpy() * f4(1.0 / math.sqrt(hd))).astype(f4)
    order = [32 * it + 16 * g + hs + u for it in range(QT) for hs in (0, 8) for u in range(8) for g in (0, 1)]
    tot = np.zeros((H, 2 * Lk - 1, hd), f4)
    for c0 in range(0, n, spc):
        acc = np.zeros((H, 2 * Lk - 1, hd), f8)
        for s in range(c0, min(c0 + spc, n)):
            for i in order:
                if i < Lq:
                    lo = Lk - 1 - i // r
                    acc[:, lo:lo + Lk] = (acc[:, lo:lo + Lk] + dSn[s, :, i, :, None].astype(f8) * qs[s, :, i, None, :].astype(f8)).astype(f4)
        tot = (tot + acc.astype(f4)).astype(f4)
    t = torch.from_numpy(tot)
    return torch.cat([t[:, :Lk].reshape(H * Lk, hd), torch.cat([torch.zeros(H, 1, hd), t[:, Lk:]], 1).reshape(H * Lk, hd)])


# =====================================================================================================================
# buffers
class Out:
    """Output columns inside a guarded, sentinel-filled (rows, ld) buffer; several outputs may share it (dk | dv, dq | dk | dv).
    check(): guards bit-unchanged, every element of the registered columns written, every other column still the sentinel."""

    def __init__(self, rows, ld):
        self.g, self.ld, self.cols = Guard((rows, ld)), ld, []

    def at(self, col, width):
        self.cols.append((col, width))
        return self.g.view[:, col:]                                     # its data_ptr is the output's base address

    def check(self):
        self.g.check(written=None)
        b = bits(self.g.view).cpu()
        w = torch.zeros(self.ld, dtype=torch.bool)
        for c, wd in self.cols:
            w[c:c + wd] = True
        assert not bool((b[:, w] == SENT_I32).any()), 'an output element was never written'
        assert bool((b[:, ~w] == SENT_I32).all()), 'a gap column of an output was written'

    def get(self, col, width):
        return self.g.view[:, col:col + width].cpu()


def make_data(n, H, Lq, Lk, hd, seed, qmul=1.0):
    g = gen(seed)
    d = H * hd
    return dict(q=torch.randn(n * Lq, d, generator=g) * qmul, k=torch.randn(n * Lk, d, generator=g), v=torch.randn(n * Lk, d, generator=g),
                e1=torch.randn(H * Lk, hd, generator=g) * 0.5, e2=torch.randn(H * Lk, hd, generator=g) * 0.5,
                go=torch.randn(n * Lq, d, generator=g))


def pack_inputs(D, d, pack):
    """-> (q, ldq, k, ldk, v, ldv) on the device, NaN in every gap column."""
    if pack == 'sep':
        return strided(D['q'], d + 4), d + 4, strided(D['k'], d + 8), d + 8, strided(D['v'], d + 12), d + 12
    if pack == 'q|kv':
        kv = strided(torch.cat([D['k'], D['v']], 1), 2 * d + 4)
        return D['q'].cuda(), d, kv, 2 * d + 4, kv[:, d:], 2 * d + 4
    qkv = strided(torch.cat([D['q'], D['k'], D['v']], 1), 3 * d + 4)
    return qkv, 3 * d + 4, qkv[:, d:], 3 * d + 4, qkv[:, 2 * d:], 3 * d + 4


def grad_outputs(n, Lq, Lk, d, pack):
    """-> [(Out, column) for dq, dk, dv], each with a leading dimension of its own where the packing allows one."""
    if pack == 'sep':
        return [(Out(n * Lq, d + 8), 0), (Out(n * Lk, d + 4), 0), (Out(n * Lk, d + 16), 0)]
    if pack == 'q|kv':
        kv = Out(n * Lk, 2 * d + 8)
        return [(Out(n * Lq, d), 0), (kv, 0), (kv, d)]
    o = Out(n * Lq, 3 * d + 4)
    return [(o, 0), (o, d), (o, 2 * d)]


def fwd_launch(dev, n, Lq, Lk, H, hd, mask, p, ldo):
    d = H * hd
    ctx, probs = Out(n * Lq, ldo), Guard((n, H, Lq, Lk))
    call('vqcpc_relattn_x_fwd', *dev['qkv'], dev['e1'], dev['e2'], ctx.at(0, d), ldo, probs.view, n, Lq, Lk, H, hd, mask, p, SEED)
    torch.cuda.synchronize()
    ctx.check()
    return ctx.get(0, d), probs.check().cpu()


def bwd_launch(dev, n, Lq, Lk, H, hd, mask, p, ldo, pack):
    d = H * hd
    outs = grad_outputs(n, Lq, Lk, d, pack)
    ptrs = []
    for o, col in outs:
        ptrs += [o.at(col, d), o.ld]
    de1, de2 = Guard((H * Lk, hd)), Guard((H * Lk, hd))
    wsb = query('vqcpc_relattn_x_bwd_workspace', n, Lq, Lk, H, hd)
    assert wsb % 4 == 0
    ws = Guard(wsb // 4, data=torch.full((wsb // 4,), NAN))
    q, ldq, k, ldk, v, ldv = dev['qkv']
    call('vqcpc_relattn_x_bwd', dev['go'], ldo, q, ldq, k, ldk, v, ldv, dev['probs'], dev['e1'], dev['e2'], *ptrs, de1.view, de2.view,
         n, Lq, Lk, H, hd, mask, p, SEED, ws.view, wsb)
    torch.cuda.synchronize()
    for o in {id(o): o for o, _ in outs}.values():
        o.check()
    ws.check(written=None)
    return [o.get(col, d) for o, col in outs] + [de1.check().cpu(), de2.check().cpu()]


def x_chunks(n_seq, Lk, H):
    """Restatement of x_chunks / x_bwd_t's launch geometry in csrc/relattn_x.hip -> (chunks, seq_per_chunk, launched chunks)."""
    RT = (2 * Lk - 1 + 31) // 32
    chunks = min(n_seq, max(1, 8192 // (H * RT)))
    spc = -(-n_seq // chunks)
    return chunks, spc, -(-n_seq // spc)


def workspace_bytes(n_seq, Lq, Lk, H, hd):
    """include/vqcpc.h's workspace as csrc/relattn_x.hip lays it out: dS, rounded up to 64 floats, + (chunks + 1) dErel images."""
    ds = n_seq * H * Lq * Lk
    return ((ds + 63) // 64 * 64 + (x_chunks(n_seq, Lk, H)[0] + 1) * H * (2 * Lk - 1) * hd) * 4


def run_case(J, label, n, H, Lq, Lk, hd, mask, p, pack, seed, D=None, backward=True, judge_backward=True):
    """One forward and one backward call (each twice), added to the test's groups.  -> dict of the kernel's outputs.
    judge_backward=False: the backward runs under every guard, NaN and repeatability check, but its accuracy is not judged."""
    d = H * hd
    assert pack != 'qkv' or Lq == Lk
    D = D or make_data(n, H, Lq, Lk, hd, seed)
    group = '<HD, 4>' if (Lk + 31) // 32 >= 4 else '<HD, 1>'
    ldo = d + 4 if pack == 'sep' else d
    scale = A.keep_scale(SEED, n, H, Lq, Lk, p)
    keep = A.keep_rule(mask, Lq, Lk)
    ctx64, probs64 = A.attn_fwd(D['q'], D['k'], D['v'], D['e1'], D['e2'], n, Lq, Lk, H, mask, scale)
    ctx32, probs32 = A.attn_fwd(D['q'], D['k'], D['v'], D['e1'], D['e2'], n, Lq, Lk, H, mask, scale, dtype=F32)
    dev = dict(qkv=pack_inputs(D, d, pack), e1=D['e1'].cuda(), e2=D['e2'].cuda())
    ctx, probs = fwd_launch(dev, n, Lq, Lk, H, hd, mask, p, ldo)
    ctx_b, probs_b = fwd_launch(dev, n, Lq, Lk, H, hd, mask, p, ldo)
    assert same_bits(ctx, ctx_b) and same_bits(probs, probs_b), f'{label}: two forward calls differ'
    assert bool((probs[:, :, ~keep] == 0).all()), f'{label}: a masked probability is not exactly 0'
    J.add('probs', group, label, probs, probs32, probs64)
    J.add('ctx', group, label, ctx, ctx32, ctx64, hd=hd)
    out = dict(ctx=ctx, probs=probs)
    if not backward:
        return out
    pin = probs64.float()                                              # the saved softmax the backward is given
    ref = A.attn_bwd(D['go'], D['q'], D['k'], D['v'], pin, D['e1'], D['e2'], n, Lq, Lk, H, mask, scale)
    dev.update(go=strided(D['go'], ldo), probs=pin.cuda())
    got = bwd_launch(dev, n, Lq, Lk, H, hd, mask, p, ldo, pack)
    got_b = bwd_launch(dev, n, Lq, Lk, H, hd, mask, p, ldo, pack)
    for name, a, b in zip(('dq', 'dk', 'dv', 'd_e1', 'd_e2'), got, got_b):
        assert same_bits(a, b), f'{label}: two backward calls differ in {name}'
        assert bool(torch.isfinite(a).all()), f'{label}: non-finite {name}'
    de, de64, nrm = (torch.cat([t[3], t[4]]) for t in (got, ref, (0, 0, 0) + tuple(ref[5:])))
    assert bool((de[nrm == 0] == 0).all()), f'{label}: a structurally zero element of d_e1 / d_e2 is not exactly 0'
    out.update(dq=got[0], dk=got[1], dv=got[2], d_e1=got[3], d_e2=got[4])
    if not judge_backward:
        return out
    pl = A.attn_bwd(D['go'], D['q'], D['k'], D['v'], pin, D['e1'], D['e2'], n, Lq, Lk, H, mask, scale, dtype=F32)
    cache = {}

    def replayed(fam):
        """The statistic of `fam` for: dS in fp32 in the kernel's order (replay_dS); dq, dk from it through float64 sums, d_e1 /
        d_e2 through the de kernel's fp32 chains (replay_de)."""
        if not cache:
            cache['dS'] = replay_dS(D['go'], D['v'], pin, scale, n, Lq, Lk, H, hd, mask)
            cache['r'] = A.attn_bwd(D['go'], D['q'], D['k'], D['v'], pin, D['e1'], D['e2'], n, Lq, Lk, H, mask, scale, dS=cache['dS'])
        rp = cache['r']
        if fam == 'de':
            return stat('de', replay_de(cache['dS'], D['q'], n, Lq, Lk, H, hd), de64, norm=nrm)
        i = ('dq', 'dk', 'dv').index(fam)
        return stat(fam, rp[i], ref[i], hd=hd)

    for i, name in enumerate(('dq', 'dk', 'dv')):
        J.add(name, group, label, got[i], pl[i], ref[i], hd=hd, replay=lambda name=name: replayed(name))
    J.add('de', group, label, de, torch.cat([pl[3], pl[4]]), de64, norm=nrm, replay=lambda: replayed('de'))
    return out


# =====================================================================================================================
# shapes
R1_LKS = [1, 2, 3, 31, 32, 33, 64, 96, 97, 129]           # ragged key tile / query strip; NW = 1 up to 96, NW = 4 from 97
CROSS_LKS = [3, 12, 33, 97]
MASKS = [0, 1, 2]
HDS = [16, 32, 64, 128]


@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('hd', HDS)
def test_square(hd, mask):
    """r = 1: <HD, 1> for Lk <= 96, <HD, 4> for Lk = 97 / 129; p in {0, 0.25}; the three packings in turn."""
    J = Judge(f'sq hd{hd} m{mask}')
    for i, Lk in enumerate(R1_LKS):
        for p in (0.0, 0.25):
            pack = PACKS[(i + (p > 0) + mask) % 3]
            run_case(J, f'sq hd{hd} m{mask} Lk{Lk} p{p} {pack}', 2, 2, Lk, Lk, hd, mask, p, pack, 100 * Lk + hd + mask)
    J.finish()


@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('r', [2, 4, 16])
@pytest.mark.parametrize('hd', HDS)
def test_cross(hd, r, mask):
    """Lq = r Lk: strips whose 32 rows span 32 / r memory positions, pmax > Lk - 1 in the last strip (rlo < 0: xerel_row clamps),
    the jt0 / KTe / it0 / itE skips with r > 1; Lk = 97: NW = 4."""
    J = Judge(f'x hd{hd} r{r} m{mask}')
    for i, Lk in enumerate(CROSS_LKS):
        p = (0.0, 0.25)[(i + r + mask) % 2]
        pack = PACKS[(i + mask + hd // 16) % 2]
        run_case(J, f'x hd{hd} r{r} m{mask} Lk{Lk} p{p} {pack}', 2, 2, r * Lk, Lk, hd, mask, p, pack, 1000 * r + 10 * Lk + hd + mask)
    J.finish()


@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('hd,p', [(16, 0.25), (128, 0.0)])
def test_largest_lk(hd, p, mask):
    """Lq = Lk = 1024 = kXMaxLk: 135 680 bytes of dynamic LDS forward, 140 288 backward (hipFuncSetAttribute; 160 KB per CU).
    [128-0.0-1] is the case behind the two dP accumulators of the dq kernel (module docstring): dk 9.00 x plain with one chain,
    3.20 x with two."""
    J = Judge(f'Lk1024 hd{hd} m{mask} p{p}')
    run_case(J, f'Lk1024 hd{hd} m{mask} p{p}', 1, 1, 1024, 1024, hd, mask, p, 'qkv' if hd == 16 else 'sep', 5000 + hd + mask)
    J.finish()


def test_lk_1025_is_refused_before_any_launch(_lib):
    n, H, L, hd = 1, 1, 1025, 16
    q = torch.zeros(L, 3 * hd, device='cuda')
    e, ctx, probs = torch.zeros(L, hd, device='cuda'), Guard((L, hd)), Guard((L, L))
    with pytest.raises(_lib.VqcpcHipError, match=r'relattn_x_fwd: unsupported Lq=1025 Lk=1025'):
        call('vqcpc_relattn_x_fwd', q, 3 * hd, q[:, hd:], 3 * hd, q[:, 2 * hd:], 3 * hd, e, e, ctx.view, hd, probs.view, n, L, L, H, hd, 0, 0.0, 0)
    wsb = query('vqcpc_relattn_x_bwd_workspace', n, L, L, H, hd)
    ws, dqkv, de = Guard(wsb // 4), Guard((L, 3 * hd)), Guard((L, hd))
    with pytest.raises(_lib.VqcpcHipError, match=r'relattn_x_bwd: unsupported Lq=1025 Lk=1025'):
        call('vqcpc_relattn_x_bwd', ctx.view, hd, q, 3 * hd, q[:, hd:], 3 * hd, q[:, 2 * hd:], 3 * hd, probs.view, e, e, dqkv.view, 3 * hd,
             dqkv.view[:, hd:], 3 * hd, dqkv.view[:, 2 * hd:], 3 * hd, de.view, de.view, n, L, L, H, hd, 0, 0.0, 0, ws.view, wsb)
    torch.cuda.synchronize()
    for g in (ctx, probs, ws, dqkv, de):
        g.check(written=False)


@pytest.mark.parametrize('r', [1, 4])
def test_chunked_de_reduction(r):
    """H = 128, Lk = 8, n_seq = 65: x_chunks gives 64, so a chunk holds 2 sequences, 33 chunks are launched and the last holds
    one (n_end = min(..)).  The three numbers are asserted from the restatement above, and the restatement is tied to the
    library through the workspace size, which contains `chunks`: a retuned constant fails here instead of un-testing the path."""
    n, H, hd, Lk = 65, 128, 16, 8
    assert x_chunks(n, Lk, H) == (64, 2, 33) and n - 32 * 2 == 1
    assert query('vqcpc_relattn_x_bwd_workspace', n, r * Lk, Lk, H, hd) == workspace_bytes(n, r * Lk, Lk, H, hd)
    assert x_chunks(64, Lk, H) == (64, 1, 64)                            # one sequence fewer and every chunk is one sequence
    J = Judge(f'chunked r{r}')
    for mask, p in ((0, 0.0), (1, 0.25), (2, 0.0)):
        run_case(J, f'chunked r{r} m{mask} p{p}', n, H, r * Lk, Lk, hd, mask, p, 'q|kv', 7000 + r + mask)
    J.finish()


@pytest.mark.parametrize('hd', HDS)
def test_wide_logits(hd):
    """q scaled so that the logits span about +-60: rows near one-hot, the max subtraction and __expf at large negative
    arguments, kNegBigX = -1e30 still below every kept logit.  The forward is judged.  The backward runs under the guards, the NaN
    poison and the repeat, but is not judged: at a one-hot row dS = P (dP - rowsum) is the difference of two equal numbers, its
    float64 value lies below the fp32 resolution of its terms, and EVERY fp32 evaluation has a relative error of order 1 against
    float64 (plain fp32 torch: 0.76 of the row's rms in dk, 7.6 in dq, the same figures as the kernel) -- the yardstick says
    nothing there."""
    J = Judge(f'wide hd{hd}')
    for mask, Lq, Lk in ((0, 33, 33), (1, 129, 129), (2, 132, 33)):
        n, H = 2, 2
        D = make_data(n, H, Lq, Lk, hd, 9000 + hd + mask)
        qs = A.heads(D['q'].double(), n, Lq, H) / math.sqrt(hd)
        s = qs @ A.heads(D['k'].double(), n, Lk, H).transpose(-1, -2) + A.rel_bias(qs, D['e1'], D['e2'], Lk)
        D['q'] = D['q'] * (60.0 / float(s.abs().max()))
        out = run_case(J, f'wide hd{hd} m{mask} Lq{Lq} Lk{Lk}', n, H, Lq, Lk, hd, mask, 0.0, 'q|kv', 0, D=D, judge_backward=False)
        assert float(out['probs'].max()) > 0.99
    J.finish()


@pytest.mark.parametrize('Lk', [32, 128])
@pytest.mark.parametrize('hd', HDS)
def test_one_hot_inputs_are_exact(hd, Lk):
    """q = 0 and zero tables: every logit is 0, the probabilities are 1 / Lk (a power of two) and, with one-hot rows of v, ctx is
    a count times 1 / Lk -- plain fp32 is exact, so the 4-ulp rule applies (Lk = 32: NW = 1, Lk = 128: NW = 4)."""
    n, H = 2, 2
    D = make_data(n, H, Lk, Lk, hd, Lk + hd)
    D['q'].zero_(), D['e1'].zero_(), D['e2'].zero_(), D['v'].zero_()
    cols = torch.randint(0, H * hd, (n * Lk,), generator=gen(3 * Lk + hd))
    D['v'][torch.arange(n * Lk), cols] = 1.0
    ctx32, probs32 = A.attn_fwd(D['q'], D['k'], D['v'], D['e1'], D['e2'], n, Lk, Lk, H, 0, dtype=F32)
    ctx64, probs64 = A.attn_fwd(D['q'], D['k'], D['v'], D['e1'], D['e2'], n, Lk, Lk, H, 0)
    assert torch.equal(ctx32.double(), ctx64) and torch.equal(probs32.double(), probs64)
    J = Judge(f'one-hot hd{hd} Lk{Lk}')
    run_case(J, f'one-hot hd{hd} Lk{Lk}', n, H, Lk, Lk, hd, 0, 0.0, 'qkv', 0, D=D, backward=False)
    J.finish()


# =====================================================================================================================
# bit-exact properties
@pytest.mark.parametrize('Lq,Lk,hd,mask', [(48, 12, 32, 2), (129, 129, 16, 1)])
def test_a_sequence_of_a_batch_has_the_bits_of_the_sequence_alone(Lq, Lk, hd, mask):
    """p = 0: ctx, probs, dq, dk, dv of sequence s do not depend on the batch around it (NW = 1 and NW = 4)."""
    n, H = 3, 2
    J = Judge(f'batch Lq{Lq} Lk{Lk}')
    D = make_data(n, H, Lq, Lk, hd, Lq + hd)
    whole = run_case(J, f'batch Lq{Lq} Lk{Lk}', n, H, Lq, Lk, hd, mask, 0.0, 'q|kv', 0, D=D)
    for s in range(n):
        Ds = dict(q=D['q'][s * Lq:(s + 1) * Lq], k=D['k'][s * Lk:(s + 1) * Lk], v=D['v'][s * Lk:(s + 1) * Lk], e1=D['e1'], e2=D['e2'],
                  go=D['go'][s * Lq:(s + 1) * Lq])
        one = run_case(J, f'alone {s} Lq{Lq} Lk{Lk}', 1, H, Lq, Lk, hd, mask, 0.0, 'q|kv', 0, D=Ds)
        assert same_bits(one['probs'][0], whole['probs'][s])
        for name, L in (('ctx', Lq), ('dq', Lq), ('dk', Lk), ('dv', Lk)):
            assert same_bits(one[name], whole[name][s * L:(s + 1) * L]), (name, s)
    J.finish()


@pytest.mark.parametrize('L', [24, 40])
def test_the_square_entry_points_route_here(L):
    """vqcpc_relattn_fwd / _bwd at an L that is neither 16 nor 4: the bits of vqcpc_relattn_x_fwd / _bwd with Lq = Lk = L, mask 0,
    on the column blocks of the same qkv buffer."""
    n, H, hd, p = 3, 2, 32, 0.25
    d = H * hd
    J = Judge(f'route L{L}')
    D = make_data(n, H, L, L, hd, 40 + L)
    ld = 3 * d + 4
    x = run_case(J, f'route L{L}', n, H, L, L, hd, 0, p, 'qkv', 0, D=D)
    qkv = strided(torch.cat([D['q'], D['k'], D['v']], 1), ld)
    e1, e2 = D['e1'].cuda(), D['e2'].cuda()
    ctx, probs = Out(n * L, d), Guard((n, H, L, L))
    call('vqcpc_relattn_fwd', qkv, ld, e1, e2, ctx.at(0, d), d, probs.view, n, L, H, hd, p, SEED)
    torch.cuda.synchronize()
    ctx.check()
    assert same_bits(ctx.get(0, d), x['ctx']) and same_bits(probs.check().cpu(), x['probs'])
    pin = A.attn_fwd(D['q'], D['k'], D['v'], D['e1'], D['e2'], n, L, L, H, 0, A.keep_scale(SEED, n, H, L, L, p))[1].float().cuda()
    wsb = query('vqcpc_relattn_bwd_workspace', n, L, H, hd)
    assert wsb == query('vqcpc_relattn_x_bwd_workspace', n, L, L, H, hd)
    ws = Guard(wsb // 4, data=torch.full((wsb // 4,), NAN))
    dqkv, de1, de2 = Out(n * L, ld), Guard((H * L, hd)), Guard((H * L, hd))
    call('vqcpc_relattn_bwd', D['go'].cuda(), d, qkv, ld, pin, e1, e2, dqkv.at(0, 3 * d), ld, de1.view, de2.view, n, L, H, hd, p, SEED,
         ws.view, wsb)
    torch.cuda.synchronize()
    dqkv.check()
    ws.check(written=None)
    for i, name in enumerate(('dq', 'dk', 'dv')):
        assert same_bits(dqkv.get(i * d, d), x[name]), name
    assert same_bits(de1.check().cpu(), x['d_e1']) and same_bits(de2.check().cpu(), x['d_e2'])
    J.finish()


def test_no_sequences_writes_nothing():
    H, Lq, Lk, hd = 2, 48, 12, 16
    d = H * hd
    q, kv, e = torch.randn(Lq, d, device='cuda'), torch.randn(Lk, 2 * d, device='cuda'), torch.randn(H * Lk, hd, device='cuda')
    ctx, probs = Guard((Lq, d)), Guard((1, H, Lq, Lk))
    call('vqcpc_relattn_x_fwd', q, d, kv, 2 * d, kv[:, d:], 2 * d, e, e, ctx.view, d, probs.view, 0, Lq, Lk, H, hd, 2, 0.25, SEED)
    torch.cuda.synchronize()
    ctx.check(written=False)
    probs.check(written=False)
