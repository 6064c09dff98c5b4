"""vqcpc_decode_rules and vqcpc_rules_audit (csrc/rules.hip) called directly: the written sets and reports equal the numpy
reference (tests/rules_reference.py) bit for bit on the case tables of tests/rules_cases.py -- M in {1, 3, 64}, nc in {1, 4, 16},
V_c in {1, 5, 31, 32, 33, 64, 65, 255, 256}, hold chains of 0, 1, 63, 64, 65 and 200 ticks (also across the window's start into
the chorale and down to column 0), static sets NULL and given, an exclude that drains what the rules leave, win NULL, given
and without a live window, columns at and past the leading dimensions, pos >= T.  Invariants: what lies at and past the
column cannot matter, guard cells around both outputs stay intact, two launches give equal bits, a row alone equals the row
among 64.  The audit kernel is checked on whole random pieces of 1, 17 and 400 ticks."""
import ctypes

import numpy as np
import pytest
import torch

import rules_cases as C
import rules_reference as R

pytestmark = pytest.mark.gpu

GUARD = 64
SET_FILL, REPORT_FILL = 0x5A5A5A5A, -77


def _offsets(vocab):
    off = [0]
    for n in vocab:
        off.append(off[-1] + int(n))
    return (ctypes.c_int32 * len(off))(*off)


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _guarded(rows, ld, inner, fill, dtype):
    """A (rows, ld[, inner]) buffer between two guard strips, all `fill`."""
    flat = torch.full((rows * ld * inner + 2 * GUARD,), fill, dtype=dtype, device='cuda')
    return flat, flat[GUARD:GUARD + rows * ld * inner].view((rows, ld, inner) if inner > 1 else (rows, ld))


def launch(c, rows=None, ld=None, tokens=None, chorale=None, pos=None, win='case', static='case', into=None):
    """One vqcpc_decode_rules launch of case c (rows: a slice of its rows; ld: the leading dimension of constraint, static
    sets, sets and report).  -> (flat sets, sets, flat report, report) on the device."""
    from vqcpc_bach_amd import hip
    rows = slice(None) if rows is None else rows
    long = c['mode'] == 'long'
    ld = c['width'] if ld is None else ld
    tok = _dev((c['tokens'] if tokens is None else tokens)[rows])
    M = tok.shape[0]
    cho = _dev((c['chorale'] if chorale is None else chorale)[rows]) if long else None
    cons = _dev(c['constraint'][rows][:, :ld])
    stat = c['static'] if static == 'case' else static
    stat = None if stat is None else _dev(stat[rows][:, :ld])
    excl = None if c['exclude'] is None else _dev(R.pack(c['exclude']))
    if into is None:
        into = _guarded(M, ld, 8, SET_FILL, torch.int32) + _guarded(M, ld, 1, REPORT_FILL, torch.int32)
    fs, sets, fr, report = into
    p = torch.tensor([c['pos'] if pos is None else pos], dtype=torch.int32, device='cuda')
    w = None
    if long:
        w = torch.tensor([c['w0'] + 1, c['w0']] if win == 'case' else win, dtype=torch.int32, device='cuda')
    hip.call('vqcpc_decode_rules', tok, c['T'], c['T'], cho, c['width'] if long else 0, cons, ld, _dev(c['kinds']),
             c['kinds'].shape[1], _offsets(c['vocab']), c['nc'], _dev(c['max_leap']), c['enabled'], excl, stat, ld, sets, ld, report,
             ld, p, w, c['U'], M)
    torch.cuda.synchronize()
    return fs, sets, fr, report


def _untouched_but(c, fs, sets, fr, report, written):
    """Every cell but column c['col'] of the rows keeps its filler -- the guard strips too; `written`: the column was written."""
    s, r = sets.clone(), report.clone()
    col = c['col']
    if written:
        assert bool((r[:, col] != REPORT_FILL).all())
        s[:, col], r[:, col] = SET_FILL, REPORT_FILL
    assert bool((s == SET_FILL).all()) and bool((r == REPORT_FILL).all())
    for flat, fill in ((fs, SET_FILL), (fr, REPORT_FILL)):
        assert bool((flat[:GUARD] == fill).all()) and bool((flat[-GUARD:] == fill).all())


def _check(c, sets, report, want=None, rows=None):
    want_sets, want_report = C.expected(c['id']) if want is None else want
    rows = slice(None) if rows is None else rows
    got = R.unpack(sets[:, c['col']].cpu().numpy())
    assert np.array_equal(report[:, c['col']].cpu().numpy(), want_report[rows]), (c['id'], report[:, c['col']].cpu(), want_report[rows])
    assert np.array_equal(got, want_sets[rows]), c['id']


ACTIVE = [c['id'] for c in C.CASES if not (c['win_off'] or c['small_ld'] or c['past_T'])]


@pytest.mark.parametrize('cid', ACTIVE)
def test_sets_and_reports_equal_the_reference(cid):
    c = C.CASES[cid]
    out = launch(c)
    _check(c, out[1], out[3])
    _untouched_but(c, *out, written=True)
    # a pure overwrite: a second launch into the same buffers, and one into buffers of other contents, give the same bits
    first = (out[1].clone(), out[3].clone())
    out = launch(c, into=out)
    assert torch.equal(out[1], first[0]) and torch.equal(out[3], first[1])
    other = (None, torch.full_like(first[0], -1), None, torch.full_like(first[1], 12345))
    out = launch(c, into=other)
    assert torch.equal(out[1][:, c['col']], first[0][:, c['col']]) and torch.equal(out[3][:, c['col']], first[1][:, c['col']])


@pytest.mark.parametrize('cid', ACTIVE[::4])
def test_what_lies_at_and_past_the_column_cannot_matter(cid):
    c = C.CASES[cid]
    rng = np.random.default_rng(77 + cid)
    tokens = c['tokens'].copy()
    for u in range(c['nc']):
        tokens[:, u::c['nc']] = np.where(np.arange(c['T'])[u::c['nc']] >= c['pos'],
                                         rng.integers(0, c['vocab'][u], size=tokens[:, u::c['nc']].shape), tokens[:, u::c['nc']])
    chorale = None
    if c['mode'] == 'long':
        chorale = c['chorale'].copy()
        base = c['w0'] * c['U']                                        # the chorale under the live window is stale, whatever it holds
        for u in range(c['nc']):
            chorale[:, base + u::c['nc']] = rng.integers(0, c['vocab'][u], size=chorale[:, base + u::c['nc']].shape)
    out = launch(c, tokens=tokens, chorale=chorale)
    _check(c, out[1], out[3])


@pytest.mark.parametrize('cid', [c['id'] for c in C.CASES if c['M'] == 64])
def test_a_row_alone_equals_the_row_among_64(cid):
    c = C.CASES[cid]
    whole = launch(c)
    for b in (0, 17, 63):
        alone = launch(c, rows=slice(b, b + 1))
        assert torch.equal(alone[1][0, c['col']], whole[1][b, c['col']]) and torch.equal(alone[3][0, c['col']], whole[3][b, c['col']])
        _check(c, alone[1], alone[3], rows=slice(b, b + 1))
    few = launch(c, rows=slice(5, 8))
    assert torch.equal(few[1][:, c['col']], whole[1][5:8, c['col']])


def _only(flag):
    return [c for c in C.CASES if c[flag]][0]


def test_without_a_live_window_nothing_is_written():
    c = _only('win_off')
    _untouched_but(c, *launch(c, win=[c['w0'], -1]), written=False)
    _check(c, *[launch(c)[i] for i in (1, 3)])                           # the same case with its window: written


def test_columns_at_and_past_the_leading_dimensions():
    c = _only('small_ld')
    assert c['col'] > c['T']
    _untouched_but(c, *launch(c, ld=c['T']), written=False)             # past every leading dimension
    _untouched_but(c, *launch(c, ld=c['col']), written=False)           # AT the leading dimension
    # one column more: written, with the constraint's columns past it free and the static set of the column read
    ld = c['col'] + 1
    want_sets, want_report = np.zeros((c['M'], 256), dtype=bool), np.zeros(c['M'], dtype=np.int32)
    for b in range(c['M']):
        want_sets[b], want_report[b] = R.position(c['rows'][b], c['col'], c['nc'], c['kinds'], c['vocab'], c['max_leap'], c['enabled'],
                                                  c['constraint'][b, :ld], R.unpack(c['static'][b, c['col']]), None)
    out = launch(c, ld=ld)
    _check(c, out[1], out[3], want=(want_sets, want_report))
    _untouched_but(c, *out, written=True)


def test_once_pos_reaches_T_nothing_happens():
    c = _only('past_T')
    for pos in (c['T'], c['T'] + 5, -1):
        _untouched_but(c, *launch(c, pos=pos), written=False)
    _check(c, *[launch(c)[i] for i in (1, 3)])


def test_the_host_entry_refuses_bad_arguments_before_any_launch():
    from vqcpc_bach_amd import hip
    c = C.CASES[4]                                                       # nc = 4, fixed window
    T, nc, ld = c['T'], c['nc'], c['width']
    tok, cons, kinds, leap = _dev(c['tokens']), _dev(c['constraint']), _dev(c['kinds']), _dev(c['max_leap'])
    sets = torch.zeros(c['M'], ld, 8, dtype=torch.int32, device='cuda')
    report = torch.zeros(c['M'], ld, dtype=torch.int32, device='cuda')
    pos = torch.tensor([c['pos']], dtype=torch.int32, device='cuda')
    win = torch.tensor([1, 0], dtype=torch.int32, device='cuda')
    ldk, off = c['kinds'].shape[1], _offsets(c['vocab'])

    def call(tokens=tok, ldtok=T, chorale=None, ldch=0, constraint=cons, ldcons=ld, kinds_=kinds, ldk_=ldk, off_=off, nc_=nc,
             leap_=leap, rules=7, static=None, ldstat=ld, sets_=sets, ldsets=ld, report_=report, ldrep=ld, pos_=pos, win_=None,
             M=c['M']):
        hip.call('vqcpc_decode_rules', tokens, ldtok, T, chorale, ldch, constraint, ldcons, kinds_, ldk_, off_, nc_, leap_, rules, None,
                 static, ldstat, sets_, ldsets, report_, ldrep, pos_, win_, c['U'], M)
    call()                                                               # the arguments as they are: accepted
    big = _offsets([257] + c['vocab'][1:])
    for bad in (dict(tokens=None), dict(kinds_=None), dict(off_=None), dict(sets_=None), dict(pos_=None), dict(M=0), dict(M=65),
                dict(nc_=17), dict(nc_=0), dict(off_=big, ldk_=300), dict(ldk_=max(c['vocab']) - 1), dict(ldtok=T - 1),
                dict(ldcons=T - 1), dict(ldsets=T - 1), dict(ldrep=T - 1), dict(static=sets, ldstat=T - 1), dict(rules=0),
                dict(rules=8), dict(leap_=None), dict(win_=win), dict(win_=win, chorale=tok, ldch=T - 1)):
        with pytest.raises(hip.VqcpcHipError):
            call(**bad)
    x = _dev(c['rows'])
    audit = lambda **kw: hip.call('vqcpc_rules_audit', kw.get('x', x), kw.get('ld', ld), kw.get('width', ld), kinds, ldk,
                                  kw.get('off', off), kw.get('nc', nc), leap, 7, kw.get('report', report), kw.get('ldrep', ld),
                                  kw.get('rows', c['M']))
    audit()
    for bad in (dict(x=None), dict(report=None), dict(rows=0), dict(nc=17), dict(off=big), dict(ld=ld - 1), dict(ldrep=ld - 1),
                dict(width=ld - 1), dict(width=0)):
        with pytest.raises(hip.VqcpcHipError):
            audit(**bad)
    torch.cuda.synchronize()


@pytest.mark.parametrize('ticks,nc,V', [(1, 4, 31), (17, 4, 31), (400, 4, 31), (17, 1, 31), (70, 16, 33)])
def test_the_audit_equals_the_reference_on_whole_pieces(ticks, nc, V):
    from vqcpc_bach_amd import hip
    rows = 3
    x, kinds, vocab, leaps = C.audit_piece(900 + ticks + nc, rows, ticks, nc, V)
    x[1, ticks * nc // 2] = -1                                          # a place without a token judges nothing
    width = ticks * nc
    for enabled in (7, 5):
        want = np.stack([R.audit(x[b], nc, kinds, vocab, leaps, enabled) for b in range(rows)])
        flat, report = _guarded(rows, width + 3, 1, REPORT_FILL, torch.int32)
        hip.call('vqcpc_rules_audit', _dev(x), width, width, _dev(kinds), kinds.shape[1], _offsets(vocab), nc, _dev(leaps), enabled,
                 report, width + 3, rows)
        torch.cuda.synchronize()
        assert np.array_equal(report[:, :width].cpu().numpy(), want), (ticks, nc, enabled)
        assert bool((report[:, width:] == REPORT_FILL).all())
        assert bool((flat[:GUARD] == REPORT_FILL).all()) and bool((flat[-GUARD:] == REPORT_FILL).all())
        if ticks >= 17 and enabled == 7:
            assert len(np.unique(want)) >= (3 if nc > 1 else 2)          # the piece breaks rules (one voice: leaps): the comparison says something
