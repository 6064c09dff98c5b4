"""The voice-leading rules of `templates.VoiceLeadingRules` (csrc/rules.hip), restated in plain numpy / Python loops.  Exact
integer logic: the kernel must agree bit for bit.

Position: chorale column `col`, tick e = col // nc, voice v = col % nc; voice 0 is the top voice.  `row` is the row's tokens in
chorale coordinates; only columns < col are read (the history), so whatever lies at and past col cannot matter.
kinds[u][tok]: a MIDI pitch >= 0, HOLD, or REST / META (no pitch)."""
import numpy as np

HOLD, REST, META = -1, -2, -3
NONE = None
CROSSING, LEAP, PARALLEL = 1, 2, 4
DROP_ORDER = (PARALLEL, LEAP, CROSSING)


def kind(kinds, vocab, u, tok):
    tok = int(tok)
    if tok < 0 or tok >= vocab[u]:
        return META
    return int(kinds[u][tok])


def pitch_at(row, kinds, vocab, nc, u, e1):
    """Walk back from tick e1 while voice u holds; the pitch where the walk stops, or NONE."""
    t = e1
    while t >= 0:
        k = kind(kinds, vocab, u, row[t * nc + u])
        if k == HOLD:
            t -= 1
            continue
        return k if k >= 0 else NONE
    return NONE


def voices_now(row, constraint, kinds, vocab, nc, col):
    """-> (prev, now): per voice the pitch of the previous tick and, for the KNOWN voices of this tick, the pitch of this one
    (NONE for the unknown ones, for voice v itself, and for a rest or meta token)."""
    e, v = divmod(col, nc)
    prev = [pitch_at(row, kinds, vocab, nc, u, e - 1) for u in range(nc)]
    now = [NONE] * nc
    for u in range(nc):
        if u == v:
            continue
        c = e * nc + u
        tok = -1
        if u < v:
            tok = int(row[c])                                   # emitted at this tick
        elif constraint is not None and c < len(constraint):
            tok = int(constraint[c])                            # forced, not yet emitted
        if tok < 0:
            continue
        k = kind(kinds, vocab, u, tok)
        now[u] = k if k >= 0 else prev[u] if k == HOLD else NONE
    return prev, now


def violations(ck, v, prev, now, max_leap):
    """The rules a candidate of kind ck of voice v breaks (all three, enabled or not)."""
    nc = len(prev)
    prev_v = prev[v]
    p = ck if ck >= 0 else prev_v if ck == HOLD else NONE
    bits = 0
    if p is not NONE:
        for u in range(nc):
            if now[u] is NONE:
                continue
            if (u < v and p > now[u]) or (u > v and p < now[u]):
                bits |= CROSSING
    if ck >= 0 and prev_v is not NONE and max_leap[v] >= 0 and abs(ck - prev_v) > max_leap[v]:
        bits |= LEAP
    if p is not NONE and prev_v is not NONE and p != prev_v:
        for u in range(nc):
            if now[u] is NONE or prev[u] is NONE or now[u] == prev[u]:
                continue
            if (now[u] > prev[u]) != (p > prev_v):
                continue
            a, b = abs(now[u] - p) % 12, abs(prev[u] - prev_v) % 12
            if a == b and a in (0, 7):
                bits |= PARALLEL
    return bits


def position(row, col, nc, kinds, vocab, max_leap, enabled, constraint=None, static=None, exclude=None):
    """One position.  static: bool (256,) or None; exclude: bool (256,) of voice v or None.
    -> (the set the kernel writes, bool (256,), and the report).  max_leap: one int per voice, < 0 = off."""
    e, v = divmod(col, nc)
    V = vocab[v]
    prev, now = voices_now(row, constraint, kinds, vocab, nc, col)
    forced = -1
    if constraint is not None and col < len(constraint):
        forced = int(constraint[col])
    if forced >= 0:
        bits = violations(kind(kinds, vocab, v, forced), v, prev, now, max_leap) & enabled
        if static is not None:
            out = np.array(static, dtype=bool).copy()
        else:
            out = np.zeros(256, dtype=bool)
            out[:V] = True
        return out, bits << 4
    vi = [violations(int(kinds[v][k]), v, prev, now, max_leap) & enabled for k in range(V)]
    in_s = [True if static is None else bool(static[k]) for k in range(V)]
    in_e = [in_s[k] and not (exclude is not None and bool(exclude[k])) for k in range(V)]
    drop = 0
    for rule in DROP_ORDER:
        if any(in_e[k] and (vi[k] & ~drop) == 0 for k in range(V)):
            break
        drop |= rule
    out = np.zeros(256, dtype=bool)
    for k in range(V):
        out[k] = in_s[k] and (vi[k] & ~drop) == 0
    if not out.any():                                           # nothing of the vocabulary in the static set: no restriction
        out[:V] = True
    return out, drop & enabled


def row_report(row, nc, kinds, vocab, max_leap, enabled, constraint=None, static=None, exclude=None, first=0, last=None):
    """Every column of [first, last) of a finished row, given its own tokens as the history.  static: bool (width, 256) or None,
    exclude: bool (nc, 256) or None.  -> (sets bool (width, 256), report int32 (width,), -1 outside [first, last))."""
    width = len(row)
    last = width if last is None else last
    sets = np.zeros((width, 256), dtype=bool)
    report = np.full(width, -1, dtype=np.int32)
    for col in range(first, last):
        s, r = position(row, col, nc, kinds, vocab, max_leap, enabled, constraint,
                        None if static is None else static[col], None if exclude is None else exclude[col % nc])
        sets[col], report[col] = s, r
    return sets, report


def audit(x, nc, kinds, vocab, max_leap, enabled):
    """x: one row of tokens (width,), every token taken as forced -> int32 (width,), the broken enabled rules << 4."""
    out = np.zeros(len(x), dtype=np.int32)
    for col in range(len(x)):
        if int(x[col]) < 0:
            continue
        out[col] = position(x, col, nc, kinds, vocab, max_leap, enabled, constraint=x)[1]
    return out


def pack(bits):
    """bool (..., 256) -> int32 (..., 8): bit i & 31 of word i >> 5."""
    b = np.asarray(bits, dtype=np.uint64).reshape(bits.shape[:-1] + (8, 32))
    words = (b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return words.view(np.int32)


def unpack(words):
    """int32 (..., 8) -> bool (..., 256)."""
    w = np.ascontiguousarray(words).view(np.uint32)
    return ((w[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(w.shape[:-1] + (256,))
