"""Allowed code sets for `PriorRelative.generate_codes(allowed=...)`: building them, checking them, packing them.  Host only
(plain torch ops on whatever device the tensors live on; no kernel of the library is called).

A set is a bool tensor whose last axis runs over the codes: (rows | 1, num_tokens, V) for a merged prior, (rows | 1, num_tokens,
ncb, K) for a product prior, whose allowed set at a column is the Cartesian product of ncb digit sets -- the one form that needs
no array of K**ncb entries.  True = the code (digit) may be drawn.  Sets combine with `&`.

  code_sets    the merged tensor from {column: codes}, full where nothing is said
  digit_sets   the product tensor from {column: [digits of codebook 0, digits of codebook 1, ...]} (None = every digit)
  check_sets   the one check of a call: the first empty set, or the first forced code its own set forbids -> ValueError
  pack_sets    bool (..., V) -> int32 (..., ceil(V / 32)): bit i & 31 of word i >> 5 is code i (the samplers' layout)

The same tensors restrict the candidates of `generate_codes(beam=W)`: a search through sets.
Out of scope: sets for `score_codes` / vqcpc_prior_score, relational (voice-leading-style) rules on codes, and arbitrary
(non-product) sets over the K**ncb codes of a product prior."""
import torch


def code_sets(num_tokens, V, columns=None):
    """-> bool (1, num_tokens, V): column c allows exactly the codes columns[c] (an iterable of ints in [0, V)), every other
    column every code.  ValueError on a column outside [0, num_tokens) or a code outside [0, V)."""
    num_tokens, V = int(num_tokens), int(V)
    out = torch.ones(1, num_tokens, V, dtype=torch.bool)
    for col, codes in (columns or {}).items():
        col = int(col)
        if not 0 <= col < num_tokens:
            raise ValueError(f'code_sets: column {col} outside [0, {num_tokens})')
        codes = [int(c) for c in codes]
        if any(not 0 <= c < V for c in codes):
            raise ValueError(f'code_sets: column {col} names a code outside [0, {V})')
        out[0, col] = False
        out[0, col, codes] = True
    return out


def digit_sets(num_tokens, ncb, K, columns=None):
    """-> bool (1, num_tokens, ncb, K): column c allows, for codebook j, exactly the digits columns[c][j] (None: every digit);
    every other column every digit.  The allowed codes of the column are the Cartesian product of its ncb digit sets (digit j of
    a merged code is (code // K**j) % K).  ValueError on a column outside [0, num_tokens), a list that is not ncb long or a digit
    outside [0, K)."""
    num_tokens, ncb, K = int(num_tokens), int(ncb), int(K)
    out = torch.ones(1, num_tokens, ncb, K, dtype=torch.bool)
    for col, per_book in (columns or {}).items():
        col = int(col)
        if not 0 <= col < num_tokens:
            raise ValueError(f'digit_sets: column {col} outside [0, {num_tokens})')
        per_book = list(per_book)
        if len(per_book) != ncb:
            raise ValueError(f'digit_sets: column {col} gives {len(per_book)} digit sets for {ncb} codebooks')
        for j, digits in enumerate(per_book):
            if digits is None:
                continue
            digits = [int(c) for c in digits]
            if any(not 0 <= c < K for c in digits):
                raise ValueError(f'digit_sets: column {col}, codebook {j} names a digit outside [0, {K})')
            out[0, col, j] = False
            out[0, col, j, digits] = True
    return out


def check_sets(allowed, constraint=None):
    """allowed: bool (R, num_tokens, V) or (R, num_tokens, ncb, K), R = rows or 1; constraint: None or int64 (rows, num_tokens),
    >= 0 = a forced merged code.  ValueError naming the first (row, column[, codebook]) whose set is empty, or whose forced code
    (for a product set: any digit of it) is outside its own set.  One host synchronisation."""
    product = allowed.dim() == 4
    sets = allowed if product else allowed.unsqueeze(2)                              # (R, nt, J, K)
    R, nt, J, K = sets.shape
    empty = ~sets.any(-1)                                                            # (R, nt, J)
    if constraint is not None:
        rows = constraint.shape[0]
        forced = constraint.to(sets.device)
        code = forced.clamp(min=0, max=K ** J - 1)
        digits = torch.stack([(code // K ** j) % K for j in range(J)], dim=-1)       # (rows, nt, J)
        picked = sets.expand(rows, nt, J, K).gather(3, digits.unsqueeze(3)).squeeze(3)
        refused = (forced >= 0).unsqueeze(2) & ~picked
        empty = empty.expand(rows, nt, J)
    else:
        refused = torch.zeros_like(empty)
    bad = (empty | refused).reshape(-1)
    at = bad.to(torch.int32).argmax()
    found, at, was_empty = torch.stack([bad.any().long(), at.long(), empty.reshape(-1)[at].long()]).tolist()
    if not found:
        return
    b, rest = divmod(at, nt * J)
    col, j = divmod(rest, J)
    where = f'(row {b}, column {col}, codebook {j})' if product else f'(row {b}, column {col})'
    if was_empty:
        raise ValueError(f'allowed: {where} has no allowed code inside the vocabulary')
    raise ValueError(f'allowed: {where} is forced to code {int(constraint[b, col])}, which its allowed set forbids')


def pack_sets(allowed):
    """bool (..., V) -> int32 (..., ceil(V / 32)): bit i & 31 of word i >> 5 is entry i; the bits past V are 0."""
    V = allowed.shape[-1]
    words = (V + 31) // 32
    bits = torch.zeros(*allowed.shape[:-1], words * 32, dtype=torch.int32, device=allowed.device)
    bits[..., :V] = allowed
    weights = torch.tensor([1 << k for k in range(31)] + [-(1 << 31)], dtype=torch.int32, device=allowed.device)
    return (bits.view(*allowed.shape[:-1], words, 32) * weights).sum(-1, dtype=torch.int32)
