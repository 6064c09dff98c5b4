"""Training on a real tokenised corpus: the corpus file, its host container, and two dataloader generators whose batches are
sampled on the device from a corpus that stays in HBM (csrc/corpus.hip).  They take the place of the reference's
BachCPCDataloaderGenerator / BachDataloaderGenerator (VQCPCB/dataloaders/bach_cpc_dataloader.py, bach_dataloader.py over
datasets/chorale_dataset.py), which need music21 and materialise every window as a host TensorDataset.

THE FILE.  A corpus is a set of PIECES; one piece is one chorale in one transposition, already tokenised by the user's own music21
job.  One `.npz` that holds only data (`save_corpus` / `load_corpus`):

    tokens           int16 or int32 (total_ticks, 4)   tick-major, the pieces concatenated
    piece_start      int64 (P + 1,)                    tick offsets; every piece length is a positive multiple of `subdivision`
    subdivision      scalar                            ticks per beat (4)
    vocab            (4,)                              tokens per voice
    start, end, pad  (4,) each                         per-voice ids of START, END and PAD
    last_start_beat  int32 (P,), optional              the last start beat of a window over piece p (below)
    names            (4, max vocab) strings, optional  the note names per voice (`index2note_dicts`); '' past a voice's vocab

THE WINDOW RULE (chorale_dataset.py:124-129 and :418-470 without music21).  For a window of W beats over a piece of nb beats the
start beats are o = -(W - 1) .. last, ascending, last = nb - 1 unless `last_start_beat[p]` gives a smaller value.  A window covers
the ticks [4 o, 4 (o + W)) of the piece; per voice, ticks < 0 are PAD except tick -1, which is START; of the ticks >= the piece
length the first is END and the rest are PAD; a piece shorter than the window gets both paddings at once.  Window ids enumerate
piece-major, then o ascending.  Splits are by id order (:542-593): the first int(0.85 n) ids are train, the next int(0.10 n) are
val, the rest are test.

What is NOT the reference's:
  * the upper bound of o: the reference stops below music21's `highestOffset` (the offset of the piece's last note), which only
    the exporter knows; it may record it in `last_start_beat`, otherwise every beat of the piece starts a window;
  * the per-window transposition range (:135-139: a window exists in the transpositions that keep ITS notes inside the voice
    ranges) is not reproduced: which transpositions exist is decided by the exporter, one piece per (chorale, transposition),
    and every window of a piece exists;
  * the val split ends at int(0.85 n) + int(0.10 n), the reference's at int(0.95 n), which can be one id later;
  * val and test are drawn in a keyed order like train (the reference iterates them in id order); an epoch still visits distinct
    windows of the split only.

THE ORDER.  Row b of step s on rank r of R holds epoch position q = (s R + r) B + b of a keyed bijection of the split
(vqcpc_corpus_permute; key = mix(seed, split, stream, epoch)), so a batch is a pure function of (corpus, seed, split, epoch, s,
r, R, B, b): nothing is drawn on the host, no permutation is materialised, nothing crosses PCIe per step and the host never
waits for the device.  Epochs are finite as in the reference (drop_last=True, zip of the loaders); every call of `dataloaders()`
starts the next epoch.

THE IDS.  The window ids behind the last batch are `loader.last_ids` / `generator.last_ids` (CPC: a dict 'positive', 'negative',
'negative_back'; the 'x' loaders: one tensor).  They are NOT a key of the batch dict: the trainers' step graph (graphs.py) bakes
every batch entry into its signature and copies every tensor entry per replay, so an unknown key is not free there.

THE DUPLICATE CHECK (`DeviceCorpus.longest_common_run`, csrc/duplicates.hip): how much of a generation is copied from the corpus, in
place of the difflib loop over every training window of decoder.py:983-1017.  Tokens are compared voice by voice in the flattened
order (tick-major, voice-minor): query position i = 4 tick + voice faces corpus position j = 4 tick' + voice of the SAME voice.  A
run is a maximal stretch of consecutive equal tokens; it may begin and end in the middle of a tick and never crosses a piece
boundary.  Only stored corpus ticks take part: the virtual PAD / START / END ticks of the window rule never match, so padding in a
generation is never counted as copied (the reference compares with the padded windows and counts it).  The answer per query row
is the longest run; among equals the smallest i; among those the smallest j (the earliest piece, then the earliest tick) -- what
`difflib.SequenceMatcher(None, a, b, autojunk=False).find_longest_match` returns per piece on lists of (voice, token) pairs,
combined by (longest, smallest a, earliest piece).  The reference matches the CHARACTERS of the dumped note names instead, so its
count depends on the names' lengths and a match may end inside a name; lengths here are tokens.

THE COPY GUARD (`DeviceCorpus.copy_index`, csrc/nocopy.hip; `Decoder.generate_from_codes(no_copy=...)`): the same run, prevented
instead of measured.  The index holds every corpus token position whose `max_copy` tokens before it lie in its own piece, keyed by
a hash of (voice, those tokens) with the position's token in the low 8 bits, sorted; the step looks the generation's last
`max_copy` tokens up and bans the tokens found, so that no run of `max_copy + 1` shared tokens can be completed.
"""
import numpy as np
import torch

from .. import hip

NUM_VOICES = 4
SPLITS = ('train', 'val', 'test')
_M64 = (1 << 64) - 1


# ---- the file ------------------------------------------------------------------------------------------------------------
class Corpus:
    """Validated host arrays of one corpus file (see the module docstring)."""

    def __init__(self, tokens, piece_start, subdivision, vocab, start, end, pad, last_start_beat=None, names=None):
        tokens = np.asarray(tokens)
        if tokens.ndim != 2 or tokens.shape[1] != NUM_VOICES:
            raise ValueError(f'corpus: tokens must be (total_ticks, {NUM_VOICES}), got {tokens.shape}: the voice count is not 4')
        if tokens.dtype not in (np.int16, np.int32):
            raise ValueError(f'corpus: tokens must be int16 or int32, got {tokens.dtype}')
        self.tokens = tokens
        self.piece_start = np.asarray(piece_start).astype(np.int64).reshape(-1)
        self.subdivision = int(np.asarray(subdivision).reshape(()))
        self.vocab, self.start, self.end, self.pad = (np.asarray(a).astype(np.int64).reshape(-1) for a in (vocab, start, end, pad))
        for name, a in (('vocab', self.vocab), ('start', self.start), ('end', self.end), ('pad', self.pad)):
            if a.shape != (NUM_VOICES,):
                raise ValueError(f'corpus: `{name}` must have {NUM_VOICES} entries, got {a.shape}: the voice count is not 4')
        if self.subdivision < 1:
            raise ValueError(f'corpus: subdivision must be positive, got {self.subdivision}')
        ps = self.piece_start
        if ps.size < 2 or ps[0] != 0 or ps[-1] != tokens.shape[0]:
            raise ValueError('corpus: piece_start must run from 0 to total_ticks over at least one piece')
        length = np.diff(ps)
        if (length <= 0).any():
            raise ValueError(f'corpus: piece_start is not monotone (piece {int(np.argmax(length <= 0))} has length '
                             f'{int(length[np.argmax(length <= 0)])})')
        if (length % self.subdivision != 0).any():
            p = int(np.argmax(length % self.subdivision != 0))
            raise ValueError(f'corpus: the length of piece {p} ({int(length[p])} ticks) is not a multiple of the subdivision '
                             f'{self.subdivision}')
        if (self.vocab < 1).any() or (self.vocab > np.iinfo(np.int32).max).any():
            raise ValueError(f'corpus: vocab {self.vocab.tolist()} out of range')
        if (tokens < 0).any():
            raise ValueError('corpus: negative token')
        too_big = tokens >= self.vocab[None, :]
        if too_big.any():
            t, v = (int(i[0]) for i in np.nonzero(too_big))
            raise ValueError(f'corpus: token {int(tokens[t, v])} of voice {v} at tick {t} is >= the vocab {int(self.vocab[v])}')
        for name, a in (('start', self.start), ('end', self.end), ('pad', self.pad)):
            if (a < 0).any() or (a >= self.vocab).any():
                raise ValueError(f'corpus: `{name}` ids {a.tolist()} are not tokens of the vocab {self.vocab.tolist()}')
        self.num_beats = length // self.subdivision
        if last_start_beat is None:
            self.last_start_beat = None
        else:
            last = np.asarray(last_start_beat).astype(np.int64).reshape(-1)
            if last.shape != self.num_beats.shape or (last < 0).any() or (last >= self.num_beats).any():
                raise ValueError('corpus: last_start_beat needs one entry per piece, each in [0, beats of the piece)')
            self.last_start_beat = last
        if names is not None:
            names = np.asarray(names).astype(str)
            if names.ndim != 2 or names.shape[0] != NUM_VOICES or names.shape[1] < int(self.vocab.max()):
                raise ValueError('corpus: names must be (4, >= max vocab) strings')
        self.names = names

    @property
    def num_pieces(self):
        return int(self.num_beats.size)

    def last(self):
        return self.num_beats - 1 if self.last_start_beat is None else self.last_start_beat

    def window_counts(self, num_beats):
        """Windows of `num_beats` beats per piece: the start beats -(W - 1) .. last."""
        assert num_beats >= 1
        return self.last() + int(num_beats)

    def window_at(self, piece, start_tick, ticks):
        """int64 (ticks, 4): the ticks [start_tick, start_tick + ticks) of `piece` under the padding of the window rule (tick -1
        START, the first tick past the piece END, every other tick outside PAD); any start tick, not only a beat."""
        lo, hi = int(self.piece_start[piece]), int(self.piece_start[piece + 1])
        rel = np.arange(int(start_tick), int(start_tick) + int(ticks))
        out = np.repeat(self.pad[None, :], len(rel), axis=0)
        out[rel == -1] = self.start
        out[rel == hi - lo] = self.end
        inside = (rel >= 0) & (rel < hi - lo)
        out[inside] = self.tokens[lo + rel[inside]]
        return out

    def index2note_dicts(self):
        if self.names is None:
            return [{i: i for i in range(int(v))} for v in self.vocab]
        return [{i: str(self.names[c, i]) for i in range(int(v))} for c, v in enumerate(self.vocab)]


def save_corpus(path, pieces, vocab, start, end, pad, subdivision=4, last_start_beat=None, names=None, dtype=np.int16):
    """pieces: a list of (ticks_p, 4) integer arrays.  names: per voice, the list of its note names (index -> name)."""
    pieces = [np.asarray(p) for p in pieces]
    if not pieces:
        raise ValueError('corpus: no piece')
    for p in pieces:
        if p.ndim != 2 or p.shape[1] != NUM_VOICES:
            raise ValueError(f'corpus: a piece must be (ticks, {NUM_VOICES}), got {p.shape}: the voice count is not 4')
    tokens = np.concatenate(pieces, axis=0)
    if tokens.size and (tokens.min() < np.iinfo(dtype).min or tokens.max() > np.iinfo(dtype).max):
        raise ValueError(f'corpus: tokens do not fit {np.dtype(dtype).name}')
    arrays = dict(tokens=tokens.astype(dtype),
                  piece_start=np.concatenate([[0], np.cumsum([p.shape[0] for p in pieces])]).astype(np.int64),
                  subdivision=np.int64(subdivision), vocab=np.asarray(vocab, dtype=np.int64), start=np.asarray(start, dtype=np.int64),
                  end=np.asarray(end, dtype=np.int64), pad=np.asarray(pad, dtype=np.int64))
    if last_start_beat is not None:
        arrays['last_start_beat'] = np.asarray(last_start_beat, dtype=np.int32)
    if names is not None:
        width = max(len(n) for n in names)
        arrays['names'] = np.array([list(map(str, n)) + [''] * (width - len(n)) for n in names])
    Corpus(**arrays)                       # never write a file load_corpus would refuse
    with open(path, 'wb') as f:            # a file object: np.savez would append '.npz' to a bare path
        np.savez(f, **arrays)


def load_corpus(path):
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ('tokens', 'piece_start', 'subdivision', 'vocab', 'start', 'end', 'pad') if k not in z.files]
        if missing:
            raise ValueError(f'corpus {path}: missing arrays {missing}')
        return Corpus(z['tokens'], z['piece_start'], z['subdivision'], z['vocab'], z['start'], z['end'], z['pad'],
                      z['last_start_beat'] if 'last_start_beat' in z.files else None, z['names'] if 'names' in z.files else None)


def split_bounds(n):
    """{'train': (lo, hi), 'val': ..., 'test': ...} of n window ids (chorale_dataset.py:561-567, split = (0.85, 0.10))."""
    a = int(0.85 * n)
    b = a + int(0.10 * n)
    return {'train': (0, a), 'val': (a, b), 'test': (b, n)}


def mix_key(seed, split, stream, epoch):
    """The 64-bit key of one (seed, split, stream, epoch) order: a splitmix64 chain over the four integers."""
    z = 0x243F6A8885A308D3
    for v in (seed, split, stream, epoch):
        z = (z ^ (int(v) & _M64)) & _M64
        z = (z + 0x9E3779B97F4A7C15) & _M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        z ^= z >> 31
    return z


# ---- the duplicate check: framing arithmetic (include/vqcpc.h, "Duplicate check") -----------------------------------------------
DUP_SENTINEL = 0xFFFF                  # the 16-bit voice value of a sentinel tick: every token of a query or a corpus is below it
DUP_MAX_TICKS = 65535 // NUM_VOICES    # a query position must fit 16 bits of the key


def pack_words(x):
    """(..., 4) tokens -> (...) uint64 words, voice v in bits 16 v .. 16 v + 15 (the host twin of vqcpc_dup_pack)."""
    x = np.asarray(x).astype(np.uint64)
    return x[..., 0] | (x[..., 1] << np.uint64(16)) | (x[..., 2] << np.uint64(32)) | (x[..., 3] << np.uint64(48))


def framed_start(piece_start):
    """(P + 1,) framed tick of the sentinel in front of piece p (p = P: the one after the last piece); piece p's first tick is
    the next one.  n_framed = framed_start[P] + 1."""
    piece_start = np.asarray(piece_start, dtype=np.int64)
    return piece_start + np.arange(piece_start.size, dtype=np.int64)


def frame_words(tokens, piece_start):
    """The framed, packed corpus as vqcpc_dup_frame builds it: (total_ticks + P + 1,) uint64."""
    fs = framed_start(piece_start)
    out = np.full(int(fs[-1]) + 1, np.iinfo(np.uint64).max, dtype=np.uint64)
    words = pack_words(tokens)
    for p in range(len(fs) - 1):
        out[fs[p] + 1:fs[p + 1]] = words[piece_start[p]:piece_start[p + 1]]
    return out


def framed_range(piece_start, lo, hi):
    """(first framed tick, framed ticks) of the pieces [lo, hi): a sub-array that starts and ends on a sentinel."""
    fs = framed_start(piece_start)
    if not 0 <= lo < hi <= len(fs) - 1:
        raise ValueError(f'corpus: pieces=({lo}, {hi}) is not a non-empty range of the {len(fs) - 1} pieces')
    return int(fs[lo]), int(fs[hi] - fs[lo]) + 1


def unpack_key(key):
    """A key of vqcpc_dup_longest_run -> (length in tokens, query position i, framed position j); (0, -1, -1) for key 0."""
    key = int(key)
    if key == 0:
        return 0, -1, -1
    return key >> 48, 0xFFFF - ((key >> 32) & 0xFFFF), 0xFFFFFFFF - (key & 0xFFFFFFFF)


def unframe(j, piece_start, first=0):
    """Token position j inside the framed sub-array that begins at framed tick `first` -> (piece, tick of the piece, voice)."""
    fs = framed_start(piece_start)
    f, voice = first + j // NUM_VOICES, j % NUM_VOICES
    piece = int(np.searchsorted(fs, f, side='right')) - 1
    tick = f - int(fs[piece]) - 1
    assert 0 <= piece < len(fs) - 1 and 0 <= tick < piece_start[piece + 1] - piece_start[piece], 'a match on a sentinel tick'
    return piece, int(tick), int(voice)


# ---- the copy guard's index (include/vqcpc.h, "Copy guard") ------------------------------------------------------------------------
COPY_MAX_N = 512                       # max_copy: a lane of the guard kernel keeps 8 history tokens
COPY_MAX_VOCAB = 256                   # the next token takes the low 8 bits of a key
COPY_RELAXED, COPY_FORCED = 1 << 16, 1 << 17           # the flags of copy_report; bits 0-8 count the removed tokens


class CopyIndex:
    """What `DeviceCorpus.copy_index` built, device resident: sorted `keys` (int64), `where` (int64, the entries' token positions
    inside the framed sub-array), `framed` (the sub-array itself, a view of the duplicate check's), `max_copy`, `pieces` = (lo, hi),
    `vocab` (per voice) and `entries_before`, the number of entries before the duplicate removal."""

    def __init__(self, keys, where, framed, max_copy, pieces, vocab, entries_before):
        self.keys, self.where, self.framed = keys, where, framed
        self.max_copy, self.pieces, self.vocab, self.entries_before = int(max_copy), tuple(pieces), tuple(vocab), int(entries_before)

    @property
    def device(self):
        return self.framed.device

    @property
    def entries(self):
        return int(self.keys.numel())

    @property
    def n_framed(self):
        return int(self.framed.numel())

    def nbytes(self):
        """Bytes of keys + where (the framed corpus is the duplicate check's and is shared)."""
        return self.keys.numel() * 8 + self.where.numel() * 8

    def args(self):
        """The index operands of vqcpc_decode_nocopy / vqcpc_nocopy_audit, in order."""
        e = self.entries
        return (self.keys if e else None, self.where if e else None, e, self.framed, self.n_framed, self.max_copy)


# ---- the corpus on the device ---------------------------------------------------------------------------------------------
def permute(ids, lo, n, key, q0):
    """ids[i] = lo + pi_key((q0 + i) mod n) for the whole int64 device tensor `ids`."""
    assert ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous()
    hip.call('vqcpc_corpus_permute', ids, int(lo), int(n), int(key) & _M64, int(q0), ids.numel())
    return ids


class DeviceCorpus:
    """The corpus in device memory: tokens as (total_ticks, 4) int32, the piece offsets, the START / END / PAD rows, one
    cumulative window-count table per window length in use, and the out-of-range flag of vqcpc_corpus_gather."""

    def __init__(self, corpus, device):
        self.corpus = corpus
        self.device = torch.device(device)
        assert self.device.type == 'cuda', 'the corpus sampler runs on the device: there is no host path'
        hip.load()
        self.tokens = torch.from_numpy(np.ascontiguousarray(corpus.tokens.astype(np.int32))).to(self.device)
        self.piece_start = torch.from_numpy(corpus.piece_start).to(self.device)
        special = np.concatenate([corpus.start, corpus.end, corpus.pad]).astype(np.int32)
        self.special = torch.from_numpy(special).to(self.device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._tables = {}
        self._framed = None

    def framed(self):
        """The framed, packed copy of the corpus for the duplicate check (vqcpc_dup_frame), built on first use."""
        if self._framed is None:
            c = self.corpus
            if int(c.vocab.max()) > DUP_SENTINEL:
                raise ValueError(f'corpus: the duplicate check packs a token into 16 bits below the sentinel {DUP_SENTINEL:#x}; '
                                 f'the vocab {c.vocab.tolist()} does not fit')
            total = int(c.piece_start[-1])
            framed = torch.empty(total + c.num_pieces + 1, dtype=torch.int64, device=self.device)
            hip.call('vqcpc_dup_frame', self.tokens, self.piece_start, c.num_pieces, total, framed)
            self._framed = framed
        return self._framed

    def split_pieces(self, split, num_beats):
        """(lo, hi): the pieces of `split` for windows of `num_beats` beats.  A piece belongs to the split that holds its first
        window id, so the ranges of the three splits are contiguous and partition the pieces; a range may be empty."""
        cum = np.concatenate([[0], np.cumsum(self.corpus.window_counts(num_beats))]).astype(np.int64)
        lo, hi = split_bounds(int(cum[-1]))[split]
        first = cum[:-1]
        return int(np.searchsorted(first, lo, side='left')), int(np.searchsorted(first, hi, side='left'))

    def longest_common_run(self, x, pieces=None):
        """The longest common run (module docstring) of every row of x, int64 tokens (G, ticks, 4) or (ticks, 4) on the device or
        the host, against the pieces [lo, hi) = `pieces` (default: all).  Returns a dict of host values, (G,) int64 arrays or, for
        a (ticks, 4) query, ints: `length` in tokens, where the run starts in the query (`query_tick`, `query_voice`) and in
        the corpus (`piece`, `piece_tick`, `voice`; voice == query_voice).  No common token: length 0 and -1 everywhere."""
        x = torch.as_tensor(x)
        single = x.dim() == 2
        if single:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[2] != NUM_VOICES or x.dtype != torch.int64:
            raise ValueError(f'longest_common_run: int64 tokens (G, ticks, {NUM_VOICES}) or (ticks, {NUM_VOICES}) expected, got '
                             f'{x.dtype} {tuple(x.shape)}')
        G, ticks = int(x.shape[0]), int(x.shape[1])
        if G < 1 or not 1 <= ticks <= DUP_MAX_TICKS:
            raise ValueError(f'longest_common_run: at least one row of 1 .. {DUP_MAX_TICKS} ticks expected, got {tuple(x.shape)}')
        x = x.to(self.device).contiguous()
        lo_tok, hi_tok = torch.stack([x.amin(dim=(0, 1)), x.amax(dim=(0, 1))]).cpu().numpy()       # one copy, one wait
        if (lo_tok < 0).any() or (hi_tok >= self.corpus.vocab).any():
            raise ValueError(f'longest_common_run: tokens in [{lo_tok.tolist()}, {hi_tok.tolist()}] per voice are not all tokens of '
                             f'the vocab {self.corpus.vocab.tolist()}')
        ps = self.corpus.piece_start
        first, n_framed = framed_range(ps, *((0, self.corpus.num_pieces) if pieces is None else map(int, pieces)))
        framed = self.framed()[first:first + n_framed]
        query = torch.empty(G, ticks, dtype=torch.int64, device=self.device)
        keys = torch.zeros(G, dtype=torch.int64, device=self.device)
        hip.call('vqcpc_dup_pack', x, x.stride(0), x.stride(1), ticks, G, query, ticks)
        hip.call('vqcpc_dup_longest_run', framed, n_framed, query, ticks, ticks, G, keys)
        names = ('length', 'query_tick', 'query_voice', 'piece', 'piece_tick', 'voice')
        out = {k: np.full(G, -1, dtype=np.int64) for k in names}
        for g, key in enumerate(keys.cpu().numpy().view(np.uint64).tolist()):
            length, i, j = unpack_key(key)
            out['length'][g] = length
            if length:
                out['query_tick'][g], out['query_voice'][g] = divmod(i, NUM_VOICES)
                out['piece'][g], out['piece_tick'][g], out['voice'][g] = unframe(j, ps, first)
        return {k: int(v[0]) for k, v in out.items()} if single else out

    def copy_index(self, max_copy, pieces=None, deduplicate=True):
        """The copy guard's index (module docstring of csrc/nocopy.hip; include/vqcpc.h, "Copy guard") over the pieces [lo, hi) =
        `pieces` (default: all), built once on the device: every corpus token position whose `max_copy` tokens before it lie in
        its own piece, keyed by hash(voice, those tokens) << 8 | its token, sorted (torch.sort), and -- deduplicate -- without the
        entries that repeat their predecessor's (voice, context, token).  ValueError: max_copy outside [1, 512], a vocab above 256,
        the duplicate check's framed limits."""
        c = self.corpus
        max_copy = int(max_copy)
        if not 1 <= max_copy <= COPY_MAX_N:
            raise ValueError(f'copy_index: 1 <= max_copy <= {COPY_MAX_N} expected, got {max_copy}')
        if int(c.vocab.max()) > COPY_MAX_VOCAB:
            raise ValueError(f'copy_index: a key keeps the next token in 8 bits; the vocab {c.vocab.tolist()} does not fit '
                             f'{COPY_MAX_VOCAB}')
        pieces = (0, c.num_pieces) if pieces is None else tuple(int(p) for p in pieces)
        first, n_framed = framed_range(c.piece_start, *pieces)
        if int(c.piece_start[-1]) + c.num_pieces + 1 >= 1 << 30:
            raise ValueError('copy_index: the framed corpus must stay below 2^30 ticks')
        framed = self.framed()[first:first + n_framed]
        keys = torch.empty(NUM_VOICES * n_framed, dtype=torch.int64, device=self.device)
        hip.call('vqcpc_copy_index_keys', framed, n_framed, max_copy, keys)
        where = torch.nonzero(keys >= 0).reshape(-1)
        keys, order = torch.sort(keys[where])
        where = where[order]
        entries = int(keys.numel())
        if deduplicate and entries:
            keep = torch.empty(entries, dtype=torch.bool, device=self.device)
            hip.call('vqcpc_copy_index_unique', framed, n_framed, max_copy, keys, where, entries, keep)
            keys, where = keys[keep].contiguous(), where[keep].contiguous()
        return CopyIndex(keys, where, framed, max_copy, pieces, tuple(int(v) for v in c.vocab), entries)

    def table(self, num_beats):
        """(win_cum on the device, number of windows) of the window set of `num_beats` beats."""
        t = self._tables.get(num_beats)
        if t is None:
            cum = np.concatenate([[0], np.cumsum(self.corpus.window_counts(num_beats))]).astype(np.int64)
            t = self._tables[num_beats] = (torch.from_numpy(cum).to(self.device), int(cum[-1]))
        return t

    def gather(self, ids, num_beats, out, out2=None):
        """Windows `ids` (any shape, int64, device) of `num_beats` beats -> out (..., ticks, 4) int64, or the first
        out.shape[-2] ticks to `out` and the rest to `out2`.  The leading dimensions of an output, flattened, are the ids; only
        the last dimension has to be dense."""
        c = self.corpus
        ticks = num_beats * c.subdivision
        ids = ids.reshape(-1)
        assert ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous()
        rows = []
        for o in (out, out2):
            if o is None:
                rows.append((None, 0, 0, 0))
                continue
            assert o.dtype == torch.int64 and o.is_cuda and o.shape[-1] == NUM_VOICES and o.stride(-1) == 1
            o3 = o if o.dim() == 3 else o.view(-1, o.shape[-2], NUM_VOICES)      # view: raises unless the rows are evenly strided
            assert o3.shape[0] == ids.numel(), (tuple(o.shape), ids.numel())
            rows.append((o3, o3.stride(0) if o3.shape[0] > 1 else 0, o3.stride(1) if o3.shape[1] > 1 else NUM_VOICES, o3.shape[1]))
        (o1, ld1, lt1, t1), (o2, ld2, lt2, t2) = rows
        assert t1 + t2 == ticks, (t1, t2, ticks)
        win_cum, _ = self.table(num_beats)
        hip.call('vqcpc_corpus_gather', self.tokens, self.piece_start, win_cum, self.special, c.num_pieces, int(num_beats),
                 c.subdivision, ids, ids.numel(), o1, ld1, lt1, t1, o2, ld2, lt2, self.flag)
        return out

    def raise_if_bad_ids(self):
        """The lazy check of the gather kernel's flag (one host synchronisation: the loaders call it when an epoch ends)."""
        if int(self.flag.item()):
            self.flag.zero_()
            raise hip.VqcpcHipError('corpus: a window id outside the corpus was requested (nothing was written for it)')


# ---- the generators --------------------------------------------------------------------------------------------------------
class _Dataset:
    """What getters.get_data_processor reads of a ChoraleBeatsDataset."""

    def __init__(self, corpus, sequences_size):
        self.index2note_dicts = corpus.index2note_dicts()
        self.sequences_size = sequences_size
        self.subdivision = corpus.subdivision


class _Loader:
    """One finite epoch of one split; `draw(step)` -> (batch dict, ids).  The split is checked when the iteration starts, so a
    split nobody iterates (test, during training) may be too small for a step."""

    def __init__(self, owner, split, steps, need, draw):
        self.owner, self.split, self.steps, self.need, self.draw = owner, split, steps, need, draw
        self.step = 0
        self.last_ids = None

    def __len__(self):
        return self.steps

    def __iter__(self):
        return self

    def __next__(self):
        if self.steps < 1:
            raise ValueError(f'corpus: the {self.split} split cannot fill one step ({self.need})')
        if self.step >= self.steps:
            self.owner.device_corpus.raise_if_bad_ids()
            raise StopIteration
        batch, ids = self.draw(self.step)
        self.step += 1
        self.last_ids = self.owner.last_ids = ids
        return batch


class _CorpusGenerator:
    def _open(self, corpus_path, seed, device, rank, world_size):
        self.corpus = corpus_path if isinstance(corpus_path, Corpus) else load_corpus(corpus_path)
        assert 0 <= rank < world_size
        self.seed, self.rank, self.world_size = int(seed), int(rank), int(world_size)
        self.device = torch.device('cuda' if device is None else device)
        self.device_corpus = DeviceCorpus(self.corpus, self.device)
        self.num_channels = NUM_VOICES
        self.epoch = 0                         # the epoch the NEXT dataloaders() call starts
        self.last_ids = None

    def _ids(self, count, stream, split, epoch, step, num_beats):
        """`count` ids per rank and step of stream `stream`: epoch positions (step R + rank) count .. + count - 1."""
        lo, hi = split_bounds(self.device_corpus.table(num_beats)[1])[split]
        ids = torch.empty(count, dtype=torch.int64, device=self.device)
        return permute(ids, lo, hi - lo, mix_key(self.seed, SPLITS.index(split), stream, epoch),
                       (step * self.world_size + self.rank) * count)

    def _split_size(self, split, num_beats):
        lo, hi = split_bounds(self.device_corpus.table(num_beats)[1])[split]
        return hi - lo


class CorpusCPCDataloaderGenerator(_CorpusGenerator):
    """The batch-dict contract of BachCPCDataloaderGenerator (bach_cpc_dataloader.py:183-259) from a corpus file:

        x_left (B, Kl * ticks_per_block, 4)   x_right (B, Kr * ticks_per_block, 4)
        negative_samples / negative_samples_back (B, N, Kr, ticks_per_block, 4)                    int64 tokens on `device`

    'random' negatives (:63-88, 204-215): a second window set of one-block windows over the same pieces with its own 85/10/5 split;
    two independent without-replacement streams (forward, back) take B N Kr ids per step each.  'same_sequence' (:110-181): the
    other blocks of the same window (ops.same_sequence_negatives), N = Kl + Kr - 1.  An epoch has
    min(n_pos // (B R), n_neg // (B N Kr R)) steps (the first term only for same-sequence negatives)."""

    def __init__(self, corpus_path, num_tokens_per_block=16, num_blocks_left=8, num_blocks_right=8, negative_sampling_method='random',
                 num_negative_samples=15, seed=1234, device=None, rank=0, world_size=1, **_):
        self._open(corpus_path, seed, device, rank, world_size)
        per_beat = self.corpus.subdivision * NUM_VOICES
        assert num_tokens_per_block % per_beat == 0, 'a block is a whole number of beats'      # bach_cpc_dataloader.py:28
        if negative_sampling_method not in ('random', 'same_sequence'):
            raise NotImplementedError(negative_sampling_method)
        self.num_tokens_per_block = num_tokens_per_block
        self.num_blocks_left, self.num_blocks_right = num_blocks_left, num_blocks_right
        self.negative_sampling_method = negative_sampling_method
        if negative_sampling_method == 'same_sequence':
            num_negative_samples = num_blocks_left + num_blocks_right - 1
        self.num_negative_samples = num_negative_samples
        self.vocab = [int(v) for v in self.corpus.vocab]
        self.beats_per_block = num_tokens_per_block // per_beat
        self.beats_positive = self.beats_per_block * (num_blocks_left + num_blocks_right)
        self.dataset_positive = _Dataset(self.corpus, self.beats_positive)
        self.dataset_negative = _Dataset(self.corpus, self.beats_per_block) if negative_sampling_method == 'random' else None
        self.dataset = self.dataset_positive

    def _loader(self, batch_size, split, epoch):
        from .. import ops
        B, N, Kl, Kr, R = batch_size, self.num_negative_samples, self.num_blocks_left, self.num_blocks_right, self.world_size
        tpb = self.beats_per_block * self.corpus.subdivision
        random = self.negative_sampling_method == 'random'
        steps = self._split_size(split, self.beats_positive) // (B * R)
        need = f'{B * R} positive windows of {self._split_size(split, self.beats_positive)}'
        if random:
            steps = min(steps, self._split_size(split, self.beats_per_block) // (B * N * Kr * R))
            need += f', {B * N * Kr * R} negative blocks of {self._split_size(split, self.beats_per_block)}'
        dc, dev = self.device_corpus, self.device

        def draw(step):
            ids = {'positive': self._ids(B, 0, split, epoch, step, self.beats_positive)}
            out = {'x_left': torch.empty(B, Kl * tpb, NUM_VOICES, dtype=torch.int64, device=dev),
                   'x_right': torch.empty(B, Kr * tpb, NUM_VOICES, dtype=torch.int64, device=dev)}
            dc.gather(ids['positive'], self.beats_positive, out['x_left'], out['x_right'])
            if random:
                for stream, (tag, key) in enumerate((('negative', 'negative_samples'), ('negative_back', 'negative_samples_back')), 1):
                    ids[tag] = self._ids(B * N * Kr, stream, split, epoch, step, self.beats_per_block).view(B, N, Kr)
                    out[key] = torch.empty(B, N, Kr, tpb, NUM_VOICES, dtype=torch.int64, device=dev)
                    dc.gather(ids[tag], self.beats_per_block, out[key])
            else:
                out['negative_samples'] = ops.same_sequence_negatives(out['x_left'], out['x_right'], tpb)
                if Kl == Kr:       # the reference's backward direction needs equal block counts (:132)
                    out['negative_samples_back'] = ops.same_sequence_negatives(out['x_right'], out['x_left'], tpb)
            return out, ids

        return _Loader(self, split, steps, need, draw)

    def dataloaders(self, batch_size, num_workers=0, **_):
        """(train, val, test) loaders of the next epoch."""
        epoch, self.epoch = self.epoch, self.epoch + 1
        return tuple(self._loader(batch_size, split, epoch) for split in SPLITS)


class CorpusDataloaderGenerator(_CorpusGenerator):
    """For the student, decoder and prior trainers (bach_dataloader.py): {'x': (B, sequences_size * subdivision, 4)}."""

    def __init__(self, corpus_path, sequences_size=24, subdivision=4, seed=1234, device=None, rank=0, world_size=1, **_):
        self._open(corpus_path, seed, device, rank, world_size)
        assert subdivision == self.corpus.subdivision, (subdivision, self.corpus.subdivision)
        self.vocab = [int(v) for v in self.corpus.vocab]
        self.sequences_size, self.subdivision = sequences_size, subdivision
        self.dataset = _Dataset(self.corpus, sequences_size)
        self.num_events = sequences_size * subdivision

    def _loader(self, batch_size, split, epoch):
        B = batch_size
        n = self._split_size(split, self.sequences_size)

        def draw(step):
            ids = self._ids(B, 0, split, epoch, step, self.sequences_size)
            x = torch.empty(B, self.num_events, NUM_VOICES, dtype=torch.int64, device=self.device)
            return {'x': self.device_corpus.gather(ids, self.sequences_size, x)}, ids

        return _Loader(self, split, n // (B * self.world_size), f'{B * self.world_size} windows of {n}', draw)

    def dataloaders(self, batch_size, num_workers=0, **_):
        epoch, self.epoch = self.epoch, self.epoch + 1
        return tuple(self._loader(batch_size, split, epoch) for split in SPLITS)
