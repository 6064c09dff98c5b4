"""Cluster census: which blocks of the corpus each codeword stands for (csrc/clusters.hip; the "Cluster census" section of
include/vqcpc.h states the definitions).  In place of the "Explore clusters" tail of the reference's main_encoder.py:
`Encoder.plot_clusters` (VQCPCB/encoder.py:112-176, a Python double loop with `.item()` per block, dict-of-lists grouping,
random.shuffle and a cap of 50 examples per code, one codebook only) and `Encoder.show_nn_clusters` (:178-185).

THE POPULATION of a census is the one-block window set of a split: the windows of tokens_per_block / (4 * subdivision) beats of
`DeviceCorpus.table(...)` in the id range `split_bounds` gives the split -- the window set the 'random' negatives of the corpus CPC
generator are drawn from.  Every stored block of the split is counted exactly once; the virtual PAD-only blocks that the
reference's padded sequences drag in (it cuts padded windows of many blocks into blocks) are not counted.  This is the choice the
duplicate check made (dataloaders/corpus.py): only what the corpus stores takes part.

What differs from the reference: the whole split is visited (not `num_batches` batches of a shuffled loader); a code's examples are
the `examples` members with the smallest keyed hash of their position in the split (`select_hash`), so they are a pure function of
(encoder weights, corpus, split, examples, seed, chunk) instead of a random.shuffle; product codebooks are handled (per codebook,
plus the statistics of the merged code); and the result is data (`ClusterCensus`, one .npz and one text table), not one MusicXML
file per code, which needs music21.
"""
import numpy as np
import torch

from . import hip
from .dataloaders.corpus import NUM_VOICES, SPLITS, mix_key, split_bounds

_M64 = (1 << 64) - 1
MAX_EXAMPLES = 64                      # vqcpc_cluster_select: 1 <= E <= 64
MAX_CODES = 1 << 24                    # vqcpc_cluster_count: K <= 2^24 (the merged code is counted up to this size)
MAX_POPULATION = (1 << 32) - 1         # ids are < 2^32 - 1: no packed key is the empty slot value
EMPTY = _M64                           # an empty slot
CENSUS_STREAM = 0x636C7573             # the `stream` of mix_key for the example selection
MAX_NEIGHBOURS = 16                    # vqcpc_codebook_knn: 1 <= k <= 16


def select_hash(key, ids):
    """h(key, id) of include/vqcpc.h for an integer or an array of ids: the low 32 bits of the splitmix64 finaliser of
    key + id * 0x9E3779B97F4A7C15 (mod 2^64).  The host twin of the kernel's hash; uint64 array (or int) of values < 2^32."""
    scalar = np.ndim(ids) == 0
    with np.errstate(over='ignore'):
        z = np.uint64(int(key) & _M64) + np.atleast_1d(np.asarray(ids)).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = (z ^ (z >> np.uint64(31))) & np.uint64(0xFFFFFFFF)
    return int(z[0]) if scalar else z


def packed_keys(key, ids):
    """h(key, id) << 32 | id: what vqcpc_cluster_select orders the members of a code by (uint64 array)."""
    ids = np.atleast_1d(np.asarray(ids)).astype(np.uint64)
    return (select_hash(key, ids) << np.uint64(32)) | ids


def census_key(seed, split):
    return mix_key(seed, SPLITS.index(split), CENSUS_STREAM, 0)


def perplexity(counts):
    """exp of the entropy (nats) of counts / counts.sum() along the last axis, in float64; 0 log 0 = 0."""
    counts = np.asarray(counts, dtype=np.float64)
    p = counts / counts.sum(axis=-1, keepdims=True)
    logp = np.log(np.where(p > 0, p, 1.0))
    return np.exp(-(p * logp).sum(axis=-1))


# ---- the three entry points --------------------------------------------------------------------------------------------------------
def _codes2d(codes):
    assert codes.dtype == torch.int64 and codes.is_cuda and codes.dim() == 2 and codes.stride(1) == 1, 'codes: (n, ncb) int64 on the device'
    return codes


def count_codes(codes, K, counts, flag):
    """counts (ncb, K) int32 += the code counts of codes (n, ncb) int64 (rows may be strided); see vqcpc_cluster_count."""
    codes = _codes2d(codes)
    n, ncb = codes.shape
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == ncb * K and flag.dtype == torch.int32
    hip.call('vqcpc_cluster_count', codes, codes.stride(0) if n > 1 else ncb, n, ncb, int(K), counts, flag)
    return counts


def select_examples(codes, K, key, slots, flag, ids=None, id0=0):
    """slots (ncb, K, E) int64 holding uint64 bits, all ones = empty: the cascade of vqcpc_cluster_select over codes (n, ncb);
    row r has id ids[r] (int64 device tensor) or id0 + r."""
    codes = _codes2d(codes)
    n, ncb = codes.shape
    assert slots.dtype == torch.int64 and slots.is_contiguous() and slots.dim() == 3 and slots.shape[:2] == (ncb, K)
    if ids is not None:
        assert ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous() and ids.numel() == n
    hip.call('vqcpc_cluster_select', codes, codes.stride(0) if n > 1 else ncb, n, ncb, int(K), ids, int(id0), int(key) & _M64,
             int(slots.shape[2]), slots, flag)
    return slots


def codebook_knn(codebooks, k):
    """codebooks (ncb, K, d) float32 on the device -> (nn (ncb, K, k) int32, dist2 (ncb, K, k) float32): per codeword the k nearest
    OTHER codewords of its codebook by (squared distance, index); see vqcpc_codebook_knn."""
    e = codebooks.detach().to(torch.float32).contiguous()
    assert e.is_cuda and e.dim() == 3
    ncb, K, d = e.shape
    if not (1 <= k <= MAX_NEIGHBOURS and k < K):
        raise ValueError(f'codebook_knn: need 1 <= k <= {MAX_NEIGHBOURS} and k < codebook_size = {K}, got k = {k}')
    nn = torch.empty(ncb, K, k, dtype=torch.int32, device=e.device)
    dist2 = torch.empty(ncb, K, k, dtype=torch.float32, device=e.device)
    hip.call('vqcpc_codebook_knn', e, ncb, K, d, int(k), nn, dist2)
    return nn, dist2


# ---- the census --------------------------------------------------------------------------------------------------------------------
class ClusterCensus:
    """The result of `cluster_census`.  Host arrays only:

        split, num_blocks, beats_per_block, seed   the population: `num_blocks` one-block windows, ids first_id .. first_id + num_blocks - 1
        counts            (ncb, K) int64           blocks per (codebook, code); every row sums to num_blocks
        used, perplexity  (ncb,) int64 / float64   codes with a member; exp of the entropy of counts / num_blocks
        joint_used, joint_perplexity               the same of the merged code, or None when codebook_size ** num_codebooks > 2^24
        example_ids       (ncb, K, E) int64        window ids of a code's examples in selection order, -1 where the code has fewer
    """
    _SAVED = ('num_blocks', 'beats_per_block', 'first_id', 'seed', 'counts', 'example_ids')

    def __init__(self, split, num_blocks, beats_per_block, first_id, seed, counts, example_ids, joint_used=None,
                 joint_perplexity=None, device_corpus=None):
        self.split = str(split)
        self.num_blocks, self.beats_per_block, self.first_id, self.seed = int(num_blocks), int(beats_per_block), int(first_id), int(seed)
        self.counts = np.asarray(counts, dtype=np.int64)
        self.example_ids = np.asarray(example_ids, dtype=np.int64)
        self.used = (self.counts > 0).sum(axis=1).astype(np.int64)
        self.perplexity = perplexity(self.counts)
        self.joint_used = None if joint_used is None else int(joint_used)
        self.joint_perplexity = None if joint_perplexity is None else float(joint_perplexity)
        self.device_corpus = device_corpus

    @property
    def num_codebooks(self):
        return int(self.counts.shape[0])

    @property
    def codebook_size(self):
        return int(self.counts.shape[1])

    def examples(self, codebook, code):
        """(m, ticks_per_block, 4) int64 tokens of the m <= E examples of `code`, in selection order (a device gather)."""
        if self.device_corpus is None:
            raise ValueError('ClusterCensus.examples: no corpus attached (pass device_corpus= to ClusterCensus.load)')
        ids = self.example_ids[codebook, code]
        ids = ids[ids >= 0]
        dc = self.device_corpus
        out = torch.empty(len(ids), self.beats_per_block * dc.corpus.subdivision, NUM_VOICES, dtype=torch.int64, device=dc.device)
        if len(ids):
            dc.gather(torch.from_numpy(np.ascontiguousarray(ids)).to(dc.device), self.beats_per_block, out)
            dc.raise_if_bad_ids()
        return out.cpu().numpy()

    def save(self, path):
        arrays = {k: np.asarray(getattr(self, k)) for k in self._SAVED}
        arrays['split'] = np.asarray(self.split)
        arrays['joint_used'] = np.int64(-1 if self.joint_used is None else self.joint_used)
        arrays['joint_perplexity'] = np.float64(np.nan if self.joint_perplexity is None else self.joint_perplexity)
        with open(path, 'wb') as f:            # a file object: np.savez would append '.npz' to a bare path
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path, device_corpus=None):
        with np.load(path, allow_pickle=False) as z:
            joint = int(z['joint_used'])
            return cls(str(z['split']), *(z[k] for k in cls._SAVED), joint_used=None if joint < 0 else joint,
                       joint_perplexity=None if joint < 0 else float(z['joint_perplexity']), device_corpus=device_corpus)

    def _block_text(self, block, names):
        """One block (ticks, 4) as text: the voices separated by ' | ', note names where the corpus has them."""
        return ' | '.join(' '.join(str(names[v][int(t)]) if names else str(int(t)) for t in block[:, v]) for v in range(NUM_VOICES))

    def table(self, codebook=0, top=None, show=3):
        """A text listing of codebook `codebook`: the `top` most frequent codes (all used ones by default; ties by code), each
        with its count, its share of the split and its first `show` examples -- as note names where the corpus has `names`, as
        token ids otherwise or when no corpus is attached."""
        counts = self.counts[codebook]
        order = [int(k) for k in np.lexsort((np.arange(counts.size), -counts)) if counts[k] > 0][:top]
        names = None
        if self.device_corpus is not None and self.device_corpus.corpus.names is not None:
            names = self.device_corpus.corpus.index2note_dicts()
        lines = [f'codebook {codebook}: {self.num_blocks} blocks of the {self.split} split, {int(self.used[codebook])} of '
                 f'{counts.size} codes used, perplexity {self.perplexity[codebook]:.3f}']
        if self.joint_used is not None:
            lines.append(f'merged code: {self.joint_used} used, perplexity {self.joint_perplexity:.3f}')
        for k in order:
            lines.append(f'{k:6d}  count {int(counts[k]):8d}  share {counts[k] / self.num_blocks:8.5f}')
            if self.device_corpus is None:
                lines.extend(f'        window {int(i)}' for i in self.example_ids[codebook, k, :show] if i >= 0)
            else:
                ids = self.example_ids[codebook, k]
                for i, block in zip(ids[ids >= 0][:show], self.examples(codebook, k)[:show]):
                    lines.append(f'        window {int(i)}: {self._block_text(block, names)}')
        return '\n'.join(lines) + '\n'


def cluster_census(encoder, device_corpus, split='train', examples=50, seed=0, chunk=4096):
    """Encode every one-block window of `split` (module docstring: THE POPULATION) with `encoder` in eval mode and group the blocks
    by code on the device: counts per (codebook, code), codebook usage and perplexity, the statistics of the merged code while
    codebook_size ** num_codebooks <= 2^24, and `examples` (1 .. 64; the reference keeps 50) deterministic examples per code.
    Ids are visited in ascending order in chunks of `chunk` blocks (the encoder's launch plan depends on the row count, so codes
    are reproducible at equal chunk sizes); nothing returns to the host before the end.  A pure function of (encoder weights,
    corpus, split, examples, seed, chunk).  Returns a `ClusterCensus`."""
    q = encoder.quantizer
    if not hasattr(q, 'embeddings') or not hasattr(q, 'codebook_size'):
        raise ValueError(f'cluster_census: a {type(q).__name__} encoder has no codes to count')
    if split not in SPLITS:
        raise ValueError(f'{split} is not a valid split value. Choose between train, val or test')
    if not 1 <= int(examples) <= MAX_EXAMPLES:
        raise ValueError(f'cluster_census: examples must be in [1, {MAX_EXAMPLES}], got {examples}')
    if int(chunk) < 1:
        raise ValueError(f'cluster_census: chunk must be positive, got {chunk}')
    E, chunk = int(examples), int(chunk)
    dc = device_corpus
    tpb, per_beat = int(encoder.downscaler.sequence_length), dc.corpus.subdivision * NUM_VOICES
    if tpb % per_beat:
        raise ValueError(f'cluster_census: a block of {tpb} tokens is not a whole number of beats of {per_beat} tokens')
    bpb = tpb // per_beat
    lo, hi = split_bounds(dc.table(bpb)[1])[split]
    n = hi - lo
    if n < 1:
        raise ValueError(f'cluster_census: the {split} split of the one-block window set is empty')
    if n > MAX_POPULATION:
        raise ValueError(f'cluster_census: {n} blocks; the example selection packs a position into 32 bits (at most 2^32 - 1 blocks)')
    ncb, K = int(q.num_codebooks), int(q.codebook_size)
    joint = K ** ncb if K ** ncb <= MAX_CODES else None
    dev = dc.device
    counts = torch.zeros(ncb, K, dtype=torch.int32, device=dev)
    joint_counts = torch.zeros(1, joint, dtype=torch.int32, device=dev) if joint else None
    slots = torch.full((ncb, K, E), -1, dtype=torch.int64, device=dev)          # all ones: empty
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    key = census_key(seed, split)
    ticks = bpb * dc.corpus.subdivision
    was_training = encoder.training
    encoder.eval()
    try:
        for s in range(0, n, chunk):
            m = min(chunk, n - s)
            ids = torch.arange(lo + s, lo + s + m, dtype=torch.int64, device=dev)
            x = torch.empty(m, ticks, NUM_VOICES, dtype=torch.int64, device=dev)
            dc.gather(ids, bpb, x)
            codes = encoder.encode_indices(x).reshape(m, ncb)
            count_codes(codes, K, counts, flag)
            if joint:
                count_codes(encoder.merge_codes(codes).reshape(m, 1), joint, joint_counts, flag)
            select_examples(codes, K, key, slots, flag, id0=s)
    finally:
        encoder.train(was_training)
    # ---- the one return to the host ------------------------------------------------------------------------------------------
    if int(flag.item()):
        raise hip.VqcpcHipError('cluster_census: a code outside the codebook or a position past 2^32 - 2 was met')
    dc.raise_if_bad_ids()
    encoder.data_processor.raise_if_bad_tokens()
    counts = counts.cpu().numpy().astype(np.int64)
    keys = slots.cpu().numpy().view(np.uint64)
    example_ids = np.where(keys == np.uint64(EMPTY), np.int64(-1), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64) + lo)
    joint_used = joint_perp = None
    if joint:
        jc = joint_counts.cpu().numpy().astype(np.int64)
        joint_used, joint_perp = int((jc > 0).sum()), float(perplexity(jc)[0])
    return ClusterCensus(split, n, bpb, lo, seed, counts, example_ids, joint_used, joint_perp, device_corpus=dc)
