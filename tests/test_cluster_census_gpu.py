"""The cluster census through its public surface (vqcpc_bach_amd/clusters.py, Encoder.plot_clusters / show_nn_clusters): a tiny
encoder on a random corpus whose pieces are 1, 2, 13 and 40 beats long, one of them with a `last_start_beat`.  Counts are compared
with the bincount of `encode_indices` over THE SAME CHUNKS (the encoder's launch plan depends on the row count, so codes are only
promised at equal shapes: nothing here compares across chunk sizes).  Exact integer equality."""
import numpy as np
import pytest
import torch

import clusters_reference as R
import corpus_reference as CR

pytestmark = pytest.mark.gpu

VOCAB = (30, 30, 30, 30)
BEATS = (1, 2, 13, 40) * 3
LAST = tuple(b - 1 for b in BEATS[:7]) + (31,) + tuple(b - 1 for b in BEATS[8:])      # piece 7 (40 beats) stops at start beat 31
K = 32
CHUNK = 48                             # 136 train blocks: 48 + 48 + 40
E = 3


def _pieces():
    return CR.seeded_pieces(BEATS, VOCAB, seed=33)


def _encoder(ncb, dc):
    """A seeded tiny encoder whose codebooks are the latents of K spread-out blocks, so that many codes are in use."""
    from oracle import vqcpc_oracle as O
    from test_trainer_gpu import build_trainer
    cfg = O.make_cfg(emb=16, vocab=list(VOCAB), d=64, H=4, layers=[1, 1], ff=128, D=16, K=K, ncb=ncb, zdim=16, up_hidden=32,
                     cdim=16, gru_hidden=32, B=4, N=7, Kl=2, Kr=2)
    enc = build_trainer(cfg, O.init_state(cfg, seed=6 + ncb)).encoder
    n = dc.table(1)[1]
    ids = torch.arange(0, n, n // K, dtype=torch.int64, device='cuda')[:K]
    x = torch.empty(K, 4, 4, dtype=torch.int64, device='cuda')
    dc.gather(ids, 1, x)
    z = enc.encode_latents(x).reshape(K, ncb, -1)
    with torch.no_grad():
        for c, p in enumerate(enc.quantizer.embeddings):
            p.copy_(z[:, c])
    return enc


@pytest.fixture(scope='module', params=[1, 2])
def world(request, tmp_path_factory):
    from vqcpc_bach_amd import clusters
    from vqcpc_bach_amd.dataloaders.corpus import CorpusCPCDataloaderGenerator, save_corpus
    ncb = request.param
    path = str(tmp_path_factory.mktemp('census') / 'corpus.npz')
    names = [[f'v{v}n{i}' for i in range(n)] for v, n in enumerate(VOCAB)]
    save_corpus(path, _pieces(), VOCAB, *CR.specials(VOCAB), last_start_beat=LAST, names=names)
    gen = CorpusCPCDataloaderGenerator(path, num_tokens_per_block=16, num_blocks_left=2, num_blocks_right=2, num_negative_samples=3,
                                       seed=5, device='cuda')
    dc = gen.device_corpus
    enc = _encoder(ncb, dc)
    enc.train()                                                               # the census must put this back
    census = clusters.cluster_census(enc, dc, split='train', examples=E, seed=0, chunk=CHUNK)
    assert enc.training, 'the previous mode is restored'
    from vqcpc_bach_amd.dataloaders.corpus import split_bounds
    lo, hi = split_bounds(dc.table(1)[1])['train']
    # the codes of the same chunks, by the same inference call
    enc.eval()
    codes = []
    for s in range(lo, hi, CHUNK):
        ids = torch.arange(s, min(s + CHUNK, hi), dtype=torch.int64, device='cuda')
        x = torch.empty(len(ids), 4, 4, dtype=torch.int64, device='cuda')
        dc.gather(ids, 1, x)
        codes.append(enc.encode_indices(x).reshape(len(ids), ncb).cpu().numpy())
    return dict(ncb=ncb, path=path, gen=gen, dc=dc, enc=enc, census=census, codes=np.concatenate(codes), lo=lo, hi=hi)


def test_the_population_is_the_one_block_window_set_of_the_split(world):
    from vqcpc_bach_amd.dataloaders.corpus import split_bounds
    c = world['census']
    n_windows = sum(LAST) + len(LAST)                                         # one-beat windows: start beats 0 .. last
    assert world['dc'].table(1)[1] == n_windows == 160
    assert (world['lo'], world['hi']) == split_bounds(n_windows)['train'] == (0, 136)
    assert (c.num_blocks, c.first_id, c.beats_per_block, c.split) == (136, 0, 1, 'train')
    assert c.counts.shape == (world['ncb'], K) and c.counts.dtype == np.int64
    assert (c.counts.sum(axis=1) == 136).all()


def test_counts_equal_the_bincount_of_encode_indices_over_the_same_chunks(world):
    from vqcpc_bach_amd import clusters
    c = world['census']
    assert np.array_equal(c.counts, R.counts(world['codes'], K))
    assert np.array_equal(c.used, (c.counts > 0).sum(axis=1)) and (c.used > 4).all(), 'a census of one code shows nothing'
    assert np.array_equal(c.perplexity, clusters.perplexity(c.counts))
    p = c.counts[0] / 136
    assert np.isclose(c.perplexity[0], np.exp(-sum(q * np.log(q) for q in p if q > 0)), rtol=1e-12)


def test_joint_statistics_equal_those_of_the_merged_codes(world):
    from vqcpc_bach_amd import clusters
    c, codes = world['census'], world['codes']
    merged = sum(codes[:, b] * K ** b for b in range(world['ncb']))
    want = np.bincount(merged, minlength=K ** world['ncb'])
    assert c.joint_used == int((want > 0).sum())
    assert c.joint_perplexity == float(clusters.perplexity(want))
    if world['ncb'] == 1:
        assert c.joint_used == c.used[0] and c.joint_perplexity == c.perplexity[0]


def test_example_ids_carry_their_code_and_equal_the_reference_selection(world):
    from vqcpc_bach_amd import clusters
    c, codes, lo = world['census'], world['codes'], world['lo']
    assert c.example_ids.shape == (world['ncb'], K, E) and c.example_ids.dtype == np.int64
    key = clusters.census_key(0, 'train')
    want = R.select(codes, np.arange(len(codes)), key, K, E)
    want_ids = np.where(want == R.EMPTY, -1, (want & np.uint64(0xFFFFFFFF)).astype(np.int64) + lo)
    assert np.array_equal(c.example_ids, want_ids)
    assert ((c.example_ids >= 0).sum(axis=2) == np.minimum(c.counts, E)).all()
    assert (c.counts > E).any(), 'some code has more members than examples, so the selection matters'
    for b in range(world['ncb']):
        for k in range(K):
            ids = c.example_ids[b, k]
            assert (codes[ids[ids >= 0] - lo, b] == k).all()


def test_examples_equal_window_at_row_by_row(world):
    c, corpus = world['census'], world['dc'].corpus
    cum = np.concatenate([[0], np.cumsum(corpus.window_counts(1))])
    seen = 0
    for b in range(world['ncb']):
        for k in range(K):
            got = c.examples(b, k)
            ids = c.example_ids[b, k]
            ids = ids[ids >= 0]
            assert got.shape == (len(ids), 4, 4) and got.dtype == np.int64
            for row, i in zip(got, ids):
                piece = int(np.searchsorted(cum, i, side='right')) - 1
                assert np.array_equal(row, corpus.window_at(piece, 4 * (i - cum[piece]), 4))
                seen += 1
    assert seen == int((c.example_ids >= 0).sum()) > 0
    last_of_piece_7 = cum[7] + 31
    assert cum[8] == last_of_piece_7 + 1, 'last_start_beat cuts piece 7 to 32 windows'


def test_two_runs_are_identical_and_another_seed_changes_the_examples_only(world):
    from vqcpc_bach_amd import clusters
    c = world['census']
    again = clusters.cluster_census(world['enc'], world['dc'], split='train', examples=E, seed=0, chunk=CHUNK)
    assert np.array_equal(again.counts, c.counts) and np.array_equal(again.example_ids, c.example_ids)
    assert (again.joint_used, again.joint_perplexity) == (c.joint_used, c.joint_perplexity)
    other = clusters.cluster_census(world['enc'], world['dc'], split='train', examples=E, seed=1, chunk=CHUNK)
    assert np.array_equal(other.counts, c.counts) and not np.array_equal(other.example_ids, c.example_ids)
    full = c.counts <= E                                                      # a code with at most E members shows them all
    assert np.array_equal(np.sort(other.example_ids[full], axis=-1), np.sort(c.example_ids[full], axis=-1))


def test_val_split_and_refusals(world):
    from vqcpc_bach_amd import clusters
    from vqcpc_bach_amd.quantizer.vector_quantizer import NoQuantization
    enc, dc = world['enc'], world['dc']
    val = clusters.cluster_census(enc, dc, split='val', examples=64, chunk=CHUNK)
    assert (val.num_blocks, val.first_id) == (16, 136) and (val.counts.sum(axis=1) == 16).all()
    ids = val.example_ids[val.example_ids >= 0]
    assert ids.min() >= 136 and ids.max() < 152
    for bad in (0, 65):
        with pytest.raises(ValueError, match='examples'):
            clusters.cluster_census(enc, dc, examples=bad)
    with pytest.raises(ValueError, match='valid split'):
        clusters.cluster_census(enc, dc, split='all')
    keep = enc.quantizer
    try:
        enc.quantizer = NoQuantization(codebook_dim=16)
        with pytest.raises(ValueError, match='NoQuantization'):
            clusters.cluster_census(enc, dc)
        with pytest.raises(ValueError, match='NoQuantization'):
            enc.show_nn_clusters()
    finally:
        enc.quantizer = keep


def test_an_empty_split_is_refused(world, tmp_path):
    from vqcpc_bach_amd import clusters
    from vqcpc_bach_amd.dataloaders.corpus import Corpus, DeviceCorpus
    piece = _pieces()[1]                                                      # 2 beats: 2 windows, int(0.85 * 2) = 1, val is empty
    start, end, pad = CR.specials(VOCAB)
    dc = DeviceCorpus(Corpus(piece.astype(np.int16), [0, len(piece)], 4, VOCAB, start, end, pad), 'cuda')
    with pytest.raises(ValueError, match='empty'):
        clusters.cluster_census(world['enc'], dc, split='val')


def test_save_and_load_round_trip_without_pickle(world, tmp_path):
    from vqcpc_bach_amd import clusters
    c = world['census']
    path = str(tmp_path / 'census.npz')
    c.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert {'counts', 'example_ids', 'num_blocks', 'split'} <= set(z.files)
    back = clusters.ClusterCensus.load(path, device_corpus=world['dc'])
    for name in ('split', 'num_blocks', 'beats_per_block', 'first_id', 'seed', 'joint_used', 'joint_perplexity'):
        assert getattr(back, name) == getattr(c, name), name
    for name in ('counts', 'example_ids', 'used', 'perplexity'):
        assert np.array_equal(getattr(back, name), getattr(c, name)), name
    assert back.table() == c.table()
    bare = clusters.ClusterCensus.load(path)
    with pytest.raises(ValueError, match='corpus'):
        bare.examples(0, 0)
    assert 'window' in bare.table(top=2)


def test_table_lists_counts_shares_and_note_names(world):
    c = world['census']
    text = c.table(codebook=0, top=2)
    lines = text.splitlines()
    order = np.lexsort((np.arange(K), -c.counts[0]))[:2]
    assert f'{int(c.used[0])} of {K} codes used' in lines[0] and '136 blocks of the train split' in lines[0]
    body = [ln for ln in lines if ln.lstrip().startswith(tuple(f'{int(k)}  count' for k in order))]
    assert len(body) == 2 and f'count {int(c.counts[0, order[0]]):8d}' in body[0]
    assert 'v0n' in text and 'v3n' in text and ' | ' in text, 'note names of the four voices'
    assert len(c.table(codebook=world['ncb'] - 1).splitlines()) > len(lines)


def test_plot_clusters_writes_both_files_and_refuses_what_it_cannot_do(world, tmp_path):
    import os

    from vqcpc_bach_amd import clusters
    from vqcpc_bach_amd.dataloaders.synthetic_cpc_dataloader import SyntheticCPCDataloaderGenerator
    enc = world['enc']
    keep = enc.model_dir
    try:
        enc.model_dir = str(tmp_path / 'model')
        census = enc.plot_clusters(world['gen'], 'val', batch_size=8, num_batches=1)
        assert census.num_blocks == 16, 'the whole split, whatever num_batches says'
        assert sorted(os.listdir(enc.model_dir)) == ['clusters_val.npz', 'clusters_val.txt']
        back = clusters.ClusterCensus.load(f'{enc.model_dir}/clusters_val.npz')
        assert np.array_equal(back.counts, census.counts) and np.array_equal(back.example_ids, census.example_ids)
        text = open(f'{enc.model_dir}/clusters_val.txt').read()
        assert text.count('codes used') == world['ncb'] and 'v1n' in text
        with pytest.raises(ValueError, match='is not a valid split value. Choose between train, val or test'):
            enc.plot_clusters(world['gen'], 'validation')
        with pytest.raises(NotImplementedError):
            enc.plot_clusters(SyntheticCPCDataloaderGenerator(num_blocks_left=2, num_blocks_right=2, num_negative_samples=3,
                                                              vocab=list(VOCAB)), 'train')
        with pytest.raises(NotImplementedError):
            enc.scatterplot_clusters_3d()
    finally:
        enc.model_dir = keep


def test_the_explore_clusters_tail_of_main_encoder_runs(world, tmp_path, capsys):
    """main_encoder.py:100-118 as written: a second generator built with training_method='decoder' from the encoder's own
    dataloader kwargs, both splits with num_batches=512, then the neighbour lists; only the 3-d scatter plot is left out."""
    import os

    from vqcpc_bach_amd import getters
    enc = world['enc']
    kwargs = dict(corpus_path=world['path'], num_tokens_per_block=16, num_blocks_left=2, num_blocks_right=2,
                  negative_sampling_method='random', num_negative_samples=3, device='cuda')
    keep = enc.model_dir
    try:
        enc.model_dir = str(tmp_path / 'model')
        dataloader_generator_clusters = getters.get_dataloader_generator(dataset='corpus', training_method='decoder',
                                                                         dataloader_generator_kwargs=kwargs)
        train = enc.plot_clusters(dataloader_generator_clusters, split_name='train', num_batches=512)
        val = enc.plot_clusters(dataloader_generator_clusters, split_name='val', num_batches=512)
        enc.show_nn_clusters()
        if enc.quantizer.codebook_dim == 3:
            enc.scatterplot_clusters_3d()
        assert sorted(os.listdir(enc.model_dir)) == ['clusters_train.npz', 'clusters_train.txt', 'clusters_val.npz', 'clusters_val.txt']
    finally:
        enc.model_dir = keep
    assert (train.num_blocks, val.num_blocks) == (136, 16) and train.example_ids.shape == (world['ncb'], K, 50)
    assert (train.counts.sum(axis=1) == 136).all() and (val.counts.sum(axis=1) == 16).all()
    assert 'Nearest neighbours list:' in capsys.readouterr().out


def test_show_nn_clusters_equals_the_reference_expression_on_well_separated_words(world, capsys):
    """encoder.py:178-185 restated in float64: norm of the pairwise differences, topk(k + 1) smallest, the first dropped.  The
    codebooks are random, 4 * N(0, 1): the test checks that every distance gap it relies on is far above float32 rounding."""
    enc, ncb = world['enc'], world['ncb']
    keep = [p.detach().clone() for p in enc.quantizer.embeddings]
    rng = np.random.RandomState(8)
    books = (rng.standard_normal((ncb, K, 16 // ncb)) * 4).astype(np.float32)
    try:
        with torch.no_grad():
            for p, b in zip(enc.quantizer.embeddings, books):
                p.copy_(torch.from_numpy(b))
        capsys.readouterr()
        got = enc.show_nn_clusters(3)
        printed = capsys.readouterr().out.splitlines()
    finally:
        with torch.no_grad():
            for p, b in zip(enc.quantizer.embeddings, keep):
                p.copy_(b)
    assert got.shape == (ncb, K, 3)
    for c in range(ncb):
        clusters = torch.from_numpy(books[c]).double()
        dists = torch.norm(clusters[None, :, :] - clusters[:, None, :], p=2, dim=2)
        nearest = torch.sort(dists, dim=1)[0][:, :5] ** 2
        bound = 4 * R.dist2_bound(books.shape[2])                               # twice the rounding of both distances of a pair
        assert bool(((nearest[:, 1:] - nearest[:, :-1]) > bound * nearest[:, 1:]).all()), 'well separated'
        want = np.stack([torch.topk(dists[i], k=4, largest=False)[1][1:].numpy() for i in range(K)])
        assert np.array_equal(got[c], want)
    assert printed[0] == 'Nearest neighbours list:'
    assert printed[1:K + 1] == [f'{i}: {got[0][i]}' for i in range(K)]
    assert len(printed) == ncb * (K + 1)
    if ncb == 2:
        assert 'codebook 1' in printed[K + 1] and printed[K + 2] == f'0: {got[1][0]}'
