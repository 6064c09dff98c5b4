"""The corpus dataloader generators (vqcpc_bach_amd/dataloaders/corpus.py) on the device: every batch tensor equals the rows of the
materialised dataset (tests/corpus_reference.py) at the batch's ids; epochs, splits, ranks, the contract of the synthetic
generators, the getters, and training steps fed from a corpus.  Exact integer equality throughout."""
import functools
import json

import numpy as np
import pytest
import torch

import corpus_reference as R

pytestmark = pytest.mark.gpu

BEATS = (1, 2, 3, 5, 7, 9, 12, 16, 20, 24, 30, 40)
VOCAB = (30, 30, 30, 30)
DEC_VOCAB = (11, 12, 13, 14)                      # tests/golden/decoder_tiny.npz


@functools.lru_cache(maxsize=None)
def _pieces(vocab):
    return R.seeded_pieces(BEATS, vocab, seed=sum(vocab))


@functools.lru_cache(maxsize=None)
def _ref(vocab, W):
    ref = R.materialise(_pieces(vocab), W, *R.specials(vocab))
    ref.setflags(write=False)
    return ref


@pytest.fixture(scope='module')
def paths(tmp_path_factory):
    from vqcpc_bach_amd.dataloaders.corpus import save_corpus
    out = {}
    for vocab in (VOCAB, DEC_VOCAB):
        out[vocab] = str(tmp_path_factory.mktemp('corpus') / 'corpus.npz')
        start, end, pad = R.specials(vocab)
        save_corpus(out[vocab], _pieces(vocab), vocab, start, end, pad)
    return out


def _cpc(path, method, **kw):
    from vqcpc_bach_amd.dataloaders.corpus import CorpusCPCDataloaderGenerator
    args = dict(num_tokens_per_block=16, num_blocks_left=2, num_blocks_right=2, negative_sampling_method=method,
                num_negative_samples=3, seed=5, device='cuda')
    args.update(kw)
    return CorpusCPCDataloaderGenerator(path, **args)


def _np(t):
    return t.cpu().numpy()


def _same_sequence(first, second):
    """bach_cpc_dataloader.py:159-181 on (B, ticks, 4) arrays: for target block k of `second`, all blocks of `first`, then the
    blocks of `second` except k -> (B, Ka + Kb - 1, Kb, 4, 4)."""
    B = first.shape[0]
    a, b = first.reshape(B, -1, 4, 4), second.reshape(B, -1, 4, 4)
    return np.stack([np.concatenate([a, np.delete(b, k, axis=1)], axis=1) for k in range(b.shape[1])], axis=2)


def _check_cpc_batch(batch, ids, method):
    pos = _ref(VOCAB, 4)[_np(ids['positive'])]
    assert np.array_equal(_np(batch['x_left']), pos[:, :8]) and np.array_equal(_np(batch['x_right']), pos[:, 8:])
    if method == 'random':
        assert sorted(ids) == ['negative', 'negative_back', 'positive']
        assert np.array_equal(_np(batch['negative_samples']), _ref(VOCAB, 1)[_np(ids['negative'])])
        assert np.array_equal(_np(batch['negative_samples_back']), _ref(VOCAB, 1)[_np(ids['negative_back'])])
    else:
        assert sorted(ids) == ['positive']
        assert np.array_equal(_np(batch['negative_samples']), _same_sequence(pos[:, :8], pos[:, 8:]))
        assert np.array_equal(_np(batch['negative_samples_back']), _same_sequence(pos[:, 8:], pos[:, :8]))


@pytest.mark.parametrize('method', ['random', 'same_sequence'])
def test_cpc_epoch_against_the_materialised_dataset(paths, method):
    B, N, Kr = 4, 3, 2
    gen = _cpc(paths[VOCAB], method)
    n_pos, n_neg = len(_ref(VOCAB, 4)), len(_ref(VOCAB, 1))
    (p_tr, p_va, p_te), (n_tr, n_va, n_te) = R.split_ranges(n_pos), R.split_ranges(n_neg)
    train, val, test = gen.dataloaders(batch_size=B)
    steps = (p_tr[1] - p_tr[0]) // B
    if method == 'random':
        steps = min(steps, (n_tr[1] - n_tr[0]) // (B * N * Kr))
    assert len(train) == steps
    seen = {'positive': [], 'negative': [], 'negative_back': []}
    first = None
    for batch in train:
        ids = train.last_ids
        assert gen.last_ids is ids
        first = first if first is not None else {k: _np(v).copy() for k, v in ids.items()}
        _check_cpc_batch(batch, ids, method)
        for k, v in ids.items():
            seen[k].append(_np(v).reshape(-1))
    assert len(seen['positive']) == steps, 'one train epoch has the stated number of steps'
    for k, (lo, hi) in (('positive', p_tr), ('negative', n_tr), ('negative_back', n_tr)):
        if seen[k]:
            got = np.concatenate(seen[k])
            assert len(np.unique(got)) == len(got), f'{k}: an id repeats inside the epoch'
            assert got.min() >= lo and got.max() < hi, f'{k}: ids outside the train split'
    if method == 'random':
        assert not np.array_equal(np.concatenate(seen['negative']), np.concatenate(seen['negative_back']))
    _, val, test = gen.dataloaders(batch_size=1)          # the 16 / 10 negative blocks of val / test fill a step of one row only
    for loader, pr, nr in ((val, p_va, n_va), (test, p_te, n_te)):
        batch = next(loader)
        _check_cpc_batch(batch, loader.last_ids, method)
        for k, v in loader.last_ids.items():
            lo, hi = pr if k == 'positive' else nr
            assert int(v.min()) >= lo and int(v.max()) < hi, f'{loader.split} {k}'
    train2 = gen.dataloaders(batch_size=B)[0]
    batch = next(train2)
    _check_cpc_batch(batch, train2.last_ids, method)
    assert not np.array_equal(_np(train2.last_ids['positive']), first['positive']), 'the next epoch has a new order'
    gen.device_corpus.raise_if_bad_ids()


def test_x_loader_against_the_materialised_dataset(paths):
    from vqcpc_bach_amd.dataloaders.corpus import CorpusDataloaderGenerator
    W, B = 6, 8
    gen = CorpusDataloaderGenerator(paths[VOCAB], sequences_size=W, seed=2, device='cuda')
    ref = _ref(VOCAB, W)
    tr, va, te = R.split_ranges(len(ref))
    train, val, test = gen.dataloaders(batch_size=B)
    assert len(train) == (tr[1] - tr[0]) // B
    seen = []
    for batch in train:
        assert sorted(batch) == ['x'] and batch['x'].shape == (B, 4 * W, 4)
        assert np.array_equal(_np(batch['x']), ref[_np(train.last_ids)])
        seen.append(_np(train.last_ids))
    seen = np.concatenate(seen)
    assert len(seen) == len(train) * B == len(np.unique(seen)) and seen.min() >= tr[0] and seen.max() < tr[1]
    for loader, (lo, hi) in ((val, va), (test, te)):
        batch = next(loader)
        ids = _np(loader.last_ids)
        assert np.array_equal(_np(batch['x']), ref[ids]) and ids.min() >= lo and ids.max() < hi
    again = gen.dataloaders(batch_size=B)[0]
    next(again)
    assert not np.array_equal(_np(again.last_ids), seen[:B])


def test_four_ranks_of_eight_equal_one_rank_of_thirty_two(paths):
    one = _cpc(paths[VOCAB], 'random', num_negative_samples=1, num_blocks_right=1).dataloaders(batch_size=32)[0]
    four = [_cpc(paths[VOCAB], 'random', num_negative_samples=1, num_blocks_right=1, rank=r, world_size=4).dataloaders(batch_size=8)[0]
            for r in range(4)]
    assert len(one) >= 2 and all(len(f) == len(one) for f in four)
    for batch in one:
        parts = [next(f) for f in four]
        for k, v in batch.items():
            assert torch.equal(torch.cat([p[k] for p in parts]), v), k
        for k, v in one.last_ids.items():
            assert torch.equal(torch.cat([f.last_ids[k] for f in four]), v), k
    for f in four:
        with pytest.raises(StopIteration):
            next(f)


@pytest.mark.parametrize('method', ['random', 'same_sequence'])
def test_cpc_contract_of_the_synthetic_generator(paths, method):
    from vqcpc_bach_amd.dataloaders.synthetic_cpc_dataloader import SyntheticCPCDataloaderGenerator
    args = dict(num_tokens_per_block=16, num_blocks_left=3, num_blocks_right=3, negative_sampling_method=method,
                num_negative_samples=2, seed=1, device='cuda')
    syn = SyntheticCPCDataloaderGenerator(vocab=VOCAB, **args)
    cor = _cpc(paths[VOCAB], method, **{k: v for k, v in args.items() if k != 'negative_sampling_method'})
    for a in ('num_blocks_left', 'num_blocks_right', 'num_tokens_per_block', 'num_channels', 'num_negative_samples',
              'negative_sampling_method', 'vocab'):
        assert getattr(cor, a) == getattr(syn, a), a
    assert cor.dataset is cor.dataset_positive
    for a in ('sequences_size', 'subdivision', 'index2note_dicts'):
        assert getattr(cor.dataset_positive, a) == getattr(syn.dataset_positive, a), a
    b_syn, b_cor = next(syn.dataloaders(batch_size=2)[0]), next(cor.dataloaders(batch_size=2)[0])
    assert sorted(b_syn) == sorted(b_cor)
    for k in b_syn:
        assert (b_cor[k].shape, b_cor[k].dtype, b_cor[k].device) == (b_syn[k].shape, b_syn[k].dtype, b_syn[k].device), k
        assert b_cor[k].is_contiguous()


def test_x_contract_of_the_synthetic_generator(paths):
    from vqcpc_bach_amd.dataloaders.corpus import CorpusDataloaderGenerator
    from vqcpc_bach_amd.dataloaders.synthetic_student_dataloader import SyntheticStudentDataloaderGenerator
    syn = SyntheticStudentDataloaderGenerator(sequences_size=5, vocab=VOCAB, seed=1, device='cuda')
    cor = CorpusDataloaderGenerator(paths[VOCAB], sequences_size=5, seed=1, device='cuda')
    for a in ('num_channels', 'num_events', 'vocab'):
        assert getattr(cor, a) == getattr(syn, a), a
    for a in ('sequences_size', 'subdivision', 'index2note_dicts'):
        assert getattr(cor.dataset, a) == getattr(syn.dataset, a), a
    x_syn, x_cor = next(syn.dataloaders(batch_size=3)[0])['x'], next(cor.dataloaders(batch_size=3)[0])['x']
    assert (x_cor.shape, x_cor.dtype, x_cor.device) == (x_syn.shape, x_syn.dtype, x_syn.device)


def test_getters_build_both_kinds(paths):
    from vqcpc_bach_amd import configs, getters
    from vqcpc_bach_amd.dataloaders.corpus import CorpusCPCDataloaderGenerator, CorpusDataloaderGenerator
    kw = dict(configs.make_config('C1')['dataloader_generator_kwargs'], corpus_path=paths[VOCAB], device='cuda', seed=3)
    cpc = getters.get_dataloader_generator('corpus', 'vqcpc', kw)
    assert type(cpc) is CorpusCPCDataloaderGenerator and (cpc.num_blocks_left, cpc.num_blocks_right) == (8, 8)
    dp = getters.get_data_processor(cpc, 'bach_cpc', dict(embedding_size=8))
    assert dp.num_tokens_per_channel == list(VOCAB) and dp.num_channels == 4
    for method in ('student', 'decoder', 'prior'):
        x = getters.get_dataloader_generator('corpus', method, dict(corpus_path=paths[VOCAB], sequences_size=4, device='cuda'))
        assert type(x) is CorpusDataloaderGenerator and x.num_events == 16
        assert next(x.dataloaders(batch_size=2)[0])['x'].shape == (2, 16, 4)
    with pytest.raises(NotImplementedError):
        getters.get_dataloader_generator('corpus', 'nothing', kw)


def test_a_split_that_cannot_fill_a_step_raises(paths):
    train, val, test = _cpc(paths[VOCAB], 'random', num_negative_samples=15, num_blocks_right=2).dataloaders(batch_size=8)
    with pytest.raises(ValueError, match='cannot fill one step'):
        next(train)                                                      # 8 * 15 * 2 negatives of a 143-window split
    with pytest.raises(ValueError, match='test split'):
        iter(test).__next__()


# ---- training from a corpus ---------------------------------------------------------------------------------------------------
def test_two_encoder_training_steps_on_corpus_batches(paths):
    from oracle import vqcpc_oracle as O
    from test_trainer_gpu import build_trainer
    from vqcpc_bach_amd import hip
    cfg = O.make_cfg(emb=16, vocab=list(VOCAB), d=64, H=4, layers=[1, 1], ff=128, D=16, K=32, ncb=2, zdim=16, up_hidden=32,
                     cdim=16, gru_hidden=32, B=4, N=7, Kl=2, Kr=2)
    gen = _cpc(paths[VOCAB], 'random', num_negative_samples=cfg['N'])
    train = gen.dataloaders(batch_size=cfg['B'])[0]
    assert len(train) >= 2
    hip.load()
    hip.set_gemm_mode(1)
    try:
        tr = build_trainer(cfg, O.init_state(cfg, seed=4), lr=1e-3)
        tr.train()
        losses = [float(tr.train_step(next(train), train=True)['loss']) for _ in range(2)]
    finally:
        hip.set_gemm_mode(0)
    assert np.isfinite(losses).all(), losses
    tr.encoder.data_processor.raise_if_bad_tokens()
    gen.device_corpus.raise_if_bad_ids()


def _decoder_steps(dec, batches, graph):
    dec.train()
    dec.enable_step_graph(graph)
    losses = [dec.train_step(b).clone() for b in batches]
    replays = dec._graph.replays if dec._graph is not None else 0
    dec.enable_step_graph(False)
    return torch.stack(losses).cpu(), dec.flat.flat.detach().cpu().clone(), replays


def test_decoder_steps_on_corpus_batches_and_replay_is_the_eager_step_bit_for_bit(paths):
    """Three Decoder.train_steps on corpus batches under train_model()'s defaults: finite losses; with the step graph the third is a
    replay, and losses and parameters equal the eager run's bit for bit."""
    from conftest import load_golden, sub_state
    from oracle import decoder_oracle as D
    from test_decoder_gpu import build_decoder
    from vqcpc_bach_amd import hip, ops
    from vqcpc_bach_amd.dataloaders.corpus import CorpusDataloaderGenerator
    g = load_golden('decoder_tiny')
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    assert tuple(cfg['vocab']) == DEC_VOCAB
    gen = CorpusDataloaderGenerator(paths[DEC_VOCAB], sequences_size=cfg['events'] // 4, seed=9, device='cuda')
    train = gen.dataloaders(batch_size=cfg['B'])[0]
    batches = [next(train) for _ in range(3)]
    assert all(sorted(b) == ['x'] for b in batches)
    mode, arith = hip.gemm_mode_state(), ops.gradient_arithmetic_state()
    res = {}
    try:
        for graph in (False, True):
            dec = build_decoder(cfg, sub_state(g, 'sd0'), lr=float(g['lr']))
            dec.use_training_defaults()
            res[graph] = _decoder_steps(dec, batches, graph)
    finally:
        hip.restore_gemm_mode_state(mode)
        ops.restore_gradient_arithmetic_state(arith)
    assert torch.isfinite(res[False][0]).all() and torch.isfinite(res[True][0]).all()
    assert res[False][2] == 0 and res[True][2] >= 1, 'the step must have been replayed'
    assert torch.equal(res[False][0], res[True][0])
    assert torch.equal(res[False][1], res[True][1])
