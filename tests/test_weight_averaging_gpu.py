"""Weight averaging through training.FlatTraining, for the four trainers at the tiny configurations of their own test modules:
the average never feeds back into training, equals the numpy float32 restatement (tests/weight_average_reference.py) applied to
the recorded parameter trajectory as BITS -- eagerly and under graph replay --, is inert when off, swaps in and out of the flat
buffer (`averaged_weights`), survives save / load / resume, lands in `{model_dir}/averaged/`, and stays rank-identical."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import weight_average_reference as R
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DECAY = 0.3            # the warm-up term (1 + u) / (10 + u) acts for u = 1, 2 and decay alone from u = 3: both sides within five steps
OPT_KEYS = {'m', 'v', 'step', 'global_step', 'dropout_stream'}


@pytest.fixture(autouse=True)
def training_gemm_mode():
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1)
    yield
    hip.set_gemm_mode(0)


# ---- the four trainers: builder() -> (trainer after init_optimizers, batch, keywords of a training step) -------------------
def _cpc():
    from test_trainer_gpu import build_trainer, golden_cfg_sd
    g = load_golden('epoch_tiny')
    cfg, sd = golden_cfg_sd(g)
    batch = {k.split('/', 1)[1]: T(v).cuda() for k, v in g.items() if k.startswith('batch/')}
    return build_trainer(cfg, sd), batch, {}


def _student():
    from oracle import student_oracle as S
    from test_student_gpu import build_student, golden_state
    g = load_golden('student_tiny')
    cfg = S.make_cfg(**json.loads(str(g['cfg_json'])))
    return build_student(cfg, golden_state(g)), {'x': T(g['batch/x']).cuda()}, dict(masked_event_index=3)


DEC_CFG = dict(vocab=[12, 12, 12, 12], emb=16, d=32, H=2, layers=[1, 1], ff=64, D=8, K=16, ncb=1, zdim=8, up_hidden=16, Kl=2, Kr=2,
               events=16, B=8, dec_d=64, dec_H=2, dec_enc_layers=1, dec_dec_layers=2, dec_ff=128)


def _decoder():
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    dec, _ = seeded_decoder(D.make_cfg(**DEC_CFG), 11)
    gen = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randint(0, 12, (8, 16, 1), generator=gen) for _ in range(4)], dim=2).cuda()
    return dec, {'x': x}, {}


def _prior():
    from test_prior_gpu import _batches, _golden_prior
    prior, cfg, _ = _golden_prior('v32')
    prior.init_optimizers(lr=1e-3)
    return prior, _batches(cfg, 1, seed=1)[0], {}


# builder, arguments of save() / load(), arguments of init_optimizers(), extra arguments of epoch(), the optimiser-state file
TRAINERS = {'cpc': (_cpc, dict(early_stopped=False), dict(lr=1e-3, schedule_lr=False), dict(corrupt_labels=False),
                    'overfitted/optimizer'),
            'student': (_student, dict(early_stopped=False), dict(lr=1e-3, schedule_lr=False), {}, 'overfitted/optimizer'),
            'decoder': (_decoder, dict(early_stopped=False), dict(lr=1e-3, schedule_lr=False), {}, 'overfitted/decoder_optimizer'),
            'prior': (_prior, {}, dict(lr=1e-3), {}, 'prior_optimizer')}


def _set_model_dir(tr, path):
    tr.model_dir = tr.encoder.model_dir = str(path)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(_np(a) if torch.is_tensor(a) else a), _bits(_np(b) if torch.is_tensor(b) else b))


@contextlib.contextmanager
def _recorded_calls():
    """The names of the library calls issued inside, in order (the real calls still happen)."""
    from vqcpc_bach_amd import hip
    names, real = [], hip.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    hip.call = call
    try:
        yield names
    finally:
        hip.call = real


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


# ---- 1. the average follows the trajectory and never feeds back; off means absent ----------------------------------------------
@pytest.mark.parametrize('name', list(TRAINERS))
def test_average_follows_the_trajectory_and_never_feeds_back(name, tmp_path):
    build, how, _, epoch_kw, opt_file = TRAINERS[name]

    # averaging never touched: the launches of a step, epoch()'s keys, the optimiser file's keys, the files of a save
    off, batch, kw = build()
    off.train()
    _set_model_dir(off, tmp_path / 'off')
    assert off.weight_average() is None
    traj_off = []
    with _recorded_calls() as names_off:
        off.train_step(batch, train=True, **kw)
    traj_off.append(_np(off.flat.flat))
    for _ in range(4):
        with _recorded_calls() as names_off_late:               # (a first step also issues one-time launches; a fifth does not)
            off.train_step(batch, train=True, **kw)
        traj_off.append(_np(off.flat.flat))
    assert 'vqcpc_weight_average' not in names_off + names_off_late
    assert names_off.count('vqcpc_adam_step') == len(off._graph_optimizers())
    keys_off = set(off.epoch(iter([batch]), train=False, num_batches=1, **epoch_kw))
    off.save(**how)
    assert set(torch.load(tmp_path / 'off' / opt_file)) == OPT_KEYS
    assert not any('averaged' in f for f in _files(tmp_path / 'off'))
    with pytest.raises(RuntimeError, match='not enabled'):
        with off.averaged_weights():
            pass
    for bad in (1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match='decay'):
            off.enable_weight_averaging(bad)
    assert off.weight_average() is None

    # averaging on: the same five steps
    on, batch, kw = build()
    on.train()
    _set_model_dir(on, tmp_path / 'on')
    start = _np(on.flat.flat)
    on.enable_weight_averaging(DECAY)
    assert on.weight_average().numel() == on.flat.numel and _same_bits(on.weight_average(), start)
    traj_on = []
    with _recorded_calls() as names_on:
        on.train_step(batch, train=True, **kw)
    traj_on.append(_np(on.flat.flat))
    for _ in range(4):
        on.train_step(batch, train=True, **kw)
        traj_on.append(_np(on.flat.flat))
    for k, (a, b) in enumerate(zip(traj_off, traj_on)):
        assert _same_bits(a, b), f'step {k + 1}: the raw parameters differ with averaging on'
    # one launch per optimiser, right after its Adam launch; nothing else changes
    assert [n for n in names_on if n != 'vqcpc_weight_average'] == names_off
    n_opt = len(on._graph_optimizers())
    assert names_on.count('vqcpc_weight_average') == n_opt == (3 if name == 'student' else 1)
    assert all(names_on[i + 1] == 'vqcpc_weight_average' for i, n in enumerate(names_on) if n == 'vqcpc_adam_step')
    # the whole flat buffer (the student's three optimisers each own their slice), as bits
    want = R.average_f32(start, traj_on, DECAY, u0=1)
    got = _np(on.weight_average())
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert not _same_bits(got, traj_on[-1]) and not _same_bits(got, start)
    moved = np.flatnonzero(_bits(traj_on[-1]) != _bits(start))
    assert moved.size > 0.5 * start.size                         # (padding between parameters never moves)
    assert set(on.epoch(iter([batch]), train=False, num_batches=1, **epoch_kw)) == keys_off
    on.save(**how)
    st = torch.load(tmp_path / 'on' / opt_file)
    assert set(st) == OPT_KEYS | {'avg', 'avg_decay', 'avg_t0'} and st['avg_t0'] == 0 and st['avg_decay'] == DECAY
    assert _same_bits(st['avg'], got)
    assert not any('averaged' in f for f in _files(tmp_path / 'on'))       # only save_averaged / train_model write there

    # off again: the step is the parent's step
    on.disable_weight_averaging()
    on.train()
    with _recorded_calls() as names_again:
        on.train_step(batch, train=True, **kw)
    assert names_again == names_off_late and on.weight_average() is None


# ---- 2. graph replay ------------------------------------------------------------------------------------------------------
def _enabled_after_one_step(build, graph):
    """One step without the average, then six with it (t0 = 1), under train_model()'s defaults.  With the step graph on, step 2 is
    the last warm-up step and steps 3..7 are replays: the captured launch reads the device counter that Adam reads."""
    tr, batch, kw = build()
    tr.train()
    tr.enable_step_graph(graph)
    tr.use_training_defaults()
    tr.train_step(batch, train=True, **kw)
    start = _np(tr.flat.flat)
    tr.enable_weight_averaging(DECAY)
    assert all(o.avg_t0 == 1 for o in tr._graph_optimizers())
    traj = []
    for _ in range(6):
        tr.train_step(batch, train=True, **kw)
        traj.append(_np(tr.flat.flat))
    replays = tr._graph.replays if tr._graph is not None else 0
    avg = _np(tr.weight_average())
    # enabling and disabling both release a captured step: the next capture has the launches of the new configuration
    if graph:
        tr.disable_weight_averaging()
        assert tr._graph is None and all(o.avg is None and o._dev is None for o in tr._graph_optimizers())
    tr.enable_step_graph(False)
    return start, traj, avg, replays


@pytest.mark.parametrize('name', list(TRAINERS))
def test_replayed_steps_average_the_replayed_trajectory(name):
    """Under graph replay the launch takes its update count from the device counter Adam reads: the average is the restatement
    applied to the trajectory the replays produced, as bits.  For the decoder (the trainer of
    test_replayed_step_is_the_eager_step_bit_for_bit) eager and replayed steps agree bit for bit, parameters and average."""
    from vqcpc_bach_amd import hip, ops
    build = TRAINERS[name][0]
    mode, arith = hip.gemm_mode_state(), ops.gradient_arithmetic_state()
    res = {}
    try:
        for graph in ((False, True) if name == 'decoder' else (True,)):
            res[graph] = _enabled_after_one_step(build, graph)
    finally:
        hip.restore_gemm_mode_state(mode)
        ops.restore_gradient_arithmetic_state(arith)
    start, traj, avg, replays = res[True]
    assert replays == 5, 'steps 3..7 must have been replayed'
    assert _same_bits(avg, R.average_f32(start, traj, DECAY, u0=1))
    if name == 'decoder':
        e_start, e_traj, e_avg, e_replays = res[False]
        assert e_replays == 0 and _same_bits(e_avg, R.average_f32(e_start, e_traj, DECAY, u0=1))
        assert _same_bits(e_start, start) and all(_same_bits(a, b) for a, b in zip(e_traj, traj))
        assert _same_bits(e_avg, avg)


def test_enabling_after_the_first_capture_captures_again_after_new_warm_up_steps():
    """Decoder, three steps (two eager, one replay of a graph WITHOUT the launch), then averaging on: the graph is released, the
    next two steps are eager warm-up steps again, the following four replay a new capture that has the launch -- and all of it
    equals the eager run bit for bit, parameters and average."""
    from vqcpc_bach_amd import hip, ops
    mode, arith = hip.gemm_mode_state(), ops.gradient_arithmetic_state()
    res = {}
    try:
        for graph in (False, True):
            dec, batch, _ = _decoder()
            dec.train()
            dec.enable_step_graph(graph)
            dec.use_training_defaults()
            for _ in range(3):
                dec.train_step(batch, train=True)
            before = dec._graph.replays if graph else 0
            start = _np(dec.flat.flat)
            dec.enable_weight_averaging(DECAY)
            assert dec._graph is None and dec._graph_optimizers()[0].avg_t0 == 3
            traj = []
            for _ in range(6):
                dec.train_step(batch, train=True)
                traj.append(_np(dec.flat.flat))
            res[graph] = (start, traj, _np(dec.weight_average()), before, dec._graph.replays if graph else 0)
            dec.enable_step_graph(False)
    finally:
        hip.restore_gemm_mode_state(mode)
        ops.restore_gradient_arithmetic_state(arith)
    assert res[True][3] == 1 and res[True][4] == 4 and res[False][3:] == (0, 0)
    for graph in (False, True):
        start, traj, avg = res[graph][:3]
        assert _same_bits(avg, R.average_f32(start, traj, DECAY, u0=1))
    assert _same_bits(res[False][0], res[True][0]) and _same_bits(res[False][2], res[True][2])
    assert all(_same_bits(a, b) for a, b in zip(res[False][1], res[True][1]))


# ---- 3. averaged_weights() -------------------------------------------------------------------------------------------------
def _greedy(dec, x):
    with torch.no_grad():
        return dec.generate_from_codes(dec.encode(x[:2]), top_k=1, seed=0)


def test_averaged_weights_swaps_the_flat_buffer_in_place():
    from vqcpc_bach_amd import hip, ops
    mode, arith = hip.gemm_mode_state(), ops.gradient_arithmetic_state()
    try:
        runs = {}
        for enter in (True, False):
            dec, batch, _ = _decoder()
            dec.train()
            dec.enable_step_graph(False)
            dec.use_training_defaults()                         # f16x3 products: weight-plane images are made per step
            dec.enable_weight_averaging(DECAY)
            for _ in range(3):
                dec.train_step(batch, train=True)
            if enter:
                raw, avg = _np(dec.flat.flat), _np(dec.weight_average())
                ptrs = [p.data_ptr() for p in dec.flat.params]
                tokens_raw = _greedy(dec, batch['x'])             # generation state made from the RAW weights exists before the swap
                version = ops._PARAM_STEPS
                with dec.averaged_weights() as inside:
                    assert inside is dec and ops._PARAM_STEPS == version + 1
                    assert _same_bits(dec.flat.flat, avg) and [p.data_ptr() for p in dec.flat.params] == ptrs
                    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
                    for p, off in zip(dec.flat.params, dec.flat.offsets):
                        assert _same_bits(p, avg[off:off + p.numel()].reshape(tuple(p.shape)))
                    dec.eval()
                    loss_inside = dec.train_step(batch, train=False).clone()
                    tokens_inside = _greedy(dec, batch['x'])
                    dec.train()
                    with pytest.raises(RuntimeError, match='averaged_weights'):
                        dec.train_step(batch, train=True)
                    with pytest.raises(RuntimeError, match='nest'):
                        with dec.averaged_weights():
                            pass
                    assert _same_bits(dec.flat.flat, avg)           # the refusals changed nothing
                assert ops._PARAM_STEPS == version + 2
                assert _same_bits(dec.flat.flat, raw) and _same_bits(dec.weight_average(), avg)
                assert [p.data_ptr() for p in dec.flat.params] == ptrs and dec.flat.check_views()
                # a twin that LOADS the averaged state_dict computes the same loss and writes the same tokens
                twin, _, _ = _decoder()
                twin.load_state_dict(sd, strict=True)
                twin.eval()
                assert torch.equal(twin.train_step(batch, train=False), loss_inside)
                assert torch.equal(_greedy(twin, batch['x']), tokens_inside)
                assert torch.equal(_greedy(dec, batch['x']), tokens_raw)        # and the raw weights write the raw tokens again
                del twin
            dec.train_step(batch, train=True)
            runs[enter] = (_np(dec.flat.flat), _np(dec.weight_average()))
        # the step after the context is the step of a run that never entered it (no stale weight-plane image)
        assert _same_bits(runs[True][0], runs[False][0]) and _same_bits(runs[True][1], runs[False][1])
    finally:
        hip.restore_gemm_mode_state(mode)
        ops.restore_gradient_arithmetic_state(arith)


# ---- 4. checkpoints -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(TRAINERS))
def test_resume_continues_the_average_and_averaged_files_load(name, tmp_path, capsys):
    build, how, init, _, opt_file = TRAINERS[name]
    a, batch, kw = build()
    a.train()
    _set_model_dir(a, tmp_path)
    a.train_step(batch, train=True, **kw)
    a.enable_weight_averaging(DECAY)                            # t0 = 1
    for _ in range(3):
        a.train_step(batch, train=True, **kw)
    a.save(**how)
    raw_saved, avg_saved = _np(a.flat.flat), _np(a.weight_average())
    a.save_averaged(**how)
    assert _same_bits(a.flat.flat, raw_saved) and not a._avg_inside and a.model_dir == a.encoder.model_dir == str(tmp_path)
    for _ in range(2):
        a.train_step(batch, train=True, **kw)

    # resume: load, init_optimizers, enable -> the same bits two steps later
    b, _, _ = build()
    _set_model_dir(b, tmp_path)
    b.load(device='cuda', **how)
    b.init_optimizers(**init)
    b.enable_weight_averaging(DECAY)
    assert all(o.avg_t0 == 1 and o.step_count == 4 for o in b._graph_optimizers())
    assert _same_bits(b.flat.flat, raw_saved) and _same_bits(b.weight_average(), avg_saved) and b._avg_resume is None
    b.train()
    for _ in range(2):
        b.train_step(batch, train=True, **kw)
    assert _same_bits(b.flat.flat, a.flat.flat) and _same_bits(b.weight_average(), a.weight_average())

    # averaged/: the same relative layout, weights only; a model built on that directory loads them as always
    files = _files(tmp_path)
    plain = [f for f in files if not f.startswith('averaged' + os.sep)]
    averaged = [os.path.relpath(f, 'averaged') for f in files if f.startswith('averaged' + os.sep)]
    assert sorted(averaged) == sorted(f for f in plain if f != opt_file) and opt_file in plain
    c, _, _ = build()
    _set_model_dir(c, tmp_path / 'averaged')
    c.load(device='cuda', **how)                                # load_state_dict(strict=True) inside
    assert c._resume_state is None
    c.init_optimizers(**init)
    assert _same_bits(c.flat.flat, avg_saved)

    # a checkpoint of another size: a fresh average from the current weights, and the line that says so
    if name == 'prior':
        from test_prior_cpu import build_prior
        from test_prior_gpu import _golden_prior
        cfg = _golden_prior('v32')[1]
        d = build_prior(dict(cfg, p_ff=2 * cfg['p_ff'])).cuda()
        d.init_optimizers(**init)
        d._avg_resume = dict(avg=torch.zeros(a.flat.numel), avg_decay=DECAY, avg_t0=1)
        capsys.readouterr()
        d.enable_weight_averaging(DECAY)
        assert capsys.readouterr().out.count('weight average ignored: parameter count differs from the checkpoint') == 1
        assert _same_bits(d.weight_average(), d.flat.flat) and d._graph_optimizers()[0].avg_t0 == 0


def test_train_model_writes_the_averaged_checkpoint(tmp_path):
    """`train_model(..., weight_average=decay)` end to end on the prior: validation under the averaged weights, `averaged/prior`
    next to `prior`, the average in the optimiser state; and nothing of it without the keyword."""
    from test_prior_cpu import build_prior
    from test_prior_gpu import _golden_prior
    from vqcpc_bach_amd.dataloaders.synthetic_student_dataloader import SyntheticStudentDataloaderGenerator
    for decay in (None, 0.9):
        prior, cfg, _ = _golden_prior('v32')
        prior.model_dir = str(tmp_path / f'prior_{decay}')
        prior.dataloader_generator = SyntheticStudentDataloaderGenerator(sequences_size=cfg['N'], subdivision=4, vocab=cfg['vocab'],
                                                                         seed=4, device='cuda')
        seen = []
        real_epoch = prior.epoch
        prior.epoch = lambda *a, **k: (seen.append((k.get('train'), prior._avg_inside)), real_epoch(*a, **k))[1]
        hist = prior.train_model(batch_size=4, num_batches=4, num_epochs=1, lr=1e-3, weight_average=decay)
        assert len(hist) == 1 and np.isfinite(hist[0][1]['loss']) and set(hist[0][1]) == {'loss'}
        files = _files(prior.model_dir)
        st = torch.load(os.path.join(prior.model_dir, 'prior_optimizer'))
        if decay is None:
            assert files == ['prior', 'prior_optimizer'] and set(st) == OPT_KEYS and seen == [(True, False), (False, False)]
            continue
        assert files == [os.path.join('averaged', 'prior'), 'prior', 'prior_optimizer']
        assert seen == [(True, False), (False, True)]            # the validation epoch ran under the averaged weights
        assert set(st) == OPT_KEYS | {'avg', 'avg_decay', 'avg_t0'} and not prior._avg_inside
        shipped = build_prior(cfg, model_dir=os.path.join(prior.model_dir, 'averaged')).cuda()
        shipped.load(device='cuda')
        assert shipped._resume_state is None
        for p, off in zip(prior.flat.params, prior.flat.offsets):
            k = next(k for k, v in prior.state_dict().items() if v.data_ptr() == p.data_ptr())
            assert torch.equal(shipped.state_dict()[k].reshape(-1), prior.weight_average()[off:off + p.numel()]), k
        assert not torch.equal(shipped.state_dict()['linear.weight'], prior.state_dict()['linear.weight'])


# ---- 5. two ranks -------------------------------------------------------------------------------------------------------------
def test_two_ranks_on_this_gpu_keep_identical_averages(tmp_path):
    """The harness of tests/test_multigpu_gpu.py (two ranks on device 0, gloo): every rank averages its own replica with no
    communication -- the same collectives as without averaging -- and the replicas' averages are bit-identical."""
    from test_multigpu_gpu import _free_port
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', VQCPC_DP_SHARE_GPU='1', VQCPC_DP_BACKEND='gloo',
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(ROOT, 'tests', 'multigpu_weight_average_worker.py'), str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [torch.load(tmp_path / f'w{k}.pt') for k in range(2)]
    for k, x in enumerate(res):
        assert x['world'] == 2 and x['rank'] == k
        assert x['replays'] >= 3 and x['restatement_ok'] and x['raw_equal_off']
        assert x['collectives_on'] == x['collectives_off'] and sum(x['collectives_on'].values()) > 0
        assert x['avg_digest'] != x['param_digest']
    assert res[0]['avg_digest'] == res[1]['avg_digest'] and res[0]['param_digest'] == res[1]['param_digest']
    assert res[0]['val_inside'] == res[1]['val_inside']
