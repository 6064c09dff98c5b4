"""Optimiser state of another size (training.FlatTraining._apply_resume_state): all four trainers ignore it alike -- the
message, a fresh Adam and schedule, no state kept for a later init_optimizers -- and then train.  Each trainer is built at the
tiny configuration of its own test module, steps twice and saves; a second one whose feed-forward width is doubled (so its
flat buffer has another size) keeps its own model files, gets the first one's optimiser file and loads.  Last, the student's
saved state is its three optimisers' moments in flat order."""
import json
import shutil

import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy
MESSAGE = 'optimizer state ignored: parameter count differs from the checkpoint'


@pytest.fixture(autouse=True)
def training_gemm_mode():
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1)
    yield
    hip.set_gemm_mode(0)


def _cpc(wide):
    from test_trainer_gpu import build_trainer, golden_cfg_sd
    g = load_golden('epoch_tiny')
    cfg, sd = golden_cfg_sd(g)
    batch = {k.split('/', 1)[1]: T(v) for k, v in g.items() if k.startswith('batch/')}
    tr = build_trainer(dict(cfg, ff=2 * cfg['ff']), {}) if wide else build_trainer(cfg, sd)
    return tr, (lambda: tr.train_step(batch, train=True)['loss']), dict(lr=1e-3, schedule_lr=False)


def _student(wide):
    from oracle import student_oracle as S
    from test_student_host_cpu import _build
    g = load_golden('student_tiny')
    cfg = S.make_cfg(**json.loads(str(g['cfg_json'])))
    tr = _build(dict(cfg, ff=2 * cfg['ff']) if wide else cfg).to('cuda')
    tr.init_optimizers(lr=1e-3, schedule_lr=False)
    batch = {'x': T(g['batch/x'])}
    return tr, (lambda: tr.train_step(batch, train=True, masked_event_index=3)['loss_encdec']), dict(lr=1e-3, schedule_lr=False)


def _decoder(wide):
    from oracle import decoder_oracle as D
    from test_decoder_gpu import seeded_decoder
    cfg = D.make_cfg(vocab=[12, 12, 12, 12], emb=16, d=32, H=2, layers=[1, 1], ff=64, D=8, K=16, ncb=1, zdim=8, up_hidden=16,
                     Kl=2, Kr=2, events=16, B=8, dec_d=64, dec_H=2, dec_enc_layers=1, dec_dec_layers=2,
                     dec_ff=256 if wide else 128)
    dec, _ = seeded_decoder(cfg, 11)
    gen = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randint(0, 12, (8, 16, 1), generator=gen) for _ in range(4)], dim=2)
    return dec, (lambda: dec.train_step({'x': x}, train=True)), dict(lr=1e-3, schedule_lr=False)


def _prior(wide):
    from test_prior_cpu import build_prior
    from test_prior_gpu import _batches, _golden_prior
    prior, cfg, _ = _golden_prior('v32')
    if wide:
        prior = build_prior(dict(cfg, p_ff=2 * cfg['p_ff'])).cuda()
    prior.init_optimizers(lr=1e-3)
    batch = _batches(cfg, 1, seed=1)[0]
    return prior, (lambda: prior.train_step(batch, train=True)), dict(lr=1e-3)


# builder, the arguments of save() and load(), the optimiser file under the directory that save() writes
TRAINERS = {'cpc': (_cpc, dict(early_stopped=False), 'overfitted/optimizer'),
            'student': (_student, dict(early_stopped=False), 'overfitted/optimizer'),
            'decoder': (_decoder, dict(early_stopped=False), 'overfitted/decoder_optimizer'),
            'prior': (_prior, {}, 'prior_optimizer')}


def _set_model_dir(tr, path):
    tr.model_dir = tr.encoder.model_dir = str(path)


@pytest.mark.parametrize('name', list(TRAINERS))
def test_optimizer_state_of_another_size_is_ignored(name, tmp_path, capsys):
    build, how, opt_file = TRAINERS[name]
    a, step_a, _ = build(wide=False)
    a.train()
    _set_model_dir(a, tmp_path / 'a')
    for _ in range(2):
        step_a()
    a.save(**how)
    saved = torch.load(tmp_path / 'a' / opt_file)
    assert int(saved['global_step']) == 2 and float(saved['m'].abs().max()) > 0

    b, step_b, init = build(wide=True)
    _set_model_dir(b, tmp_path / 'b')
    b.save(**how)                                              # b's own model files ...
    shutil.copy(tmp_path / 'a' / opt_file, tmp_path / 'b' / opt_file)      # ... next to a's optimiser state
    b.load(device='cuda', **how)
    assert b._resume_state is not None and b._resume_state['m'].numel() == a.flat.numel != b.flat.numel
    capsys.readouterr()
    b.init_optimizers(**init)
    assert capsys.readouterr().out.count(MESSAGE) == 1
    assert b._resume_state is None and b.global_step == 0
    for opt in b._graph_optimizers():
        assert opt.step_count == 0 and float(opt.m.abs().max()) == 0.0 and float(opt.v.abs().max()) == 0.0
    b.init_optimizers(**init)                                  # nothing is kept for a later call
    assert MESSAGE not in capsys.readouterr().out
    b.train()
    loss = step_b()
    assert bool(torch.isfinite(loss)) and b.global_step == 1
    assert all(opt.step_count == 1 and float(opt.m.abs().max()) > 0 for opt in b._graph_optimizers())


def test_student_state_is_the_three_optimizers_in_flat_order(tmp_path):
    tr, step, _ = _student(wide=False)
    tr.train()
    _set_model_dir(tr, tmp_path)
    for _ in range(2):
        step()
    tr.save(early_stopped=False)
    st = torch.load(tmp_path / 'overfitted/optimizer')
    assert st['m'].numel() == st['v'].numel() == tr.flat.numel and int(st['step']) == 2
    opts = [tr.optimizer_teacher, *tr.optimizer_enc_dec]
    assert all(o is p for o, p in zip(opts, tr._graph_optimizers())) and len(tr._graph_optimizers()) == 3
    for opt, module in zip(opts, [tr.teacher, tr.auxiliary_decoder, tr.encoder]):
        lo, hi = tr.flat.range_of(module)
        assert float(opt.m.abs().max()) > 0
        assert torch.equal(st['m'][lo:hi].cuda(), opt.m) and torch.equal(st['v'][lo:hi].cuda(), opt.v)
