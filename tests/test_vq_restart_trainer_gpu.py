"""Dead-code restarts end to end: VQCPCEncoderTrainer with quantizer_type 'ema' and ema_restart_threshold on the C0-sized
configuration of tests/test_vq_ema_trainer_gpu.py (two codebooks, no dropout).  The feature copies rows of the step's quantiser
input and sets constants: every comparison is on the bits, against tests/vq_restart_reference.py."""
import numpy as np
import pytest
import torch

import vq_restart_reference as Rr
from test_vq_ema_trainer_gpu import batches, buffers, same

pytestmark = pytest.mark.gpu

TODAY = {'loss', 'accuracy', 'loss_quantize', 'loss_contrastive', 'num_codewords', 'num_codewords_negative', 'loss_monitor'}


@pytest.fixture(scope='module', autouse=True)
def _mode():
    from vqcpc_bach_amd import hip
    hip.load()
    hip.set_gemm_mode(1)
    yield
    hip.set_gemm_mode(0)


def build(model_dir, seed=11, lr=1e-3, initialize=False, **restart):
    """build() of tests/test_vq_ema_trainer_gpu.py with the restart keys passed through make_config."""
    from vqcpc_bach_amd import configs, getters
    torch.manual_seed(seed)
    config = configs.make_config('C0', dropout=0.0, quantizer_type='ema', **restart)
    config['quantizer_kwargs'].update(num_codebooks=2, initialize=initialize)
    dlg = getters.get_dataloader_generator('bach', 'vqcpc', dict(config['dataloader_generator_kwargs'], device='cuda'))
    enc = getters.get_encoder(str(model_dir), dlg, config)
    tr = getters.get_encoder_trainer(str(model_dir), dlg, 'vqcpc', enc, config['auxiliary_networks_kwargs'])
    tr.to('cuda')
    tr.init_optimizers(lr=lr, schedule_lr=False)
    return tr, dlg


class CallLog:
    """Names of the hip.call entry points issued inside the block."""

    def __enter__(self):
        from vqcpc_bach_amd import hip
        self.hip, self.raw, self.names = hip, hip.call, []

        def rec(name, *args):
            self.names.append(name)
            return self.raw(name, *args)
        hip.call = rec
        return self

    def __exit__(self, *exc):
        self.hip.call = self.raw


def quantizer_input(tr, batch):
    """z of the merged pass [negatives | left | right] with the trainer's present weights, from an evaluation step."""
    rec = {}
    q = tr.encoder.quantizer
    h = q.register_forward_hook(lambda mod, args, out: rec.update(z=args[0].detach().reshape(-1, mod.codebook_dim).clone()))
    tr.eval()
    tr.train_step(batch, train=False)
    h.remove()
    tr.train()
    return rec['z']


def kill_odd_codes(q):
    """Half of the codes far away from any data, with the cluster size of a code that has had no row for 230 steps."""
    with torch.no_grad():
        q.embeddings[:, 1::2] += 1000.0
        q.ema_sum[:, 1::2] = q.embeddings[:, 1::2]
        q.ema_cluster_size[:, 1::2] = 0.1


def test_dead_codes_come_back_as_rows_of_the_steps_encoder_outputs(tmp_path):
    seed = 0x1234567812345678
    tr, dlg = build(tmp_path / 'a', ema_restart_threshold=0.5, ema_restart_seed=seed)
    plain, _ = build(tmp_path / 'b')
    q, pq = tr.encoder.quantizer, plain.encoder.quantizer
    assert q.restarting and not pq.restarting and torch.equal(tr.flat.flat, plain.flat.flat) and same(buffers(q), buffers(pq))
    kill_odd_codes(q), kill_odd_codes(pq)
    b = batches(dlg, 1)[0]
    z = quantizer_input(tr, b)
    before = buffers(q)
    means = tr.epoch(iter([b]), train=True, num_batches=1, corrupt_labels=False)
    plain.train()
    plain.train_step(b, train=True)
    torch.cuda.synchronize()
    ncb, K, dsub = q.embeddings.shape
    dead = torch.zeros(ncb, K, dtype=torch.bool, device='cuda')
    dead[:, 1::2] = True
    e, N, m = buffers(q)
    pe, pN, pm = buffers(pq)
    assert bool((pN[dead] < 0.5).all()) and bool((pN[~dead] >= 0.5).all()), 'the plain EMA step leaves exactly the odd codes dead'
    # every other cell holds what the plain EMA step gives
    for got, want in ((e, pe), (N, pN), (m, pm)):
        assert same([got[~dead]], [want[~dead]])
    # the dead codes: sub-vector c of the row of z the reference names for step 1 (Adam's t of the first step), one rank
    want = torch.from_numpy(Rr.candidates([z.cpu().numpy()], seed, 1, ncb, K)[0]).cuda()
    assert same([q.restart_rows], [want]), 'the candidates of the step are rows of the z an evaluation pass gives'
    assert same([e[dead]], [want[dead]]) and same([m[dead]], [want[dead]]) and bool((N[dead] == 1.0).all())
    assert not same([e[dead]], [before[0][dead]])
    assert means['codebook_restarts'] == [K // 2] * ncb and q.restarts.tolist() == [K // 2] * ncb
    ppl = means['codebook_perplexity']
    assert len(ppl) == ncb and all(np.isfinite(v) and 1.0 <= v <= K * (1 + 1e-5) for v in ppl), ppl
    assert TODAY <= set(means)
    # an evaluation epoch reports today's keys, and the next training epoch starts its count at zero
    assert set(tr.epoch(iter([b]), train=False, num_batches=1, corrupt_labels=False)) == TODAY
    means = tr.epoch(iter([b]), train=True, num_batches=1, corrupt_labels=False)
    assert means['codebook_restarts'] == [0] * ncb, 'restarted codes have 70 steps of grace'


def test_off_is_off(tmp_path):
    absent, dlg = build(tmp_path / 'a')
    zero, _ = build(tmp_path / 'b', ema_restart_threshold=0)
    assert not hasattr(zero.encoder.quantizer, 'restart_rows') and zero.encoder.quantizer.restart_context is None
    bs = batches(dlg, 3)
    logs = []
    for tr in (absent, zero):
        tr.train()
        with CallLog() as log:
            for b in bs:
                tr.train_step(b, train=True)
        torch.cuda.synchronize()
        logs.append(log.names)
    assert logs[0] == logs[1] and 'vqcpc_vq_ema_update' in logs[0]
    assert 'vqcpc_vq_restart_candidates' not in logs[0] and 'vqcpc_vq_ema_restart' not in logs[0]
    assert same(buffers(absent.encoder.quantizer), buffers(zero.encoder.quantizer)) and same([absent.flat.flat], [zero.flat.flat])
    for tr in (absent, zero):
        means = tr.epoch(iter(bs[:1]), train=True, num_batches=1, corrupt_labels=False)
        assert set(means) - {'f16x3_scale_saturations'} == TODAY
    # ... and with the option on the step has exactly the two launches more, after the update
    on, _ = build(tmp_path / 'c', ema_restart_threshold=0.5)
    on.train()
    with CallLog() as log:
        on.train_step(bs[0], train=True)
    names = [n for n in log.names if n not in ('vqcpc_vq_restart_candidates', 'vqcpc_vq_ema_restart')]
    assert names == logs[0][:len(names)] and len(log.names) == len(names) + 2
    assert log.names.index('vqcpc_vq_ema_restart') == log.names.index('vqcpc_vq_ema_update') + 1
    assert log.names.index('vqcpc_vq_ema_update') > log.names.index('vqcpc_adam_step'), 'after Adam'
    assert log.names.index('vqcpc_vq_restart_candidates') == log.names.index('vqcpc_vq_ema_stats') + 1, 'next to the statistics'


def test_replayed_steps_are_the_eager_steps_and_draw_new_rows_every_step(tmp_path):
    """Five steps (two eager warm-up steps, three replays) at a threshold of 1, which restarts every code that misses a single
    step.  As in tests/test_vq_ema_trainer_gpu.py the eager twin starts each step from the replayed trainer's state; after the
    step the three EMA buffers, the flat parameters, the candidates and the restart counts are bit-identical."""
    tr, dlg = build(tmp_path / 'a', ema_restart_threshold=1.0, ema_restart_seed=5)
    twin, _ = build(tmp_path / 'b', ema_restart_threshold=1.0, ema_restart_seed=5)
    tr.train(), twin.train()
    tr.enable_step_graph(True)
    q, tq = tr.encoder.quantizer, twin.encoder.quantizer
    bs = batches(dlg, 5)
    rows, counts = [], []
    try:
        for i, b in enumerate(bs):
            twin.flat.flat.copy_(tr.flat.flat)
            twin.optimizer.m.copy_(tr.optimizer.m)
            twin.optimizer.v.copy_(tr.optimizer.v)
            twin.optimizer.step_count = tr.optimizer.step_count
            for dst, src in zip(tq.ema_buffers(), q.ema_buffers()):
                dst.copy_(src)
            q.restarts.zero_(), tq.restarts.zero_()
            tr.train_step(b, train=True)
            twin.train_step(b, train=True)
            torch.cuda.synchronize()
            assert same(buffers(q), buffers(tq)), i
            assert same([tr.flat.flat], [twin.flat.flat]), i
            assert same([q.restart_rows], [tq.restart_rows]) and q.restarts.tolist() == tq.restarts.tolist(), i
            rows.append(q.restart_rows.clone())
            counts.append(int(q.restarts.sum()))
        assert tr._graph is not None and tr._graph.replays == 3 and len(tr._graph.stages) == 1, 'one graph per step on one rank'
        assert twin._graph is None
    finally:
        tr.enable_step_graph(False)
    assert sum(c > 0 for c in counts) >= 3 and sum(c > 0 for c in counts[2:]) >= 2, counts
    # the replays drew new rows every step: the step count is read on the device, not frozen in the captured arguments
    # (and the count it reads is the host's: the eager twin, which passes Adam's t as an argument, drew the same rows above)
    assert not same([rows[2]], [rows[3]]) and not same([rows[3]], [rows[4]])
    assert tr.optimizer.step_count == 5


def test_checkpoints_are_interchangeable_with_and_without_the_option(tmp_path):
    on, dlg = build(tmp_path / 'a', ema_restart_threshold=0.5)
    on.train()
    for b in batches(dlg, 2):
        on.train_step(b, train=True)
    on.save(early_stopped=False)
    off, _ = build(tmp_path / 'a', seed=12)
    assert not same(buffers(on.encoder.quantizer), buffers(off.encoder.quantizer))
    off.load(early_stopped=False, device='cuda')
    assert same(buffers(on.encoder.quantizer), buffers(off.encoder.quantizer))
    off.train()
    off.train_step(batches(dlg, 1)[0], train=True)
    off.save(early_stopped=False)
    back, _ = build(tmp_path / 'a', seed=13, ema_restart_threshold=0.5)
    back.load(early_stopped=False, device='cuda')
    assert same(buffers(off.encoder.quantizer), buffers(back.encoder.quantizer))
    sd_on, sd_off = on.encoder.quantizer.state_dict(), off.encoder.quantizer.state_dict()
    assert sorted(sd_on) == sorted(sd_off)
    off.encoder.quantizer.load_state_dict(sd_on, strict=True)
    on.encoder.quantizer.load_state_dict(sd_off, strict=True)
    back.init_optimizers(lr=1e-3, schedule_lr=False)
    back.train()
    out = back.train_step(batches(dlg, 1)[0], train=True)
    assert np.isfinite(float(out['loss']))
