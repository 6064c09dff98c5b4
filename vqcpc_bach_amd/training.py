"""The host side of a training step, once, for the four trainers (VQCPCEncoderTrainer, StudentEncoderTrainer,
decoders.Decoder, priors.PriorRelative): flat parameters, a per-rank dropout-seed stream, forward under
`ops.forward_arithmetic`, zero_grad, backward under `ops.direct_weight_gradients`, ONE all-reduce, clip + Adam, graph replay
or the eager fallback, the resume state, and the epoch loop of `train_model`.  No counterpart in the reference, whose trainers
each spell their own loop.  DESIGN.md ("The step protocol") says what a new trainer has to supply.
"""
import contextlib
import os
from itertools import islice

import torch

from . import hip, ops
from .graphs import GraphedTraining, StepGraph, dp_graph_mode
from .parallel import DataParallelContext, FlatParameters
from .utils import SEEDS, dict_pretty_print


def checkpoint_dir(model_dir, early_stopped):
    return f'{model_dir}/early_stopped' if early_stopped else f'{model_dir}/overfitted'


class FlatTraining(GraphedTraining):
    flat = None             # parallel.FlatParameters, set by init_optimizers
    dp = None
    optimizer = None        # the trainer's ops.FlatAdam when it has one (else it overrides _graph_optimizers)
    lr = None
    schedule_lr = False
    global_step = 0
    is_main = True
    _resume_state = None    # what `load` found next to the checkpoint, until init_optimizers applies it
    _avg = None             # weight averaging (opt-in): dict(decay, buf = the average of the whole flat buffer) while it is on
    _avg_resume = None      # the checkpoint's average, until enable_weight_averaging continues it
    _avg_inside = False     # inside averaged_weights(): the flat buffer holds the average
    _avg_saving = False     # inside save_averaged(): weights only

    @staticmethod
    def lr_lambda(step):
        """init_optimizers' LambdaLR factor (vqcpc_encoder_trainer.py:96-107, decoders/decoder.py:237-249): linear warm-up
        0.1 -> 1 over 10 000 steps, then a 10x slower linear decay, floored at 0.1."""
        warmup, lo, hi = 10000, 0.1, 1.0
        s1 = (hi - lo) / warmup
        return max(min(lo + s1 * step, hi + (step - warmup) * (-s1 * 0.1)), lo)

    def current_lr(self):
        return self.lr * (self.lr_lambda(self.global_step) if self.schedule_lr else 1.0)

    def _dir(self, early_stopped):
        return checkpoint_dir(self.model_dir, early_stopped)

    def _init_flat(self, owners, device, dp=None):
        """The head of every init_optimizers: `owners` (modules / parameters, in flat order) become self.flat, identical on
        every rank of self.dp."""
        assert device.type == 'cuda', 'call .to(device) first: the training step has no CPU path'
        self.dp = dp if dp is not None else (self.dp or DataParallelContext(device=device))
        self.is_main = self.dp.rank == 0
        SEEDS.set_rank(self.dp.rank)            # per-rank dropout masks, whatever the launcher seeded
        self.flat = FlatParameters(owners)
        self.dp.broadcast_(self.flat.flat, src=0)                       # identical replicas
        self._avg = self._avg_resume = None     # an average of an earlier flat buffer is not an average of this one

    # ---- optimiser state: an extension over the reference, which restarts Adam and the LR schedule on every resume
    # (SURVEY.md section 5).  `save` writes it, `load` stashes it, init_optimizers applies it once the flat buffers exist ----
    def _graph_optimizers(self):
        """The step's ops.FlatAdam objects, in flat order."""
        return [self.optimizer]

    def _save_optimizer_state(self, path):
        opts = self._graph_optimizers()
        if opts[0] is None:                     # before init_optimizers: nothing to save
            return
        if self._avg_saving:                    # averaged/ holds weights only
            return
        cat = (lambda ts: ts[0]) if len(opts) == 1 else torch.cat
        state = dict(m=cat([o.m for o in opts]), v=cat([o.v for o in opts]), step=opts[0].step_count,
                     global_step=self.global_step, dropout_stream=self.dropout_stream_state())
        if self._avg is not None:
            state.update(avg=self._avg['buf'], avg_decay=self._avg['decay'], avg_t0=opts[0].avg_t0)
        torch.save(state, path)

    def _load_optimizer_state(self, path, map_location):
        self._resume_state = torch.load(path, map_location=map_location) if os.path.exists(path) else None

    def _apply_resume_state(self):
        st, self._resume_state = self._resume_state, None
        if st is None:
            return
        opts = self._graph_optimizers()
        if 'avg' in st:
            self._avg_resume = {k: st[k] for k in ('avg', 'avg_decay', 'avg_t0')}
        if st['m'].numel() != sum(o.m.numel() for o in opts):
            print('optimizer state ignored: parameter count differs from the checkpoint')
            return
        a = 0
        for o in opts:
            b = a + o.m.numel()
            o.m.copy_(st['m'][a:b])
            o.v.copy_(st['v'][a:b])
            o.step_count = int(st['step'])
            a = b
        self.global_step = int(st['global_step'])
        self.restore_dropout_stream(st.get('dropout_stream'))

    # ---- weight averaging (opt-in; no counterpart in the reference): an exponential moving average of the flat parameters,
    # one launch after each optimiser's Adam launch (ops.FlatAdam.enable_average); the training trajectory never reads it ----
    def enable_weight_averaging(self, decay=0.999):
        """Call after init_optimizers.  From the next training step on self.weight_average() follows the parameters with
        d_u = min(decay, (1 + u) / (10 + u)) at its u-th update; after a `load` whose optimiser state holds an average, that
        average is continued.  Buffers outside the flat parameters (EMA codebooks: averages already) are not covered."""
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f'weight_average: decay must be in [0, 1), got {decay}')
        opts = self._graph_optimizers()
        assert self.flat is not None and opts[0] is not None, 'call init_optimizers first'
        if self._avg_inside:
            raise RuntimeError('enable_weight_averaging inside averaged_weights()')
        flat = self.flat.flat
        buf, t0 = flat.clone(), None
        st, self._avg_resume = self._avg_resume, None
        if st is not None:
            if st['avg'].numel() != flat.numel():
                print('weight average ignored: parameter count differs from the checkpoint')
            else:
                buf.copy_(st['avg'])
                t0 = int(st['avg_t0'])
        for o in opts:                          # every optimiser averages its own slice of the one buffer
            a = (o.p.data_ptr() - flat.data_ptr()) // 4
            o.enable_average(decay, avg=buf[a:a + o.p.numel()], t0=t0)
        self._avg = dict(decay=decay, buf=buf)
        self._release_step_graph()
        return self

    def disable_weight_averaging(self):
        if self._avg_inside:
            raise RuntimeError('disable_weight_averaging inside averaged_weights()')
        for o in self._graph_optimizers():
            if o is not None:
                o.disable_average()
        self._avg = None
        self._release_step_graph()
        return self

    def _release_step_graph(self):
        """A captured step holds the launches of the configuration it was captured in: the next replayable step captures anew,
        after the eager warm-up steps of a first capture (a capture taken right after a replay of the released graph gave the
        decoder and the prior a wrong gradient from its second replay on; after two eager steps it replays the eager steps bit
        for bit)."""
        if self._graph is not None:
            self._graph.release()
            self._graph = None
            self._graph_eager_steps = 0

    def weight_average(self):
        """The average of the flat parameter buffer (the live tensor, flat order), or None when averaging is off."""
        return None if self._avg is None else self._avg['buf']

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside, the flat parameter buffer HOLDS the average (copied in place: every parameter view and every captured
        generation graph keeps its address) and the raw weights wait in a scratch buffer; on exit they are back bit for bit.
        Both copies bump ops._PARAM_STEPS, as an optimiser step does: no f16x3 plane image made from one set of weights is
        paired with the other.  A training step inside, or a nested context, raises RuntimeError."""
        if self._avg is None:
            raise RuntimeError('averaged_weights(): weight averaging is not enabled')
        if self._avg_inside:
            raise RuntimeError('averaged_weights() does not nest')
        flat = self.flat.flat
        parked = flat.clone()
        flat.copy_(self._avg['buf'])
        ops._PARAM_STEPS += 1
        self._avg_inside = True
        try:
            yield self
        finally:
            flat.copy_(parked)
            ops._PARAM_STEPS += 1
            self._avg_inside = False

    def _checkpoint_owners(self):
        """The objects whose `model_dir` the trainer's `save` writes under."""
        return [self]

    def _save_averaged_with(self, save):
        owners = self._checkpoint_owners()
        dirs = [o.model_dir for o in owners]
        with contextlib.ExitStack() as stack:
            if not self._avg_inside:
                stack.enter_context(self.averaged_weights())
            self._avg_saving = True
            try:
                for o, d in zip(owners, dirs):
                    o.model_dir = f'{d}/averaged'
                save()
            finally:
                for o, d in zip(owners, dirs):
                    o.model_dir = d
                self._avg_saving = False

    def save_averaged(self, *args, **kwargs):
        """The trainer's own `save(*args, **kwargs)` under the averaged weights, into `{model_dir}/averaged/`: the same relative
        layout and file names, weights only (no optimiser state).  A model built with model_dir=.../averaged loads them with
        `load` as always."""
        self._save_averaged_with(lambda: self.save(*args, **kwargs))

    # ---- one step ------------------------------------------------------------------------------------------------
    def _forward_backward(self, forward, tag=None, zero_grad=True):
        """forward() -> (loss, outputs), run under the training step's forward arithmetic whatever the caller's ambient grad
        mode; then zero_grad (unless the caller has done it: a second pass of one step adds to the bucket), then backward
        straight into the flat gradient bucket.  Returns `outputs`; forward() detaches what it puts there, because a step
        output that keeps the autograd graph alive breaks the next capture (graphs.py).  tag: several passes per step over one
        flat buffer own one f16x3 scale table each."""
        with torch.enable_grad(), ops.forward_arithmetic(self.flat, tag=tag):
            loss, out = forward()
        if zero_grad:
            self.flat.zero_grad()
        with ops.direct_weight_gradients(self.flat, tag=tag):
            loss.backward()
        return out

    def _all_reduce_gradients(self):
        self.dp.all_reduce_sum_(self.flat.flat_grad)

    def _step_apply(self, out):
        """clip + Adam on the (all-reduced) flat gradient; the rank sum becomes a mean inside the kernels."""
        lr, scale = self.current_lr(), 1.0 / self.dp.world_size
        for opt in self._graph_optimizers():
            opt.step(lr=lr, grad_scale=scale)
        return out

    def _train_step_body(self, batch, *args):
        """Everything a step enqueues on the device: compute, ONE all-reduce of the gradient bucket, apply."""
        out = self._step_compute(batch, *args)
        self._all_reduce_gradients()
        return self._step_apply(out)

    # ---- the step as graph replays (graphs.StepGraph) ------------------------------------------------------------------
    def _graph_key(self, batch):
        return None

    def _dp_stages(self):
        """(stages, betweens) of the multi-rank step: by default [compute, apply] around ONE all-reduce of the flat gradient
        bucket.  A trainer whose step has independent halves overrides this (student: bucketed all-reduces)."""
        return [self._step_compute, self._step_apply], [self._all_reduce_gradients]

    def _new_step_graph(self):
        stages, betweens = [self._train_step_body], []
        if self.dp.distributed and not (dp_graph_mode() == 'capture' and self.dp.backend == 'nccl'):
            stages, betweens = self._dp_stages()
        return StepGraph(stages, betweens, self._graph_optimizers(), self.current_lr, self.flat.flat.device, key_fn=self._graph_key)

    def _graphed_step(self, batch):
        """Returns the step's outputs from a graph replay, or None when this step has to run eagerly."""
        if not self._graph_on:
            return None
        if self.dp.distributed and dp_graph_mode() == 'off':
            return None
        if self._graph_eager_steps < self.graph_warmup_steps:
            self._graph_eager_steps += 1
            return None
        if self._graph is None:
            self._graph = self._new_step_graph()
        try:
            return self._graph(batch)
        except RuntimeError as e:
            # a failed CAPTURE (e.g. a runtime that cannot record one of the step's calls) must not take the training run
            # down: fall back to eager steps for good and say so once.  Errors of a replayed step are real errors.
            if self._graph.replays > 0:
                raise
            import warnings
            warnings.warn(f'step-graph capture failed ({str(e)[:200]}); continuing with eager steps')
            torch.cuda.synchronize()
            hip.clear_runtime_error()       # the failed capture's HIP error must not be reported by the next kernel launch check
            self._graph_on = False
            self._graph.release()
            self._graph = None
            return None

    def _train_step(self, batch, *args, eager=False):
        """The training half of `train_step`: a replay of the captured step (graphs.py) once the first eager steps have done
        the lazy initialisations, unless this step must be `eager`; *args go to the eager `_train_step_body`."""
        if self._avg_inside:
            raise RuntimeError('training step inside averaged_weights(): the flat buffer holds the average, not the weights')
        out = None
        with SEEDS.stream_of(self):            # this trainer's own dropout-seed stream (utils.DropoutSeeds.stream_of)
            if not eager:
                out = self._graphed_step(batch)
            if out is None:
                out = self._train_step_body(batch, *args)
        self.global_step += 1
        return out

    # ---- epochs --------------------------------------------------------------------------------------------------
    def _report_scale_saturation(self, means):
        """End of a TRAINING epoch, every trainer (the host has just synchronised for the metric means): the f16x3 scale tables of
        this trainer's flat parameters are asked whether a tensor outgrew the 16-32 x head-room of its previous-step scale (its
        largest elements were clamped to 65504 / scale for that ONE step -- in a forward product that can move a loss or a code
        assignment of that step; the next step already runs under the followed scale).  `means['f16x3_scale_saturations']` = the
        number of (call site, operand) pairs it happened to during THIS epoch (0.0 in every run of this repository); when non-zero
        the marked step indices are logged through `warnings` and kept in `self.scale_saturation_log`."""
        if self.flat is None or not getattr(self.flat, '_grad_scales', None):
            return means
        total = ops.scale_saturations(self.flat)
        seen = getattr(self, '_scale_saturations_seen', 0)
        means['f16x3_scale_saturations'] = float(total - seen)
        if total > seen:
            import warnings
            rep = ops.scale_saturation_report(self.flat)
            self.scale_saturation_log = rep
            warnings.warn(f'f16x3 GEMM arithmetic: {total - seen} operand tensors outgrew the fp16 range under their previous-step scale '
                          f'during this epoch (clamped for one step each; marked steps by scale table: '
                          f'{ {k: v["step_indices"] for k, v in rep.items()} }); '
                          'ops.set_gradient_arithmetic("six") / ops.set_forward_arithmetic("six") select the scale-free arithmetic')
            self._scale_saturations_seen = total
        return means

    def _scalar_loss_epoch(self, data_loader, train, num_batches, data_processors):
        """`epoch` of a trainer whose step returns its loss: the mean over batches and ranks, one host sync;
        data_processors: those whose out-of-range-token flag is read afterwards."""
        self.train() if train else self.eval()
        total = torch.zeros((), dtype=torch.float32, device=self.flat.flat.device)
        n = 0
        for tensor_dict in islice(data_loader, num_batches):
            total += self.train_step(tensor_dict, train=train)
            n += 1
        total /= max(n, 1)
        if self.dp.distributed:
            self.dp.all_reduce_sum_(total)
            total /= self.dp.world_size
        means = {'loss': float(total.item())}                    # the host sync of the epoch
        for dproc in data_processors:
            dproc.raise_if_bad_tokens(dp=self.dp)
        if train:
            self._report_scale_saturation(means)
        return means

    @contextlib.contextmanager
    def _training_defaults(self):
        """Around the body of `train_model`: bf16x6 GEMMs + step-graph replay unless the caller chose otherwise
        (`use_training_defaults`).  The GEMM arithmetic is a process-wide setting: a caller who chose nothing gets back what was
        there before (evaluation / generation code that runs after training sees the mode it would have seen without it)."""
        mode_before, arith_before = hip.gemm_mode_state(), ops.gradient_arithmetic_state()
        self.use_training_defaults()
        self.trained_gemm_mode = hip.get_gemm_mode()        # what the epochs run in (0 fp32 MFMA / 1 bf16x6 / 2 bf16)
        try:
            yield
        finally:
            hip.restore_gemm_mode_state(mode_before)
            ops.restore_gradient_arithmetic_state(arith_before)

    def _train_epochs(self, batch_size, num_batches, num_epochs, num_workers, monitor, save_best, save_every=None,
                      after_epoch=None, **epoch_kwargs):
        """The epoch loop of `train_model` (encoder.py:244-325, decoders/decoder.py:354-429, priors/prior_relative.py:243-306).
        monitor: the key of the validation means that selects the best epoch; rank 0 calls save_every() after every epoch and
        save_best() after the best one so far (the trainer's `save` with the arguments it takes).
        after_epoch(epoch_id, train means, val means): rank 0's hook (plots); epoch_kwargs go to `epoch`."""
        best_val = 1e8
        history = []
        for epoch_id in range(num_epochs):
            gen_train, gen_val, _ = self.dataloader_generator.dataloaders(batch_size=batch_size, num_workers=num_workers)
            train = self.epoch(data_loader=gen_train, train=True, num_batches=num_batches, **epoch_kwargs)
            del gen_train
            # with weight averaging on, the best epoch is chosen by the weights a user would ship
            with self.averaged_weights() if self._avg is not None else contextlib.nullcontext():
                val = self.epoch(data_loader=gen_val, train=False,
                                 num_batches=num_batches // 2 if num_batches is not None else None, **epoch_kwargs)
            del gen_val
            if self.is_main:
                print(f'======= Epoch {epoch_id} =======')
                print('---Train---')
                dict_pretty_print(train, endstr=' ' * 5)
                print()
                print('---Val---')
                dict_pretty_print(val, endstr=' ' * 5)
                print('\n')
                if save_every is not None:
                    save_every()
                    if self._avg is not None:
                        self._save_averaged_with(save_every)
                if val[monitor] < best_val:
                    save_best()
                    if self._avg is not None:
                        self._save_averaged_with(save_best)
                    best_val = val[monitor]
                if after_epoch is not None:
                    after_epoch(epoch_id, train, val)
            history.append((train, val))
        return history
