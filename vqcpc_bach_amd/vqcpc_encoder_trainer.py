"""VQCPCEncoderTrainer -- the hot path (reference: VQCPCB/vqcpc_encoder_trainer.py:14-354).

One iteration of `epoch()`:
  1. every block of the batch (negatives, [negatives_back,] left, right: R = B (N Kr [x2] + Kl + Kr) blocks) goes through
     the encoder in ONE pass (Encoder.encode_many);
  2. GRU context on z_left, fused bilinear scores + InfoNCE + hits (vqcpc_nce_*), quantisation loss;
  3. backward (hand-scheduled per layer), ONE RCCL all-reduce of the flat gradient, global-norm clip + Adam as two flat
     kernels (no host synchronisation anywhere in the step);
  4. metrics accumulate on the device and are read once at the end of the epoch (the reference syncs 6+ times a step).
"""
import os
from itertools import islice

import numpy as np
import torch

from . import hip, ops, vqcpc_helper
from .encoder import EncoderTrainer
from .utils import STEP_LOCK
from .vqcpc_helper import cpc_scores_and_loss


class VQCPCEncoderTrainer(EncoderTrainer):
    def __init__(self, model_dir, dataloader_generator, encoder, c_net_kwargs, quantization_weighting):
        super().__init__(dataloader_generator=dataloader_generator)
        self.model_dir = model_dir
        self.dataloader_generator = dataloader_generator
        self.encoder = encoder
        self.data_processor = encoder.data_processor
        self.codebook_dim = self.encoder.quantizer.codebook_dim
        self.upscale_factors = list(reversed(self.encoder.downscaler.downscale_factors))
        self.num_tokens_per_channel = self.encoder.data_processor.num_tokens_per_channel
        self.num_channels = len(self.num_tokens_per_channel)
        assert self.data_processor.num_tokens % np.prod(self.upscale_factors) == 0
        z_dim = encoder.upscaler.output_dim if encoder.upscaler is not None else self.codebook_dim
        c_dim = c_net_kwargs['output_dim']
        k_max = self.dataloader_generator.num_blocks_right

        def c_net():
            return vqcpc_helper.CModule(input_dim=z_dim, hidden_size=c_net_kwargs['hidden_size'], output_dim=c_dim,
                                        num_layers=c_net_kwargs['num_layers'], dropout=c_net_kwargs['dropout'])

        self.c_module = c_net()
        self.fks_module = vqcpc_helper.FksModule(z_dim=z_dim, c_dim=c_dim, k_max=k_max)
        # the shipped transformer configs omit 'bidirectional' (defect 2): default to False
        if c_net_kwargs.get('bidirectional', False):
            self.c_module_back = c_net()
            self.fks_module_back = vqcpc_helper.FksModule(z_dim=z_dim, c_dim=c_dim, k_max=k_max)
        else:
            self.c_module_back = None
        self.quantization_weighting = quantization_weighting
        self.scheduler = None

    @property
    def _ema(self):
        """The quantiser when its codebooks are EMA buffers (EMAProductVectorQuantizer), else None."""
        q = self.encoder.quantizer
        return q if hasattr(q, 'apply_update') else None

    @property
    def _restarting(self):
        """True when the EMA quantiser restarts dead codewords (its restart_threshold > 0)."""
        return self._ema is not None and self._ema.restarting

    def _restart_context(self):
        """(step, step_dev, rank, world) for the restart candidates of the step being enqueued.  step is Adam's t of this step:
        the forward runs before optimizer.step() counts it, hence + 1; a captured step reads the device counter instead, which
        the graph's first node has already incremented to the same t."""
        opt = self.optimizer
        capturing = opt._dev is not None and torch.cuda.is_current_stream_capturing()
        return opt.step_count + 1, (opt._dev[1] if capturing else None), self.dp.rank, self.dp.world_size

    # ---- optimiser ---------------------------------------------------------------------------------------------
    def _modules_with_params(self):
        mods = [self.c_module, self.fks_module, self.encoder]
        if self.c_module_back is not None:
            mods += [self.fks_module_back, self.c_module_back]
        return mods

    def init_optimizers(self, lr, schedule_lr, dp=None):
        self._init_flat(self._modules_with_params(), next(self.encoder.parameters()).device, dp)
        if self.dp.distributed:
            self.encoder.quantizer.init_broadcast = lambda tensors: [self.dp.broadcast_(t.data, 0) for t in tensors]
        # EMA codebooks are buffers, not parameters: outside the flat buffer, so rank 0's go to every rank on their own
        if self._ema is not None:
            for t in self._ema.ema_buffers():
                self.dp.broadcast_(t, src=0)
        if self._restarting:
            self._ema.restart_context = self._restart_context
        self.lr, self.schedule_lr = lr, schedule_lr
        self.optimizer = ops.FlatAdam(self.flat.flat, self.flat.flat_grad, lr=lr, max_norm=5.0)
        self.scheduler = self.lr_lambda if schedule_lr else None
        self.global_step = 0
        self._apply_resume_state()

    # ---- checkpoints (:117-151) ----------------------------------------------------------------------------------
    def save(self, early_stopped):
        model_dir = self._dir(early_stopped)
        os.makedirs(model_dir, exist_ok=True)
        self.encoder.save(early_stopped=early_stopped)
        torch.save(self.c_module.state_dict(), f'{model_dir}/c_module')
        torch.save(self.fks_module.state_dict(), f'{model_dir}/fks_module')
        if self.c_module_back is not None:
            torch.save(self.c_module_back.state_dict(), f'{model_dir}/c_module_back')
            torch.save(self.fks_module_back.state_dict(), f'{model_dir}/fks_module_back')
        self._save_optimizer_state(f'{model_dir}/optimizer')

    def load(self, early_stopped, device):
        print(f'Loading models {self.__repr__()}')
        model_dir = self._dir(early_stopped)
        if not os.path.exists(model_dir):
            model_dir = self.model_dir
        ml = torch.device(device)
        self.encoder.load(early_stopped=early_stopped, device=device)
        self.c_module.load_state_dict(torch.load(f'{model_dir}/c_module', map_location=ml))
        self.fks_module.load_state_dict(torch.load(f'{model_dir}/fks_module', map_location=ml))
        if self.c_module_back is not None:
            self.c_module_back.load_state_dict(torch.load(f'{model_dir}/c_module_back', map_location=ml))
            self.fks_module_back.load_state_dict(torch.load(f'{model_dir}/fks_module_back', map_location=ml))
        self._load_optimizer_state(f'{model_dir}/optimizer', ml)

    # ---- one step ------------------------------------------------------------------------------------------------
    def compute_losses(self, tensor_dict, corrupt_labels=False):
        """Forward half of one iteration (:195-307).  Returns (loss, dict of device tensors)."""
        neg = tensor_dict['negative_samples']
        B, N, Kr, num_events, num_channels = neg.shape
        xs = [neg.reshape(B * N * Kr, num_events, num_channels)]
        corrupt = [corrupt_labels]
        bidir = self.c_module_back is not None
        if bidir:
            xs.append(tensor_dict['negative_samples_back'].reshape(B * N * Kr, num_events, num_channels))
            corrupt.append(corrupt_labels)
        xs += [tensor_dict['x_left'], tensor_dict['x_right']]
        corrupt += [False, False]
        enc, ql_rows = self.encoder.encode_many(xs, corrupt, with_loss_rows=True)
        (z_neg, idx_neg, ql_neg) = enc[0]
        (z_left, idx_left, ql_left), (z_right, idx_right, ql_right) = enc[-2], enc[-1]
        zdim = z_neg.shape[-1]
        z_neg = z_neg.reshape(B, N, Kr, -1, zdim)[:, :, :, 0, :]                  # (B, N, K, z), first block (:245)

        c = self.c_module(z_left, h=None)
        contrastive, hits = cpc_scores_and_loss(self.fks_module, c, z_right, z_neg)
        # quantization_loss (vqcpc_helper.py:32-51) sums the per-block losses of EVERY encoder call of the step: one sum over
        # the rows of the merged pass instead of one per segment (and their slice / add backward nodes)
        ql_total = ql_rows.sum()
        n_terms = 3 * B
        hits_back = None
        if bidir:                                                                 # :277-296
            z_nb = enc[1][0]
            # reference quirk kept for parity: the backward negatives are NOT permuted to negative-major before
            # FksModule's raw .view (:286-292), so window b is scored against rows n*B + b of the (B*N, K, z) tensor
            z_nb = z_nb.reshape(B, N, Kr, -1, zdim)[:, :, :, 0, :].reshape(B * N, Kr, zdim)
            z_nb = z_nb.reshape(N, B, Kr, zdim).permute(1, 0, 2, 3)
            c_back = self.c_module_back(z_right.flip(dims=[1]), h=None)
            contrastive_back, hits_back = cpc_scores_and_loss(self.fks_module_back, c_back, z_left, z_nb)
            contrastive = contrastive + contrastive_back
            n_terms = 4 * B                                                       # ql_total already holds the fourth segment
        q_loss = ql_total / n_terms                                               # quantization_loss, helper :32-51
        loss = contrastive + self.quantization_weighting * q_loss
        accuracy = hits.mean(0)
        if hits_back is not None:
            accuracy = (accuracy + hits_back.mean(0)) / 2
        return loss, dict(loss=loss.detach(), loss_contrastive=contrastive.detach(), loss_quantize=q_loss.detach(),
                          accuracy=accuracy, idx_left=idx_left, idx_right=idx_right, idx_negative=idx_neg)

    def _count_codewords(self, *idx_tensors):
        """len(torch.unique(.)) without a host sync: sort + count boundaries.  With a product quantiser
        (num_codebooks > 1, which the reference's epoch() cannot run: SURVEY.md section 0 defect 1) the count is over
        merged code tuples sum_c idx_c K^c -- the number of distinct product codes in use.  Without a quantiser
        (NoQuantization returns encoding_indices None) the counters stay 0, as in the reference (:325)."""
        if any(i is None for i in idx_tensors):
            return torch.zeros((), dtype=torch.float32, device=self.flat.flat.device)
        flat = [i.reshape(-1, i.shape[-1]).contiguous() for i in idx_tensors]
        ncb, K = flat[0].shape[1], int(self.encoder.quantizer.codebook_size)
        if flat[0].is_cuda and len(flat) <= 2 and hip.query('vqcpc_count_distinct_codes_supported', ncb, K):
            # one launch (a bit per possible product code in LDS) instead of cat + sort + compare + sum
            out = torch.empty(1, dtype=torch.float32, device=flat[0].device)
            b = flat[1] if len(flat) == 2 else None
            hip.call('vqcpc_count_distinct_codes', flat[0], flat[0].shape[0], b, 0 if b is None else b.shape[0], ncb, K, out)
            return out[0]
        merged = torch.cat([self.encoder.merge_codes(i) for i in flat])
        s = torch.sort(merged)[0]
        return (s[1:] != s[:-1]).sum().float() + 1.0

    def _step_metrics(self, out):
        """The per-step summands of epoch()'s means as ONE device vector: loss, quantize, contrastive, num_codewords,
        num_codewords_negative, accuracy[k] (vqcpc_encoder_trainer.py:320-340).  Computed inside the step so that a
        captured step (graphs.py) replays it with the rest."""
        return torch.cat([torch.stack([out['loss'], out['loss_quantize'], out['loss_contrastive'],
                                       self._count_codewords(out['idx_left'], out['idx_right']),
                                       self._count_codewords(out['idx_negative'])]), out['accuracy']])

    def _step_compute(self, tensor_dict, corrupt_labels=False):
        """zero_grad / forward / backward (:310-312) + the step's metric vector: everything before the gradient all-reduce."""
        out = self._forward_backward(lambda: self.compute_losses(tensor_dict, corrupt_labels))
        out['metrics'] = self._step_metrics(out)
        return out

    def _step_apply(self, out):
        """clip + Adam (:313-316), then the EMA codebooks' update (and, when asked for, the restart of the dead codewords)."""
        super()._step_apply(out)
        if self._ema is not None:
            self._ema.apply_update()          # EMA codebooks: counts and sums of the step (summed over ranks, not averaged)
        return out

    def _all_reduce_gradients(self):
        """The flat gradient bucket and, with EMA codebooks, the step's per-code counts and sums next to it; with restarts the
        candidate rows too: exactly one rank holds a non-zero row per code, so the sum is that row on every rank."""
        super()._all_reduce_gradients()
        if self._ema is not None:
            self.dp.all_reduce_sum_(self._ema.stats)
            if self._ema.restarting:
                self.dp.all_reduce_sum_(self._ema.restart_rows)

    def train_step(self, tensor_dict, train=True, corrupt_labels=False):
        """One iteration.  Returns device-side metrics.  With `enable_step_graph()` a training step is a HIP-graph replay
        (graphs.py) once the first eager steps have done the lazy initialisations."""
        if not train:
            with STEP_LOCK, torch.no_grad():
                out = self.compute_losses(tensor_dict, corrupt_labels)[1]
                out['metrics'] = self._step_metrics(out)
                return out
        # label corruption is not in the captured step, and the codebooks' data init must have happened before a capture
        return self._train_step(tensor_dict, corrupt_labels, eager=corrupt_labels or self.encoder.quantizer_needs_init())

    def epoch(self, data_loader, train, num_batches, corrupt_labels):
        assert self.optimizer is not None, 'call init_optimizers(lr, schedule_lr) first'
        dev = self.flat.flat.device
        if self.is_main:
            print(f'lr: {self.current_lr()}')
        self.train() if train else self.eval()
        k_r = self.dataloader_generator.num_blocks_right
        sums = torch.zeros(5 + k_r, dtype=torch.float32, device=dev)   # loss, quantize, contrastive, ncw, ncw_neg, acc[k]
        dproc = self.encoder.data_processor
        restarting = train and self._restarting
        if restarting:
            self._ema.restarts.zero_()
        n = 0
        for tensor_dict in islice(data_loader, num_batches):
            out = self.train_step(tensor_dict, train=train, corrupt_labels=corrupt_labels)
            sums += out['metrics']
            n += 1
        sums /= max(n, 1) * self.dp.world_size
        if restarting:
            # every rank holds the same counts and cluster sizes: divided by the world size they ride in the rank sum below
            ncb = self._ema.num_codebooks
            sums = torch.cat([sums, torch.cat([self._ema.restarts.float(), self._ema.codebook_perplexity()]) / self.dp.world_size])
        flag = dproc.bad_token_flag()
        if flag is not None:
            sums = torch.cat([sums, flag.float()])
        # metrics are means over ranks; the out-of-range-token flag rides in the same all-reduce, so EVERY rank raises
        # together (a rank raising alone would leave the others blocked in their next collective)
        self.dp.all_reduce_sum_(sums)
        host = sums.cpu().tolist()                                    # the only host sync of the epoch
        if flag is not None:
            dproc.raise_if_bad_tokens(host.pop())                     # nn.Embedding's IndexError, one epoch late at most
        if restarting:
            host, tail = host[:-2 * ncb], host[-2 * ncb:]
        means = dict(loss=host[0], accuracy=host[5:], loss_quantize=host[1], loss_contrastive=host[2],
                     num_codewords=host[3], num_codewords_negative=host[4])
        means['loss_monitor'] = -sum(means['accuracy']) / len(means['accuracy'])
        if restarting:
            means['codebook_restarts'] = [int(round(v)) for v in tail[:ncb]]      # total over the epoch, per codebook
            means['codebook_perplexity'] = tail[ncb:]                             # of N at the end of the epoch, per codebook
        if train:
            self._report_scale_saturation(means)      # training.FlatTraining: means['f16x3_scale_saturations'] + marked steps
        return means
