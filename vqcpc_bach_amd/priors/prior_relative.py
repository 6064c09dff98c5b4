"""The code prior (reference: VQCPCB/priors/prior_relative.py:17-368): an autoregressive relative transformer over the
frozen encoder's merged codes.  It is what makes generation unconditional: sample a code sequence of any length
(`generate_codes`), hand it to `Decoder.generate_from_code_long`, get a chorale (`generate`).

`__init__`, `forward`, `epoch`, `train_model`, `init_optimizers`, `save` / `load` keep the reference's names, argument
meaning, state_dict keys (a reference state_dict loads with strict=True) and return contracts; the training step follows
`decoders.decoder.Decoder` (GraphedTraining step graph, utils.STEP_LOCK, flat parameters + FlatAdam, data-parallel
all-reduce through parallel.py, frozen encoder).

Hot path (`compute_loss`), all numerics in libvqcpc_hip.so: `linear(embedding)` depends on the code only, so it is
evaluated on the V table rows by ONE small GEMM; with the start-of-sentence row appended, the reference's shift-by-one
(:137-144) is a lookup with shifted indices (ops.EmbeddingFn, as `Decoder._target_table`); the stack is
`TransformerEncoderCustom.forward_rows_masked` under ops.MASK_CAUSAL; one head, softmax cross-entropy kernels.

Reference defects fixed.  `epoch` (:188-241) cannot run as written: it clips `self.decoder.parameters()` (no such attribute)
and `self.encoder.parameters()` (frozen, no gradients), and feeds the encoder's (B, S, num_codebooks) indices to a `forward`
that wants (B, S).  Built here is its evident intent: frozen encoder under no_grad -> `Encoder.merge_codes` -> `forward` ->
backward -> global-norm clip at 5 over the prior's own trainable parameters -> Adam.  The reference's means divide by
`num_batches` (None by default, :238); here by the number of batches seen.

Sampling (`generate_codes`, priors/generation.py) runs on the GPU: KV-cached steps where they are the cheaper form, the
stack over the window per code (the reference's algorithm, as one captured graph per window move) where that is.
TEMPERATURE: the reference computes p = softmax(logits), then p ** temperature renormalised (:341-347), i.e.
softmax(temperature * logits): a LARGER temperature gives a MORE peaked distribution -- the opposite sense of the decoder's
`logits / temperature` -- and it passes the same number on to the decoder (:356-358).  Both are kept: `temperature` means
for the prior what the reference makes it mean and goes to the decoder unchanged unless `decoder_temperature` is given.
`generate` returns (codes, tokens) tensors; music21 scores and XML writing are out of scope, as in the decoder.

The reference ships no prior configuration; `configs.make_prior_config()` is this package's own.
"""
import os
from itertools import islice

import torch
from torch import nn

from .. import ops
from ..decoders.decoder import HeadsFn
from ..graphs import GraphedTraining
from ..parallel import DataParallelContext, FlatParameters
from ..transformer.transformer_custom import TransformerEncoderCustom, TransformerEncoderLayerCustom
from ..utils import dict_pretty_print, SEEDS, STEP_LOCK

MAX_SAMPLED_VOCAB = 4096         # vqcpc_prior_sample: codes per step of `generate_codes`


class PriorRelative(GraphedTraining, nn.Module):
    def __init__(self, model_dir, dataloader_generator, encoder, d_model, num_layers, n_head, dim_feedforward, embedding_size,
                 num_channels, num_events, dropout):
        super().__init__()
        self.model_dir = model_dir
        self.encoder = encoder
        self.encoder.eval()                                # frozen (:49-52)
        for p in self.encoder.parameters():
            p.requires_grad = False
        self.dataloader_generator = dataloader_generator
        if type(self.encoder.quantizer).__name__ == 'NoQuantization':
            raise NotImplementedError('a prior over continuous (NoQuantization) codes does not exist')
        self.num_tokens_per_channel = [encoder.quantizer.codebook_size ** encoder.quantizer.num_codebooks]
        self.num_channels = num_channels
        assert self.num_channels == 1                      # one channel of merged codes (:59-60)
        self.d_model = d_model
        self.num_tokens = num_channels * num_events
        encoder_layer = TransformerEncoderLayerCustom(d_model=d_model, nhead=n_head, attention_bias_type='relative_attention',
                                                      num_channels=num_channels, num_events=num_events,
                                                      dim_feedforward=dim_feedforward, dropout=dropout)
        self.transformer = TransformerEncoderCustom(encoder_layer=encoder_layer, num_layers=num_layers)
        self.embedding = nn.Embedding(self.num_tokens_per_channel[0], embedding_size)
        self.linear = nn.Linear(embedding_size, self.d_model)
        self.sos = nn.Parameter(torch.randn((1, 1, self.d_model)))
        self.pre_softmaxes = nn.ModuleList([nn.Linear(self.d_model, n) for n in self.num_tokens_per_channel])
        self.optimizer = None
        self.dp = None
        self.is_main = True
        self.global_step = 0
        self.lr = 1e-3

    def __repr__(self):
        return 'PriorRelative'

    def _generate_square_subsequent_mask(self, sz):
        """API-compatible matrix (:183-186); the kernels evaluate the same rule from indices."""
        mask = (torch.triu(torch.ones(sz, sz)) == 1).transpose(0, 1)
        return mask.float().masked_fill(mask == 0, float('-inf')).masked_fill(mask == 1, float(0.0))

    # ---- the trainable parameters (the frozen encoder is excluded) -------------------------------------------------
    def _trainable(self):
        return [self.transformer, self.embedding, self.linear, self.sos, self.pre_softmaxes]

    def init_optimizers(self, lr=1e-3, dp=None):
        dev = self.sos.device
        assert dev.type == 'cuda', 'call .to(device) first: the training step has no CPU path'
        self.dp = dp if dp is not None else (self.dp or DataParallelContext(device=dev))
        self.is_main = self.dp.rank == 0
        SEEDS.set_rank(self.dp.rank)            # per-rank dropout masks, whatever the launcher seeded
        self.flat = FlatParameters(self._trainable())
        self.dp.broadcast_(self.flat.flat, src=0)
        self.lr = lr
        self.optimizer = ops.FlatAdam(self.flat.flat, self.flat.flat_grad, lr=lr, max_norm=5.0)
        self.global_step = 0
        st = getattr(self, '_resume_state', None)
        if st is not None and st['m'].numel() == self.optimizer.m.numel():
            self.optimizer.m.copy_(st['m'])
            self.optimizer.v.copy_(st['v'])
            self.optimizer.step_count = int(st['step'])
            self.global_step = int(st['global_step'])
            self.restore_dropout_stream(st.get('dropout_stream'))
        self._resume_state = None

    def current_lr(self):
        return self.lr

    # ---- checkpoints (:109-120): one file `prior` holding the whole state_dict, encoder included ---------------------
    def save(self):
        os.makedirs(self.model_dir, exist_ok=True)
        torch.save(self.state_dict(), f'{self.model_dir}/prior')
        if self.optimizer is not None:       # extension: the reference restarts Adam on every resume
            torch.save(dict(m=self.optimizer.m, v=self.optimizer.v, step=self.optimizer.step_count,
                            global_step=self.global_step, dropout_stream=self.dropout_stream_state()),
                       f'{self.model_dir}/prior_optimizer')

    def load(self, device):
        print(f'Loading models {self.__repr__()}')
        ml = torch.device(device)
        self.load_state_dict(torch.load(f'{self.model_dir}/prior', map_location=ml))
        opt = f'{self.model_dir}/prior_optimizer'
        self._resume_state = torch.load(opt, map_location=ml) if os.path.exists(opt) else None

    def train(self, mode=True):
        super().train(mode)
        self.encoder.eval()                  # :195-196: the encoder stays in eval mode
        return self

    # ---- forward ---------------------------------------------------------------------------------------------------
    def _input_table(self):
        """(V + 1, d_model): row v = linear(embedding[v]), the last row is the start-of-sentence row."""
        table = ops.linear(self.embedding.weight, self.linear.weight, self.linear.bias)
        return torch.cat([table, self.sos.view(1, self.d_model)], dim=0)

    def compute_loss(self, codes):
        """codes (B, N) merged codes, device int64 -> (loss, logits (B, N, V))."""
        B, N = codes.shape
        V = self.num_tokens_per_channel[0]
        if N != self.num_tokens:
            raise ValueError(f'PriorRelative: windows of {self.num_tokens} codes expected, got {N}')
        table = self._input_table()
        shifted = torch.cat([torch.full((B, 1), V, dtype=torch.int64, device=codes.device), codes[:, :-1]], dim=1)
        rows = ops.EmbeddingFn.apply(table, shifted.reshape(-1))                             # (B * N, d), shifted by one
        out, _ = self.transformer.forward_rows_masked(rows, B, ops.MASK_CAUSAL)
        head = self.pre_softmaxes[0]
        (logits,) = HeadsFn.apply(out, 1, head.weight, head.bias)                            # (B * N, V)
        loss = ops.SoftmaxCEFn.apply(logits, codes.reshape(-1), None).mean()                 # :168-174
        return loss, logits.reshape(B, N, V)

    def _checked_codes(self, x):
        x = torch.as_tensor(x).to(self.sos.device, torch.int64)
        if x.dim() != 2:
            raise ValueError(f'x: (batch, {self.num_tokens}) merged codes expected, got {tuple(x.shape)}')
        return x.contiguous()

    def forward(self, x):
        """API-compatible `PriorRelative.forward` (:122-181): x (B, N) merged codes."""
        loss, logits = self.compute_loss(self._checked_codes(x))
        return {'loss': loss, 'weights_per_category': [logits], 'monitored_quantities': {'loss': loss.item()}}

    def encode(self, x):
        """:205-208 + the merge the reference forgot: frozen encoder, inference only -> merged codes (B, N)."""
        return self.encoder.encode_indices(x, merged=True)

    def _step_compute(self, tensor_dict):
        codes = self.encode(tensor_dict['x'])
        with torch.enable_grad(), ops.forward_arithmetic(self.flat):      # whatever the caller's ambient grad mode
            loss, _ = self.compute_loss(codes)
        self.flat.zero_grad()
        with ops.direct_weight_gradients(self.flat):
            loss.backward()
        return loss.detach()

    def _step_apply(self, loss):
        self.optimizer.step(lr=self.current_lr(), grad_scale=1.0 / self.dp.world_size)       # clip 5 + Adam
        return loss

    def _train_step_body(self, tensor_dict):
        loss = self._step_compute(tensor_dict)
        self._all_reduce_gradients()
        return self._step_apply(loss)

    def _graph_optimizers(self):
        return [self.optimizer]

    def train_step(self, tensor_dict, train=True):
        if not train:
            with STEP_LOCK:
                codes = self.encode(tensor_dict['x'])
                with torch.no_grad():
                    return self.compute_loss(codes)[0].detach()
        with SEEDS.stream_of(self):            # this trainer's own dropout-seed stream (utils.DropoutSeeds.stream_of)
            out = self._graphed_step(tensor_dict, self._train_step_body, parts=(self._step_compute, self._step_apply))
            if out is None:
                out = self._train_step_body(tensor_dict)
        self.global_step += 1
        return out

    def epoch(self, data_loader, train=True, num_batches=None):
        assert self.optimizer is not None, 'call init_optimizers(lr) first'
        self.train() if train else self.eval()
        total = torch.zeros((), dtype=torch.float32, device=self.sos.device)
        n = 0
        for tensor_dict in islice(data_loader, num_batches):
            total += self.train_step(tensor_dict, train=train)
            n += 1
        total /= max(n, 1)
        if self.dp.distributed:
            self.dp.all_reduce_sum_(total)
            total /= self.dp.world_size
        means = {'loss': float(total.item())}                    # the host sync of the epoch
        self.encoder.data_processor.raise_if_bad_tokens(dp=self.dp)
        if train:
            self._report_scale_saturation(means)
        return means

    def train_model(self, batch_size, num_batches=None, num_epochs=10, lr=1e-3, plot=False, num_workers=0, **kwargs):
        from .. import hip
        mode_before, arith_before = hip.gemm_mode_state(), ops.gradient_arithmetic_state()
        self.use_training_defaults()               # bf16x6 GEMMs + step-graph replay unless the caller chose otherwise
        self.trained_gemm_mode = hip.get_gemm_mode()
        try:
            return self._train_epochs(batch_size, num_batches, num_epochs, lr, num_workers)
        finally:
            hip.restore_gemm_mode_state(mode_before)      # process-wide settings: put back what the caller had
            ops.restore_gradient_arithmetic_state(arith_before)

    def _train_epochs(self, batch_size, num_batches, num_epochs, lr, num_workers):
        best_val = 1e8
        self.init_optimizers(lr=lr)
        history = []
        for epoch_id in range(num_epochs):
            gen_train, gen_val, _ = self.dataloader_generator.dataloaders(batch_size=batch_size, num_workers=num_workers)
            train = self.epoch(data_loader=gen_train, train=True, num_batches=num_batches)
            del gen_train
            val = self.epoch(data_loader=gen_val, train=False,
                             num_batches=num_batches // 2 if num_batches is not None else None)
            del gen_val
            if self.is_main:
                print(f'======= Epoch {epoch_id} =======')
                print('---Train---')
                dict_pretty_print(train, endstr=' ' * 5)
                print()
                print('---Val---')
                dict_pretty_print(val, endstr=' ' * 5)
                print('\n')
                if val['loss'] < best_val:                 # :292-294
                    self.save()
                    best_val = val['loss']
            history.append((train, val))
        return history

    # ---- generation (:308-368): KV-cached sampling on the GPU, priors/generation.py -----------------------------------
    def generate_codes(self, num_tokens, temperature=1.0, num_generated_codes=1, top_k=0, top_p=1.0, seed=None, use_graph=True,
                       window_stride=1, method='auto'):
        """Samples `num_generated_codes` sequences of `num_tokens` >= N merged codes (:315-353).  Code e < N comes from the
        first window (one cached step per code); code e >= N from the window that ends at e, as in the reference, when
        `window_stride` = 1.  window_stride = k > 1 (an opt-in of this package, NOT the reference's model context) moves the
        window k codes at a time, so code e sees between N - k and N - 1 previous codes instead of always N - 1; it costs
        1 / k of the re-prefills.  temperature: softmax(temperature * logits), the reference's sense (module docstring);
        top_k / top_p: the filter of utils.py:101-128 (off by default, as the reference has none here); seed: an int (per-row
        seeds derived from it), a per-row int64 tensor, or None (drawn from torch's generator); use_graph=False runs the same
        launches eagerly (same codes).  method: 'auto' picks per regime and batch between the KV-cached step and the
        full-stack step on the window (priors/generation.py: the faster of the two as measured), 'cached' / 'forward' force
        one; both compute the same logits to rounding.  -> int64 (num_generated_codes, num_tokens) on the device."""
        from ..transformer.incremental import generate_in_chunks, row_seeds
        from .generation import IncrementalPrior
        V, N = self.num_tokens_per_channel[0], self.num_tokens
        if V > MAX_SAMPLED_VOCAB:
            raise ValueError(f'generate_codes: {V} merged codes, the sampling kernel (vqcpc_prior_sample) takes at most '
                             f'{MAX_SAMPLED_VOCAB}')
        num_tokens, B, stride = int(num_tokens), int(num_generated_codes), int(window_stride)
        if num_tokens < N:
            raise ValueError(f'generate_codes: num_tokens >= {N} (one model window) expected, got {num_tokens}')
        if B < 1:
            raise ValueError('generate_codes: num_generated_codes >= 1')
        if not 1 <= stride < max(N, 2):
            raise ValueError(f'generate_codes: 1 <= window_stride < {N} (got {window_stride})')
        if not temperature > 0:
            raise ValueError('temperature must be > 0')
        seeds = row_seeds(seed, B)

        def chunk(n, rows):
            inc = IncrementalPrior(self, n)
            inc.start(num_tokens, seeds=seeds[rows], temperature=temperature, top_k=top_k, top_p=top_p)
            return inc.run(use_graph=use_graph, window_stride=stride, method=method)
        return generate_in_chunks(self, B, num_tokens, chunk)

    def generate(self, num_tokens, decoder, temperature=1.0, num_generated_codes=1, num_decodings_per_generating_code=1,
                 decoder_temperature=None, seed=None, **decoder_sampling):
        """:308-368: `generate_codes`, then `decoder.generate_from_code_long` on them.  `temperature` goes to BOTH, as in the
        reference (where it sharpens the prior and flattens the decoder as it grows, module docstring);
        decoder_temperature overrides the decoder's.  decoder_sampling: top_k, top_p, pad, start, ... of
        `generate_from_code_long`.  -> (codes (B, num_tokens), tokens (B * decodings, events, channels)) int64 tensors on the
        device; score objects and XML files need music21 and are out of scope."""
        codes = self.generate_codes(num_tokens, temperature=temperature, num_generated_codes=num_generated_codes, seed=seed)
        tokens = decoder.generate_from_code_long(encoding_indices=codes,
                                                 temperature=temperature if decoder_temperature is None else decoder_temperature,
                                                 num_decodings=num_decodings_per_generating_code, seed=seed, **decoder_sampling)
        return codes, tokens

    def plot(self, *a, **k):
        raise NotImplementedError('tensorboard plots (:301-306) are out of scope')
