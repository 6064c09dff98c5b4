"""The code prior (reference: VQCPCB/priors/prior_relative.py:17-368): an autoregressive relative transformer over the
frozen encoder's merged codes.  It is what makes generation unconditional: sample a code sequence of any length
(`generate_codes`), hand it to `Decoder.generate_from_code_long`, get a chorale (`generate`).

`__init__`, `forward`, `epoch`, `train_model`, `init_optimizers`, `save` / `load` keep the reference's names, argument
meaning, state_dict keys (a reference state_dict loads with strict=True) and return contracts; the training step is
`training.FlatTraining`'s, shared with the other three trainers (step graph, utils.STEP_LOCK, flat parameters + FlatAdam,
data-parallel all-reduce through parallel.py); what is this class's own is the loss on the frozen encoder's codes.

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
GIVEN CODES AND SCORES: `generate_codes(constraint=..., return_logp=True)` emits the given codes where the constraint holds
one, draws the others as it would without the constraint given the same prefix (a draw is keyed by seed and position), and
returns every emitted code's log-probability -- under the model's UNMODIFIED row: temperature 1 and no filter, whatever
`temperature`, `top_k` and `top_p` are (vqcpc_prior_sample_constrained; the default path launches vqcpc_prior_sample as
before).  `score_codes` is the everything-forced call; `continue_tokens` encodes the opening of a piece, lets the prior go on
from its codes and has the decoder write tokens around the given ones.  `score_codes(method='windows')` computes the same scores
without generating -- every window of every piece is a row of one batched teacher-forced forward (priors/scoring.py,
vqcpc_prior_score) -- and `score_chorale` adds the decoder's token scores to them: the nats the pipeline spends on a piece.
ALLOWED CODES AND PARTICLES: `generate_codes(allowed=..., return_allowed_mass=True)` restricts every column to a set of codes (a
product prior: to a Cartesian product of digit sets; priors/code_sets.py builds them) and returns the log of the probability the
model gives to each set; `particles=P` runs P rows per requested plan, weighs them by the forced codes' logp and the sets' mass and
resamples after every code, so that codes forced AFTER free ones select the plans that lead to them (vqcpc_prior_sample_masked,
vqcpc_prior_sample_product_masked; csrc/particles.hip).  `generate` and `continue_tokens` pass them through as `code_allowed`,
`code_particles`, and `continue_tokens(code_constraint=...)` fixes codes after the opening, e.g. a close.

PRODUCT CODES: `code_model='product'` (ours, `prior_kwargs['code_model']`; default 'merged' = the reference's model, one symbol
of a vocabulary of V = K**ncb, which `generate_codes` samples up to V = 4096).  A merged code is ncb digits c_j = (code // K**j)
% K.  `embedding` is a `ProductEmbedding` (ncb, K, embedding_size) and a code's input row linear(sum_j E_j[c_j]), evaluated as
sum_j T_j[c_j] over per-codebook tables of ncb * K rows (`_input_tables`); `pre_softmaxes` is ncb heads Linear(d_model, K);
`digit_embeddings` a `ProductEmbedding` (ncb - 1, K, d_model), absent when ncb = 1.  With h_e the stack's output at position e,
stage j's logits are pre_softmaxes[j](h_e + sum_{i<j} D_i[c_{e,i}]): p(code_e | codes < e) = prod_j softmax(logits_{e,j})[c_{e,j}],
the loss sum_j mean CE_j, and no tensor of V rows exists anywhere.  Merged int64 codes stay the interface of every method;
`forward` returns the ncb logit tensors.  In `generate_codes`, `temperature`, `top_k` and `top_p` filter EACH DIGIT'S conditional
distribution (a filter on the joint distribution over K**ncb codes does not exist), and `logp` is the sum of the ncb stage
log-probabilities.  With ncb = 1 the model, its kernels' bits and its codes are the merged prior's.

The reference ships no prior configuration; `configs.make_prior_config()` is this package's own.
"""
import os

import numpy as np
import torch
from torch import nn

from .. import ops
from ..decoders.decoder import HeadsFn
from ..quantizer.product_embedding import ProductEmbedding
from ..training import FlatTraining
from ..transformer.transformer_custom import TransformerEncoderCustom, TransformerEncoderLayerCustom
from ..utils import STEP_LOCK

MAX_SAMPLED_VOCAB = 4096         # vqcpc_prior_sample / _constrained / _masked: codes per step of `generate_codes`


class PriorRelative(FlatTraining, nn.Module):
    def __init__(self, model_dir, dataloader_generator, encoder, d_model, num_layers, n_head, dim_feedforward, embedding_size,
                 num_channels, num_events, dropout, code_model='merged'):
        super().__init__()
        if code_model not in ('merged', 'product'):
            raise ValueError(f"code_model {code_model!r}: 'merged' or 'product'")
        self.code_model = code_model
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
        self.num_codebooks, self.codebook_size = int(encoder.quantizer.num_codebooks), int(encoder.quantizer.codebook_size)
        if code_model == 'product':                        # ours: a code is predicted digit by digit (module docstring)
            ncb, K = self.num_codebooks, self.codebook_size
            ops.check_product_shape(ncb, K, 1)
            if d_model % 4 != 0:
                raise ValueError(f"code_model 'product': d_model = {d_model}, a multiple of 4 is needed")
            self.embedding = ProductEmbedding(ncb, K, embedding_size)
        else:
            self.embedding = nn.Embedding(self.num_tokens_per_channel[0], embedding_size)
        self.linear = nn.Linear(embedding_size, self.d_model)
        self.sos = nn.Parameter(torch.randn((1, 1, self.d_model)))
        if code_model == 'product':
            self.pre_softmaxes = nn.ModuleList([nn.Linear(self.d_model, K) for _ in range(ncb)])
            if ncb > 1:
                self.digit_embeddings = ProductEmbedding(ncb - 1, K, self.d_model)
        else:
            self.pre_softmaxes = nn.ModuleList([nn.Linear(self.d_model, n) for n in self.num_tokens_per_channel])
        self.lr = 1e-3

    def __repr__(self):
        return 'PriorRelative'

    def _generate_square_subsequent_mask(self, sz):
        """API-compatible matrix (:183-186); the kernels evaluate the same rule from indices."""
        mask = (torch.triu(torch.ones(sz, sz)) == 1).transpose(0, 1)
        return mask.float().masked_fill(mask == 0, float('-inf')).masked_fill(mask == 1, float(0.0))

    # ---- the trainable parameters (the frozen encoder is excluded) -------------------------------------------------
    def _trainable(self):
        own = [self.transformer, self.embedding, self.linear, self.sos, self.pre_softmaxes]
        return own + ([self.digit_embeddings] if hasattr(self, 'digit_embeddings') else [])

    def init_optimizers(self, lr=1e-3, dp=None):
        self._init_flat(self._trainable(), self.sos.device, dp)
        self.lr = lr
        self.optimizer = ops.FlatAdam(self.flat.flat, self.flat.flat_grad, lr=lr, max_norm=5.0)
        self.global_step = 0
        self._apply_resume_state()

    def current_lr(self):
        return self.lr

    # ---- checkpoints (:109-120): one file `prior` holding the whole state_dict, encoder included ---------------------
    def save(self):
        os.makedirs(self.model_dir, exist_ok=True)
        torch.save(self.state_dict(), f'{self.model_dir}/prior')
        self._save_optimizer_state(f'{self.model_dir}/prior_optimizer')

    def load(self, device):
        print(f'Loading models {self.__repr__()}')
        ml = torch.device(device)
        self.load_state_dict(torch.load(f'{self.model_dir}/prior', map_location=ml))
        self._load_optimizer_state(f'{self.model_dir}/prior_optimizer', ml)

    def train(self, mode=True):
        super().train(mode)
        self.encoder.eval()                  # :195-196: the encoder stays in eval mode
        return self

    # ---- forward ---------------------------------------------------------------------------------------------------
    def _input_table(self):
        """(V + 1, d_model): row v = linear(embedding[v]), the last row is the start-of-sentence row."""
        table = ops.linear(self.embedding.weight, self.linear.weight, self.linear.bias)
        return torch.cat([table, self.sos.view(1, self.d_model)], dim=0)

    def _input_tables(self):
        """code_model 'product': (ncb, K, d_model) per-codebook input rows, T_0 = linear(E_0) with the bias, T_j = E_j W^T without
        it for j >= 1, so that a code's input row sum_j T_j[c_j] is linear(sum_j E_j[c_j]): two small GEMMs on ncb * K rows."""
        E, lin = self.embedding.weight, self.linear
        first = ops.linear(E[0], lin.weight, lin.bias)
        if self.num_codebooks == 1:
            return first.unsqueeze(0)
        rest = ops.linear(E[1:].reshape(-1, E.shape[2]), lin.weight, None)
        return torch.cat([first, rest], dim=0).view(self.num_codebooks, self.codebook_size, self.d_model)

    def _compute_loss_product(self, codes):
        """codes (B, N) -> (loss, [logits_j (B, N, K) for the ncb digits]).  Stage j's head reads the stack's output plus the
        digit-conditioning rows of the digits i < j of the SAME code: p(code) = prod_j softmax(logits_j)[c_j], and the loss
        sum_j mean CE_j is minus the mean log-probability per code, the merged prior's scale."""
        B, N = codes.shape
        ncb, K, V, d = self.num_codebooks, self.codebook_size, self.num_tokens_per_channel[0], self.d_model
        shifted = torch.cat([torch.full((B, 1), V, dtype=torch.int64, device=codes.device), codes[:, :-1]], dim=1)
        rows = ops.ProductEmbeddingFn.apply(self._input_tables(), self.sos.view(1, d), shifted.reshape(-1))   # (B * N, d)
        out, _ = self.transformer.forward_rows_masked(rows, B, ops.MASK_CAUSAL)
        flat = codes.reshape(-1)
        low = flat % (K ** (ncb - 1))                      # the digits the conditioning table knows: all but the last
        loss, logits = None, []
        for j, head in enumerate(self.pre_softmaxes):
            h = out if j == 0 else ops.ProductEmbeddingFn.apply(self.digit_embeddings.weight, None, low, j, out)
            (lg,) = HeadsFn.apply(h, 1, head.weight, head.bias)                              # (B * N, K)
            ce = ops.SoftmaxCEFn.apply(lg, (flat // (K ** j)) % K, None).mean()
            loss = ce if loss is None else loss + ce
            logits.append(lg.reshape(B, N, K))
        return loss, logits

    def compute_loss(self, codes):
        """codes (B, N) merged codes, device int64 -> (loss, logits (B, N, V)) [code_model 'product': the list of the ncb
        digits' logits (B, N, K)]."""
        B, N = codes.shape
        V = self.num_tokens_per_channel[0]
        if N != self.num_tokens:
            raise ValueError(f'PriorRelative: windows of {self.num_tokens} codes expected, got {N}')
        if self.code_model == 'product':
            return self._compute_loss_product(codes)
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
        return {'loss': loss, 'weights_per_category': logits if self.code_model == 'product' else [logits],
                'monitored_quantities': {'loss': loss.item()}}

    def encode(self, x):
        """:205-208 + the merge the reference forgot: frozen encoder, inference only -> merged codes (B, N)."""
        return self.encoder.encode_indices(x, merged=True)

    def _step_compute(self, tensor_dict):
        codes = self.encode(tensor_dict['x'])

        def forward():
            loss = self.compute_loss(codes)[0]
            return loss, loss.detach()
        return self._forward_backward(forward)

    def train_step(self, tensor_dict, train=True):
        if not train:
            with STEP_LOCK:
                codes = self.encode(tensor_dict['x'])
                with torch.no_grad():
                    return self.compute_loss(codes)[0].detach()
        return self._train_step(tensor_dict)

    def epoch(self, data_loader, train=True, num_batches=None):
        assert self.optimizer is not None, 'call init_optimizers(lr) first'
        return self._scalar_loss_epoch(data_loader, train, num_batches, [self.encoder.data_processor])

    def train_model(self, batch_size, num_batches=None, num_epochs=10, lr=1e-3, plot=False, num_workers=0, weight_average=None,
                    **kwargs):
        with self._training_defaults():
            self.init_optimizers(lr=lr)
            if weight_average is not None:
                self.enable_weight_averaging(weight_average)
            return self._train_epochs(batch_size, num_batches, num_epochs, num_workers, monitor='loss', save_best=self.save)     # :292-294

    # ---- generation (:308-368): KV-cached sampling on the GPU, priors/generation.py -----------------------------------
    def _code_constraint(self, constraint, rows, num_tokens):
        """A public code constraint (rows, num_tokens) or (1, num_tokens) int64, -1 = free -> (rows, num_tokens) int64 on the
        device."""
        constraint = torch.as_tensor(constraint)
        if constraint.dim() != 2 or constraint.shape[0] not in (1, rows) or constraint.shape[1] != num_tokens or \
                constraint.dtype != torch.int64:
            raise ValueError(f'constraint: ({rows}, {num_tokens}) or (1, {num_tokens}) int64 expected (-1 = free), got '
                             f'{tuple(constraint.shape)} {constraint.dtype}')
        V = self.num_tokens_per_channel[0]
        if bool((constraint >= V).any()):
            raise ValueError(f'constraint: a forced code is outside the {V} merged codes')
        return constraint.to(self.sos.device).expand(rows, num_tokens).contiguous()

    def generate_codes(self, num_tokens, temperature=1.0, num_generated_codes=1, top_k=0, top_p=1.0, seed=None, use_graph=True,
                       window_stride=1, method='auto', constraint=None, return_logp=False, allowed=None,
                       return_allowed_mass=False, particles=None, resample_threshold=0.5, return_particles=False, beam=None,
                       return_beams=False):
        """Samples `num_generated_codes` sequences of `num_tokens` >= N merged codes (:315-353).  Code e < N comes from the
        first window (one cached step per code); code e >= N from the window that ends at e, as in the reference, when
        `window_stride` = 1.  window_stride = k > 1 (an opt-in of this package, NOT the reference's model context) moves the
        window k codes at a time, so code e sees between N - k and N - 1 previous codes instead of always N - 1; it costs
        1 / k of the re-prefills.  temperature: softmax(temperature * logits), the reference's sense (module docstring);
        top_k / top_p: the filter of utils.py:101-128 (off by default, as the reference has none here); seed: an int (per-row
        seeds derived from it), a per-row int64 tensor, or None (drawn from torch's generator); use_graph=False runs the same
        launches eagerly (same codes).  method: 'auto' picks per regime and batch between the KV-cached step and the
        full-stack step on the window (priors/generation.py: the faster of the two as measured), 'cached' / 'forward' force
        one; both compute the same logits to rounding.  -> int64 (num_generated_codes, num_tokens) on the device.
        constraint: (num_generated_codes, num_tokens) int64, or (1, num_tokens) for every row: a code >= 0 is emitted at its
        place (whatever top_k / top_p would leave of it), -1 is free; the free codes are what they would be without the
        constraint given the same codes before them.  return_logp=True -> (codes, logp): logp float32 of the codes' shape,
        every emitted code's log-probability, forced or drawn, under the model's unmodified distribution at that place --
        temperature 1, no filter, whatever `temperature` is.
        code_model 'product': a code is drawn digit by digit; temperature, top_k and top_p filter EACH DIGIT'S conditional
        distribution over its K values (not the joint distribution over the K**ncb codes), a forced code forces every digit,
        and logp is the sum of the ncb digits' log-probabilities.  Any K**ncb < 2**31 is sampled.
        allowed: bool (num_generated_codes | 1, num_tokens, V) [code_model 'product': (num_generated_codes | 1, num_tokens, ncb, K),
        a digit set per codebook: the column's allowed codes are their Cartesian product]; True = the code may be drawn at that
        column (priors/code_sets.py builds such tensors from {column: codes}).  A code outside the set gets probability 0 BEFORE
        top_k / top_p, which then choose among the allowed codes; a forced code must lie in its own set.  ValueError, from one
        check per call, naming the first (row, column[, codebook]) whose set is empty or forbids its forced code.
        return_allowed_mass=True -> `allowed_mass` after codes and logp, float32 of the codes' shape: the log of the probability
        the model's unmodified distribution gives to the column's set (0 where nothing is restricted; 'product': the sum of the
        per-digit conditional masses along the emitted digits, the importance weight of the digit-by-digit proposal, not the
        marginal mass of the product set).
        particles=P in [2, 64]: every requested row is a group of P rows of the stack with the seeds row_seeds(seed, rows * P),
        group g at [g P, (g + 1) P).  After every code a row's weight grows by the logp of a forced code / the allowed_mass of a
        restricted one, and a group whose effective sample size falls below resample_threshold * P is resampled (systematic;
        csrc/particles.hip): forced codes that come AFTER free ones then select the prefixes that lead to them.  The result has
        the shapes of a call without the keyword: each group's first row after a final forced resampling.  return_particles=True
        skips that and returns all rows * P rows followed by a dict: 'weights' (rows, P) the final normalised weights,
        'log_evidence' (rows,), and per code 'ancestors' (num_tokens, rows * P), 'wn', 'ess' -- `Decoder.generate_from_codes`'
        contract.  Results come in the order (codes[, logp][, allowed_mass][, particles]).  Any of the keywords switches the
        step's sampler to vqcpc_prior_sample_masked (vqcpc_prior_sample_product_masked); without them every launch is what it was.
        beam=W in [1, 64] (csrc/prior_beam.hip): a deterministic search in the sampler's place.  Every
        requested row is a group of W rows of the stack, the W most probable plans so far: at each column every row is expanded
        into its candidate codes -- the forced code, else the codes of the column's set, else all V --, and the group's W best
        (row, code) pairs by total log-probability become the new rows, best first (equal totals: the lower row, then the lower
        code).  The result has the shapes of a call without the keyword: each group's slot 0, the best plan found.
        return_beams=True returns all rows * W rows in slot order followed by a dict: 'scores' (rows, W) float32, the plans' total
        log-probabilities -- the ordered fp32 sum of their logp --, non-increasing along W and -inf for a dead slot (fewer than W
        plans exist), and 'ancestors' (num_tokens, rows * W) int32, per column the row each slot descends from.  W at least the
        number of admitted plans makes the search exhaustive; beam=1 is greedy decoding.  `seed` is accepted and unused.
        code_model 'product': the search PRUNES AFTER EVERY DIGIT.  A code is ncb digit stages; at each stage the rows are expanded
        into the stage's candidate digits (the forced code's digit, else the stage's digit set, else all K) and the group's W best
        (row, digit) pairs go on to the next stage: it is a beam over the digit sequence, not over the K**ncb merged codes, so
        a code whose first digit is not among the W best prefixes is never scored, and W >= the admitted plans is exhaustive only
        if it also covers every stage's partial codes.  logp and scores are the sums of the digits' log-probabilities, with
        vqcpc_prior_sample_product's bits.
        ValueError with `particles`, a filter (temperature other than 1, top_k, top_p) or return_beams without beam.  Results come
        in the order (codes[, logp][, allowed_mass][, particles | beams]).  Chunks are whole groups.  Without the keywords every
        launch, buffer and result is what it was.
        Out of scope: sets for `score_codes`, relational rules on codes, and sets over the K**ncb codes of a product prior that
        are not a product of digit sets."""
        from ..transformer.incremental import MAX_ROWS, generate_in_chunks, row_seeds
        from .generation import IncrementalPrior, IncrementalProductPrior
        if self.code_model == 'product':
            IncrementalPrior = IncrementalProductPrior
        V, N = self.num_tokens_per_channel[0], self.num_tokens
        if V > MAX_SAMPLED_VOCAB and self.code_model != 'product':
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
        if constraint is not None:
            constraint = self._code_constraint(constraint, B, num_tokens)
        # with `particles` every requested row is a group of P rows of the stack (P = 1 without)
        from ..decoders.decoder import Decoder
        P = Decoder._particle_count(particles, resample_threshold, return_particles, None)
        W = Decoder._beam_width(beam, return_beams, particles, None, 1, temperature, top_k, top_p)
        if beam is not None:
            P = W                                             # the group size of the chunks below, whichever kind the groups are
        packed = None if allowed is None else self._code_sets(allowed, B, num_tokens, constraint)       # (B | 1, ...)
        rows_all = B * P
        if P > 1 and constraint is not None:
            constraint = constraint.repeat_interleave(P, dim=0)
        seeds = row_seeds(seed, rows_all)
        dev = self.sos.device
        kept = {'logp': return_logp, 'logmass': return_allowed_mass}
        records = {key: torch.empty(rows_all, num_tokens, dtype=torch.float32, device=dev) for key, on in kept.items() if on}
        filt = {} if particles is not None or beam is not None else None

        def chunk(n, rows):
            inc = IncrementalPrior(self, n)
            sets = None
            if packed is not None:                            # row r of the stack belongs to requested row r // P
                idx = torch.arange(rows.start, rows.stop, device=dev) // P if packed.shape[0] > 1 else \
                    torch.zeros(n, dtype=torch.int64, device=dev)
                sets = packed[idx]
            inc.start(num_tokens, seeds=seeds[rows], temperature=temperature, top_k=top_k, top_p=top_p,
                      constraint=None if constraint is None else constraint[rows], want_logp=return_logp, allowed=sets,
                      want_allowed_mass=return_allowed_mass, particles=None if particles is None else P,
                      resample_threshold=resample_threshold, final_resample=not return_particles,
                      beam=None if beam is None else W)
            codes = inc.run(use_graph=use_graph, window_stride=stride, method=method)
            for key, buf in records.items():
                buf[rows] = getattr(inc, key)
            if filt is not None:
                Decoder._keep_particle_results(filt, inc.particle_results() if beam is None else inc.beam_results(), rows.start)
            return codes
        codes = generate_in_chunks(self, rows_all, num_tokens, chunk, MAX_ROWS // P * P)             # whole groups
        whole = return_particles if beam is None else return_beams
        keep = slice(None) if P == 1 or whole else slice(0, rows_all, P)        # a group's first row: the survivor / the best plan
        out = [codes[keep]] + [records[key][keep] for key in ('logp', 'logmass') if key in records]
        if return_particles or return_beams:
            out.append(Decoder._join_particle_results(filt))
        return out[0] if len(out) == 1 else tuple(out)

    def _code_sets(self, allowed, rows, num_tokens, constraint):
        """A public `allowed` -> packed sets int32 (rows | 1, num_tokens, words) [code_model 'product': (rows | 1, num_tokens, ncb,
        words)] on the device, after the one host check of the call (priors/code_sets.py)."""
        from .code_sets import check_sets, pack_sets
        allowed = torch.as_tensor(allowed)
        V = self.num_tokens_per_channel[0]
        tail = (self.num_codebooks, self.codebook_size) if self.code_model == 'product' else (V,)
        shape = tuple(allowed.shape)
        if allowed.dtype != torch.bool or len(shape) != 2 + len(tail) or shape[0] not in (1, rows) or \
                shape[1:] != (num_tokens,) + tail:
            raise ValueError(f'allowed: bool ({rows} | 1, {num_tokens}, {", ".join(map(str, tail))}) expected, got {shape} '
                             f'{allowed.dtype}')
        allowed = allowed.to(self.sos.device)
        check_sets(allowed, constraint)
        return pack_sets(allowed)

    @staticmethod
    def score_window_plan(num_tokens, N, window_stride=1):
        """Host only: the distinct model windows in which `generate_codes` emits the `num_tokens` >= N codes of a sequence at
        `window_stride` = k, as a list of (first code of the window, first scored column, one past the last scored column) in
        sequence coordinates, windows ascending -- the columns `IncrementalPrior.run` scores in each window.  Window 0 scores
        columns [0, N); window i * k its last k columns; when (num_tokens - N) % k != 0 a last window at num_tokens - N scores the
        last (num_tokens - N) % k columns.  Every column lies in exactly one window; num_tokens == N gives one window.
        ValueError on num_tokens < N or a stride outside [1, max(N, 2))."""
        from .scoring import window_plan
        return window_plan(num_tokens, N, window_stride)

    def score_codes(self, codes, use_graph=True, window_stride=1, method='auto', return_details=False, window_rows=None):
        """log-probability of every code of `codes` (B, L) int64, L >= N, given the codes before it: float32 (B, L).  Column
        e < N is scored in the first window, column e >= N in the window that ends at e (the reference's window rule, at
        `window_stride` = 1).  With method 'auto' / 'cached' / 'forward' it is `generate_codes` with every code forced, so it is
        the model's distribution at temperature 1 without a filter; use_graph / window_stride / method as there.
        method='windows' computes the same scores without generating (priors/scoring.py): the windows `score_window_plan` names
        are rows of one batched, teacher-forced forward, `window_rows` (piece, window) rows at a time (None: the measured
        default), and vqcpc_prior_score (csrc/prior_score.hip) scores the rows.  The scores agree with the forced call's within
        the teacher-forced tolerance, not bit for bit; `use_graph` is ignored.  'auto' never routes here.
        return_details=True (method='windows' only) -> a dict of (B, L) tensors: 'logp'; 'entropy' (float32, nats) of the model's
        distribution at the column; 'rank' (int32) of the given code, 0 = the model's first choice, equal logits in index order;
        'best' (int64), the arg-max, the lowest index among equals; 'best_logp' (float32).  code_model 'product': the stages are
        teacher-forced with the piece's own digits, 'logp' is the sum of the ncb stages in ascending order, and the other arrays
        are (B, L, ncb) and describe each digit's conditional distribution ('best': the greedy digit given the piece's own
        earlier digits); any K**ncb < 2**31 is scored, a merged prior up to 4096 codes.
        Runs in eval mode without gradients under STEP_LOCK; the previous mode is restored.  ValueError on L < N, negative codes
        or codes >= V, a bad stride, window_rows that is not an integer >= 1, and return_details / window_rows with another
        method."""
        codes = self._checked_codes(codes)
        if bool((codes < 0).any()):
            raise ValueError('score_codes: negative codes')
        if method == 'windows':
            from .scoring import score_codes_windows
            return score_codes_windows(self, codes, window_stride, return_details, window_rows)
        if return_details or window_rows is not None:
            raise ValueError(f"score_codes: return_details / window_rows belong to method='windows' (got method={method!r})")
        B, L = codes.shape
        return self.generate_codes(L, num_generated_codes=B, seed=0, use_graph=use_graph, window_stride=window_stride,
                                   method=method, constraint=codes, return_logp=True)[1]

    def score_chorale(self, x, decoder, return_details=False, window_rows=None, decoder_window_rows=32):
        """The bits the pipeline spends on an existing piece x (1, events, channels): -log p(codes) - log p(tokens | codes), a
        bound on -log p(piece).  x is framed and encoded as `Decoder.score_chorale` frames it (one PAD ... START chunk, the END /
        PAD completion; needs the dataset's START / END / XX symbols; the compatibility checks of `continue_tokens`); the prior
        scores the framed code sequence with `score_codes(method='windows')`, `decoder.score_tokens` the tokens.  The framed
        chunks go through this prior's frozen encoder for the prior's codes and through the decoder's for the decoder's: in a
        trained pipeline one and the same encoder.
        -> dict: 'code_logp' float32 (1, codes of x's own chunks), each code conditioned on everything before it, the framing
        chunk's codes included; 'token_logp' float32 (1, events, channels) on x's own events (`Decoder.score_chorale`'s);
        'total_logp', the float64 sum of both; 'nats_per_token' = -total_logp / (events * channels).  return_details=True adds
        'code_details' and 'token_details', the two halves' detail dicts on the same ranges.  window_rows / decoder_window_rows:
        the two halves' rows per forward.  A decoder on continuous latents raises NotImplementedError."""
        from .scoring import score_chorale
        return score_chorale(self, x, decoder, return_details, window_rows, decoder_window_rows)

    def generate(self, num_tokens, decoder, temperature=1.0, num_generated_codes=1, num_decodings_per_generating_code=1,
                 decoder_temperature=None, seed=None, code_constraint=None, return_logp=False, code_allowed=None,
                 code_particles=None, code_resample_threshold=0.5, code_beam=None, **decoder_sampling):
        """:308-368: `generate_codes`, then `decoder.generate_from_code_long` on them.  `temperature` goes to BOTH, as in the
        reference (where it sharpens the prior and flattens the decoder as it grows, module docstring);
        decoder_temperature overrides the decoder's.  decoder_sampling: top_k, top_p, pad, start, ... of
        `generate_from_code_long`.  -> (codes (B, num_tokens), tokens (B * decodings, events, channels)) int64 tensors on the
        device; score objects and XML files need music21 and are out of scope.
        code_constraint / return_logp: `generate_codes`' constraint / return_logp; with return_logp=True the result is
        (codes, tokens, code_logp (B, num_tokens) float32).  code_allowed / code_particles / code_resample_threshold:
        `generate_codes`' allowed / particles / resample_threshold (each group's surviving row goes to the decoder).
        code_beam: `generate_codes`' beam (the prior then takes temperature 1, whatever `temperature` is): the decoder receives each
        group's best plan; with the decoder's own `beam=` in decoder_sampling the whole chain prior -> codes -> tokens is
        deterministic and most-probable-first."""
        out = self.generate_codes(num_tokens, temperature=1.0 if code_beam is not None else temperature,
                                  num_generated_codes=num_generated_codes, seed=seed,
                                  constraint=code_constraint, return_logp=return_logp, allowed=code_allowed,
                                  particles=code_particles, resample_threshold=code_resample_threshold, beam=code_beam)
        codes, code_logp = out if return_logp else (out, None)
        tokens = decoder.generate_from_code_long(encoding_indices=codes,
                                                 temperature=temperature if decoder_temperature is None else decoder_temperature,
                                                 num_decodings=num_decodings_per_generating_code, seed=seed, **decoder_sampling)
        return (codes, tokens, code_logp) if return_logp else (codes, tokens)

    def continue_tokens(self, x, num_new_codes, decoder, temperature=1.0, decoder_temperature=None, num_continuations=1,
                        seed=None, return_logp=False, code_constraint=None, code_allowed=None, code_particles=None,
                        code_resample_threshold=0.5, code_beam=None, **decoder_sampling):
        """"Here are the first bars, go on": x (1, events, channels) tokens of a piece's opening, events a multiple of the
        events per code.  The opening is framed at the front as `Decoder.reharmonise_tokens` frames a chorale (one model-sized
        PAD ... START chunk, then x; no END completion), encoded by this prior's frozen encoder in model-sized chunks and the
        codes glued: the L given codes.  The prior then samples `num_continuations` sequences of L + num_new_codes codes whose
        first L are the given ones (`generate_codes(constraint=...)`), and `decoder.generate_from_code_long` decodes the
        codes after the framing chunk with x's tokens forced at their chorale events.  temperature / decoder_temperature as
        in `generate`; decoder_sampling: top_k, top_p, ... of `generate_from_code_long`.
        -> (codes (num_continuations, L + num_new_codes), tokens (num_continuations, x's events + num_new_codes * events per
        code, channels)): events [0, x.shape[1]) of every token row equal x.  return_logp=True -> (codes, tokens, code_logp,
        token_logp), the scores of `generate_codes` and of `generate_from_code_long` (each at temperature 1, unfiltered).
        code_constraint: (1 | num_continuations, L + num_new_codes) int64, -1 = free, over ALL columns: the given opening is merged
        into it, so "continue this opening and close on that cadence" is one call; a value >= 0 inside the opening that differs
        from the encoded code is a ValueError.  code_allowed: `generate_codes`' allowed over the same columns; code_particles /
        code_resample_threshold: its particles / resample_threshold, which make the free codes lead to the forced close.
        code_beam: its beam (the prior then takes temperature 1): every continuation is the most probable plan the search finds
        from the opening, through the constraint and the sets.
        Needs the decoder's dataset's START / XX symbols."""
        if decoder.continuous_source:
            raise NotImplementedError('a prior over continuous (NoQuantization) codes does not exist')
        n2i = getattr(getattr(decoder.dataloader_generator, 'dataset', None), 'note2index_dicts', None)
        if n2i is None:
            raise ValueError('continue_tokens needs dataset.note2index_dicts with the START / XX symbols')
        nc, E, epc, U = decoder.num_channels, decoder.data_processor.num_events, decoder.num_events_per_code, decoder.total_upscaling
        if int(np.prod(self.encoder.downscaler.downscale_factors)) != U:
            raise ValueError(f"continue_tokens: the prior's encoder makes one code of "
                             f'{int(np.prod(self.encoder.downscaler.downscale_factors))} tokens, the decoder of {U}')
        x = torch.as_tensor(x).long().cpu()
        if x.dim() != 3 or x.shape[0] != 1 or x.shape[2] != nc:
            raise ValueError(f'x: (1, events, {nc}) tokens expected, got {tuple(x.shape)}')
        if x.shape[1] < epc or x.shape[1] % epc != 0:
            raise ValueError(f'x: a multiple of {epc} events (the events of one code), at least {epc}, expected; got {x.shape[1]}')
        num_new_codes = int(num_new_codes)
        if num_new_codes < 0:
            raise ValueError('continue_tokens: num_new_codes >= 0')
        PAD, START = ([int(n2i[c][sym]) for c in range(nc)] for sym in ('XX', 'START'))
        row = lambda ids, n: torch.tensor(ids, dtype=torch.int64).view(1, 1, nc).repeat(1, n, 1)
        framed = torch.cat([row(PAD, E - 1), row(START, 1), x], dim=1).to(self.sos.device)
        was_training = self.training
        self.eval()
        try:
            prefix = torch.cat([self.encode(c) for c in framed.split(E, 1)], dim=1)           # glued: (1, L)
        finally:
            self.train(was_training)
        L = prefix.shape[1]
        total = L + num_new_codes
        if total < max(self.num_tokens, decoder.num_tokens_source):
            raise ValueError(f'continue_tokens: {L} given + {num_new_codes} new codes, fewer than one model window '
                             f'({max(self.num_tokens, decoder.num_tokens_source)})')
        if code_constraint is None:
            constraint = torch.full((1, total), -1, dtype=torch.int64, device=prefix.device)
        else:
            constraint = self._code_constraint(code_constraint, int(num_continuations), total).clone()
            given = constraint[:, :L]
            if bool(((given >= 0) & (given != prefix)).any()):
                raise ValueError("continue_tokens: code_constraint forces a code inside the opening that differs from the opening's "
                                 'own encoded code')
        constraint[:, :L] = prefix
        out = self.generate_codes(total, temperature=1.0 if code_beam is not None else temperature,
                                  num_generated_codes=num_continuations, seed=seed,
                                  constraint=constraint, return_logp=return_logp, allowed=code_allowed, particles=code_particles,
                                  resample_threshold=code_resample_threshold, beam=code_beam)
        codes, code_logp = out if return_logp else (out, None)
        token_constraint = torch.full((int(num_continuations), total * epc, nc), -1, dtype=torch.int64)
        token_constraint[:, E:E + x.shape[1]] = x
        res = decoder.generate_from_code_long(encoding_indices=codes,
                                              temperature=temperature if decoder_temperature is None else decoder_temperature,
                                              code_index_start=E * nc // U, seed=seed, constraint=token_constraint,
                                              return_logp=return_logp, **decoder_sampling)
        if return_logp:
            return codes, res[0], code_logp, res[1]
        return codes, res

    def plot(self, *a, **k):
        raise NotImplementedError('tensorboard plots (:301-306) are out of scope')
