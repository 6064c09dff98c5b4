"""Decoder training step (reference: VQCPCB/decoders/decoder.py:25-543): a seq2seq
relative transformer that reconstructs the token sequence from the frozen encoder's codes.

Covered: `transformer_type='relative'` with causal target self-attention, anticausal or full source self-attention and
anticausal or full cross-attention, or the aligned ('diagonal') cross block -- getters.py decoder_type 'transformer_relative' /
'transformer_relative_fullCross' / 'transformer_relative_full' / 'transformer_relative_diagonal'.  The diagonal decoder
(TransformerAlignedDecoderLayerCustom, transformer_custom.py:389-492) has no cross-attention: an MLP on the memory gives
every code one vector per voice, which every target token of that code and voice receives (csrc/aligned.hip).
`__init__`, `forward`, `epoch`, `train_model`, `init_optimizers`, `save` / `load` keep the reference's names, argument
meaning, state_dict keys and return contracts.  `generate` / `generate_from_codes` / `init_generation` (:552-726) run
KV-cached incremental decoding on the GPU (decoders/generation.py); `generate_from_code_long`, `generate_alla_mano`,
`compute_start_end_times`, `init_generation_chorale` (:728-854, :960-981, :1054-1062) decode code sequences of any length
by sliding the window, with a K/V-cache re-prefill per move; `reharmonise_tokens` is the body of
`generate_reharmonisation` (:856-958) on a token tensor (the music21 corpus it reads is absent, so that method raises).
A decoder on continuous latents (a `NoQuantization` encoder without upscaler, decoder.py:222-229, :327-336, :595-600) has
`source_embeddings = nn.Linear(dz, d_model)` and takes the encoder's (B, S, dz) latents wherever the others take merged codes.
`check_duplicate` / `check_duplicate_all_corpus` (:983-1017) report the longest run of tokens a generation shares with another
sequence or with the training corpus (csrc/duplicates.hip; dataloaders/corpus.py states the definition and where it departs from
the reference's character-level difflib match).  Plots and the absolute-position variant are out of scope and raise.
`score_tokens` / `score_chorale` / `score_window_plan` (ours) give the log-probability, entropy, rank and arg-max of GIVEN tokens
under the long form's window rule, every window of a piece as one row of a teacher-forced forward (decoders/scoring.py,
csrc/score.hip).
`source_embedding='product'` (ours, `decoder_kwargs['source_embedding']`; default 'merged' = the reference's table of
K**ncb rows): `source_embeddings` is a `ProductEmbedding` (ncb, K, d_model) and a code's source row the sum of the rows of its
ncb digits (quantizer/product_embedding.py).  Merged codes stay the interface; only the lookup differs.

Hot path (`compute_loss`), all numerics in libvqcpc_hip.so:
  * source: `source_embeddings` lookup of the merged codes (gather + deterministic segment-sum gradient), or, on continuous
    latents, `ops.linear(z, W, b)` (z is the frozen encoder's output: no input gradient);
  * target: `linear_target(cat[embed(x), channel emb, event-in-code emb])` depends only on (token, position in a code
    block), so it is evaluated on the vmax * U table rows (U = total_upscaling) by ONE small GEMM and looked up per
    token -- with the start-of-sentence row appended, the reference's shift-by-one (:474-480) is the same lookup with
    shifted indices;
  * transformer: masked / rectangular relative attention kernels (csrc/relattn_x.hip), fused add + LayerNorm, GEMMs;
  * per-voice output projections on the strided rows of each voice, softmax cross-entropy kernels.

Reference defect fixed: `epoch` (:327-344) passes the quantizer's (B, S, num_codebooks) indices to `forward`, which
raises; the codes are merged with `Encoder.merge_codes` first, as `generate` (:600) does.
"""
import ctypes
import os
from datetime import datetime

import numpy as np
import torch
from torch import nn

from .. import ops
from ..quantizer.product_embedding import ProductEmbedding
from ..training import FlatTraining
from ..transformer.transformer_custom import (TransformerAlignedDecoderLayerCustom, TransformerCustom, TransformerDecoderCustom,
                                              TransformerDecoderLayerCustom, TransformerEncoderCustom,
                                              TransformerEncoderLayerCustom, mask_code)
from ..utils import flatten, STEP_LOCK


class HeadsFn(torch.autograd.Function):
    """Per-voice output projections (decoder.py:523-526): logits_c = out[c::nc] W_c^T + b_c on the row-strided view of
    voice c; the input gradient of every voice is written straight into its rows of ONE buffer."""

    @staticmethod
    def forward(ctx, out, nc, *params):
        out = out.contiguous()
        ws, bs = params[0::2], params[1::2]
        logits, padded = [], []
        for c in range(nc):
            N = ws[c].shape[0]
            pn = -N % 4
            wp = torch.nn.functional.pad(ws[c], (0, 0, 0, pn)) if pn else ws[c]
            bp = torch.nn.functional.pad(bs[c], (0, pn)) if pn else bs[c]
            padded.append(wp)
            logits.append(ops.gemm_nt(out[c::nc], wp, bias=bp)[:, :N])
        ctx.save_for_backward(out, *padded)
        ctx.nc = nc
        ctx.sizes = [w.shape[0] for w in ws]
        return tuple(logits)

    @staticmethod
    def backward(ctx, *grads):
        out, *padded = ctx.saved_tensors
        nc = ctx.nc
        d_out = torch.empty_like(out)
        d_params = []
        for c in range(nc):
            N, wp = ctx.sizes[c], padded[c]
            g = grads[c]
            g = torch.nn.functional.pad(g, (0, wp.shape[0] - N)) if wp.shape[0] != N else g.contiguous()
            ops.gemm_nt(g, ops.transpose(wp), out=d_out[c::nc])
            dw, db = ops.gemm_tn(g, out[c::nc])
            d_params += [dw[:N], db[:N]]
        return (d_out, None, *d_params)


class Decoder(FlatTraining, nn.Module):
    def __init__(self, model_dir, dataloader_generator, data_processor, encoder, transformer_type, encoder_attention_type,
                 cross_attention_type, d_model, num_encoder_layers, num_decoder_layers, n_head, dim_feedforward,
                 positional_embedding_size, num_channels_encoder, num_events_encoder, num_channels_decoder,
                 num_events_decoder, dropout, source_embedding='merged'):
        super().__init__()
        if source_embedding not in ('merged', 'product'):
            raise ValueError(f"source_embedding {source_embedding!r}: 'merged' or 'product'")
        if transformer_type != 'relative':
            raise NotImplementedError("transformer_type 'absolute' (learned absolute positions, nn attention without "
                                      'relative bias) is not on the path: SURVEY.md section 8(f) N4 covers the relative decoder')
        assert encoder_attention_type in ['anticausal', 'causal', 'full']
        assert cross_attention_type in ['anticausal', 'causal', 'diagonal', 'full']
        if cross_attention_type == 'causal':
            raise NotImplementedError                      # as the reference (decoder.py:487-488)
        self.transformer_type = transformer_type
        self.encoder_attention_type = encoder_attention_type
        self.cross_attention_type = cross_attention_type
        self.model_dir = model_dir
        self.encoder = encoder
        self.encoder.eval()                                # frozen (:72-75)
        for p in self.encoder.parameters():
            p.requires_grad = False
        self.dataloader_generator = dataloader_generator
        self.data_processor = data_processor
        self.num_tokens_per_channel = self.data_processor.num_tokens_per_channel
        self.num_channels = len(self.num_tokens_per_channel)
        self.d_model = d_model
        self.num_tokens_target = self.data_processor.num_tokens
        self.total_upscaling = int(np.prod(self.encoder.downscaler.downscale_factors))
        assert self.num_tokens_target % self.total_upscaling == 0
        assert self.num_tokens_target == num_channels_decoder * num_events_decoder
        self.target_channel_embeddings = nn.Parameter(torch.randn((1, self.num_channels, positional_embedding_size)))
        self.num_events_per_code = self.total_upscaling // self.num_channels
        self.target_events_positioning_embeddings = nn.Parameter(
            torch.randn((1, self.num_events_per_code, positional_embedding_size)))
        encoder_layer = TransformerEncoderLayerCustom(d_model=d_model, nhead=n_head,
                                                      attention_bias_type='relative_attention',
                                                      num_channels=num_channels_encoder, num_events=num_events_encoder,
                                                      dim_feedforward=dim_feedforward, dropout=dropout)
        diagonal = cross_attention_type == 'diagonal'                                        # :161-186
        layer_class = TransformerAlignedDecoderLayerCustom if diagonal else TransformerDecoderLayerCustom
        decoder_layer = layer_class(d_model=d_model, nhead=n_head, attention_bias_type_self='relative_attention',
                                    attention_bias_type_cross=None if diagonal else 'relative_attention_target_source',
                                    num_channels_encoder=num_channels_encoder, num_events_encoder=num_events_encoder,
                                    num_channels_decoder=num_channels_decoder, num_events_decoder=num_events_decoder,
                                    dim_feedforward=dim_feedforward, dropout=dropout)
        self.transformer = TransformerCustom(
            d_model=self.d_model, nhead=n_head,
            custom_encoder=TransformerEncoderCustom(encoder_layer=encoder_layer, num_layers=num_encoder_layers),
            custom_decoder=TransformerDecoderCustom(decoder_layer=decoder_layer, num_layers=num_decoder_layers))
        self.linear_target = nn.Linear(self.data_processor.embedding_size + positional_embedding_size * 2, self.d_model)
        self.sos = nn.Parameter(torch.randn((1, 1, self.d_model)))
        self.continuous_source = type(self.encoder.quantizer).__name__ == 'NoQuantization'
        self.source_embedding = source_embedding
        if self.continuous_source and source_embedding == 'product':
            raise ValueError("source_embedding 'product' needs a quantised encoder: a NoQuantization encoder has no codes")
        if self.continuous_source:                                                           # :222-229
            if self.encoder.upscaler is not None:
                raise NotImplementedError('a NoQuantization encoder WITH an upscaler: the decoder reads the latents before the '
                                          'upscaler, which the reference does only when upscaler_type is None')
            self.source_dim = int(self.encoder.quantizer.codebook_dim)
            if self.source_dim % 4 != 0 or not 4 <= self.source_dim <= 256:
                raise NotImplementedError(f'continuous source of dimension {self.source_dim}: a multiple of 4 in [4, 256] is needed')
            self.source_embeddings = nn.Linear(self.source_dim, self.d_model)
        elif source_embedding == 'product':                  # ours: a code's row is the sum of one row per codebook
            self.source_dim = None
            self.source_embeddings = ProductEmbedding(self.encoder.quantizer.num_codebooks, self.encoder.quantizer.codebook_size,
                                                      self.d_model)
        else:
            self.source_dim = None
            codebook_size = self.encoder.quantizer.codebook_size ** self.encoder.quantizer.num_codebooks
            self.source_embeddings = nn.Embedding(codebook_size, self.d_model)
        self.pre_softmaxes = nn.ModuleList([nn.Linear(self.d_model, n) for n in self.num_tokens_per_channel])
        self.num_tokens_source = num_channels_encoder * num_events_encoder
        self.scheduler = None

    def __repr__(self):
        names = dict(anticausal='AC', causal='C', full='F', diagonal='D')
        return f'Decoder-{self.transformer_type}-{names[self.encoder_attention_type]}-{names[self.cross_attention_type]}'

    # ---- masks: API-compatible matrices (:292-308); the kernels evaluate the same rules from indices ---------------
    def _generate_square_subsequent_mask(self, sz):
        mask = (torch.triu(torch.ones(sz, sz)) == 1).transpose(0, 1)
        return mask.float().masked_fill(mask == 0, float('-inf')).masked_fill(mask == 1, float(0.0))

    def _generate_anticausal_mask(self, sz, sz_tgt=None):
        mask = self._generate_square_subsequent_mask(sz).t()
        if sz_tgt is not None:
            assert sz_tgt % sz == 0
            mask = torch.repeat_interleave(mask, sz_tgt // sz, dim=0)
        return mask.to(self.sos.device)

    def _generate_causal_mask(self, sz):
        return self._generate_square_subsequent_mask(sz).to(self.sos.device)

    # ---- the trainable parameters (the frozen encoder is excluded) -------------------------------------------------
    def _trainable(self):
        return [self.data_processor, self.target_channel_embeddings, self.target_events_positioning_embeddings,
                self.transformer, self.linear_target, self.sos, self.source_embeddings, self.pre_softmaxes]

    def init_optimizers(self, lr, schedule_lr, dp=None):
        self._init_flat(self._trainable(), self.sos.device, dp)
        self.lr, self.schedule_lr = lr, schedule_lr
        self.optimizer = ops.FlatAdam(self.flat.flat, self.flat.flat_grad, lr=lr, max_norm=5.0)
        self.scheduler = self.lr_lambda if schedule_lr else None
        self.global_step = 0
        self._apply_resume_state()

    # ---- checkpoints (:254-274): one file `decoder` holding the whole state_dict, encoder included -------------------
    def save(self, early_stopped):
        model_dir = self._dir(early_stopped)
        os.makedirs(model_dir, exist_ok=True)
        torch.save(self.state_dict(), f'{model_dir}/decoder')
        self._save_optimizer_state(f'{model_dir}/decoder_optimizer')

    def load(self, early_stopped, device):
        print(f'Loading models {self.__repr__()}')
        model_dir = self._dir(early_stopped)
        ml = torch.device(device)
        self.load_state_dict(torch.load(f'{model_dir}/decoder', map_location=ml))
        self._load_optimizer_state(f'{model_dir}/decoder_optimizer', ml)

    def train(self, mode=True):
        super().train(mode)
        self.encoder.eval()                  # :319-320: the encoder stays in eval mode
        return self

    # ---- forward ---------------------------------------------------------------------------------------------------
    def _target_table(self, dev):
        """(vmax * U + 1, d_model) rows of `linear_target(cat[embed(token), channel emb, event-in-code emb])`: row v * U + u
        holds token v at position u of a code block, the last row is the start-of-sentence row (see module docstring)."""
        nc, U, d = self.num_channels, self.total_upscaling, self.d_model
        tables = self.data_processor.stacked_tables()                                       # (nc, vmax, emb)
        vmax = tables.shape[1]
        syn = torch.arange(vmax, device=dev).repeat_interleave(U)                            # table row v * U + u holds token v
        x_table = ops.EmbedPosFn.apply(syn, tables, self.target_channel_embeddings.view(nc, -1),
                                       self.target_events_positioning_embeddings.view(self.num_events_per_code, -1), U)
        tgt_table = ops.linear(x_table, self.linear_target.weight, self.linear_target.bias)  # (vmax * U, d)
        return torch.cat([tgt_table, self.sos.view(1, d)], dim=0)                            # + start-of-sentence row

    def _target_rows(self, x, table=None):
        """(B, events, channels) int64 on the device -> (B * T, d_model) shifted target rows (see module docstring).  table: a
        `_target_table` the caller already has (one evaluation for many batches of the same weights)."""
        B = x.shape[0]
        U = self.total_upscaling
        dev = x.device
        table = self._target_table(dev) if table is None else table
        vmax = (table.shape[0] - 1) // U
        tok = flatten(x)                                                                     # (B, T), t = event * nc + voice
        T = tok.shape[1]
        idx = tok * U + (torch.arange(T, device=dev) % U)
        shifted = torch.cat([torch.full((B, 1), vmax * U, dtype=idx.dtype, device=dev), idx[:, :-1]], dim=1)
        return ops.EmbeddingFn.apply(table, shifted.reshape(-1))

    def source_rows(self, codes):
        """Merged codes (...) -> (codes.numel(), d_model) source rows: the `source_embeddings` lookup, or, with
        source_embedding='product', the sum of the per-codebook rows of the code's digits."""
        if self.source_embedding == 'product':
            return self.source_embeddings(codes)
        return ops.EmbeddingFn.apply(self.source_embeddings.weight, codes.reshape(-1))

    def _check_source(self, source, name, length=None):
        """The source of this decoder's kind: (B, n) integer merged codes, or (B, n, dz) floating-point latents for a
        continuous decoder; n == length unless length is None.  ValueError otherwise."""
        cont = self.continuous_source
        want = (f'(batch, {length or "num_codes"}, {self.source_dim}) floating-point latents (continuous decoder)' if cont else
                f'(batch, {length or "num_codes"}) merged codes')
        ok = source.dim() == (3 if cont else 2) and source.is_floating_point() == cont and not source.is_complex()
        ok = ok and (not cont or source.shape[2] == self.source_dim) and (length is None or source.shape[1] == length)
        if not ok:
            raise ValueError(f'{name}: {want} expected, got {tuple(source.shape)} {source.dtype}')

    def compute_loss(self, source, x):
        """source (B, S) merged codes [continuous decoder: (B, S, dz) latents], x (B, events, channels) device int64 ->
        (loss, logits per voice, attentions)."""
        self._check_source(source, 'source', self.num_tokens_source)
        B, S = source.shape[:2]
        nc = self.num_channels
        assert x.shape[1] * nc == self.num_tokens_target
        if self.continuous_source:                                                          # :327-336: no gradient into z
            z = source.detach().to(torch.float32).reshape(-1, self.source_dim)
            src = ops.linear(z, self.source_embeddings.weight, self.source_embeddings.bias)
        else:
            src = self.source_rows(source)                                                  # (B * S, d)
        tgt = self._target_rows(x)
        memory_mask = ops.MASK_NONE if self.cross_attention_type == 'diagonal' else mask_code(self.cross_attention_type)   # :487-488
        out, att_dec, att_enc = self.transformer.forward_rows(
            src, tgt, B, mask_code(self.encoder_attention_type), ops.MASK_CAUSAL, memory_mask)
        params = [t for m in self.pre_softmaxes for t in (m.weight, m.bias)]
        logits = HeadsFn.apply(out, nc, *params)                                            # nc x (B * events, V_c)
        ce = sum(ops.SoftmaxCEFn.apply(lg, x[:, :, c].reshape(-1), None) for c, lg in enumerate(logits))
        loss = ce.mean()                                                                    # :529-535
        E = x.shape[1]
        return loss, [lg.reshape(B, E, -1) for lg in logits], att_dec, att_enc

    def forward(self, source, target):
        """API-compatible `Decoder.forward` (:431-543): source (B, S) merged codes [continuous decoder: (B, S, dz) latents],
        target (B, events, channels)."""
        target = self.data_processor.checked(self.data_processor.preprocess(target))
        loss, logits, att_dec, att_enc = self.compute_loss(source.to(target.device), target)
        return {'loss': loss, 'attentions_decoder': att_dec, 'attentions_encoder': att_enc,
                'weights_per_category': logits, 'monitored_quantities': {'loss': loss.item()}}

    def encode(self, x):
        """:327-336 + the merge the reference forgot: frozen encoder, inference only -> merged codes (B, S); continuous
        decoder: the encoder's latents (B, S, dz) float32."""
        if self.continuous_source:
            return self.encoder.encode_latents(x)
        return self.encoder.encode_indices(x, merged=True)

    def _step_compute(self, tensor_dict):
        x = self.data_processor.checked(self.data_processor.preprocess(tensor_dict['x']))
        codes = self.encode(tensor_dict['x'])
        # (the frozen encoder above is inference and stays outside the step's forward arithmetic, on six products)
        def forward():
            loss = self.compute_loss(codes, x)[0]
            return loss, loss.detach()
        return self._forward_backward(forward)

    def train_step(self, tensor_dict, train=True):
        if not train:
            with STEP_LOCK:
                x = self.data_processor.checked(self.data_processor.preprocess(tensor_dict['x']))
                codes = self.encode(tensor_dict['x'])
                with torch.no_grad():
                    return self.compute_loss(codes, x)[0].detach()
        return self._train_step(tensor_dict)

    def epoch(self, data_loader, train=True, num_batches=None):
        assert self.optimizer is not None, 'call init_optimizers(lr, schedule_lr) first'
        return self._scalar_loss_epoch(data_loader, train, num_batches, [self.data_processor, self.encoder.data_processor])

    def train_model(self, batch_size, num_batches, num_epochs, lr, schedule_lr, plot=False, num_workers=0, weight_average=None,
                    **kwargs):
        with self._training_defaults():
            self.init_optimizers(lr=lr, schedule_lr=schedule_lr)
            if weight_average is not None:
                self.enable_weight_averaging(weight_average)
            return self._train_epochs(batch_size, num_batches, num_epochs, num_workers, monitor='loss',
                                      save_best=lambda: self.save(early_stopped=True),
                                      save_every=lambda: self.save(early_stopped=False))

    # ---- generation (:552-726): KV-cached incremental decoding on the GPU, decoders/generation.py --------------------
    def init_generation(self, num_events):
        """:723-726: an all-zero (1, num_events, num_channels) token tensor on the device."""
        return torch.zeros(1, num_events, self.num_channels, dtype=torch.int64, device=self.sos.device)

    def _keep_voices(self, keep_voices):
        """keep_voices -> sorted voice indices (ValueError outside [0, channels))."""
        voices = sorted({int(v) for v in keep_voices})
        if any(not 0 <= v < self.num_channels for v in voices):
            raise ValueError(f'keep_voices: voice indices in [0, {self.num_channels}) expected, got {list(keep_voices)}')
        return voices

    def _constraint_rows(self, constraint, rows, events, first=0, last=None):
        """A public constraint (rows, events, channels) int64, -1 = free -> (rows, events * channels) int64 on the device,
        position-major, with the events outside [first, last) freed.  ValueError on a wrong shape or dtype and -- one host
        check per call -- on a forced token outside its voice's vocabulary."""
        constraint = torch.as_tensor(constraint)
        nc = self.num_channels
        if tuple(constraint.shape) != (rows, events, nc) or constraint.dtype != torch.int64:
            raise ValueError(f'constraint: ({rows}, {events}, {nc}) int64 expected (-1 = free), got {tuple(constraint.shape)} '
                             f'{constraint.dtype}')
        constraint = constraint.to(self.sos.device).clone()
        constraint[:, :first] = -1
        if last is not None:
            constraint[:, last:] = -1
        vocab = torch.tensor([int(v) for v in self.num_tokens_per_channel], dtype=torch.int64, device=constraint.device)
        if bool((constraint >= vocab).any()):
            raise ValueError(f'constraint: a forced token is outside its voice\'s vocabulary {vocab.tolist()}')
        return constraint.reshape(rows, events * nc)

    def _allowed_words(self, allowed, rows, events, first=0, last=None, exclude=None, constraint=None):
        """A public mask `allowed`, bool (rows, events, channels, vmax) or (events, channels, vmax) shared by all rows ->
        the sampler's packed sets (rows or 1, events * channels, 8) int32 on the device: bit i & 31 of word i >> 5 = token i may
        be drawn.  Entries past a voice's vocabulary are ignored (packed as given: the kernel ignores them too) and so are the
        events outside [first, last).  exclude: the per-voice excluded token ids of the call; constraint: its (rows, events *
        channels) constraint as `_constraint_rows` returns it.  ValueError on a wrong shape or dtype and -- one host check per
        call -- on a generated (row, event, voice) that has no allowed token in its vocabulary, none left after `exclude`, or
        a forced token outside its set; the message names the first one."""
        allowed = torch.as_tensor(allowed)
        nc, dev = self.num_channels, self.sos.device
        sizes = [int(v) for v in self.num_tokens_per_channel]
        shape = tuple(allowed.shape)
        if allowed.dtype != torch.bool or allowed.dim() not in (3, 4) or shape[-3:-1] != (events, nc) or \
                (allowed.dim() == 4 and shape[0] != rows):
            raise ValueError(f'allowed: bool ({rows}, {events}, {nc}, vmax) or ({events}, {nc}, vmax) expected, got {shape} '
                             f'{allowed.dtype}')
        vmax = shape[-1]
        if vmax > 256:
            raise ValueError(f'allowed: vmax = {vmax} > 256, the sampler\'s largest vocabulary')
        if vmax < max(sizes):
            raise ValueError(f'allowed: vmax = {vmax} is smaller than the largest voice vocabulary {max(sizes)}')
        allowed = allowed.to(dev).reshape(-1, events, nc, vmax)                                  # (R, ...), R = rows or 1
        last = events if last is None else last
        ids = torch.arange(vmax, device=dev)
        live = allowed & (ids < torch.tensor(sizes, device=dev).unsqueeze(1))                   # inside the voice's vocabulary
        banned = torch.zeros(nc, vmax, dtype=torch.bool, device=dev)
        for c, toks in enumerate(exclude or []):
            for t in toks:
                if 0 <= int(t) < vmax:
                    banned[c, int(t)] = True
        generated = ((torch.arange(events, device=dev) >= first) & (torch.arange(events, device=dev) < last)).view(1, -1, 1)
        empty = ~live.any(-1) & generated
        drained = ~(live & ~banned).any(-1) & generated
        if constraint is not None:
            forced = constraint.view(rows, events, nc)
            picked = live.expand(rows, -1, -1, -1).gather(3, forced.clamp(min=0).unsqueeze(3)).squeeze(3)
            refused = (forced >= 0) & ~picked & generated
        else:
            refused = torch.zeros_like(empty)
        R = max(empty.shape[0], refused.shape[0])
        kinds = torch.stack([k.expand(R, -1, -1).reshape(-1) for k in (empty, drained, refused)])
        bad = kinds.any(0)
        at = bad.to(torch.int32).argmax()
        found, at, e_, d_, r_ = torch.stack([bad.any().long(), at.long(), *kinds[:, at].long()]).tolist()   # the one host check
        if found:
            b, rest = divmod(at, events * nc)
            e, c = divmod(rest, nc)
            what = 'has no allowed token inside its vocabulary' if e_ else \
                'has no allowed token left after exclude_tokens' if d_ else \
                f'is forced to token {int(constraint.view(rows, events, nc)[b, e, c])}, which its allowed set forbids'
            raise ValueError(f'allowed: (row {b}, event {e}, voice {c}) {what}')
        bits = torch.zeros(allowed.shape[0], events * nc, 256, dtype=torch.int32, device=dev)
        bits[:, :, :vmax] = allowed.reshape(-1, events * nc, vmax)
        weights = torch.tensor([1 << k for k in range(31)] + [-(1 << 31)], dtype=torch.int32, device=dev)
        return (bits.view(-1, events * nc, 8, 32) * weights).sum(-1, dtype=torch.int32)

    def _attention_layers(self, return_attentions, default=None):
        """return_attentions -> None (False), or the sorted tuple of decoder-layer indices to record: True = every layer
        (`default`, when given), an iterable = those layers.  ValueError on an index outside the stack or an empty choice."""
        nl = len(self.transformer.decoder.layers)
        if return_attentions is False or return_attentions is None:
            return None
        if return_attentions is True:
            return tuple(range(nl)) if default is None else tuple(default)
        try:
            layers = sorted({int(li) for li in return_attentions})
        except TypeError:
            raise ValueError(f'return_attentions: False, True or an iterable of layer indices expected, got {return_attentions!r}')
        if not layers or layers[0] < 0 or layers[-1] >= nl:
            raise ValueError(f'return_attentions: layer indices in [0, {nl}) expected, got {list(return_attentions)}')
        return tuple(layers)

    def _check_attention_bytes(self, B, layers, rows, with_encoder, max_attention_bytes):
        """The bytes of the requested maps for B sequences and `rows` recorded positions; ValueError above the limit."""
        H = self.transformer.nhead
        T, S = self.num_tokens_target, self.num_tokens_source
        keys = T + (0 if self.cross_attention_type == 'diagonal' else S)
        nbytes = 4 * B * len(layers) * H * rows * keys
        if with_encoder:
            nbytes += 4 * B * len(self.transformer.encoder.layers) * H * S * S
        if nbytes > max_attention_bytes:
            raise ValueError(f'return_attentions: the maps of {len(layers)} layer(s) for {B} sequences take {nbytes} bytes '
                             f'({nbytes / 2 ** 30:.2f} GiB), above max_attention_bytes = {max_attention_bytes}; ask for fewer '
                             'layers or fewer sequences, or raise max_attention_bytes')
        return nbytes

    @staticmethod
    def attention_window_starts(num_blocks, num_blocks_model, tokens_per_block, code_index_start, code_index_end):
        """(num_blocks * tokens_per_block,) int64 on the host: for every chorale position, the first code of the model window
        in which `generate_from_code_long` emits it -- `compute_start_end_times` of its code, as `run_long` walks it -- or -1
        for the positions of codes outside [code_index_start, code_index_end), which are never emitted."""
        out = torch.full((num_blocks * tokens_per_block,), -1, dtype=torch.int64)
        for ci in range(code_index_start, code_index_end):
            out[ci * tokens_per_block:(ci + 1) * tokens_per_block] = Decoder.compute_start_end_times(ci, num_blocks,
                                                                                                     num_blocks_model)[0]
        return out

    def generate_from_codes(self, codes, temperature=1.0, top_k=0, top_p=1.0, num_decodings=1, exclude_tokens=None, seed=None,
                            use_graph=True, constraint=None, return_logp=False, return_attentions=False,
                            max_attention_bytes=4 << 30, allowed=None, return_allowed_mass=False, particles=None,
                            resample_threshold=0.5, return_particles=False, rules=None, return_rule_report=False, beam=None,
                            return_beams=False, no_copy=None, return_copy_report=False):
        """Samples target sequences from MERGED codes (B, S) (what `forward` takes; a continuous decoder takes (B, S, dz)
        latents, ValueError on the other kind): each row repeated `num_decodings` times
        (repeat_interleave, as generate_from_code_long :747-752), then one token per position with the reference's
        temperature / top-k / top-p rule (utils.py:101-128) on the GPU.
        exclude_tokens: per voice, token ids never drawn (the meta symbols of exclude_meta_symbols); seed: an int (per-row
        seeds derived from it), a per-row int64 tensor, or None (drawn from torch's generator).  use_graph=False runs the
        steps eagerly (same tokens).  -> int64 tokens (B * num_decodings, events, channels) on the device.
        constraint: (B, events, channels) int64, a token >= 0 is emitted at its place (also one listed in exclude_tokens),
        -1 leaves it to the sampler; rows are repeated with num_decodings like the codes.  The free positions draw what
        they would draw without the constraint given the same prefix (the draw is keyed by seed and position).
        return_logp=True -> (tokens, logp): logp float32 of the tokens' shape, every emitted token's log-probability
        under the model's unfiltered distribution (temperature 1, no top-k / top-p / exclusion).
        return_attentions: True (every decoder layer) or an iterable of decoder-layer indices (ValueError outside the stack)
        -> `attentions` as the LAST element of the result, (tokens, attentions) or (tokens, logp, attentions): what every
        emitted token attended to (the reference keeps these rows in its generate loop, :647-667), a dict of
          'layers'              the recorded decoder layers, a tuple
          'self_attns_decoder'  (B', layers, H, T, T) float32, row t = the attention of token t over the tokens written so far
                                (exactly 0 above the diagonal)
          'attns_cross'         (B', layers, H, T, S) over the codes; None for the diagonal decoder, which has no cross attention
          'self_attns_encoder'  (B', encoder layers, H, S, S), the source encoder's maps (every layer: they are computed anyway)
        with B' = B * num_decodings, on the device.  The rows are the ones the step's attention kernel multiplies V by
        (vqcpc_decode_attn_probs); tokens and logp are bit-identical to a call without the keyword.  The maps' bytes are computed
        first: ValueError above max_attention_bytes (default 4 GiB).
        allowed: bool (B, events, channels, vmax) or (events, channels, vmax) shared by all rows, max V_c <= vmax <= 256: at
        (row, event, voice) only the tokens whose entry is True may be drawn (entries past the voice's vocabulary are
        ignored); rows are repeated with num_decodings.  The set acts where exclude_tokens does -- before top-k / top-p, which
        then choose among the allowed tokens -- and a token forced by `constraint` must be in its set.  ValueError, from one
        host check per call, naming the first (row, event, voice) whose set has no token of its vocabulary, none left after
        exclude_tokens, or forbids its forced token (`templates.py` builds such masks from a corpus's token names).
        return_allowed_mass=True -> `allowed_mass` after tokens and logp, float32 of the tokens' shape: the log of the
        probability the model's unfiltered distribution gives to the position's allowed set (0 where nothing is restricted).
        Results come in the order (tokens[, logp][, allowed_mass][, attentions]).  Either keyword switches the step's sampler
        to vqcpc_decode_sample_masked; without them every launch is what it was.
        particles: None, or P in [2, 64]: a particle filter over the forced tokens and the sets.  Every row (after
        num_decodings) becomes a group of P consecutive rows with their own seeds; after every code a row's weight grows by
        the log-probability of its forced tokens and the allowed mass of its restricted ones, and a group whose effective
        sample size fell below resample_threshold * P (0: never, 1: whenever the weights differ) is resampled systematically:
        whole rows -- tokens, scores, K/V caches -- are copied onto others (vqcpc_particle_resample, vqcpc_particle_permute_*),
        so the free choices that the later forced tokens make unlikely die out.  After the last code one forced resampling
        makes the first row of every group a draw from the final weights, and that row is returned: the result shapes are
        those of a call without particles.  return_particles=True skips it and returns all B' * P rows (tokens[, logp]
        [, allowed_mass]) followed by a dict: 'weights' (B', P) the final normalised weights, 'log_evidence' (B',) the log of
        the estimated probability of the constraints, and per code 'ancestors' (codes, B' * P) int32 row indices (-1: no code
        finished there), 'wn' (codes, B' * P) and 'ess' (codes, B').  The filter is exact -- a properly weighted sample and
        an unbiased evidence estimate -- for temperature=1, top_k=0, top_p=1; with a filtered proposal it is the heuristic
        that logp itself is, which always scores the unfiltered distribution.  ValueError with return_attentions.  Without
        `particles` every launch, buffer and result is what it was.
        rules: None, or a `templates.VoiceLeadingRules` (no crossing, bounded leaps, no parallel fifths / octaves): before every
        draw vqcpc_decode_rules narrows the position's set -- `allowed`'s, or the whole vocabulary -- to the tokens that break
        no rule against the voices already drawn at the tick and those `constraint` forces, relaxing the rules where none is
        left.  It switches the step to the masked sampler as `allowed` does and combines with `allowed`, `constraint`,
        `exclude_tokens` and `particles`; `allowed_mass` is then the mass of the narrowed set, so the particle weights see the
        rules and rows that paint themselves into a corner die out.  return_rule_report=True -> `rule_report` after
        allowed_mass and before attentions, int32 of the tokens' shape: at a drawn position the rules that had to be dropped
        (bit 0 crossing, 1 leap, 2 parallel), at a forced one the rules its token breaks << 4.  Results:
        (tokens[, logp][, allowed_mass][, rule_report][, attentions][, particles][, beams]).  Without the keywords every launch,
        buffer and result is what it was.
        beam: None, or W in [1, 64]: a beam search in the sampler's place, the model's W most probable continuations instead of a
        draw.  Every row becomes a group of W consecutive rows of the stack; at every position vqcpc_decode_beam_select expands each
        row into its candidate tokens -- the forced token, or the tokens `allowed`, `rules` and `exclude_tokens` leave -- scores
        them by the hypothesis's total log-probability under the model's own distribution (what `logp` scores), keeps the
        group's W best (ties: the lower row, then the lower token) and the rows' tokens, scores and K/V caches follow their
        ancestors (vqcpc_particle_permute_*).  The search is deterministic: `seed` is accepted and unused.  The result has the
        shapes of a call without the keyword and holds each group's best hypothesis, for tokens[, logp][, allowed_mass]
        [, rule_report].  return_beams=True returns all B * W rows in slot order, best first, followed by a dict: 'scores' (B, W)
        float32, the hypotheses' total log-probabilities, non-increasing along W and -inf for a dead slot (fewer than W
        sequences exist), and 'ancestors' (positions, B * W) int32, per generated position the row each slot descends from (-1
        where nothing was generated).  ValueError with `particles`, `return_attentions`, num_decodings != 1, or a filter
        (temperature other than 1, top_k, top_p): a filter has no meaning for a search.  Without `beam` every launch, buffer
        and result is what it was.
        no_copy: None, or a `dataloaders.corpus.CopyIndex` (`copy_index(max_copy)`): a generation that cannot recite the corpus.
        Before every draw vqcpc_decode_nocopy looks the row's last max_copy tokens up in the index and takes out of the
        position's set -- `allowed`'s, the rules', or the whole vocabulary -- every token that would complete a run of
        max_copy + 1 tokens shared with the corpus (same voice, inside one piece: `check_duplicate_all_corpus`'s run).  It
        switches the step to the masked sampler and combines with `constraint`, `allowed`, `exclude_tokens`, `rules`,
        `particles` and `beam`; `allowed_mass` is the mass of the narrowed set, so particles that can only go on by copying
        lose weight.  return_copy_report=True -> `copy_report` after rule_report and before attentions, int32 of the tokens'
        shape: bits 0-8 the number of tokens the guard took out of the set; bit 16 RELAXED, every token left was banned and
        the set was used as it came; bit 17 FORCED_COPY, a token forced by `constraint` was banned.  A row without either
        flag shares no run longer than max_copy with the index's pieces.  ValueError for a decoder whose voices or
        vocabularies are not the index's, or an index on another device.  Without the keyword every launch, buffer and
        result is what it was."""
        return self._result_tuple(self._window_results(
            codes, exclude_tokens, use_graph, temperature=temperature, top_k=top_k, top_p=top_p, num_decodings=num_decodings,
            seed=seed, constraint=constraint, return_logp=return_logp, return_attentions=return_attentions,
            max_attention_bytes=max_attention_bytes, allowed=allowed, return_allowed_mass=return_allowed_mass, particles=particles,
            resample_threshold=resample_threshold, return_particles=return_particles, rules=rules,
            return_rule_report=return_rule_report, beam=beam, return_beams=return_beams, no_copy=no_copy,
            return_copy_report=return_copy_report))

    def _window_results(self, codes, exclude_tokens, use_graph, **options):
        """`generate_from_codes` with its results by name (`_generate_rows`)."""
        def drive(inc, codes, settings):
            inc.prefill(codes)
            inc.start(**settings)
            return inc.run(use_graph=use_graph)
        form = lambda codes: dict(events=self.num_tokens_target // self.num_channels, first=0, last=None, exclude=exclude_tokens,
                                  drive=drive, maps=lambda: {'self_attns_encoder': []})
        return self._generate_rows(codes, 'codes', self.num_tokens_source, form, **options)

    def _generate_rows(self, source, name, length, form, temperature=1.0, top_k=0, top_p=1.0, num_decodings=1, seed=None,
                       constraint=None, return_logp=False, return_attentions=False, max_attention_bytes=4 << 30, allowed=None,
                       return_allowed_mass=False, particles=None, resample_threshold=0.5, return_particles=False, rules=None,
                       return_rule_report=False, beam=None, return_beams=False, no_copy=None, return_copy_report=False):
        """The body the public generators share: the option checks, then the source (`_source_on_device(source, name, length)`),
        then `form(codes)`, what the fixed window and the chorale differ in -- a dict of
          events, first, last   the events of a row, and the range [first, last) of them that is generated
          exclude               the per-voice excluded token ids
          drive                 drive(stack, the chunk's codes, the keywords of its `start`) -> the chunk's (n, events * channels) tokens
          maps                  maps() -> the attention maps kept next to the decoder's: 'self_attns_encoder': [] (the stack's
                                `enc_probs` of every chunk) or 'window_start': a tensor
        -- then packing, repetition by num_decodings * particles (or the beam width), seeds, the chunks on their own stacks and their records.
        -> a dict in the documented order of the results, every row (a group's first one with particles or a beam, unless they are
        returned) as (rows, events, channels): 'tokens', 'logp', 'allowed_mass', 'rule_report', 'copy_report', then 'attentions',
        'particles' and 'beams'; what was not asked for is None."""
        from ..transformer.incremental import MAX_ROWS, generate_in_chunks, row_seeds
        from .generation import IncrementalDecoder
        dev, nc = self.sos.device, self.num_channels
        layers = self._attention_layers(return_attentions)
        P = self._particle_count(particles, resample_threshold, return_particles, layers)
        W = self._beam_width(beam, return_beams, particles, layers, num_decodings, temperature, top_k, top_p)
        if beam is not None:
            P, temperature = W, 1.0                           # the group size of the chunks below, whichever kind the groups are
        self._check_rules(rules, return_rule_report)
        self._check_no_copy(no_copy, return_copy_report)
        codes = self._source_on_device(source, name, length)
        form = form(codes)
        events, first, last, exclude = form['events'], form['first'], form['last'], form['exclude']
        if constraint is not None:
            constraint = self._constraint_rows(constraint, codes.shape[0], events, first, last)
        if allowed is not None:
            allowed = self._allowed_words(allowed, codes.shape[0], events, first, last, exclude=exclude, constraint=constraint)
        if num_decodings * P > 1:
            codes = codes.repeat_interleave(num_decodings * P, dim=0)
            if constraint is not None:
                constraint = constraint.repeat_interleave(num_decodings * P, dim=0)
            if allowed is not None and allowed.shape[0] > 1:
                allowed = allowed.repeat_interleave(num_decodings * P, dim=0)
        B, width = codes.shape[0], events * nc
        seeds = row_seeds(seed, B)
        settings = dict(temperature=temperature, top_k=top_k, top_p=top_p, exclude=exclude, want_logp=return_logp,
                        want_attentions=layers, want_allowed_mass=return_allowed_mass, particles=None if particles is None else P,
                        resample_threshold=resample_threshold, final_resample=not return_particles, rules=rules,
                        beam=None if beam is None else W)
        if no_copy is not None:                               # only then: the stacks' `start` is called as before without it
            settings['no_copy'] = no_copy
        kept = {'logp': ('logp', torch.float32, return_logp), 'allowed_mass': ('logmass', torch.float32, return_allowed_mass),
                'rule_report': ('rule_report', torch.int32, return_rule_report),          # result: the stack's buffer, ...
                'copy_report': ('copy_report', torch.int32, return_copy_report)}
        records = {key: torch.empty(B, width, dtype=dtype, device=dev) for key, (_, dtype, wanted) in kept.items() if wanted}
        maps = filt = None
        if layers is not None:
            maps = {'layers': layers, 'self_attns_decoder': [], 'attns_cross': [], **form['maps']()}
            self._check_attention_bytes(B, layers, width, 'self_attns_encoder' in maps, max_attention_bytes)
        if particles is not None or beam is not None:
            filt = {}

        def chunk(n, rows):
            inc = IncrementalDecoder(self, n)
            tokens = form['drive'](inc, codes[rows], dict(settings, seeds=seeds[rows],
                                                          constraint=None if constraint is None else constraint[rows],
                                                          allowed=self._allowed_rows(allowed, n, rows)))
            for key, buf in records.items():
                buf[rows] = getattr(inc, kept[key][0])
            if maps is not None:
                maps['self_attns_decoder'].append(inc.self_probs.transpose(0, 1))
                maps['attns_cross'].append(None if inc.cross_probs is None else inc.cross_probs.transpose(0, 1))
                if 'self_attns_encoder' in maps:
                    maps['self_attns_encoder'].append(torch.stack(inc.enc_probs, dim=1))
            if filt is not None:
                self._keep_particle_results(filt, inc.particle_results() if beam is None else inc.beam_results(), rows.start)
            return tokens
        tokens = generate_in_chunks(self, B, width, chunk, MAX_ROWS // P * P)        # whole groups (P = 1: MAX_ROWS, as before)
        whole = return_particles if beam is None else return_beams
        keep = slice(None) if P == 1 or whole else slice(0, B, P)        # a group's first row: the survivor / the best hypothesis
        nk = len(range(B)[keep])
        res = {'tokens': tokens, **{key: records.get(key) for key in kept}}
        res = {key: None if t is None else t[keep].view(nk, events, nc) for key, t in res.items()}
        res['attentions'] = None if maps is None else self._join_attention_chunks(maps)
        res['particles'] = self._join_particle_results(filt) if return_particles and filt is not None else None
        res['beams'] = self._join_particle_results(filt) if return_beams and filt is not None else None
        return res

    @staticmethod
    def _result_tuple(res, cut=lambda t: t):
        """`_generate_rows`'s results -> the documented (tokens[, logp][, allowed_mass][, rule_report][, attentions][, particles]
        [, beams]),
        `tokens` alone when nothing else was asked for; cut: applied to the per-token tensors."""
        out = tuple(cut(v) if torch.is_tensor(v) else v for v in res.values() if v is not None)
        return out if len(out) > 1 else out[0]

    def _check_rules(self, rules, return_rule_report):
        """The checks of the rule keywords, once per call."""
        from ..templates import VoiceLeadingRules
        if rules is None:
            if return_rule_report:
                raise ValueError('return_rule_report=True needs rules=templates.VoiceLeadingRules(...)')
            return
        sizes = [int(v) for v in self.num_tokens_per_channel]
        if not isinstance(rules, VoiceLeadingRules):
            raise ValueError(f'rules: None or a templates.VoiceLeadingRules expected, got {type(rules).__name__}')
        if rules.kinds.shape[0] != self.num_channels or rules.kinds.shape[1] < max(sizes):
            raise ValueError(f'rules: a kinds table ({self.num_channels}, >= {max(sizes)}) expected for this decoder, got '
                             f'{tuple(rules.kinds.shape)}')

    def _check_no_copy(self, no_copy, return_copy_report):
        """The checks of the copy-guard keywords, once per call."""
        from ..dataloaders.corpus import CopyIndex
        if no_copy is None:
            if return_copy_report:
                raise ValueError('return_copy_report=True needs no_copy=copy_index(max_copy)')
            return
        if not isinstance(no_copy, CopyIndex):
            raise ValueError(f'no_copy: None or a dataloaders.corpus.CopyIndex expected, got {type(no_copy).__name__}')
        sizes = tuple(int(v) for v in self.num_tokens_per_channel)
        if self.num_channels != 4 or sizes != tuple(no_copy.vocab):
            raise ValueError(f'no_copy: the index is of a corpus with 4 voices and the vocab {tuple(no_copy.vocab)}, the decoder has '
                             f'{self.num_channels} voices and {sizes}')
        if no_copy.device != self.sos.device:
            raise ValueError(f'no_copy: the index lives on {no_copy.device}, the decoder on {self.sos.device}')

    def copy_index(self, max_copy, split='train'):
        """The copy guard's index (`generate_from_codes(no_copy=...)`) over the pieces of `split`, resolved as
        `check_duplicate_all_corpus` resolves it (None: every piece): `DeviceCorpus.copy_index`, built once and device resident.
        Needs a corpus dataloader generator; the synthetic ones have no corpus and raise ValueError."""
        dc = getattr(self.dataloader_generator, 'device_corpus', None)
        if dc is None:
            raise ValueError('copy_index needs a corpus dataloader generator (dataloaders/corpus.py); '
                             f'{type(self.dataloader_generator).__name__} has no corpus')
        pieces = None
        if split is not None:
            pieces = dc.split_pieces(split, self.dataloader_generator.sequences_size)
            if pieces[0] == pieces[1]:
                raise ValueError(f'copy_index: no piece begins in the {split} split')
        return dc.copy_index(max_copy, pieces=pieces)

    def audit_copies(self, x, index):
        """x: (rows, events, 4) tokens, index: a `CopyIndex` -> int32 of x's shape: FORCED_COPY (bit 17) where the token completes a
        run of max_copy + 1 tokens shared with the index's pieces, else 0 -- a copy map of an existing piece, without running the
        model (vqcpc_nocopy_audit).  Every token is taken as given."""
        from .. import hip
        self._check_no_copy(index, False)
        if index is None:
            raise ValueError('audit_copies: index=copy_index(max_copy) is needed')
        x = torch.as_tensor(x)
        nc, dev = self.num_channels, self.sos.device
        if x.dim() != 3 or x.shape[2] != nc or x.shape[0] < 1 or x.shape[1] < 1 or x.dtype != torch.int64:
            raise ValueError(f'x: (rows, events, {nc}) int64 tokens expected, got {tuple(x.shape)} {x.dtype}')
        rows, events = x.shape[0], x.shape[1]
        flat = x.to(dev).reshape(rows, events * nc).contiguous()
        report = torch.empty(rows, events * nc, dtype=torch.int32, device=dev)
        for r0 in range(0, rows, 65535):
            n = min(65535, rows - r0)
            hip.call('vqcpc_nocopy_audit', flat[r0:r0 + n], events * nc, events * nc, *index.args(), report[r0:r0 + n], events * nc, n)
        return report.view(rows, events, nc)

    def audit_voice_leading(self, x, rules):
        """x: (rows, events, channels) tokens, rules: a `templates.VoiceLeadingRules` -> int32 of x's shape: the enabled rules
        every token breaks against the other voices of its tick and the pitches held before it, << 4 (bit 4 crossing, 5 leap,
        6 parallel) -- the forced half of `rule_report`, for a whole piece and without running the model (vqcpc_rules_audit).
        Every token is taken as given, so a pair of voices that breaks a rule is reported at both."""
        from .. import hip
        self._check_rules(rules, False)
        if rules is None:
            raise ValueError('audit_voice_leading: rules=templates.VoiceLeadingRules(...) is needed')
        x = torch.as_tensor(x)
        nc, dev = self.num_channels, self.sos.device
        if x.dim() != 3 or x.shape[2] != nc or x.shape[0] < 1 or x.shape[1] < 1 or x.dtype != torch.int64:
            raise ValueError(f'x: (rows, events, {nc}) int64 tokens expected, got {tuple(x.shape)} {x.dtype}')
        rows, events = x.shape[0], x.shape[1]
        flat = x.to(dev).reshape(rows, events * nc).contiguous()
        offsets = [0]
        for v in self.num_tokens_per_channel:
            offsets.append(offsets[-1] + int(v))
        report = torch.empty(rows, events * nc, dtype=torch.int32, device=dev)
        kinds, leap = rules.kinds.to(dev).contiguous(), rules.max_leap.to(dev).contiguous()
        for r0 in range(0, rows, 65535):
            n = min(65535, rows - r0)
            hip.call('vqcpc_rules_audit', flat[r0:r0 + n], events * nc, events * nc, kinds, kinds.shape[1],
                     (ctypes.c_int32 * (nc + 1))(*offsets), nc, leap, rules.mask, report[r0:r0 + n], events * nc, n)
        return report.view(rows, events, nc)

    @staticmethod
    def _particle_count(particles, resample_threshold, return_particles, attention_layers):
        """The checks of the particle keywords, once per call -> the group size (1 without particles)."""
        if particles is None:
            if return_particles:
                raise ValueError('return_particles=True needs particles=P')
            return 1
        if isinstance(particles, bool) or int(particles) != particles or not 2 <= int(particles) <= 64:
            raise ValueError(f'particles: None or an integer in [2, 64] expected, got {particles!r}')
        if not 0.0 <= float(resample_threshold) <= 1.0:
            raise ValueError(f'resample_threshold: a share of the particles in [0, 1] expected, got {resample_threshold!r}')
        if attention_layers is not None:
            raise ValueError('return_attentions with particles: the maps of a row are not moved when the row is resampled')
        return int(particles)

    @staticmethod
    def _beam_width(beam, return_beams, particles, attention_layers, num_decodings, temperature, top_k, top_p):
        """The checks of the beam keywords, once per call -> the beam width (1 without a beam).  temperature None: the caller's
        default."""
        if beam is None:
            if return_beams:
                raise ValueError('return_beams=True needs beam=W')
            return 1
        if isinstance(beam, bool) or int(beam) != beam or not 1 <= int(beam) <= 64:
            raise ValueError(f'beam: None or an integer in [1, 64] expected, got {beam!r}')
        if particles is not None:
            raise ValueError('beam with particles: a search and a particle filter both own the groups of rows; pass one of the two')
        if attention_layers is not None:
            raise ValueError('return_attentions with beam: the maps of a row are not moved when a hypothesis takes the row')
        if num_decodings != 1:
            raise ValueError(f'beam with num_decodings={num_decodings}: the search is deterministic, every decoding would be the '
                             f'same; num_decodings must be 1 (return_beams=True returns the W best)')
        if (temperature is not None and float(temperature) != 1.0) or top_k != 0 or 0.0 < float(top_p) < 1.0:
            raise ValueError(f'beam with temperature={temperature}, top_k={top_k}, top_p={top_p}: the search scores the model\'s '
                             f'own distribution, a filter has no meaning for it; temperature 1, top_k 0 and top_p 1 expected')
        return int(beam)

    @staticmethod
    def _keep_particle_results(filt, res, row0):
        """A chunk's filter results; its ancestors become row indices of the whole call (the chunk starts at row `row0`)."""
        anc = res['ancestors']
        res = dict(res, ancestors=torch.where(anc >= 0, anc + row0, anc))
        for key, val in res.items():
            filt.setdefault(key, []).append(val)

    @staticmethod
    def _join_particle_results(filt):
        return {key: torch.cat(parts, dim=0 if key in ('weights', 'log_evidence', 'scores') else 1).contiguous()
                for key, parts in filt.items()}

    @staticmethod
    def _allowed_rows(words, n, rows):
        """The packed sets of a chunk's n rows (a shared mask has one row: a broadcast view, copied by the stack)."""
        if words is None:
            return None
        return words.expand(n, -1, -1) if words.shape[0] == 1 else words[rows]

    @staticmethod
    def _join_attention_chunks(maps):
        """The per-chunk lists of (n, ...) maps -> one (B, ...) tensor each (a single chunk's buffer is returned as it is)."""
        for key, parts in list(maps.items()):
            if key in ('layers', 'window_start'):
                continue
            maps[key] = None if parts[0] is None else (parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)).contiguous()
        return maps

    def _source_on_device(self, source, name, length=None):
        source = torch.as_tensor(source)
        self._check_source(source, name, length)
        return source.to(self.sos.device, torch.float32 if self.continuous_source else torch.int64).contiguous()

    def _meta_symbol_ids(self):
        ds = getattr(self.dataloader_generator, 'dataset', None)
        n2i = getattr(ds, 'note2index_dicts', None)
        if n2i is None:
            raise ValueError('exclude_meta_symbols=True needs dataset.note2index_dicts with the START / END / PAD symbols; '
                             'this dataset (e.g. the synthetic one) has no meta symbols')
        syms = ('START', 'END', 'XX')                  # START_SYMBOL, END_SYMBOL, PAD_SYMBOL (datasets/helpers.py:5-9)
        return [[n2i[c][s] for s in syms if s in n2i[c]] for c in range(self.num_channels)]

    def generate(self, temperature, batch_size=1, top_k=0, top_p=1., seed_set=None, exclude_meta_symbols=False,
                 plot_attentions=False, code_juxtaposition=False, seed=None, keep_voices=None, return_attentions=False,
                 max_attention_bytes=4 << 30, particles=None, resample_threshold=0.5, rules=None, return_rule_report=False,
                 beam=None, return_beams=False, no_copy=None, return_copy_report=False):
        """:552-721: a seed chorale from the train / val stream (or, code_juxtaposition, the first half of one and the
        second half of another), its merged codes, `batch_size` generations from them, the codes of original +
        generations written to {model_dir}/generations/<timestamp>.txt ({model_dir}/juxtapositions with
        code_juxtaposition) as the reference writes them.  Returns {'original', 'generation', 'codes', 'recoding'} tensors
        instead of music21 scores (no score writing here).  seed: as generate_from_codes.  A continuous decoder returns
        the latents as 'codes', 'recoding' None and writes no file (:674-701).  keep_voices: voice indices whose tokens
        are forced to the seed chorale's (`generate_from_codes(constraint=...)`): the other voices are written around them.
        return_attentions: True records decoder layer min(2, layers - 1) (the reference's plot_attentions block hard-codes layer
        2, :649), an iterable chooses the layers; the result gains 'attentions', the dict of `generate_from_codes`, and next to
        the codes file {timestamp}_attentions.npz holds the reference's three stems as arrays (no PDF is drawn): attns_cross
        (absent for the diagonal decoder), self_attns_decoder and self_attns_encoder, each (batch, H, T, keys) for the FIRST
        recorded layer (the encoder's layer of that index, or its last), plus `layers`.  Row t of self_attns_encoder is the
        encoder's row (t // channels * channels) // tokens-per-code, the code of t's event (:650-659).
        particles, resample_threshold: `generate_from_codes`'s particle filter over the kept voices (each of the `batch_size`
        generations is the survivor of its own group of `particles` rows).
        rules, return_rule_report: `generate_from_codes`'s voice-leading rules; the result gains 'rule_report'.
        beam, return_beams: `generate_from_codes`'s beam search (temperature must be 1): each of the `batch_size` generations is
        the best hypothesis of its own group -- the same one, the search being deterministic --; with return_beams 'generation'
        holds all batch_size * beam rows and the result gains 'beams'.
        no_copy, return_copy_report: `generate_from_codes`'s copy guard; the result gains 'copy_report'."""
        if plot_attentions:
            raise NotImplementedError('plot_attentions: no plots are drawn here (no matplotlib); return_attentions=True returns '
                                      'the attention maps of every emitted token and writes them as arrays')
        nl = len(self.transformer.decoder.layers)
        layers = self._attention_layers(return_attentions, default=(min(2, nl - 1),))
        exclude = self._meta_symbol_ids() if exclude_meta_symbols else None
        voices = None if keep_voices is None else self._keep_voices(keep_voices)
        generator_train, generator_val, _ = self.dataloader_generator.dataloaders(batch_size=1, shuffle_val=True)
        if seed_set == 'val':
            stream = generator_val
        elif seed_set == 'train':
            stream = generator_train
        else:
            raise Exception('Need to indicate seeds dataset')
        dev = self.sos.device
        if code_juxtaposition:
            beginning, end = next(iter(stream)), next(iter(stream))
            half = beginning['x'].shape[1] // 2
            x_original_single = torch.cat([beginning['x'][:, :half], end['x'][:, half:]], dim=1)
        else:
            x_original_single = next(iter(stream))['x']
        x_original_single = x_original_single.to(dev).long()
        x_original = x_original_single.repeat(batch_size, 1, 1)
        was_training = self.training
        self.eval()
        try:
            codes = self.encode(x_original)
            constraint = None
            if voices is not None:
                constraint = torch.full_like(x_original, -1)
                constraint[:, :, voices] = x_original[:, :, voices]
            res = self._window_results(codes, exclude, True, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                       constraint=constraint, return_attentions=layers or False,
                                       max_attention_bytes=max_attention_bytes, particles=particles,
                                       resample_threshold=resample_threshold, rules=rules, return_rule_report=return_rule_report,
                                       beam=beam, return_beams=return_beams, no_copy=no_copy,
                                       return_copy_report=return_copy_report)
            x, rule_report, attentions = res['tokens'], res['rule_report'], res['attentions']
            recoding = None if self.continuous_source else self.encode(torch.cat([x_original_single, x], dim=0))
        finally:
            self.train(was_training)
        extra = {} if attentions is None else {'attentions': attentions}
        if rule_report is not None:
            extra['rule_report'] = rule_report
        if res['copy_report'] is not None:
            extra['copy_report'] = res['copy_report']
        if res['beams'] is not None:
            extra['beams'] = res['beams']
        if recoding is None:
            return {'original': x_original, 'generation': x, 'codes': codes, 'recoding': None, **extra}
        timestamp = datetime.now().strftime('%Y-%m-%d_%H-%M-%S')
        save_dir = f'{self.model_dir}/juxtapositions' if code_juxtaposition else f'{self.model_dir}/generations'
        os.makedirs(save_dir, exist_ok=True)
        with open(f'{save_dir}/{timestamp}.txt', 'w') as ff:
            for aa in recoding.cpu().numpy():
                ff.write(' , '.join(map(str, list(aa))))
                ff.write('\n')
        if attentions is not None:
            np.savez(f'{save_dir}/{timestamp}_attentions.npz', **self._attention_arrays(attentions))
        print(f'Saved in {save_dir}/{timestamp}')
        return {'original': x_original, 'generation': x, 'codes': codes, 'recoding': recoding, **extra}

    def _attention_arrays(self, attentions):
        """The three stems of the reference's plot_attentions block (:647-667, :711-720) for the first recorded layer, as
        host arrays (batch, H, T, keys)."""
        layer = attentions['layers'][0]
        enc = attentions['self_attns_encoder']
        enc = enc[:, min(layer, enc.shape[1] - 1)]                                           # (B, H, S, S)
        t = torch.arange(self.num_tokens_target, device=enc.device)
        enc_rows = (t // self.num_channels * self.num_channels) // self.total_upscaling      # the code of t's event
        arrays = {'layers': np.asarray(attentions['layers'], dtype=np.int64),
                  'self_attns_decoder': attentions['self_attns_decoder'][:, 0].cpu().numpy(),
                  'self_attns_encoder': enc[:, :, enc_rows].cpu().numpy()}
        if attentions['attns_cross'] is not None:
            arrays['attns_cross'] = attentions['attns_cross'][:, 0].cpu().numpy()
        return arrays

    # ---- long-form generation (:728-1062): sliding-window decoding with KV-cache re-prefill, decoders/generation.py --
    @staticmethod
    def compute_start_end_times(t, num_blocks, num_blocks_model):
        """:831-854: the model window [t_begin, t_end) of codes used to generate code t of a sequence of `num_blocks`
        codes, and t's index in it.  Head (t < S // 2): the first window, t_relative = t; middle: t sits at S // 2 of a
        window that moves with it; tail (t >= num_blocks - S // 2): the last window."""
        half = num_blocks_model // 2
        if half <= t < num_blocks - half:
            t_relative = half
        elif t < half:
            t_relative = t
        else:
            t_relative = num_blocks_model - (num_blocks - t)
        t_begin = min(max(0, t - half), num_blocks - num_blocks_model)
        return t_begin, t_begin + num_blocks_model, t_relative

    def _meta_symbol(self, name, given, symbol):
        if given is not None:
            ids = [int(v) for v in given]
            if len(ids) != self.num_channels:
                raise ValueError(f'{name}: one token id per voice expected ({self.num_channels}), got {len(ids)}')
            return ids
        ds = getattr(self.dataloader_generator, 'dataset', None)
        n2i = getattr(ds, 'note2index_dicts', None)
        if n2i is None or any(symbol not in n2i[c] for c in range(self.num_channels)):
            raise ValueError(f"init_generation_chorale needs dataset.note2index_dicts with the '{symbol}' symbol, or explicit "
                             'per-voice lists pad= and start=; this dataset (e.g. the synthetic one) has no meta symbols')
        return [int(n2i[c][symbol]) for c in range(self.num_channels)]

    def init_generation_chorale(self, num_events, start_index, pad=None, start=None):
        """:1054-1062: (1, num_events, num_channels) int64 on the device, PAD everywhere and START at event
        start_index - 1.  pad / start: per-voice token ids for datasets without meta symbols (default: the dataset's 'XX' /
        'START').  start_index = 0 puts no START (the reference fails there on a negative repeat count)."""
        if not 0 <= start_index <= num_events:
            raise ValueError(f'init_generation_chorale: 0 <= start_index <= {num_events} (got {start_index})')
        PAD = self._meta_symbol('pad', pad, 'XX')
        out = torch.tensor(PAD, dtype=torch.int64).view(1, 1, -1).repeat(1, num_events, 1)
        if start_index >= 1:
            out[0, start_index - 1] = torch.tensor(self._meta_symbol('start', start, 'START'), dtype=torch.int64)
        return out.to(self.sos.device)

    def generate_from_code_long(self, encoding_indices=None, temperature=None, top_k=0, top_p=1., exclude_meta_symbols=False,
                                num_decodings=1, code_index_start=None, code_index_end=None, seed=None, pad=None, start=None,
                                use_graph=True, constraint=None, return_logp=False, return_attentions=False,
                                max_attention_bytes=4 << 30, graph_slides=None, allowed=None, return_allowed_mass=False,
                                particles=None, resample_threshold=0.5, return_particles=False, rules=None,
                                return_rule_report=False, beam=None, return_beams=False, no_copy=None, return_copy_report=False):
        """:729-829: decodes MERGED codes (B, nb) [continuous decoder: latents (B, nb, dz)] of any length nb >= S by sliding
        the model window one code at a time
        (`compute_start_end_times`), each row repeated `num_decodings` times (repeat_interleave).  The reference runs one
        full forward on the window per token; here the window's prefix is re-prefilled into the K/V caches when it moves
        and the tokens come from incremental steps (decoders/generation.py), which computes the same function.
        Returns int64 tokens (B * num_decodings, events, channels) on the device, sliced to the events of codes
        [code_index_start, code_index_end) -- tensors, not music21 scores, as `generate`.
        Differences from the reference: code_index_start / code_index_end = None mean the whole sequence (the reference
        multiplies them before applying its own default, :747-755, and crashes); code_index_start = 0 works (no START
        token, an all-PAD chorale and an empty first prefill); exclude_meta_symbols=True is honoured as in `generate` (the
        reference ignores it, its code is commented out, :786-793; the default False is its behaviour).  pad / start: see
        `init_generation_chorale`.  seed: as `generate_from_codes`; a row's draw is a function of (row seed, absolute
        chorale position).  A bare call without codes raises NotImplementedError, as before this method existed.
        constraint: (B, nb * events_per_code, channels) int64 over the WHOLE code sequence, in chorale coordinates: a token
        >= 0 is emitted at its place, -1 is free; events outside [code_index_start, code_index_end) are ignored.  Rows are
        repeated with num_decodings.  return_logp=True -> (tokens, logp), logp float32 of the tokens' shape (see
        `generate_from_codes`).
        return_attentions: as in `generate_from_codes` (the last element of the result), over the WHOLE code sequence in chorale
        coordinates: 'self_attns_decoder' (B', layers, H, nb * U, T), 'attns_cross' (B', layers, H, nb * U, S; None for the
        diagonal decoder) and 'window_start' (nb * U,) int64 on the host (`attention_window_starts`): the first code w of the
        window in which position c was emitted, -1 where none was -- those rows stay NaN.  Key j of row c is chorale token
        w * U + j (self) / code w + j (cross).  No encoder maps: they change with every window.
        graph_slides: `IncrementalDecoder.run_long`'s (None: as use_graph).
        allowed, return_allowed_mass: as in `generate_from_codes`, with allowed (B, nb * events_per_code, channels, vmax) or
        (nb * events_per_code, channels, vmax) over the WHOLE code sequence in chorale coordinates, like the constraint: the sets
        hold whichever window a position is emitted in, events outside [code_index_start, code_index_end) are ignored.
        allowed_mass has the tokens' shape.  Results: (tokens[, logp][, allowed_mass][, attentions]).
        particles, resample_threshold, return_particles: as in `generate_from_codes`; the groups are resampled after every
        generated code, the K/V caches move where the next code is generated in the same window (a slide recomputes them from
        the moved tokens), and the histories of the returned dict have one row per code of the WHOLE sequence.
        rules, return_rule_report: as in `generate_from_codes`.  A held pitch is followed back through the chorale however far
        it reaches, also past the model window and before code_index_start (the PAD / START frame has no pitch).  rule_report
        has the tokens' shape, after allowed_mass and before attentions.
        beam, return_beams: as in `generate_from_codes`; temperature may stay None.  The hypotheses' chorale rows move with them, the
        K/V caches too (a slide recomputes them from the moved tokens anyway), and 'ancestors' of the returned dict has one row
        per position of the WHOLE sequence, in chorale coordinates.
        no_copy, return_copy_report: as in `generate_from_codes`.  A context reaches back through the chorale however far
        max_copy asks, also past the model window and before code_index_start (the PAD / START frame is compared like any
        token; the corpus holds stored ticks only).  copy_report has the tokens' shape, after rule_report and before attentions."""
        if temperature is None and beam is not None:
            temperature = 1.0
        if encoding_indices is None or temperature is None:
            raise NotImplementedError('generate_from_code_long(encoding_indices, temperature, ...): generation without codes '
                                      'is not implemented')
        S, U, epc = self.num_tokens_source, self.total_upscaling, self.num_events_per_code

        def form(codes):
            nonlocal code_index_start, code_index_end
            nb = codes.shape[1]
            if nb < S:
                raise ValueError(f'encoding_indices: at least {S} codes (one model window) are needed, got {nb}')
            code_index_start = 0 if code_index_start is None else int(code_index_start)
            code_index_end = nb if code_index_end is None else int(code_index_end)
            if not 0 <= code_index_start <= code_index_end <= nb:
                raise ValueError(f'0 <= code_index_start <= code_index_end <= {nb} expected, got {code_index_start}, {code_index_end}')
            exclude = self._meta_symbol_ids() if exclude_meta_symbols else None
            chorale = self.init_generation_chorale(num_events=nb * epc, start_index=code_index_start * epc, pad=pad, start=start)

            def drive(inc, codes, settings):
                inc.start_long(codes, chorale.reshape(1, -1).expand(codes.shape[0], -1), **settings)
                return inc.run_long(code_index_start, code_index_end, use_graph=use_graph, graph_slides=graph_slides)
            return dict(events=nb * epc, first=code_index_start * epc, last=code_index_end * epc, exclude=exclude, drive=drive,
                        maps=lambda: {'window_start': self.attention_window_starts(nb, S, U, code_index_start, code_index_end)})
        res = self._generate_rows(
            encoding_indices, 'encoding_indices', None, form, temperature=temperature, top_k=top_k, top_p=top_p,
            num_decodings=num_decodings, seed=seed, constraint=constraint, return_logp=return_logp,
            return_attentions=return_attentions, max_attention_bytes=max_attention_bytes, allowed=allowed,
            return_allowed_mass=return_allowed_mass, particles=particles, resample_threshold=resample_threshold,
            return_particles=return_particles, rules=rules, return_rule_report=return_rule_report, beam=beam,
            return_beams=return_beams, no_copy=no_copy, return_copy_report=return_copy_report)
        return self._result_tuple(res, lambda t: t[:, code_index_start * epc:code_index_end * epc].contiguous())

    def generate_alla_mano(self, start_codes=None, end_codes=None, body_codes=None, temperature=None, num_decodings=3, beam=None,
                           return_beams=False, **kwargs):
        """:960-981: start_codes + body_codes + end_codes (lists of merged codes; continuous decoder: (n_i, dz) latent
        tensors, concatenated along time) decoded as one sequence, the body's events returned: int64 (num_decodings, events,
        channels).  kwargs go to `generate_from_code_long` -- `allowed` and `return_allowed_mass` among them, in the coordinates
        of the whole start + body + end sequence, and `rules` / `return_rule_report` and `no_copy` / `return_copy_report`, which
        need no coordinates.
        beam, return_beams: `generate_from_code_long`'s beam search; it needs num_decodings=1 and temperature may stay None."""
        if temperature is None and beam is not None:
            temperature = 1.0
        if start_codes is None or end_codes is None or body_codes is None or temperature is None:
            raise NotImplementedError('generate_alla_mano(start_codes, end_codes, body_codes, temperature): generation '
                                      'without codes is not implemented')
        if self.continuous_source:
            parts = [torch.as_tensor(c, dtype=torch.float32).reshape(-1, self.source_dim).cpu()
                     for c in (start_codes, body_codes, end_codes)]
            start_codes, body_codes, end_codes = parts
            codes = torch.cat(parts, dim=0).unsqueeze(0)
        else:
            start_codes, body_codes, end_codes = list(start_codes), list(body_codes), list(end_codes)
            codes = torch.tensor(start_codes + body_codes + end_codes, dtype=torch.int64).unsqueeze(0)
        return self.generate_from_code_long(codes, temperature=temperature, num_decodings=num_decodings,
                                            code_index_start=len(start_codes),
                                            code_index_end=len(start_codes) + len(body_codes), beam=beam, return_beams=return_beams,
                                            **kwargs)

    def _frame_and_encode(self, x, n2i):
        """The framing of generate_reharmonisation (:871-941): x (1, events, channels) int64 on the host is cut into model-sized
        chunks, framed by a PAD...START chunk and an END / PAD chunk (the last chunk completed with END + PAD), every chunk is
        encoded and the codes are glued.  -> (codes (1, chunks * S [, dz]), code_index_start, code_index_end -- the codes of x's own
        chunks without the completion's --, the framed tokens (chunks, E, channels) on the device)."""
        nc, E, dev = self.num_channels, self.data_processor.num_events, self.sos.device
        PAD, START, END = ([int(n2i[c][sym]) for c in range(nc)] for sym in ('XX', 'START', 'END'))
        row = lambda ids, n: torch.tensor(ids, dtype=torch.int64).view(1, 1, nc).repeat(1, n, 1)
        x_chunks = list(x.split(E, 1))
        last_chunk = x_chunks[-1]
        start_chunk = torch.cat([row(PAD, E - 1), row(START, 1)], 1)
        completion_length = E - last_chunk.size(1)
        if completion_length >= 1:
            x_chunks[-1] = torch.cat([last_chunk, row(END, 1), row(PAD, completion_length - 1)], 1)
            end_chunk = row(PAD, E)
        else:
            end_chunk = torch.cat([row(END, 1), row(PAD, E - 1)], 1)
        chunks = torch.cat([start_chunk] + x_chunks + [end_chunk], dim=0).to(dev)
        was_training = self.training
        self.eval()
        try:
            codes = self.encode(chunks)                                               # glued: (1, chunks * S [, dz])
            codes = codes.reshape(1, -1, self.source_dim) if self.continuous_source else codes.reshape(1, -1)
        finally:
            self.train(was_training)
        U = self.total_upscaling
        code_index_start = start_chunk.size(1) * nc // U
        code_index_end = codes.size(1) - (end_chunk.size(1) + completion_length) * nc // U
        return codes, code_index_start, code_index_end, chunks

    # ---- scoring given tokens: every window of a piece at once, decoders/scoring.py, csrc/score.hip ----------------------------
    @staticmethod
    def score_window_plan(num_blocks, num_blocks_model, code_index_start, code_index_end):
        """Host only: the distinct model windows in which `generate_from_code_long` emits the codes of [code_index_start,
        code_index_end) of a sequence of `num_blocks` codes, as a list of (first code of the window, first code scored in it, one
        past the last code scored in it), windows ascending.  Code t's window is `compute_start_end_times(t, ...)`'s, the one
        `attention_window_starts` reports for its positions: every code of the range lies in exactly one window, no window is
        without a code, and num_blocks == num_blocks_model gives one window.  ValueError on num_blocks < num_blocks_model or a
        bad code range."""
        from .scoring import window_plan
        return window_plan(num_blocks, num_blocks_model, code_index_start, code_index_end, Decoder.compute_start_end_times)

    def score_tokens(self, x, codes, code_index_start=None, code_index_end=None, pad=None, start=None, allowed=None,
                     return_details=False, window_rows=32):
        """How probable the tokens x are under this decoder, given the codes: the log-probabilities a forced
        `generate_from_code_long(codes, constraint=x, return_logp=True)` returns, computed without generating -- every model
        window of every piece is one row of a batched, teacher-forced forward (decoders/scoring.py).
        x: (B, nb * events_per_code, channels) int64 over the WHOLE code sequence, in chorale coordinates, like `constraint`;
        codes: (B, nb) merged codes [continuous decoder: (B, nb, dz) latents], nb >= S.  The scored chorale is
        `init_generation_chorale` (PAD, START at the event before code_index_start; pad / start as there) with x written over the
        events of codes [code_index_start, code_index_end) (None: the whole sequence) -- the chorale a forced generation ends
        with; x outside that range is ignored.
        -> logp float32 (B, events of the range, channels), the shape `generate_from_code_long` returns.
        return_details=True -> a dict of tensors of that shape: 'logp'; 'entropy' (float32, nats) of the model's distribution at
        the position; 'rank' (int32) of the written token, 0 = the model's first choice, equal logits in index order; 'best'
        (int64), what the model would have written (arg-max, the lowest index among equals); 'best_logp' (float32); and with
        `allowed` 'allowed_mass' (float32), the log of the probability the position's set leaves open.
        allowed: `generate_from_code_long`'s mask, bool (B, nb * events_per_code, channels, vmax) or shared by the rows, with its
        validation and packing; a written token outside its set is scored all the same.
        window_rows: (piece, window) rows per forward; 32 is the decoder's training batch, the shape the forward's launches are
        tuned for.  The results of two values agree within the teacher-forced tolerance, not necessarily bit for bit.
        Runs in eval mode without gradients under STEP_LOCK; the previous mode is restored.  ValueError on wrong shapes or dtypes,
        nb < S, a bad code range, a source of the wrong kind, window_rows < 1, and a token of the range outside its voice's
        vocabulary (the first (row, event, voice) is named)."""
        from .scoring import score_tokens
        return score_tokens(self, x, codes, code_index_start, code_index_end, pad, start, allowed, return_details, window_rows)

    def score_chorale(self, x, allowed=None, **kwargs):
        """`score_tokens` for a bare piece x (1, events, channels): x is framed and encoded as `reharmonise_tokens` frames it
        (PAD...START chunk, END / PAD completion; needs the dataset's START / END / XX symbols), its own codes are scored, and
        the results come back on x's own events -- the END / PAD completion is scored with the last chunk but not returned.
        allowed: bool (events, channels, vmax) or (1, events, channels, vmax) in x's OWN event coordinates, as in
        `reharmonise_tokens`; the other events are unrestricted.  kwargs: `return_details`, `window_rows`."""
        n2i = getattr(getattr(self.dataloader_generator, 'dataset', None), 'note2index_dicts', None)
        if n2i is None:
            raise ValueError('score_chorale needs dataset.note2index_dicts with the START / END / XX symbols')
        nc, E = self.num_channels, self.data_processor.num_events
        x = torch.as_tensor(x).long().cpu()
        if x.dim() != 3 or x.shape[0] != 1 or x.shape[2] != nc or x.shape[1] < 1:
            raise ValueError(f'x: (1, events, {nc}) tokens expected, got {tuple(x.shape)}')
        vocab = torch.tensor([int(v) for v in self.num_tokens_per_channel], dtype=torch.int64)
        bad = ((x < 0) | (x >= vocab)).reshape(-1)                                        # checked before the encoder embeds x
        if bool(bad.any()):
            e, c = divmod(int(bad.to(torch.int32).argmax()), nc)
            raise ValueError(f'x: (row 0, event {e}, voice {c}) holds token {int(x[0, e, c])}, outside its voice\'s vocabulary '
                             f'[0, {int(vocab[c])})')
        unknown = set(kwargs) - {'return_details', 'window_rows'}
        if unknown:
            raise TypeError(f'score_chorale: unexpected keyword arguments {sorted(unknown)}')
        n = x.shape[1]
        codes, code_index_start, code_index_end, chunks = self._frame_and_encode(x, n2i)
        framed = chunks.reshape(1, -1, nc)
        if allowed is not None:
            allowed = torch.as_tensor(allowed)
            if allowed.dtype != torch.bool or allowed.dim() not in (3, 4) or allowed.shape[-3:-1] != (n, nc) or \
                    (allowed.dim() == 4 and allowed.shape[0] != 1):
                raise ValueError(f'allowed: bool ({n}, {nc}, vmax) in x\'s event coordinates expected, got '
                                 f'{tuple(allowed.shape)} {allowed.dtype}')
            whole = torch.ones(framed.shape[1], nc, allowed.shape[-1], dtype=torch.bool, device=allowed.device)
            whole[E:E + n] = allowed.reshape(n, nc, -1)
            allowed = whole
        n2 = [n2i[c] for c in range(nc)]
        res = self.score_tokens(framed, codes, code_index_start=code_index_start, code_index_end=code_index_end,
                                pad=[int(d['XX']) for d in n2], start=[int(d['START']) for d in n2], allowed=allowed, **kwargs)
        first = E - code_index_start * self.num_events_per_code                           # x's event 0 in the returned range
        take = lambda t: t[:, first:first + n].contiguous()
        return {k: take(v) for k, v in res.items()} if isinstance(res, dict) else take(res)

    def reharmonise_tokens(self, x, num_reharmonisations, temperature, top_k=0, top_p=1., return_bounds=False,
                           keep_voices=None, return_logp=False, allowed=None, return_allowed_mass=False, rules=None,
                           return_rule_report=False, beam=None, return_beams=False, no_copy=None, return_copy_report=False,
                           **kwargs):
        """The body of generate_reharmonisation (:871-941) on a (1, events, channels) token tensor: the chorale is cut into
        model-sized chunks, framed by a PAD...START chunk and an END / PAD chunk (the last chunk completed with END + PAD),
        every chunk is encoded, the codes are glued and the chorale's own codes are decoded `num_reharmonisations` times.
        Needs the dataset's START / END / XX symbols.  -> int64 (num_reharmonisations, events', channels), or with
        return_bounds=True (tokens, code_index_start, code_index_end, number of codes).  kwargs go to
        `generate_from_code_long`.
        keep_voices: voice indices whose tokens are forced to x's -- harmonising a given melody is keep_voices=(0,).  Event
        e of x sits at chorale event E + e (after the PAD...START chunk); everything else, the END / PAD completion
        included, stays free, so events [0, x.shape[1]) of the kept voices come back equal to x.  return_logp=True: `tokens`
        above is the pair (tokens, logp) of `generate_from_code_long`.
        allowed: bool (x.shape[1], channels, vmax) or (1, x.shape[1], channels, vmax), the token sets of `generate_from_codes` in
        x's OWN event coordinates (what `templates.rhythm_mask(x, kinds)` returns): event e of x restricts chorale event E + e,
        every other event stays unrestricted.  return_allowed_mass=True: `tokens` above is the tuple of
        `generate_from_code_long`, (tokens[, logp], allowed_mass).
        rules, return_rule_report: `generate_from_code_long`'s; the rules compare the voices of a tick, so they need no
        coordinates, and rule_report comes back with the tokens, in the same events.
        beam, return_beams: `generate_from_code_long`'s beam search -- the most probable harmonisations of the kept voices --; it
        needs num_reharmonisations=1 and temperature 1.
        no_copy, return_copy_report: `generate_from_code_long`'s copy guard; the kept voices are forced, so where they are the
        corpus's own the report says FORCED_COPY rather than hiding it.  copy_report comes back with the tokens."""
        n2i = getattr(getattr(self.dataloader_generator, 'dataset', None), 'note2index_dicts', None)
        if n2i is None:
            raise ValueError('reharmonise_tokens needs dataset.note2index_dicts with the START / END / XX symbols')
        nc, E, dev = self.num_channels, self.data_processor.num_events, self.sos.device
        x = torch.as_tensor(x).long().cpu()
        if x.dim() != 3 or x.shape[0] != 1 or x.shape[2] != nc or x.shape[1] < 1:
            raise ValueError(f'x: (1, events, {nc}) tokens expected, got {tuple(x.shape)}')
        voices = None if keep_voices is None else self._keep_voices(keep_voices)
        if voices is not None and kwargs.get('constraint') is not None:
            raise ValueError('reharmonise_tokens: keep_voices builds the constraint; pass one of the two')
        kept = None
        if voices is not None:                           # checked before the encoder embeds x
            kept = torch.full_like(x, -1)
            kept[:, :, voices] = x[:, :, voices]
            self._constraint_rows(kept, 1, x.shape[1])
        codes, code_index_start, code_index_end, _ = self._frame_and_encode(x, n2i)
        if voices is not None:
            constraint = torch.full((1, codes.size(1) * self.num_events_per_code, nc), -1, dtype=torch.int64)
            constraint[:, E:E + x.shape[1]] = kept
            kwargs['constraint'] = constraint
        if allowed is not None:
            allowed = torch.as_tensor(allowed)
            if allowed.dtype != torch.bool or allowed.dim() not in (3, 4) or allowed.shape[-3:-1] != (x.shape[1], nc) or \
                    (allowed.dim() == 4 and allowed.shape[0] != 1):
                raise ValueError(f'allowed: bool ({x.shape[1]}, {nc}, vmax) in x\'s event coordinates expected, got '
                                 f'{tuple(allowed.shape)} {allowed.dtype}')
            whole = torch.ones(codes.size(1) * self.num_events_per_code, nc, allowed.shape[-1], dtype=torch.bool,
                               device=allowed.device)
            whole[E:E + x.shape[1]] = allowed.reshape(x.shape[1], nc, -1)
            kwargs['allowed'] = whole
        kwargs['return_allowed_mass'] = return_allowed_mass
        tokens = self.generate_from_code_long(codes, temperature=temperature, top_k=top_k, top_p=top_p,
                                              num_decodings=num_reharmonisations, code_index_start=code_index_start,
                                              code_index_end=code_index_end, return_logp=return_logp, rules=rules,
                                              return_rule_report=return_rule_report, beam=beam, return_beams=return_beams,
                                              no_copy=no_copy, return_copy_report=return_copy_report, **kwargs)
        return (tokens, code_index_start, code_index_end, codes.size(1)) if return_bounds else tokens

    def generate_reharmonisation(self, *a, **k):
        raise NotImplementedError('generate_reharmonisation (:856-958) reads its chorale from the music21 corpus, which this '
                                  'package does not ship; pass the token tensor to reharmonise_tokens instead')

    # ---- duplicate checks (:983-1017): the longest common run on the device, dataloaders/corpus.py, csrc/duplicates.hip ----------
    def _print_duplicates(self, lengths, subdivision):
        best = int(np.max(lengths))
        print(f'Num tokens plagiarisms: {best}')
        print(f'Num beats plagiarisms: {best / self.num_channels / subdivision}')

    def check_duplicate(self, generation=None, original=None):
        """:983-991, pairwise: the longest common run (dataloaders/corpus.py: same voice, consecutive tokens in tick-major order,
        ties to the earliest query position, then the earliest position of `original`) of two (events, channels) token tensors;
        `original` is framed as a one-piece corpus on the fly.  Returns the dict of `DeviceCorpus.longest_common_run` (host ints;
        `piece` is 0, or -1 without a common token) and prints the reference's two lines with the TRUE token count (the
        reference prints (characters - 1) / 3 of a match on the dumped note names).  The two tensors carry no subdivision: the
        beats line divides by the one of the decoder's dataloader generator, or by the reference's constant 4 (:1015) when the
        generator states none.  A bare call raises NotImplementedError, as before this method existed."""
        if generation is None or original is None:
            raise NotImplementedError('check_duplicate(generation, original): two (events, channels) token tensors are needed')
        from ..dataloaders.corpus import Corpus, DeviceCorpus
        original = torch.as_tensor(original).cpu().numpy()
        if original.ndim != 2 or original.shape[1] != self.num_channels or original.shape[0] < 1:
            raise ValueError(f'original: (events, {self.num_channels}) tokens expected, got {original.shape}')
        if original.min() < 0 or original.max() > np.iinfo(np.int32).max:
            raise ValueError('original: a token is negative or does not fit 32 bits')
        # START / END / PAD take no part in the check: only `longest_common_run` is called on this corpus, never `gather` or
        # `window_at`, so any ids the constructor accepts will do; subdivision 1 lets `original` have any length
        zero = np.zeros(self.num_channels, dtype=np.int64)
        corpus = Corpus(original.astype(np.int32), [0, original.shape[0]], 1, self.num_tokens_per_channel, zero, zero, zero)
        generation = torch.as_tensor(generation)
        if generation.dim() != 2:
            raise ValueError(f'generation: (events, {self.num_channels}) tokens expected, got {tuple(generation.shape)}')
        out = DeviceCorpus(corpus, self.sos.device).longest_common_run(generation)
        self._print_duplicates(out['length'], getattr(getattr(self.dataloader_generator, 'dataset', None), 'subdivision', 4))
        return out

    def check_duplicate_all_corpus(self, generation, split='train'):
        """:993-1017 on the device-resident corpus: the longest common run of every row of `generation`, (events, channels) or
        (G, events, channels), with the pieces of `split` ('train' / 'val' / 'test': a piece belongs to the split that holds its
        first window; None: every piece).  Needs a corpus dataloader generator (dataloaders/corpus.py); the synthetic ones have no
        corpus and raise ValueError.  Returns the dict of `DeviceCorpus.longest_common_run` plus 'best_x': int64 (events of the
        decoder, channels) per row, host -- the ticks of the matched piece that face the decoder-sized chunk of the generation in
        which the run begins (the run starts at row query_tick % events), padded by the window rule outside the piece; all PAD
        for a row without a common token.  The reference returns the training window with the longest character match instead
        and counts padding as copied."""
        dc = getattr(self.dataloader_generator, 'device_corpus', None)
        if dc is None:
            raise ValueError('check_duplicate_all_corpus needs a corpus dataloader generator (dataloaders/corpus.py); '
                             f'{type(self.dataloader_generator).__name__} has no corpus')
        pieces = None
        if split is not None:
            pieces = dc.split_pieces(split, self.dataloader_generator.sequences_size)
            if pieces[0] == pieces[1]:
                raise ValueError(f'check_duplicate_all_corpus: no piece begins in the {split} split')
        out = dc.longest_common_run(generation, pieces=pieces)
        E = self.data_processor.num_events
        single = np.ndim(out['length']) == 0
        rows = []
        for piece, tick, q in zip(*(np.atleast_1d(out[k]) for k in ('piece', 'piece_tick', 'query_tick'))):
            rows.append(dc.corpus.window_at(int(piece), int(tick) - int(q) % E, E) if piece >= 0
                        else np.repeat(dc.corpus.pad[None, :], E, axis=0))
        out['best_x'] = rows[0] if single else np.stack(rows)
        self._print_duplicates(out['length'], dc.corpus.subdivision)
        return out

    def plot(self, *a, **k):
        raise NotImplementedError('plots (decoder.py:1019-1052) are out of scope')
