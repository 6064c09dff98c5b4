"""KV-cached autoregressive generation of the decoder (reference: VQCPCB/decoders/decoder.py:552-723, which runs one full
seq2seq forward per generated token and samples on the host).

The incremental step, the prefix re-prefill and the captured graphs are the shared stack's (transformer/incremental.py);
this module adds what the decoder has on top of it:

  prefill (once per call, existing kernels): source embedding + source encoder stack -> memory; per decoder layer the
  cross-attention k | v of the memory; the target table of `Decoder._target_rows`; the per-voice heads concatenated into
  one [sum V_c, d] weight.

  the step's cross hook (csrc/decode.hip, 11 launches per layer + 2 in all): cross q -> cross-attention on the memory's k | v
  -> out_proj + residual -> add & LayerNorm;  and vqcpc_decode_sample, which draws the token of position pos.  With a
  constraint or token scores (`start(constraint=..., want_logp=...)`) the sampler is vqcpc_decode_sample_constrained: the same
  kernel body, which emits the given token where the constraint holds one and writes the emitted token's log-probability; it
  reads both at the position's CHORALE column through the device window index, so nothing else of the step or slide changes.
  With a per-position token set or its mass (`start(allowed=..., want_allowed_mass=...)`) the sampler is
  vqcpc_decode_sample_masked, one more flag on the same body: the packed sets (M, width, 8) and the mass (M, width) live in
  the stack's own buffers and are read / written at that same column, so again nothing else changes.
  Attention maps (`start(want_attentions=layers)`): the listed layers' self- and cross-attention launches are
  vqcpc_decode_attn_probs, which also stores the row of probabilities of the emitted token into `self_probs` / `cross_probs` at
  the row of the position's chorale coordinate (the same window index); the encoder's maps of the prefill are kept as `enc_probs`.

Long mode (reference: generate_from_code_long, decoder.py:729-854, one full forward on the moved window per token): a code
sequence of any length nb >= S is decoded by sliding the window one code at a time.  The chorale (M, nb * U) and the codes
(M, nb) live on the device.  When the window moves, its first position gets the start-of-sentence row and every row loses U
tokens of context, so every cache is stale:

  slide: vqcpc_decode_window (commit the live window's tokens, load the next window's codes / tokens / prefix rows / seeds,
  pos = P) -> memory and cross k | v of the new source window -> the decoder stack teacher-forced over the P = t_relative * U
  prefix rows of every sequence (`prefill_prefix`).  Then U steps as above.

The window index is read from device memory and advanced by the window kernel, so ONE captured slide serves every middle
window of a generation (all have P = (S // 2) * U), next to the one captured step.

Diagonal decoder (cross_attention_type 'diagonal', TransformerAlignedDecoderLayerCustom): the layer has no cross-attention.
The prefill computes per layer C_l = cross_attn_l(memory) (n * S, nc * d) instead of the cross k | v; the step replaces its
three cross launches (q projection, attention, out-projection + residual) by ONE vqcpc_decode_aligned_add, which adds the
position's code-and-voice vector of C_l to the row (9 launches per layer + 2); the re-prefill expands C_l over the P prefix
rows with vqcpc_aligned_expand.  Everything else -- one captured step, one captured slide -- is as above.

Continuous decoder (`Decoder.continuous_source`, a NoQuantization encoder): the source is the latents (M, nb, dz) and
`source_embeddings` a linear layer.  The first launch of `_encode_memory` is then vqcpc_decode_source_rows instead of the
embedding gather: it reads the live window's S latents of every sequence from `z_full` through the device window index `win`
(NULL in the fixed-window prefill), so the captured slide still serves every middle window; vqcpc_decode_window gets a dummy
all-zero code tensor and keeps its token / seed / position bookkeeping.  Everything after `src` is shared.

Particles (`start(particles=P)`, csrc/particles.hip): the rows are groups of P consecutive rows with their own seeds.  After the U
steps of a code, vqcpc_particle_resample adds the code's forced logp / free logmass to every row's log-weight and, where a
group's effective sample size fell below the threshold, draws its ancestors; vqcpc_particle_permute_* then moves the ancestors'
state -- live tokens, chorale row, logp / logmass rows, next input row, K/V cache rows [0, pos) -- onto the rows in place.  Both
read `pos` and `win` from device memory and sit BETWEEN the replays: the captured step and slide are what they were.

Voice-leading rules (`start(rules=...)`, csrc/rules.hip): the caller's static sets move to `rule_static` and `allowed` becomes the
rule kernel's output; vqcpc_decode_rules runs immediately before vqcpc_decode_sample_masked, INSIDE the captured step, and
overwrites the live column's set from the tokens emitted so far (the live window's, and the chorale's before it) and the
column of `rule_report`.  The sampler, the mass and the particle weights read that set unchanged.

Copy guard (`start(no_copy=CopyIndex)`, csrc/nocopy.hip): the same kind of thing with another question.  vqcpc_decode_nocopy runs
after vqcpc_decode_rules and immediately before the sampler or the beam select, INSIDE the captured step: it looks the row's last
max_copy tokens up in the corpus index and takes every token that would complete a shared run of max_copy + 1 out of the live
column's set (`copy_static`'s, the rule kernel's in place, or the whole vocabulary), and writes the column of `copy_report`.  It is
stateless per step, so whatever moves rows -- particles, the beam -- only has to move `copy_report` with them.

Beam search (`start(beam=W)`, csrc/beam.hip): the rows are groups of W consecutive rows, the W best hypotheses of one user row.
vqcpc_decode_beam_select takes the sampler's place (after vqcpc_decode_rules when rules are on): it expands every row into its
candidate tokens, keeps each group's W best by total log-probability and writes the whole live column -- tokens, next input rows,
logp, logmass, rule_report -- in SLOT order, with the ancestors and the two device words `b_bound` = {pos, col} before the
increment.  The moves that follow (`_beam_moves`, vqcpc_particle_permute_* with P = W) bring the history behind the slots: the live
tokens' columns [0, b_bound[0]), the record rows' columns [0, b_bound[1]) -- the new column must not move, it is in slot order
already --, the chorale row, and the K/V cache rows [0, pos) of the incremented pos, because position pos's K/V were written by
this step for the ancestor.  The moves read only device words, so they live INSIDE the captured step (`beam_moves_in_step`) or
between the replays, where the cache move is skipped before a slide (profiles/generate_beam_perf_log.md compares the two).

Where the options are set up: `start` and `start_long` take the sampling settings (`_sampling`) and then make ONE call of
`_configure` with the generation's coordinate frame (`Frame`, transformer/incremental.py): (T, None, 1, S, seeds) for the fixed
window, (nb * U, win, U, nb, row_seeds) for a chorale.  Every option buffer above has `frame.width` columns and is addressed
through `frame.win`; the step, the cross hook, the sampler and the resampling read the frame and nothing else about the
coordinates.  `_configure` sets every option at every call, so a second `start` leaves the earlier call's options off.  The
record buffers (`logp`, `logmass`, `rule_report`, `copy_report`, `self_probs`, `cross_probs`, the `p_*` and `b_*` state) are allocated there and get their
initial values in one place, `_clear_records`, which `reset` and the post-warm-up path of `run_long` call."""
import ctypes

import torch

from .. import hip, ops
from ..transformer.incremental import MAX_ROWS, Frame, IncrementalStack, _splitmix64, row_seeds    # noqa: F401 (re-exported)
from ..transformer.transformer_custom import mask_code


class IncrementalDecoder(IncrementalStack):
    """One generation of `batch` <= 64 rows of `decoder` (a Decoder in eval mode; the caller holds utils.STEP_LOCK).

        inc = IncrementalDecoder(dec, B)
        inc.prefill(codes)                                        # (B, S) merged codes [continuous decoder: (B, S, dz) latents]
        tokens = inc.run(seeds, temperature, top_k, top_p)        # (B, T) int64, position-major (t = event * nc + voice)

    `start` + `step` expose the single steps (teacher forcing, the sampler's inputs `logits` and its optional
    probability output `probs`) for the tests."""

    beam_moves_in_step = True         # the beam's moves are launches of the (captured) step; False: between the steps

    def __init__(self, decoder, batch):
        if not 1 <= batch <= MAX_ROWS:
            raise ValueError(f'IncrementalDecoder: 1 <= batch <= {MAX_ROWS} (got {batch})')
        dec = self.dec = decoder
        M, dev, d = int(batch), dec.sos.device, dec.d_model
        layers = list(dec.transformer.decoder.layers)
        self.T, self.S = dec.num_tokens_target, dec.num_tokens_source
        super().__init__(dev, M, layers, [lay.norm3 for lay in layers], self.T, d)
        self.nc, self.U = dec.num_channels, dec.total_upscaling
        self.diagonal = dec.cross_attention_type == 'diagonal'
        self.cross_mask = None if self.diagonal else mask_code(dec.cross_attention_type)
        cls = IncrementalDecoder
        self._cross = cls._cross_aligned if self.diagonal else cls._cross_attention
        self._prefix_cross = cls._prefix_cross_aligned if self.diagonal else cls._prefix_cross_attention
        sizes = [int(n) for n in dec.num_tokens_per_channel]
        self.offsets = [0]
        for n in sizes:
            self.offsets.append(self.offsets[-1] + n)
        self._offsets_c = (ctypes.c_int32 * (self.nc + 1))(*self.offsets)
        self.vmax = max(sizes)
        f32 = dict(dtype=torch.float32, device=dev)
        self.h2, self.qc = torch.empty(M, d, **f32), torch.empty(M, d, **f32)
        self.logits = torch.empty(M, self.offsets[-1], **f32)
        self.tokens = torch.zeros(M, self.T, dtype=torch.int64, device=dev)
        self.exclude = torch.zeros(self.nc, 8, dtype=torch.int32, device=dev)     # uint32 bits
        self.memkv = None
        self.allowed, self.logmass, self.masked = None, None, False
        self.rules, self.rule_static, self.rule_report = None, None, None
        self.no_copy, self.copy_static, self.copy_report = None, None, None
        self.cross_probs, self.enc_probs, self.attn_layers = None, None, None
        self.particles = None                                                     # group size P, or None: plain rows
        self.beam = None                                                          # beam width W, or None: the rows are sampled
        self.continuous = bool(getattr(dec, 'continuous_source', False))
        if self.continuous:
            self.dz = dec.source_dim
            self.src = torch.empty(M * self.S, d, **f32)                          # fixed address: a captured slide writes it
            self.z_full, self.z_nb = None, 0

    # ---- prefill ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prefill(self, codes):
        dec, M, d = self.dec, self.M, self.d
        if self.continuous:
            assert tuple(codes.shape) == (M, self.S, self.dz) and codes.is_floating_point(), (codes.shape, (M, self.S, self.dz))
            self.z_full, self.z_nb = codes.to(self.dev, torch.float32).contiguous(), self.S
            self._encode_memory(None)
        else:
            codes = codes.to(self.dev, torch.int64)
            assert codes.shape == (M, self.S), (codes.shape, (M, self.S))
            self._encode_memory(codes)
        self.table = dec._target_table(self.dev).contiguous()                          # (vmax * U + 1, d)
        self.head_w = torch.cat([m.weight for m in dec.pre_softmaxes], dim=0).contiguous()
        self.head_b = torch.cat([m.bias for m in dec.pre_softmaxes], dim=0).contiguous()

    def _encode_memory(self, codes, windowed=False):
        """codes (M, S) -> memory -> every layer's cross k | v (diagonal decoder: its C = cross_attn(memory), (M * S, nc * d)),
        written into buffers that keep their address (a captured step reads them).  Continuous decoder: `codes` is unused, the
        source rows come from the S latents of `z_full` at the live window of `win` (windowed) or at 0."""
        dec, M, d = self.dec, self.M, self.d
        if self.memkv is None:
            width = self.nc * d if self.diagonal else 2 * d
            self.memkv = [torch.empty(M * self.S, width, dtype=torch.float32, device=self.dev) for _ in self.layers]
        if self.continuous:
            lin, src = dec.source_embeddings, self.src
            hip.call('vqcpc_decode_source_rows', self.z_full, self.z_nb, self.dz, self.win if windowed else None, lin.weight,
                     lin.bias, src, d, M, self.S, d)
        else:
            src = dec.source_rows(codes)
        memory, att = dec.transformer.encoder.forward_rows_masked(src, M, mask_code(dec.encoder_attention_type))
        # per encoder layer (M, H, S, S); a moved window's maps are not kept (a captured slide would pin its own pool's tensors)
        self.enc_probs = None if windowed else [a['a_self_encoder'] for a in att]
        if self.diagonal:
            for lay, C in zip(self.layers, self.memkv):
                l1, l2 = lay.cross_attn[0], lay.cross_attn[2]
                h = ops.gemm_nt(memory.reshape(-1, l1.weight.shape[1]), l1.weight, bias=l1.bias)
                ops.gemm_nt(ops.EluFn.apply(h), l2.weight, bias=l2.bias, out=C)
            return
        for lay, kv in zip(self.layers, self.memkv):                                    # (M * S, 2d): k | v
            ops.gemm_nt(memory, lay.multihead_attn.in_proj_weight[d:], bias=lay.multihead_attn.in_proj_bias[d:], out=kv)

    def start(self, seeds=None, temperature=1.0, top_k=0, top_p=1.0, exclude=None, teacher=None, want_probs=False,
              constraint=None, want_logp=False, want_attentions=None, allowed=None, want_allowed_mass=False, particles=None,
              resample_threshold=0.5, final_resample=True, rules=None, beam=None, no_copy=None):
        """Resets the generation to position 0 with the given sampling settings.  exclude: per voice, a list of token ids
        never drawn; teacher: (M, T) int64 tokens to force instead of drawing; want_probs: keep the filtered
        probabilities of the last step in `probs` (M, max V_c).
        constraint: (M, T) int64, a token >= 0 is emitted at its position, < 0 leaves the draw free; want_logp: keep every
        emitted token's log-probability under the unfiltered distribution in `logp` (M, T) float32, NaN where no token was
        emitted yet.  Either one switches the step's sampler to vqcpc_decode_sample_constrained.
        want_attentions: None, or a sorted tuple of decoder-layer indices whose attention rows are kept for every emitted token:
        `self_probs` (layers, M, H, T, T) and `cross_probs` (layers, M, H, T, S; None for the diagonal decoder), float32, NaN
        where no token was emitted yet.  Those layers' attention launches become vqcpc_decode_attn_probs.
        allowed: (M, T, 8) int32, per (row, position) the 256-bit set of the tokens that may be drawn (bit i & 31 of word i >> 5;
        the caller has checked that every set has a token of its voice); want_allowed_mass: keep in `logmass` (M, T) float32
        the log of the probability the unfiltered distribution gives to the position's set, NaN where no token was emitted yet.
        Either one switches the step's sampler to vqcpc_decode_sample_masked.
        particles: None, or P in [2, 64] dividing M: the rows are M / P groups of P particles, resampled after every code
        (`_resample`); logp / logmass are then kept whenever a constraint / sets are given.  resample_threshold: a group
        resamples when its effective sample size falls below resample_threshold * P; final_resample: after the last code one
        forced resampling makes the first row of every group an unweighted draw from the final weights.
        rules: None, or a `templates.VoiceLeadingRules`: vqcpc_decode_rules writes every position's set before the masked
        sampler reads it (`_rule_sets`); `rule_report` (M, T) int32 keeps what was relaxed or broken, -1 where no token was
        emitted yet.
        beam: None, or W in [1, 64] dividing M: the rows are M / W groups of W hypotheses and vqcpc_decode_beam_select replaces the
        sampler (`_beam`); seeds, temperature, top_k and top_p are then unused.
        no_copy: None, or a `dataloaders.corpus.CopyIndex`: vqcpc_decode_nocopy takes the tokens that would complete a run of
        max_copy + 1 tokens shared with the corpus out of every position's set (`_copy_guard`); `copy_report` (M, T) int32 keeps
        how many it took and the RELAXED / FORCED_COPY flags, -1 where no token was emitted yet."""
        self._sampling(seeds, temperature, top_k, top_p, exclude, teacher, want_probs)
        self._configure(Frame(self.T, None, 1, self.S, self.seeds), constraint, want_logp, allowed, want_allowed_mass, particles,
                        resample_threshold, final_resample, rules, want_attentions, beam, no_copy)

    def _sampling(self, seeds=None, temperature=1.0, top_k=0, top_p=1.0, exclude=None, teacher=None, want_probs=False):
        """The sampling settings of `start`: what the sampler takes whatever options are on."""
        if not temperature > 0:
            raise ValueError('temperature must be > 0')
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        if seeds is not None:
            self.seeds.copy_(row_seeds(seeds, self.M))
        bits = torch.zeros(self.nc, 8, dtype=torch.int64)
        for c, toks in enumerate(exclude or []):
            for t in toks:
                bits[c, int(t) // 32] |= 1 << (int(t) % 32)
        self.exclude.copy_(torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32))
        self.excluding = bool((bits != 0).any())
        if teacher is not None:
            self.teacher = teacher.to(self.dev, torch.int64).reshape(self.M, self.T).contiguous()
        else:
            self.teacher = None
        self.probs = torch.zeros(self.M, self.vmax, dtype=torch.float32, device=self.dev) if want_probs else None

    def _configure(self, frame, constraint, want_logp, allowed, want_allowed_mass, particles, resample_threshold, final_resample,
                   rules, want_attentions, beam=None, no_copy=None):
        """The options of one generation, all of them at every call (what is not asked for is switched off), in the coordinates
        of `frame`: `Frame(T, None, 1, S, seeds)` for the fixed window, `Frame(nb * U, win, U, nb, row_seeds)` for a chorale,
        whose buffers are addressed through the device window index.  The record buffers are allocated here, once and before any
        warm-up step (a captured step or slide holds their addresses), and get their values from `reset`, which ends the call."""
        self.frame = frame
        self._particles(particles, resample_threshold, final_resample, want_attentions)
        self._beam(beam, want_attentions)
        scored = particles is not None                        # the weights are the forced tokens' logp and the sets' mass
        self._constrain(constraint, want_logp or (scored and constraint is not None), frame.width)
        narrowed = allowed is not None or rules is not None or no_copy is not None
        self._mask(allowed, want_allowed_mass or (scored and narrowed))
        self._rule_sets(rules)
        self._copy_guard(no_copy)
        self._record_attentions(want_attentions)
        self.reset()

    def _beam(self, W, want_attentions):
        """The beam's state: per row the hypothesis's total log-probability `b_score` and its last ancestor `b_anc`; the device
        flag `b_flag` (some row moved), the two words `b_bound` = {pos, col} of the last select before its increment, and per
        column of the frame the ancestors `b_hist` (int32, -1 where nothing was generated)."""
        self.beam = None
        if W is None:
            return
        W = int(W)
        if not 1 <= W <= MAX_ROWS or self.M % W:
            raise ValueError(f'beam: 1 <= beam <= {MAX_ROWS} dividing the stack\'s {self.M} rows expected, got {W}')
        if self.particles is not None:
            raise ValueError('beam and particles exclude each other')
        if want_attentions is not None:
            raise ValueError('beam: attention maps are not moved with a hypothesis; want_attentions must be None')
        if self.teacher is not None or self.probs is not None:
            raise ValueError('beam and teacher / want_probs exclude each other')
        f32, i32 = dict(dtype=torch.float32, device=self.dev), dict(dtype=torch.int32, device=self.dev)
        self.beam = W
        self.b_score, self.b_anc = torch.empty(self.M, **f32), torch.empty(self.M, **i32)
        self.b_flag, self.b_bound = torch.empty(1, **i32), torch.empty(2, **i32)
        self.b_hist = torch.empty(self.frame.width, self.M, **i32)

    def _beam_moves(self, move_cache=True):
        """After vqcpc_decode_beam_select: row k <- row b_anc[k] of everything behind the live column, which the select wrote in
        slot order already.  The bounds are device words: the tokens move in [0, b_bound[0]), the record rows in [0, b_bound[1]),
        the caches in [0, pos) of the incremented pos.  move_cache=False before a slide, which recomputes the caches from the
        moved tokens.  W = 1 has nothing to move."""
        W, M, w = self.beam, self.M, self.frame.width
        if W == 1:
            return
        anc, flag, bound = self.b_anc, self.b_flag, self.b_bound
        hip.call('vqcpc_particle_permute_i64', self.tokens, self.T, self.T, bound[0:1], anc, flag, M, W)
        if self.frame.win is not None:                        # long mode: the history before the live window
            hip.call('vqcpc_particle_permute_i64', self.chorale, w, w, None, anc, flag, M, W)
        for rows in (self.logp, self.logmass, self.rule_report, self.copy_report):
            if rows is not None:
                hip.call('vqcpc_particle_permute_f32', rows, w, w, bound[1:2], anc, flag, M, W)
        if move_cache:
            for cache in (self.kcache, self.vcache):
                hip.call('vqcpc_particle_permute_cache', cache, len(self.layers), self.W, self.d, self.pos, anc, flag, M, W)

    def beam_results(self):
        """After a run: the hypotheses' total log-probabilities (G, W), non-increasing along W and -inf for a dead slot, and the
        ancestors per column of the frame."""
        return {'scores': self.b_score.view(self.M // self.beam, self.beam).clone(), 'ancestors': self.b_hist}

    def _resample(self, last, move_cache, chorale=None):
        """After the U steps of a code: the weight update and the resampling decision (vqcpc_particle_resample), then the
        group's generation state follows the ancestors in place (vqcpc_particle_permute_*): the live window's tokens [0, pos),
        the chorale row (long mode), the logp / logmass rows, the next input row and, with move_cache -- no slide follows, which
        would recompute them from the tokens --, every layer's K and V cache rows [0, pos).  The permute launches return at once
        on the device flag when no row moved.  The launches are issued eagerly between the step replays of a graphed run: replaying
        them from a captured graph of their own measured slower (profiles/generate_particles_perf_log.md).  last: the code is the generation's last one -- a forced resampling
        (`final_resample`), or the weight update alone (threshold 0, nothing moves, no permute launch)."""
        P, M, w = self.particles, self.M, self.frame.width
        force = bool(last and self.p_final)
        threshold = 0.0 if last and not self.p_final else self.p_threshold
        hip.call('vqcpc_particle_resample', self.p_lw, self.p_evidence, self.p_pending, self.p_seeds, self.constraint, w,
                 self.logp if self.constraint is not None else None, w, self.logmass if self.allowed is not None else None, w,
                 self.pos, self.frame.win, self.U, threshold, int(force), self.p_anc, self.p_wn, self.p_ess, self.p_flag,
                 self.p_hist_anc, self.p_hist_wn, self.p_hist_ess, self.p_hist_anc.shape[0], M, P)
        if threshold == 0.0 and not force:
            return
        anc, flag = self.p_anc, self.p_flag
        hip.call('vqcpc_particle_permute_i64', self.tokens, self.T, self.T, self.pos, anc, flag, M, P)
        if chorale is not None:
            hip.call('vqcpc_particle_permute_i64', chorale, chorale.shape[1], chorale.shape[1], None, anc, flag, M, P)
        for rows in (self.logp, self.logmass, self.rule_report, self.copy_report):    # the reports' int32 rows move as 4-byte words
            if rows is not None:
                hip.call('vqcpc_particle_permute_f32', rows, w, w, None, anc, flag, M, P)
        if not last:
            hip.call('vqcpc_particle_permute_f32', self.x, self.d, self.d, None, anc, flag, M, P)
            if move_cache:
                for cache in (self.kcache, self.vcache):
                    hip.call('vqcpc_particle_permute_cache', cache, len(self.layers), self.W, self.d, self.pos, anc, flag, M, P)

    def _mask(self, allowed, want_mass):
        """The masked sampler's buffers, addressed like the constrained sampler's: the packed sets are COPIED into a buffer of
        this stack, (M, width, 8) int32, so a captured step or slide reads every window's sets through the window index."""
        width = self.frame.width
        if (allowed is not None or want_mass) and self.teacher is not None:
            raise ValueError('allowed / want_allowed_mass and teacher exclude each other')
        self.allowed = None
        if allowed is not None:
            if tuple(allowed.shape) != (self.M, width, 8) or allowed.dtype != torch.int32:
                raise ValueError(f'allowed: packed sets ({self.M}, {width}, 8) int32 expected, got {tuple(allowed.shape)} '
                                 f'{allowed.dtype}')
            self.allowed = torch.empty(self.M, width, 8, dtype=torch.int32, device=self.dev)
            self.allowed.copy_(allowed)
        self.logmass = torch.empty(self.M, width, dtype=torch.float32, device=self.dev) if want_mass else None
        self.masked = allowed is not None or bool(want_mass)

    def _rule_sets(self, rules):
        """The rule kernel's buffers (after `_mask`): `kinds` and `max_leap` are uploaded once; the caller's sets stay in
        `rule_static` (None: none) and `allowed`, the buffer the sampler reads, becomes the kernel's output, which overwrites the
        live column at every step; `rule_report` (M, width) int32 -- a dtype vqcpc_particle_permute_f32 moves."""
        self.rules = self.rule_static = self.rule_report = None
        if rules is None:
            return
        if self.teacher is not None:
            raise ValueError('rules and teacher exclude each other')
        kinds = rules.kinds
        if kinds.shape[0] != self.nc or kinds.shape[1] < self.vmax:
            raise ValueError(f'rules: a kinds table ({self.nc}, >= {self.vmax}) expected, got {tuple(kinds.shape)}')
        self.rules = rules
        self.rule_kinds = kinds.to(self.dev, torch.int32).contiguous()
        self.rule_leap = rules.max_leap.to(self.dev, torch.int32).contiguous()
        self.rule_static = self.allowed
        self.allowed = torch.zeros(self.M, self.frame.width, 8, dtype=torch.int32, device=self.dev)
        self.rule_report = torch.empty(self.M, self.frame.width, dtype=torch.int32, device=self.dev)
        self.masked = True

    def _copy_guard(self, index):
        """The copy guard's buffers (after `_rule_sets`).  `copy_static` is the set the guard kernel reads.  Without rules the
        caller's sets move there (None: none) and `allowed`, the buffer the sampler reads, becomes the kernel's output; with rules
        the rule kernel has written the live column of `allowed` this step, `copy_static` IS `allowed` and the guard narrows it in
        place.  `copy_report` (M, width) int32 moves with its row like `rule_report`."""
        self.no_copy = self.copy_static = self.copy_report = None
        if index is None:
            return
        if self.teacher is not None:
            raise ValueError('no_copy and teacher exclude each other')
        sizes = tuple(b - a for a, b in zip(self.offsets[:-1], self.offsets[1:]))
        if self.nc != 4 or sizes != tuple(index.vocab):
            raise ValueError(f'no_copy: the index is of a corpus with 4 voices and the vocab {tuple(index.vocab)}, the decoder has '
                             f'{self.nc} voices and {sizes}')
        if index.device != self.dev:
            raise ValueError(f'no_copy: the index lives on {index.device}, the decoder on {self.dev}')
        self.no_copy = index
        self.copy_static = self.allowed
        if self.rules is None:
            self.allowed = torch.zeros(self.M, self.frame.width, 8, dtype=torch.int32, device=self.dev)
        self.copy_report = torch.empty(self.M, self.frame.width, dtype=torch.int32, device=self.dev)
        self.masked = True

    def _record_attentions(self, layers):
        """The attention-map buffers, one row per column of the frame.  layers=None frees them and every launch is the plain one
        again."""
        self.self_probs = self.cross_probs = None
        self._attn_slot, self.attn_layers = {}, None
        if layers is None:
            return
        layers = tuple(int(li) for li in layers)
        if not layers or list(layers) != sorted(set(layers)) or layers[0] < 0 or layers[-1] >= len(self.layers):
            raise ValueError(f'want_attentions: a sorted tuple of distinct layer indices in [0, {len(self.layers)}) expected, '
                             f'got {layers}')
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.self_probs = torch.empty(len(layers), self.M, self.H, self.frame.width, self.T, **f32)
        if not self.diagonal:
            self.cross_probs = torch.empty(len(layers), self.M, self.H, self.frame.width, self.S, **f32)
        self.attn_layers = layers
        self._attn_slot = {li: k for k, li in enumerate(layers)}

    def reset(self):
        self.pos.zero_()
        self.tokens.zero_()
        self.x.copy_(self.table[-1].expand(self.M, self.d))                            # start-of-sentence row
        self._clear_records()

    def _clear_records(self):
        """The initial values of everything a step records, in one place: NaN (report: -1) where no token was emitted yet, and
        the filter before its first code.  A warm-up step of a capture writes into these buffers, so a run clears them again."""
        nan = float('nan')
        for rows, value in ((self.logp, nan), (self.logmass, nan), (self.rule_report, -1), (self.copy_report, -1),
                            (self.self_probs, nan), (self.cross_probs, nan)):
            if rows is not None:
                rows.fill_(value)
        if self.beam is not None:                             # the standard start: identical rows would fill the beam with copies
            self.b_score.fill_(float('-inf'))
            self.b_score[0::self.beam] = 0.0
            self.b_anc.copy_(torch.arange(self.M, dtype=torch.int32))
            for rows, value in ((self.b_flag, 0), (self.b_bound, 0), (self.b_hist, -1)):
                rows.fill_(value)
        self._clear_particles()

    # ---- one step: the cross hooks and the sampler ----------------------------------------------------------------------
    def _cross_attention(self, li, lay):
        d, ca, kv = self.d, lay.multihead_attn, self.memkv[li]
        hip.call('vqcpc_decode_linear', self.h1, d, None, ca.in_proj_weight, ca.in_proj_bias, None, 0, self.qc, d, self.M, d, d,
                 0)
        slot = self._attn_slot.get(li)
        if slot is None:
            hip.call('vqcpc_decode_attn', self.qc, d, kv, kv.data_ptr() + 4 * d, 2 * d, None, None, 0, ca.attn_bias.e1,
                     ca.attn_bias.e2, self.att, d, self.pos, self.M, self.S, self.T // self.S, self.H, self.hd, self.cross_mask)
        else:
            hip.call('vqcpc_decode_attn_probs', self.qc, d, kv, kv.data_ptr() + 4 * d, 2 * d, None, None, 0, ca.attn_bias.e1,
                     ca.attn_bias.e2, self.att, d, self.pos, self.M, self.S, self.T // self.S, self.H, self.hd, self.cross_mask,
                     self.cross_probs[slot], self.S, self.frame.width, self.frame.win, self.frame.stride)
        self._linear(self.att, ca.out_proj.weight, ca.out_proj.bias, self.s, res=self.h1)
        self._ln(self.s, lay.norm2, self.h2)
        return self.h2

    def _cross_aligned(self, li, lay):
        d = self.d
        hip.call('vqcpc_decode_aligned_add', self.h1, d, self.memkv[li], self.s, d, self.pos, self.M, self.S, self.U, self.nc, d)
        self._ln(self.s, lay.norm2, self.h2)
        return self.h2

    def _sample(self):
        """One of the three sampler entry points: plain unless `constrained`, and masked wins over constrained.  They share
        the operands before (`head`) and after (`tail`) what each one adds."""
        T, d = self.T, self.d
        if self.beam is not None:
            w, win = self.frame.width, self.frame.win
            if self.rules is not None:
                self._rules_launch()
            if self.no_copy is not None:
                self._nocopy_launch()
            hip.call('vqcpc_decode_beam_select', self.logits, self.logits.shape[1], self._offsets_c, self.nc, self.M, self.beam,
                     self.exclude if self.excluding else None, self.constraint, w, self.allowed, w, self.logp, w, self.logmass, w,
                     self.rule_report, w, win, self.tokens, T, T, self.table, self.table.shape[0], d, self.U, self.x, d,
                     self.b_score, self.b_anc, self.b_flag, self.b_bound, self.b_hist, self.b_hist.shape[0], None, self.pos)
            if self.no_copy is not None and self.beam > 1:    # the select does not know this record: its live column follows
                hip.call('vqcpc_nocopy_beam_column', self.copy_report, w, self.b_anc, self.b_flag, self.b_bound, self.M, self.beam)
            if self.beam_moves_in_step:
                self._beam_moves()
            return
        head = (self.logits, self.logits.shape[1], self._offsets_c, self.nc, self.M, self.temperature, self.top_k, self.top_p,
                self.exclude if self.excluding else None, self.seeds)
        tail = (self.tokens, T, T, self.table, self.table.shape[0], d, self.U, self.x, d, self.probs, self.vmax, self.pos)
        if not (self.masked or self.constrained):
            hip.call('vqcpc_decode_sample', *head, self.teacher, T, *tail)
            return
        w, win = self.frame.width, self.frame.win
        forced = (self.constraint, w, self.logp, w, win)
        if not self.masked:
            hip.call('vqcpc_decode_sample_constrained', *head, *forced, *tail)
            return
        if self.rules is not None:
            self._rules_launch()
        if self.no_copy is not None:
            self._nocopy_launch()
        hip.call('vqcpc_decode_sample_masked', *head, *forced, self.allowed, w, self.logmass, w, *tail)

    def _rules_launch(self):
        """The live column's set, from the tokens emitted so far."""
        T, w, win = self.T, self.frame.width, self.frame.win
        windowed = win is not None                            # long mode: the history before the live window is the chorale's
        hip.call('vqcpc_decode_rules', self.tokens, T, T, self.chorale if windowed else None, w if windowed else 0,
                 self.constraint, w, self.rule_kinds, self.rule_kinds.shape[1], self._offsets_c, self.nc, self.rule_leap,
                 self.rules.mask, self.exclude if self.excluding else None, self.rule_static, w, self.allowed, w,
                 self.rule_report, w, self.pos, win, self.U, self.M)

    def _nocopy_launch(self):
        """The live column's set without the tokens that would complete a copied run."""
        T, w, win = self.T, self.frame.width, self.frame.win
        windowed = win is not None                            # long mode: the history before the live window is the chorale's
        hip.call('vqcpc_decode_nocopy', self.tokens, T, T, self.chorale if windowed else None, w if windowed else 0,
                 self.constraint, w, *self.no_copy.args(), self._offsets_c, self.nc, self.exclude if self.excluding else None,
                 self.copy_static, w, self.allowed, w, self.copy_report, w, self.pos, win, self.U, self.M)

    # ---- a whole generation --------------------------------------------------------------------------------------------
    def run(self, use_graph=True):
        """T steps from position 0 (after `start`): one captured step replayed T times, or (use_graph=False) T eager
        steps.  Returns the (M, T) token buffer."""
        if use_graph:
            self.step()                       # first launches outside the capture
            graph = self.capture(self.step)
            self.reset()
            for t in range(self.T):
                graph.replay()
                self._code_done(t + 1)
            torch.cuda.current_stream(self.dev).synchronize()
            del graph
        else:
            for t in range(self.T):
                self.step()
                self._code_done(t + 1)
        return self.tokens

    def _code_done(self, steps):
        """Fixed window, after `steps` steps: resamples when they complete a code (the caches always move, nothing slides); a
        beam's moves follow every step where the step does not hold them."""
        if self.beam is not None and not self.beam_moves_in_step:
            self._beam_moves(move_cache=steps < self.T)
        if self.particles is not None and steps % self.U == 0:
            self._resample(steps == self.T, True)

    # ---- long mode: sliding window -----------------------------------------------------------------------------------
    @torch.no_grad()
    def start_long(self, codes_full, chorale, seeds=None, constraint=None, want_logp=False, want_attentions=None, allowed=None,
                   want_allowed_mass=False, particles=None, resample_threshold=0.5, final_resample=True, rules=None, beam=None,
                   no_copy=None, **sampling):
        """codes_full (M, nb) merged codes [continuous decoder: (M, nb, dz) latents], nb >= S; chorale (M, nb * U) int64
        tokens, position-major (the initial PAD / START sequence; generated tokens are written into it).  constraint,
        want_logp: as in `start`, but (M, nb * U), position-major like `chorale`: the sampler reads and writes them at the
        live window's chorale column (the device window index), so the captured step and slide serve every window.
        want_attentions: as in `start`, with `self_probs` (layers, M, H, nb * U, T) and `cross_probs` (layers, M, H, nb * U, S):
        the row is the emitted token's chorale position, its keys are those of the window it was emitted in.
        allowed, want_allowed_mass: as in `start`, but (M, nb * U, 8) / `logmass` (M, nb * U), in chorale coordinates like the
        constraint.
        particles, resample_threshold, final_resample: as in `start`; the histories have one row per code of the chorale.
        rules: as in `start`, with `rule_report` (M, nb * U) in chorale coordinates; the history of a position reaches back through
        the chorale, wherever the model window lies.
        beam: as in `start`; `b_hist` has one row per chorale position.
        no_copy: as in `start`, with `copy_report` (M, nb * U) in chorale coordinates; a context reaches back through the chorale.
        sampling: the other keywords of `start`."""
        M, S, U = self.M, self.S, self.U
        z_full = None
        if self.continuous:
            if codes_full.dim() != 3 or not codes_full.is_floating_point() or codes_full.shape[0] != M or \
                    codes_full.shape[1] < S or codes_full.shape[2] != self.dz:
                raise ValueError(f'codes_full: ({M}, nb >= {S}, {self.dz}) latents expected, got {tuple(codes_full.shape)}')
            z_full = codes_full.to(self.dev, torch.float32).contiguous()
            codes_full = torch.zeros(M, z_full.shape[1], dtype=torch.int64, device=self.dev)   # the window kernel's dummy codes
        codes_full = codes_full.to(self.dev, torch.int64).contiguous()
        if codes_full.dim() != 2 or codes_full.shape[0] != M or codes_full.shape[1] < S:
            raise ValueError(f'codes_full: ({M}, nb >= {S}) expected, got {tuple(codes_full.shape)}')
        self.nb = nb = codes_full.shape[1]
        self.codes_full = codes_full
        self.chorale = chorale.to(self.dev, torch.int64).reshape(M, nb * U).contiguous().clone()
        self.codes_win = torch.zeros(M, S, dtype=torch.int64, device=self.dev)
        self.win.copy_(torch.tensor([0, -1], dtype=torch.int32))
        self.prefix_rows.zero_()
        if self.memkv is None:
            self.prefill(z_full[:, :S] if self.continuous else codes_full[:, :S])
        if self.continuous:
            self.z_full, self.z_nb = z_full, nb
        self._sampling(seeds, **sampling)
        self._configure(Frame(nb * U, self.win, U, nb, self.row_seeds), constraint, want_logp, allowed, want_allowed_mass,
                        particles, resample_threshold, final_resample, rules, want_attentions, beam, no_copy)
        self.row_seeds.copy_(self.seeds)

    def _window(self, P, advance):
        hip.call('vqcpc_decode_window', self.codes_full, self.nb, self.chorale, self.nb * self.U, self.win, int(advance),
                 self.codes_win, self.S, self.tokens, self.T, self.U, int(P), self.prefix_rows, self.table, self.table.shape[0],
                 self.d, self.x, self.d, self.row_seeds, self.seeds, self.pos, self.M)

    def _prefix_cross_attention(self, li, lay, h1, att, P):
        d, ca, kv = self.d, lay.multihead_attn, self.memkv[li]
        qc = ops.gemm_nt(h1, ca.in_proj_weight[:d], bias=ca.in_proj_bias[:d])
        hip.call('vqcpc_decode_prefill_attn', qc, d, kv, kv.data_ptr() + 4 * d, 2 * d, None, None, 0, ca.attn_bias.e1,
                 ca.attn_bias.e2, att, d, self.M, P, self.S, self.T // self.S, self.H, self.hd, self.cross_mask)
        return self._prefix_ln(h1, ops.gemm_nt(att, ca.out_proj.weight, bias=ca.out_proj.bias), lay.norm2)

    def _prefix_cross_aligned(self, li, lay, h1, att, P):
        hip.call('vqcpc_aligned_expand', self.memkv[li], att, self.M, self.S, P, self.U, self.nc, self.d)
        return self._prefix_ln(h1, att, lay.norm2)

    @torch.no_grad()
    def slide(self, t_begin=None, t_relative=0, advance=1):
        """Moves the generation to the window of codes [t_begin, t_begin + S) at position P = t_relative * U: commits the
        live window, loads the new one, recomputes the memory and the cross k | v of its codes and re-prefills the
        prefix.  t_begin=None takes the window index the device holds (the previous window's + `advance`)."""
        if t_begin is not None:
            if not 0 <= t_begin <= self.nb - self.S:
                raise ValueError(f'slide: 0 <= t_begin <= {self.nb - self.S} (got {t_begin})')
            self.win[0:1].fill_(int(t_begin))
        P = int(t_relative) * self.U
        if not 0 <= P < self.T:
            raise ValueError(f'slide: 0 <= t_relative < {self.S} (got {t_relative})')
        self._window(P, advance)
        self._encode_memory(self.codes_win, windowed=True)
        self.prefill_prefix(P)

    def commit(self):
        """Puts the live window's tokens back into the chorale (no new window is loaded)."""
        self.win[0:1].fill_(-1)
        self._window(0, 0)

    @torch.no_grad()
    def run_long(self, code_index_start, code_index_end, use_graph=True, graph_slides=None):
        """Generates the codes [code_index_start, code_index_end) (after `start_long`): head / middle / tail regimes of
        `Decoder.compute_start_end_times`; a slide whenever the window of a code differs from the live one, then U steps.
        use_graph: the step is one captured graph; graph_slides (default: use_graph): the middle slides, which all have
        P = (S // 2) * U and windows that advance by one, are ONE captured graph too.  Returns the chorale (M, nb * U)."""
        from .decoder import Decoder
        S, U, nb = self.S, self.U, self.nb
        if not 0 <= code_index_start <= code_index_end <= nb:
            raise ValueError(f'run_long: 0 <= code_index_start <= code_index_end <= {nb}')
        plan = [(ci,) + tuple(Decoder.compute_start_end_times(ci, nb, S)) for ci in range(code_index_start, code_index_end)]
        if not plan:
            return self.chorale
        graph_slides = use_graph if graph_slides is None else graph_slides
        step_graph = slide_graph = None
        tr_mid = S // 2
        if use_graph or graph_slides:
            chorale0 = self.chorale.clone()
            _, tb0, _, tr0 = plan[0]
            self.slide(tb0, tr0)                  # a live state for the first launches, which stay outside the captures
            if use_graph:
                self.step()
                step_graph = self.capture(self.step)
            n_mid = sum(1 for k in range(1, len(plan)) if plan[k][1] == plan[k - 1][1] + 1 and plan[k][3] == tr_mid)
            if graph_slides and n_mid >= 2:
                self.slide(tb0, tr_mid)
                slide_graph = self.capture(lambda: self.slide(None, tr_mid, advance=1))
            self.chorale.copy_(chorale0)          # the warm-up launches drew and committed tokens: start again
            self._clear_records()
            self.win.copy_(torch.tensor([0, -1], dtype=torch.int32))
        live = None
        for k, (_, tb, _, tr) in enumerate(plan):
            if tb != live:
                if slide_graph is not None and live is not None and tb == live + 1 and tr == tr_mid:
                    slide_graph.replay()          # the device's window index is live + 1 already
                else:
                    self.slide(tb, tr)
                live = tb
            between = self.beam is not None and not self.beam_moves_in_step
            for j in range(U):
                step_graph.replay() if step_graph is not None else self.step()
                if between:                               # the caches move only where the next token is generated without a slide
                    nxt = tb if j + 1 < U else plan[k + 1][1] if k + 1 < len(plan) else None
                    self._beam_moves(move_cache=nxt == tb)
            if self.particles is not None:                # the caches move only where the next code is generated without a slide
                last = k + 1 == len(plan)
                self._resample(last, not last and plan[k + 1][1] == tb, self.chorale)
        self.commit()
        torch.cuda.current_stream(self.dev).synchronize()
        del step_graph, slide_graph
        return self.chorale
