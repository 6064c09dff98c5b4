"""KV-cached sampling of code sequences from the prior (reference: VQCPCB/priors/prior_relative.py:308-353, which runs one
full forward on the model window per code and samples on the host).

The prior is one causal stack: position e's logits depend on codes < e of the window only (row-wise table lookup /
LayerNorm / FFN, causal self-attention), so an incremental step per code computes the same function.  The step is the
shared stack's (transformer/incremental.py) with no cross block, i.e. the decoder's without the cross-attention, 7 launches
per layer + 2; its sampler is vqcpc_prior_sample, which draws the code of position pos, writes the input row of position
pos + 1 and advances the device counter `pos`.  With given codes or code scores (`start(constraint=..., want_logp=...)`) the
sampler is vqcpc_prior_sample_constrained: the same kernel body, which emits the given code where the constraint holds one
and writes the emitted code's log-probability under the model's unmodified row (temperature 1, no filter); it addresses both
at the sequence column win[1] + pos through the device's window index, so the captured step and the captured move below
serve it unchanged.  The default path launches the plain sampler, exactly as before.  With a set of allowed codes per column, its
mass or particles (`start(allowed=..., want_allowed_mass=..., particles=...)`) the sampler is vqcpc_prior_sample_masked, one more
compile-time flag on the same body: a code outside the column's set becomes -inf before the filters, and `logmass` receives the
log of the probability the unmodified row gives to the set; sets and masses are addressed at the same sequence column.

Particles (`start(particles=P)`, csrc/particles.hip with U = 1): the rows are groups of P consecutive rows with their own seeds.
After every code vqcpc_particle_resample adds the code's forced logp / free logmass to every row's log-weight and, where a group's
effective sample size fell below the threshold, draws its ancestors; vqcpc_particle_permute_* then moves the ancestors' state --
the live window's codes, ALL of `seq` (older windows committed the history there, and the next window reloads from it), the logp /
logmass rows, the next input row and, where a cached step follows, every layer's K/V cache rows [0, pos) -- onto the rows in
place.  Before a slide or a forward-form step no cache moves: both recompute from the moved codes.

Beam search (`start(beam=W)`, csrc/prior_beam.hip): the rows are groups of W consecutive rows, the W best plans of one user row so
far.  vqcpc_prior_beam_expand + vqcpc_prior_beam_select take the sampler's place, in both step forms: every row is expanded into
its candidate codes (a forced column's one code, else the column's set, else the vocabulary), scored by the row's total
log-probability plus the code's, and the group's W best (row, code) pairs become the new rows, best first.  The select writes the
live column -- code, next input row, logp, logmass -- in SLOT order, with the ancestors and the two device words `b_bound` =
{pos, col} before the increment.  The moves that follow (`_beam_moves`, vqcpc_particle_permute_* with P = W) bring the history
behind the slots: the live window's codes [0, b_bound[0]), ALL of `seq` (as `_resample` does and for its reason), the logp /
logmass rows' columns [0, b_bound[1]) -- the new column must not move, it is in slot order already -- and, in the cached step only,
the K/V cache rows [0, pos): position p's K/V were written for the ancestor; the forward form and a slide recompute from the moved
codes.  The moves read only device words, so they are launches of the step and a captured step holds them.  Seeds, temperature,
top_k and top_p are unused: the search is deterministic.  A product prior (`IncrementalProductPrior`) launches one
vqcpc_prior_beam_expand_product + vqcpc_prior_beam_select_product pair PER DIGIT STAGE: its search prunes to the W best after
every digit -- a beam over the digit sequence, not over the merged codes -- and only the last stage moves the stack's state, by
the ancestors composed over the stages.

Two regimes, as in the reference (:331-336):

  head (e < N): the first window.  One step per code; ONE captured step replayed N times.
  sliding (e >= N): the reference's window is [e - N + 1, e] and the code comes from its LAST position, i.e. the window
  moves by one code per code.  The window's first input row becomes the start-of-sentence row and every other row loses
  one code of context, so EVERY cache row is stale.  Per move: vqcpc_prior_window (commit the live window's codes, load the
  next window's, the prefix's table rows, the input row of position P, the window's seeds, pos = P) -> the stack
  teacher-forced over the P prefix rows of every sequence (`prefill_prefix`) -> N - P cached steps.
  window_stride = 1 is the reference exactly: P = N - 1, one step per move.  At that stride the cache saves only the last
  layer's prefix outputs and the head over the window's rows; a move costs about one full forward minus those, and what the
  captured move buys is host launch time.  window_stride = k > 1 (opt-in) moves k codes at a time: P = N - k, k steps per
  move, 1 / k of the re-prefills, but code e then sees N - k .. N - 1 previous codes instead of always N - 1 -- a slightly
  different model context, not the reference's.

Window index, position and seeds live in device memory and the window kernel advances the index by the stride, so ONE
captured move (window kernel + re-prefill) and the ONE captured step serve every move of a generation.  A last, shorter
move (when (num_tokens - N) % stride != 0) runs eagerly.

Two forms of a step.  The CACHED form above streams every weight once per step and applies it row by row
(vqcpc_decode_linear), which is the cheap form for a few rows.  The FORWARD form (`step_forward`) runs the training path's
stack over all N rows of the window (table lookup, `forward_rows_masked`: well-filled GEMMs at 24 rows per sequence), the head
on the one row of the position (vqcpc_decode_linear reading that row of every sequence through its leading dimension) and
the same sampler: the reference's algorithm on this package's kernels.  In the sliding regime at stride 1 a cached move is a
re-prefill of N - 1 rows (about one forward) PLUS one cached step, so the forward form is never more work there: a move is
the window kernel + forward + head + sampler.  Its launches are not captured: the stack is GPU-bound from one row on (650 us
eager, 654 us replayed at B = 1), so a graph returns nothing and its capture costs a few ms per generation.  In the head
regime the forward form recomputes the rows before the position, so it wins only when the cached step's row-by-row linears
dominate (measured: from 32 rows).  `run(method='auto')` picks per regime and batch from the
measurements in profiles/generate_prior_perf_log.md (`FORWARD_HEAD_MIN_ROWS`, `FORWARD_SLIDE_MIN_ROWS`); 'cached' and
'forward' force one form.  Strides > 1 always use the cached form.

Rows are independent and every kernel reduces in an order that does not depend on the number of rows, so a row's codes do
not depend on which other rows share the call (given the same seed and the same form; the two forms agree to rounding, so
a draw that sits within ~1e-6 of a cumulative-probability boundary can differ between them)."""
import torch

from .. import hip, ops
from ..transformer.incremental import MAX_ROWS, Frame, IncrementalStack, row_seeds

# method='auto': rows from which the forward form replaces the cached step (profiles/generate_prior_perf_log.md: at the PRI
# shape the head step costs 376 / 1 096 us cached against 735 / 995 us forward at 8 / 32 rows; a stride-1 move 651 / 910 / 1 916 us
# cached against 650 / 742 / 1 012 us forward at 1 / 8 / 32 rows)
FORWARD_HEAD_MIN_ROWS = 32
FORWARD_SLIDE_MIN_ROWS = 1


class IncrementalPrior(IncrementalStack):
    """One generation of `batch` <= 64 rows of `prior` (a PriorRelative in eval mode; the caller holds utils.STEP_LOCK).

        inc = IncrementalPrior(prior, B)
        inc.start(num_tokens, seeds, temperature, top_k, top_p)   # constraint=, want_logp=: given codes, code scores;
                                                                  # allowed=, want_allowed_mass=, particles=: sets, their mass, a filter
                                                                  # beam=W: the W best plans per group of W rows (`beam_results`)
        codes = inc.run(use_graph, window_stride)                 # (B, num_tokens) int64; inc.logp, inc.logmass (B, num_tokens) float32

    `start` + `slide` + `step` expose the single launches (teacher forcing, the sampler's input `logits` and its optional
    probability output `probs`) for the tests."""

    def __init__(self, prior, batch):
        if not 1 <= batch <= MAX_ROWS:
            raise ValueError(f'IncrementalPrior: 1 <= batch <= {MAX_ROWS} (got {batch})')
        pr = self.prior = prior
        M, dev = int(batch), pr.sos.device
        N = self.N = pr.num_tokens
        self.V = pr.num_tokens_per_channel[0]
        layers = list(pr.transformer.layers)
        super().__init__(dev, M, layers, [lay.norm2 for lay in layers], N, pr.d_model)
        self.codes_win = torch.zeros(M, N, dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.allowed, self.logmass, self.masked = None, None, False
        self.beam, self._beam_cache = None, True              # beam width W, or None: the rows are sampled
        self._sos_col = torch.full((M, 1), self.V, dtype=torch.int64, device=dev)    # table row of the start-of-sentence input
        self._init_model()

    def _init_model(self):
        """The model-side buffers of the merged code: the input table, the head and its logits."""
        pr = self.prior
        self.logits = torch.empty(self.M, self.V, dtype=torch.float32, device=self.dev)
        with torch.no_grad():
            self.table = pr._input_table().contiguous()                    # (V + 1, d)
        head = pr.pre_softmaxes[0]
        self.head_w, self.head_b = head.weight, head.bias

    def _probs_buffer(self):
        return torch.zeros(self.M, self.V, dtype=torch.float32, device=self.dev)

    def start(self, num_tokens, seeds=None, temperature=1.0, top_k=0, top_p=1.0, teacher=None, want_probs=False,
              constraint=None, want_logp=False, allowed=None, want_allowed_mass=False, particles=None, resample_threshold=0.5,
              final_resample=True, beam=None):
        """A new generation of `num_tokens` >= N codes per row.  teacher: (M, N) codes of the live window to force instead
        of drawing (single-step use); want_probs: keep the filtered probabilities of the last step in `probs` (M, V).
        constraint: (M, num_tokens) int64 in sequence coordinates, a code >= 0 is emitted at its column, < 0 leaves the draw
        free; want_logp: keep every emitted code's log-probability under the unfiltered row at temperature 1 in `logp`
        (M, num_tokens) float32 (NaN where no step has written yet).  Either one switches the sampler to
        vqcpc_prior_sample_constrained, in both step forms.
        allowed: packed sets (code_sets.pack_sets) int32 (M, num_tokens, words) -- a product prior: (M, num_tokens, ncb, words) --,
        per (row, sequence column) the codes (digits) that may be drawn; the caller has checked that no set is empty and that
        no forced code lies outside its set.  want_allowed_mass: keep in `logmass` (M, num_tokens) float32 the log of the
        probability the unmodified row gives to the column's set (0 where nothing is restricted; a product prior: the sum of
        the stages' conditional masses along the emitted digits).  particles: None, or P in [2, 64] dividing M: the rows are
        M / P groups of P particles, resampled after every code (`_resample`); logp / logmass are then kept whenever a
        constraint / sets are given.  resample_threshold, final_resample: as in `IncrementalDecoder.start`.  Any of the three
        switches the sampler to vqcpc_prior_sample_masked (vqcpc_prior_sample_product_masked), in both step forms.  teacher
        excludes all of them, want_probs excludes particles.
        beam: None, or W in [1, 64] dividing M: the rows are M / W groups of W hypotheses and vqcpc_prior_beam_expand +
        vqcpc_prior_beam_select (a product prior: their _product forms, a pair per digit stage) replace the sampler (`_beam`);
        seeds, temperature, top_k and top_p are then unused.  It excludes particles, teacher and want_probs."""
        if not temperature > 0:
            raise ValueError('temperature must be > 0')
        if num_tokens < self.N:
            raise ValueError(f'IncrementalPrior: num_tokens >= {self.N} (got {num_tokens})')
        self.nt = int(num_tokens)
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        if seeds is not None:
            self.row_seeds.copy_(row_seeds(seeds, self.M))
        self.teacher = None if teacher is None else teacher.to(self.dev, torch.int64).reshape(self.M, self.N).contiguous()
        if particles is not None and want_probs:
            raise ValueError('particles and want_probs exclude each other (the probabilities are not moved with a resampled row)')
        if particles is not None and self.d % 4:
            raise ValueError(f'particles: d_model = {self.d}, a multiple of 4 is needed to move the K/V cache rows')
        self.frame = Frame(self.nt, self.win, 1, self.nt, self.row_seeds)
        self._particles(particles, resample_threshold, final_resample, None)
        scored = particles is not None                        # the weights are the forced codes' logp and the sets' mass
        self._constrain(constraint, want_logp or (scored and constraint is not None), self.nt)
        self._mask(allowed, want_allowed_mass or (scored and allowed is not None))
        self.probs = self._probs_buffer() if want_probs else None
        self._beam(beam)
        self.seq = torch.zeros(self.M, self.nt, dtype=torch.int64, device=self.dev)
        self.reset()

    def _set_shape(self):
        """The shape of the packed sets of one generation."""
        return (self.M, self.nt, (self.V + 31) // 32)

    def _mask(self, allowed, want_mass):
        """The masked sampler's buffers, addressed like the constrained sampler's: the packed sets are COPIED into a buffer of
        this stack before any warm-up launch, so a captured step or move reads every window's sets through the window index."""
        if (allowed is not None or want_mass) and self.teacher is not None:
            raise ValueError('allowed / want_allowed_mass and teacher exclude each other')
        self.allowed = None
        if allowed is not None:
            if tuple(allowed.shape) != self._set_shape() or allowed.dtype != torch.int32:
                raise ValueError(f'allowed: packed sets {self._set_shape()} int32 expected, got {tuple(allowed.shape)} '
                                 f'{allowed.dtype}')
            self.allowed = torch.empty(self._set_shape(), dtype=torch.int32, device=self.dev)
            self.allowed.copy_(allowed)
        self.logmass = torch.empty(self.M, self.nt, dtype=torch.float32, device=self.dev) if want_mass else None
        self.masked = allowed is not None or bool(want_mass) or self.particles is not None

    # ---- beam search (csrc/prior_beam.hip) -------------------------------------------------------------------------------
    def _beam(self, W):
        """The beam's state: per row the plan's total log-probability `b_score` and its last ancestor `b_anc`; the device flag
        `b_flag` (some row moved), the two words `b_bound` = {pos, col} of the last select before its increment, per column of the
        sequence the ancestors `b_hist` (int32, -1 where nothing was generated), and the scratch the expansion hands to the
        select: per row its W best (cand, code, lp), its set's log-mass and its lowest candidate code with that code's lp."""
        self.beam = None
        if W is None:
            return
        if isinstance(W, bool) or int(W) != W or not 1 <= int(W) <= MAX_ROWS or self.M % int(W):
            raise ValueError(f'beam: 1 <= beam <= {MAX_ROWS} dividing the stack\'s {self.M} rows expected, got {W}')
        W = int(W)
        if self.particles is not None:
            raise ValueError('beam and particles exclude each other')
        if self.teacher is not None or self.probs is not None:
            raise ValueError('beam and teacher / want_probs exclude each other')
        if W > 1 and self.d % 4:
            raise ValueError(f'beam: d_model = {self.d}, a multiple of 4 is needed to move the K/V cache rows')
        self._beam_buffers(W)
        self.beam = W

    def _beam_buffers(self, W):
        M = self.M
        f32, i32 = dict(dtype=torch.float32, device=self.dev), dict(dtype=torch.int32, device=self.dev)
        self.b_score, self.b_anc = torch.empty(M, **f32), torch.empty(M, **i32)
        self.b_flag, self.b_bound = torch.empty(1, **i32), torch.empty(2, **i32)
        self.b_hist = torch.empty(self.nt, M, **i32)
        self.b_cand, self.b_code, self.b_lp = torch.empty(M, W, **f32), torch.zeros(M, W, **i32), torch.empty(M, W, **f32)
        self.b_mass, self.b_low, self.b_lowlp = torch.empty(M, **f32), torch.zeros(M, **i32), torch.empty(M, **f32)

    def _clear_beam(self):
        """The standard start: score 0 for a group's first row, -inf for the others -- identical rows would fill the beam with
        copies of one plan."""
        if self.beam is None:
            return
        self.b_score.fill_(float('-inf'))
        self.b_score[0::self.beam] = 0.0
        self.b_anc.copy_(torch.arange(self.M, dtype=torch.int32))
        for rows, value in ((self.b_flag, 0), (self.b_bound, 0), (self.b_hist, -1)):
            rows.fill_(value)

    def _beam_moves(self, move_cache):
        """After vqcpc_prior_beam_select: row k <- row b_anc[k] of everything behind the live column, which the select wrote in
        slot order already.  The bounds are device words: the window's codes move in [0, b_bound[0]), the record rows in
        [0, b_bound[1]), the caches in [0, pos) of the incremented pos; `seq` moves whole (`_resample`).  move_cache=False in the
        forward form, which recomputes from the moved codes.  W = 1 has nothing to move."""
        W, M, nt, N = self.beam, self.M, self.nt, self.N
        if W == 1:
            return
        anc, flag, bound = self.b_anc, self.b_flag, self.b_bound
        hip.call('vqcpc_particle_permute_i64', self.codes_win, N, N, bound[0:1], anc, flag, M, W)
        hip.call('vqcpc_particle_permute_i64', self.seq, nt, nt, None, anc, flag, M, W)
        for rows in (self.logp, self.logmass):
            if rows is not None:
                hip.call('vqcpc_particle_permute_f32', rows, nt, nt, bound[1:2], anc, flag, M, W)
        if move_cache:
            for cache in (self.kcache, self.vcache):
                hip.call('vqcpc_particle_permute_cache', cache, len(self.layers), self.W, self.d, self.pos, anc, flag, M, W)

    def _beam_step(self):
        """The two launches in the sampler's place, and the moves."""
        N, nt, M = self.N, self.nt, self.M
        hip.call('vqcpc_prior_beam_expand', self.logits, self.V, self.V, M, self.beam, self.constraint, nt, self.allowed, nt,
                 self.win, self.b_score, N, self.pos, self.b_cand, self.b_code, self.b_lp, self.b_mass, self.b_low, self.b_lowlp,
                 None)
        hip.call('vqcpc_prior_beam_select', self.b_cand, self.b_code, self.b_lp, self.b_mass, self.b_low, self.b_lowlp, self.V, M,
                 self.beam, self.logp, nt, self.logmass, nt, self.win, self.codes_win, N, N, self.table, self.table.shape[0], self.d,
                 self.x, self.d, self.b_score, self.b_anc, self.b_flag, self.b_bound, self.b_hist, nt, self.pos)
        self._beam_moves(self._beam_cache)

    def beam_results(self):
        """After a run: the plans' total log-probabilities (G, W), non-increasing along W and -inf for a dead slot, and the
        ancestors per column of the sequence."""
        return {'scores': self.b_score.view(self.M // self.beam, self.beam).clone(), 'ancestors': self.b_hist}

    def reset(self):
        """Back to the head regime's first position; the sequence is cleared, and so is every log-probability and log-mass (NaN:
        a run writes each column once, so none stays) and the particle filter's state."""
        self.seq.zero_()
        for rows in (self.logp, self.logmass):
            if rows is not None:
                rows.fill_(float('nan'))
        self._clear_particles()
        self._clear_beam()
        self.codes_win.zero_()
        self.ticket.zero_()
        self.win.copy_(torch.tensor([0, -1], dtype=torch.int32))
        self._window(0, 0)                                    # window 0, P = 0: start-of-sentence row, the rows' own seeds

    # ---- one step: the sampler, and the forward form ---------------------------------------------------------------------
    def _sample(self):
        N = self.N
        if self.beam is not None:
            self._beam_step()
            return
        if self.masked:
            hip.call('vqcpc_prior_sample_masked', self.logits, self.V, self.V, self.M, self.temperature, self.top_k, self.top_p,
                     self.seeds, self.constraint, self.nt, self.logp, self.nt, self.win, self.allowed, self.nt, self.logmass,
                     self.nt, self.codes_win, N, N, self.table, self.table.shape[0], self.d, self.x, self.d, self.probs, self.V,
                     self.pos, self.ticket)
            return
        if self.constrained:
            hip.call('vqcpc_prior_sample_constrained', self.logits, self.V, self.V, self.M, self.temperature, self.top_k,
                     self.top_p, self.seeds, self.constraint, self.nt, self.logp, self.nt, self.win, self.codes_win, N, N,
                     self.table, self.table.shape[0], self.d, self.x, self.d, self.probs, self.V, self.pos, self.ticket)
            return
        hip.call('vqcpc_prior_sample', self.logits, self.V, self.V, self.M, self.temperature, self.top_k, self.top_p,
                 self.seeds, self.teacher, N, self.codes_win, N, N, self.table, self.table.shape[0], self.d, self.x, self.d,
                 self.probs, self.V, self.pos, self.ticket)

    def step_forward(self, p):
        """The forward form of the step at position p (the caller's p must be the device's `pos`): the training path's
        stack over the window's N rows, the head on row p of every sequence, the sampler."""
        M, N, d, V = self.M, self.N, self.d, self.V
        if not 0 <= p < N:
            raise ValueError(f'step_forward: 0 <= p < {N} (got {p})')
        idx = torch.cat([self._sos_col, self.codes_win[:, :N - 1]], dim=1).reshape(-1)       # the shift by one
        rows = self._input_rows(idx)                                                         # (M * N, d)
        out, _ = self.prior.transformer.forward_rows_masked(rows, M, ops.MASK_CAUSAL)
        self._forward_tail(out, p)

    def _forward_tail(self, out, p):
        """The head on row p of every sequence of `out` (M * N, d), and the sampler."""
        M, N, d, V = self.M, self.N, self.d, self.V
        hip.call('vqcpc_decode_linear', out.data_ptr() + 4 * p * d, N * d, None, self.head_w, self.head_b, None, 0, self.logits,
                 V, M, V, d, 0)
        self._beam_cache = False                              # the forward form keeps no cache: a beam moves codes and records only
        try:
            self._sample()
        finally:
            self._beam_cache = True

    def _move_forward(self):
        """One stride-1 move in the forward form: commit / load the next window at position N - 1, then its one code."""
        self._window(self.N - 1, 1)
        self.step_forward(self.N - 1)

    # ---- moving the window ---------------------------------------------------------------------------------------------
    def _window(self, P, advance):
        hip.call('vqcpc_prior_window', self.seq, self.nt, self.nt, self.win, int(advance), self.codes_win, self.N, int(P),
                 self.prefix_rows, self.table, self.table.shape[0], self.d, self.x, self.d, self.row_seeds, self.seeds,
                 self.pos, self.M)

    @torch.no_grad()
    def slide(self, w=None, P=0, advance=1):
        """Moves the generation to the window of codes [w, w + N) at position P: commits the live window, loads the new one
        and re-prefills its prefix.  w=None takes the window index the device holds (the previous window's + its advance)."""
        if w is not None:
            if not 0 <= w <= self.nt - self.N:
                raise ValueError(f'slide: 0 <= w <= {self.nt - self.N} (got {w})')
            self.win[0:1].fill_(int(w))
        if not 0 <= P < self.N:
            raise ValueError(f'slide: 0 <= P < {self.N} (got {P})')
        self._window(P, advance)
        self.prefill_prefix(int(P))

    def commit(self):
        """Puts the live window's codes into the sequence (no new window is loaded)."""
        self.win[0:1].fill_(-1)
        self._window(0, 0)

    # ---- particles -----------------------------------------------------------------------------------------------------
    def _resample(self, last, move_cache):
        """After a code (one step: U = 1): the weight update and the resampling decision (vqcpc_particle_resample, the forced
        code's logp or the set's logmass at the column win[1] + pos - 1), then the group's generation state follows the
        ancestors in place (vqcpc_particle_permute_*): the live window's codes [0, pos), ALL of `seq` -- older windows committed
        the history before the live window there, and the next vqcpc_prior_window reloads from it --, the logp / logmass rows,
        the next input row and, with move_cache -- a cached step follows; a slide or a forward-form step recomputes from the
        moved codes --, every layer's K and V cache rows [0, pos).  The seeds stay with their slots, so copies of one ancestor
        diverge.  The launches are issued eagerly between the step replays of a graphed run, as the decoder's are.  last: the
        code is the generation's last one -- a forced resampling (`final_resample`), or the weight update alone."""
        P, M, nt, N = self.particles, self.M, self.nt, self.N
        force = bool(last and self.p_final)
        threshold = 0.0 if last and not self.p_final else self.p_threshold
        hip.call('vqcpc_particle_resample', self.p_lw, self.p_evidence, self.p_pending, self.p_seeds, self.constraint, nt,
                 self.logp if self.constraint is not None else None, nt, self.logmass if self.allowed is not None else None, nt,
                 self.pos, self.win, 1, threshold, int(force), self.p_anc, self.p_wn, self.p_ess, self.p_flag,
                 self.p_hist_anc, self.p_hist_wn, self.p_hist_ess, self.p_hist_anc.shape[0], M, P)
        if threshold == 0.0 and not force:
            return
        anc, flag = self.p_anc, self.p_flag
        hip.call('vqcpc_particle_permute_i64', self.codes_win, N, N, self.pos, anc, flag, M, P)
        hip.call('vqcpc_particle_permute_i64', self.seq, nt, nt, None, anc, flag, M, P)
        for rows in (self.logp, self.logmass):
            if rows is not None:
                hip.call('vqcpc_particle_permute_f32', rows, nt, nt, None, anc, flag, M, P)
        if not last:
            hip.call('vqcpc_particle_permute_f32', self.x, self.d, self.d, None, anc, flag, M, P)
            if move_cache:
                for cache in (self.kcache, self.vcache):
                    hip.call('vqcpc_particle_permute_cache', cache, len(self.layers), self.W, self.d, self.pos, anc, flag, M, P)

    # ---- a whole generation --------------------------------------------------------------------------------------------
    def _forms(self, method, stride):
        if method not in ('auto', 'cached', 'forward'):
            raise ValueError(f"method: 'auto', 'cached' or 'forward' (got {method!r})")
        if method == 'forward' and stride != 1:
            raise ValueError("method='forward' moves the window one code at a time (window_stride = 1)")
        if method == 'auto':
            head = 'forward' if self.M >= FORWARD_HEAD_MIN_ROWS else 'cached'
            slide = 'forward' if stride == 1 and self.M >= FORWARD_SLIDE_MIN_ROWS else 'cached'
            return head, slide
        return method, method

    @torch.no_grad()
    def run(self, use_graph=True, window_stride=1, graph_slides=None, method='auto'):
        """Generates the `num_tokens` codes of `start`: N steps in window 0, then moves of `window_stride` codes.
        method: the form of the steps per regime (module docstring).  use_graph: the cached step is a captured graph (the
        forward form's launches are always eager); graph_slides (default: use_graph): the cached form's full-stride moves are ONE captured graph
        too.  Returns the sequence (M, num_tokens).  With `start(want_logp=True)` every column of `logp` is written exactly
        once: columns 0 .. N - 1 in window 0, then `window_stride` columns per move, then the last, shorter move's; what the
        warm-up launches of a capture wrote is cleared by the `reset` that follows them."""
        N, nt, k = self.N, self.nt, int(window_stride)
        if not 1 <= k < max(N, 2):
            raise ValueError(f'run: 1 <= window_stride < {N} (got {window_stride})')
        head_form, slide_form = self._forms(method, k)
        n_full, rem = divmod(nt - N, k)
        graph_slides = use_graph if graph_slides is None else graph_slides
        step_graph = slide_graph = None
        warmed = False
        if use_graph and (head_form == 'cached' or (slide_form == 'cached' and nt > N)):
            self.step()                           # first launches outside the capture
            step_graph = self.capture(self.step)
            warmed = True
        if slide_form == 'cached' and graph_slides and n_full >= 2:
            self.slide(0, N - k, advance=k)
            slide_graph = self.capture(lambda: self.slide(None, N - k, advance=k))
            warmed = True
        if warmed:
            self.reset()                          # the warm-up launches drew and committed codes: start again
        step = step_graph.replay if step_graph is not None else self.step
        done = 0                                  # codes emitted; with particles every code ends in `_resample`

        def emitted(cached_step_follows):
            nonlocal done
            done += 1
            if self.particles is not None:
                self._resample(done == nt, cached_step_follows)
        for p in range(N):
            if head_form == 'forward':
                self.step_forward(p)
            else:
                step()
            emitted(head_form == 'cached' and p < N - 1)
        for i in range(n_full):
            if slide_form == 'forward':
                if i == 0:
                    self.win[0:1].fill_(1)        # afterwards the window kernel advances the device's index by one per move
                self._move_forward()
                emitted(False)
            elif slide_graph is not None and i >= 1:
                slide_graph.replay()              # the device's window index is (i + 1) * k already
            else:
                self.slide((i + 1) * k, N - k, advance=k)
            if slide_form == 'cached':
                for j in range(k):
                    step()
                    emitted(j < k - 1)
        if rem:
            self.slide(nt - N, N - rem, advance=0)
            for j in range(rem):
                step()
                emitted(j < rem - 1)
        self.commit()
        torch.cuda.current_stream(self.dev).synchronize()
        del step_graph, slide_graph
        return self.seq


class IncrementalProductPrior(IncrementalPrior):
    """`IncrementalPrior` for a prior with code_model = 'product' (priors/prior_relative.py): the same stack, moves, regimes and
    forms on merged codes; what differs is where a code enters and leaves the stack.

      inputs: a code's input row is the sum of its digits' rows of the (ncb, K, d) tables (vqcpc_product_gather; the sampler and
      vqcpc_prior_window_product write the same chain), the start of sentence is row V = K**ncb, `sos`.
      a step's tail: per stage j, ONE vqcpc_decode_linear (head j on h_j) and ONE vqcpc_prior_sample_product, which draws or
      forces digit j, adds the stage's log-probability and hands h_{j+1} = h_j + D_j[digit] to the next stage; the last stage
      emits the merged code, the next input row and advances `pos`.  2 ncb launches in place of 2; `stage_logits` holds the ncb
      stages' rows (ncb, M, K) (`logits` is stage 0's), `probs` likewise.  temperature / top_k / top_p act on each digit's conditional distribution.

    No buffer of K**ncb rows exists."""

    def _init_model(self):
        pr, M, dev, d = self.prior, self.M, self.dev, self.d
        ncb, K = self.ncb, self.K = pr.num_codebooks, pr.codebook_size
        f32 = dict(dtype=torch.float32, device=dev)
        self.stage_logits = torch.empty(ncb, M, K, **f32)
        self.logits = self.stage_logits[0]                                 # what the stack's step fills: stage 0's
        with torch.no_grad():
            self.tables = pr._input_tables().contiguous()                  # (ncb, K, d)
            self.sos = pr.sos.detach().reshape(1, d).contiguous()
        self.heads = [(h.weight, h.bias) for h in pr.pre_softmaxes]
        self.head_w, self.head_b = self.heads[0]                           # the stack's step runs head 0 on its output
        self.dtab = pr.digit_embeddings.weight if ncb > 1 else None
        self.hs = [torch.empty(M, d, **f32) for _ in range(ncb - 1)]       # h_1 .. h_{ncb-1}
        self.digits = torch.zeros(M, ncb, dtype=torch.int32, device=dev)
        self.logp_acc = torch.zeros(M, **f32)

    def _probs_buffer(self):
        return torch.zeros(self.ncb, self.M, self.K, dtype=torch.float32, device=self.dev)

    def _beam_buffers(self, W):
        """On top of the merged beam's: the stage's scores (the next stage's base), the ancestors composed over the stages of a
        position, and the log-mass accumulator (the masked sampler's exists only with sets)."""
        super()._beam_buffers(W)
        self.b_stage = torch.empty(self.M, dtype=torch.float32, device=self.dev)
        self.b_anc_total = torch.zeros(self.M, dtype=torch.int32, device=self.dev)
        self.b_mass_acc = torch.zeros(self.M, dtype=torch.float32, device=self.dev)

    def _beam_stages(self, h0, ldh0):
        """`_stages` under a beam: per stage the head (stage 0's logits are there), the expansion of the stage's K digits on the
        base the stage adds to, and the select, which prunes to the group's W best (row, digit) pairs and hands the next stage
        its rows in slot order; the last stage emits the merged codes with the composed ancestors, and the moves follow."""
        M, N, K, ncb, d, nt, W = self.M, self.N, self.K, self.ncb, self.d, self.nt, self.beam
        scratch = (self.b_cand, self.b_code, self.b_lp, self.b_mass, self.b_low, self.b_lowlp)
        for j in range(ncb):
            h, ldh = (h0, ldh0) if j == 0 else (self.hs[j - 1], d)
            if j > 0:
                w, b = self.heads[j]
                hip.call('vqcpc_decode_linear', h, d, None, w, b, None, 0, self.stage_logits[j], K, M, K, d, 0)
            last = j == ncb - 1
            hip.call('vqcpc_prior_beam_expand_product', self.stage_logits[j], K, K, ncb, j, M, W, self.constraint, nt, self.allowed,
                     nt, self.win, self.b_score if j == 0 else self.b_stage, None if j == 0 else self.b_anc_total, N, self.pos,
                     *scratch, None)
            hip.call('vqcpc_prior_beam_select_product', *scratch, K, ncb, j, M, W, self.digits, self.logp_acc, self.b_mass_acc,
                     self.b_stage, self.b_anc_total, None if last else h, ldh, None if last else self.dtab,
                     None if last else self.hs[j], d, self.logp, nt, self.logmass, nt, self.win, self.codes_win, N, N, self.tables, d,
                     self.x, d, self.b_score, self.b_anc, self.b_flag, self.b_bound, self.b_hist, nt, self.pos)
        self._beam_moves(self._beam_cache)

    def _set_shape(self):
        return (self.M, self.nt, self.ncb, (self.K + 31) // 32)

    def _mask(self, allowed, want_mass):
        super()._mask(allowed, want_mass)
        self.mass_acc = torch.zeros(self.M, dtype=torch.float32, device=self.dev) if self.masked else None

    def _input_rows(self, idx):
        return ops.ProductEmbeddingFn.apply(self.tables, self.sos, idx)

    def _stages(self, h0, ldh0):
        """The ncb stages on h_0 = the stack's output rows (a pointer and its leading dimension); stage 0's logits are there."""
        M, N, K, ncb, d = self.M, self.N, self.K, self.ncb, self.d
        if self.beam is not None:
            self._beam_stages(h0, ldh0)
            return
        for j in range(ncb):
            h, ldh = (h0, ldh0) if j == 0 else (self.hs[j - 1], d)
            if j > 0:
                w, b = self.heads[j]
                hip.call('vqcpc_decode_linear', h, d, None, w, b, None, 0, self.stage_logits[j], K, M, K, d, 0)
            last = j == ncb - 1
            if self.masked:
                hip.call('vqcpc_prior_sample_product_masked', self.stage_logits[j], K, K, ncb, j, M, self.temperature, self.top_k,
                         self.top_p, self.seeds, self.teacher, N, self.constraint, self.nt, self.logp, self.nt, self.win,
                         self.allowed, self.nt, self.logmass, self.nt, self.digits, self.logp_acc, self.mass_acc,
                         None if last else h, ldh, None if last else self.dtab, None if last else self.hs[j], d, self.codes_win, N,
                         N, self.tables, d, self.x, d, None if self.probs is None else self.probs[j], K, self.pos, self.ticket)
                continue
            hip.call('vqcpc_prior_sample_product', self.stage_logits[j], K, K, ncb, j, M, self.temperature, self.top_k, self.top_p,
                     self.seeds, self.teacher, N, self.constraint, self.nt, self.logp, self.nt, self.win, self.digits,
                     self.logp_acc, None if last else h, ldh, None if last else self.dtab, None if last else self.hs[j], d,
                     self.codes_win, N, N, self.tables, d, self.x, d, None if self.probs is None else self.probs[j], K, self.pos,
                     self.ticket)

    def _sample(self):
        self._stages(self.hb[(len(self.layers) - 1) % 2], self.d)          # the cached step's last LayerNorm wrote h_0 there

    def _forward_tail(self, out, p):
        M, N, d, K = self.M, self.N, self.d, self.K
        h0 = out.data_ptr() + 4 * p * d                                     # row p of every sequence
        hip.call('vqcpc_decode_linear', h0, N * d, None, self.head_w, self.head_b, None, 0, self.logits, K, M, K, d, 0)
        self._beam_cache = False                              # as the merged tail: no cache moves in the forward form
        try:
            self._stages(h0, N * d)
        finally:
            self._beam_cache = True

    def _window(self, P, advance):
        hip.call('vqcpc_prior_window_product', self.seq, self.nt, self.nt, self.win, int(advance), self.codes_win, self.N, int(P),
                 self.prefix_rows, self.tables, self.ncb, self.K, self.sos, self.d, self.x, self.d, self.row_seeds, self.seeds,
                 self.pos, self.M)
