"""The incremental (KV-cached) transformer stack that the decoder's and the prior's generation share
(decoders/generation.py, priors/generation.py; kernels: csrc/decode.hip, csrc/prior.hip).

Both generators run one causal stack a position at a time over a window of W positions (the decoder's T target tokens, the
prior's N codes): position t's output depends on positions < t only (causal self-attention, row-wise embedding / LayerNorm
/ FFN), so one incremental step per position computes the same function as the full forward.

  step, per layer:  in_proj -> self-attention on the layer's K/V cache (the step's k / v row is stored at row pos) ->
  out_proj + residual -> add & LayerNorm -> the cross hook -> linear1 + ReLU -> linear2 + residual -> add & LayerNorm;  then
  the head(s) and the subclass's sampler, which draws the position's token, writes the input row of position pos + 1 and
  advances the device counter `pos`.  7 launches per layer + 2 plus the cross hook's: none (prior, whose stack has no
  cross block), 3 + a LayerNorm (decoder: cross q -> cross-attention -> out_proj + residual), 1 + a LayerNorm (diagonal
  decoder: vqcpc_decode_aligned_add).  A layer whose attention maps are recorded (the decoder's `want_attentions`) calls
  vqcpc_decode_attn_probs where the others call vqcpc_decode_attn: same launch count, same ctx bits.

  prefix (`prefill_prefix`): when a window moves, every cache row is stale.  The stack is teacher-forced over the P prefix
  rows of every sequence (vqcpc_gemm_nt, vqcpc_add_layernorm_fwd, vqcpc_decode_prefill_attn, the prefix-side cross hook),
  which leaves every layer's K/V cache rows [0, P) filled; the last layer stops after its self-attention k | v.

Every kernel of the step reads `pos` from device memory, so ONE captured step (`capture`) is replayed for every position.
Rows are independent and every kernel reduces in an order that does not depend on the number of rows, so a row's tokens do
not depend on which other rows share the call (given the same inputs and seed).

The stack also owns what both generators' constrained samplers need (`_constrain`: the constraint, `logp`, the `constrained`
flag), the particle filter's state (`_particles`, `_clear_particles`, `particle_results`; each generator has its own `_resample`,
which knows what of its state follows a resampled row) and the coordinate frame of a generation's per-position buffers (`Frame`), which the recorded attention launch reads."""
import collections
import gc

import torch

from .. import hip, ops
from ..utils import STEP_LOCK

MAX_ROWS = 64                # rows of one incremental stack (vqcpc_decode_*); larger batches run in chunks


# The coordinates the per-position buffers of a generation are addressed in: `width` columns per row; `win` None (the column is
# the window's position) or the device window index (the column is the position's place in the whole sequence); `stride`
# positions per window step (the recorded attention rows'); `codes` rows of the per-code histories; `seeds` the per-row seeds
# that never move.  Tensors and ints only: a bound method of the stack in it would be a reference cycle (`IncrementalStack`).
Frame = collections.namedtuple('Frame', 'width win stride codes seeds')


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


def row_seeds(seed, n):
    """int -> n per-row int64 seeds (splitmix64 of (seed, row)); a tensor of n int64 is taken as it is; None draws one
    int from torch's CPU generator."""
    if torch.is_tensor(seed):
        s = seed.reshape(-1).to(torch.int64)
        if s.numel() != n:
            raise ValueError(f'seed: {s.numel()} per-row seeds for {n} rows')
        return s.cpu()
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    vals = [_splitmix64((int(seed) * 0x100000001B3 + r) & 0xFFFFFFFFFFFFFFFF) for r in range(n)]
    return torch.tensor([v - (1 << 64) if v >= 1 << 63 else v for v in vals], dtype=torch.int64)


def generate_in_chunks(model, B, width, chunk, chunk_rows=MAX_ROWS):
    """The public generation methods' loop: `chunk(n, rows)` -> (n, width) int64 tokens of the rows `rows` (a slice of
    n <= chunk_rows <= MAX_ROWS of the B rows), from an incremental stack that lives for that chunk only.  Runs under STEP_LOCK
    (never interleaved with a training step of another thread), without gradients and with `model` in eval mode.  -> (B, width).
    chunk_rows: a multiple of the group size when the rows come in groups that must share a stack (particles)."""
    if not 1 <= chunk_rows <= MAX_ROWS:
        raise ValueError(f'generate_in_chunks: 1 <= chunk_rows <= {MAX_ROWS} (got {chunk_rows})')
    out = torch.empty(B, width, dtype=torch.int64, device=model.sos.device)
    with STEP_LOCK, torch.no_grad():
        was_training = model.training
        model.eval()
        try:
            for b0 in range(0, B, chunk_rows):
                n = min(chunk_rows, B - b0)
                out[b0:b0 + n] = chunk(n, slice(b0, b0 + n))
        finally:
            model.train(was_training)
    return out


class IncrementalStack:
    """The buffers, the step and the prefix re-prefill of M <= 64 rows of a stack `layers` over a window of W positions.
    last_norms: per layer, the LayerNorm after the FFN (the decoder's norm3, the prior's norm2).  A subclass provides
    `table`, `head_w`, `head_b`, `logits` and `_sample`, and, where its layers have a cross block, sets the hooks `_cross` /
    `_prefix_cross` once at construction.  The hooks are plain functions of (stack, layer index, layer, ...), not bound
    methods: an instance that held its own bound methods would be a reference cycle, and its caches would outlive `del`."""

    def __init__(self, dev, M, layers, last_norms, W, d):
        self.dev, self.M, self.W, self.d = dev, M, W, d
        self.layers, self.last_norms = layers, last_norms
        a = layers[0].self_attn
        self.H, self.hd = a.num_heads, a.head_dim
        self.ff = layers[0].linear1.weight.shape[0]
        f32 = dict(dtype=torch.float32, device=dev)
        self.x = torch.empty(M, d, **f32)                     # input rows of the current position
        self.hb = [torch.empty(M, d, **f32) for _ in range(2)]
        self.h1, self.s, self.att = (torch.empty(M, d, **f32) for _ in range(3))
        self.qkv = torch.empty(M, 3 * d, **f32)
        self.f = torch.empty(M, self.ff, **f32)
        self.mean, self.rstd = torch.empty(M, **f32), torch.empty(M, **f32)
        self.kcache = torch.empty(len(layers), M, W, d, **f32)
        self.vcache = torch.empty(len(layers), M, W, d, **f32)
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.seeds = torch.zeros(M, dtype=torch.int64, device=dev)        # the live window's effective seeds
        self.row_seeds = torch.zeros(M, dtype=torch.int64, device=dev)
        self.win = torch.tensor([0, -1], dtype=torch.int32, device=dev)   # {next window, live window}
        self.prefix_rows = torch.zeros(M * W, dtype=torch.int64, device=dev)
        self._pmean, self._prstd = torch.empty(M * W, **f32), torch.empty(M * W, **f32)
        self.teacher = None
        self.probs = None
        self.self_probs, self._attn_slot = None, {}           # attention maps: off (a subclass's `start` may turn them on)
        self.frame = None                                     # the `Frame` of the generation's option buffers
        self.constraint, self.logp, self.constrained = None, None, False
        self.particles = None                                 # group size P, or None: plain rows (`_particles`)
        self._cross, self._prefix_cross = IncrementalStack._no_cross, IncrementalStack._no_prefix_cross

    def _constrain(self, constraint, want_logp, width):
        """The constrained sampler's set-up: `constraint` (M, width) int64 or None, `logp` (M, width) float32 -- allocated here,
        filled by the subclass's `reset` -- or None, and `constrained`, which chooses the sampler."""
        if (constraint is not None or want_logp) and self.teacher is not None:
            raise ValueError('constraint / want_logp and teacher exclude each other (an all-forced constraint is teacher forcing)')
        if constraint is not None:
            if tuple(constraint.shape) != (self.M, width) or constraint.dtype != torch.int64:
                raise ValueError(f'constraint: ({self.M}, {width}) int64 expected, got {tuple(constraint.shape)} '
                                 f'{constraint.dtype}')
            constraint = constraint.to(self.dev).contiguous()
        self.constraint = constraint
        self.logp = torch.empty(self.M, width, dtype=torch.float32, device=self.dev) if want_logp else None
        self.constrained = constraint is not None or bool(want_logp)

    # ---- particles (csrc/particles.hip): the state both generators' filters keep -----------------------------------------
    def _particles(self, P, threshold, final, want_attentions):
        """The particle filter's state: per row the running log-weight `p_lw`, the last normalised weights `p_wn` and
        ancestors `p_anc`; per group the log-evidence `p_evidence`, the last code's increment `p_pending` and effective sample
        size `p_ess`; the device flag `p_flag`; and per code of the frame the histories `p_hist_anc` (int32, -1 where no code
        was finished), `p_hist_wn`, `p_hist_ess` (NaN there).  `p_seeds`: the frame's seeds (the resampling uniform is keyed by
        the group's first one and the code's chorale index)."""
        self.particles = None
        if P is None:
            return
        P = int(P)
        if not 2 <= P <= MAX_ROWS or self.M % P:
            raise ValueError(f'particles: 2 <= particles <= {MAX_ROWS} dividing the stack\'s {self.M} rows expected, got {P}')
        if not 0.0 <= float(threshold) <= 1.0:
            raise ValueError(f'resample_threshold: a share of the particles in [0, 1] expected, got {threshold}')
        if want_attentions is not None:
            raise ValueError('particles: attention maps are not moved with a resampled row; want_attentions must be None')
        if self.teacher is not None:
            raise ValueError('particles and teacher exclude each other')
        M, G, codes = self.M, self.M // P, self.frame.codes
        self.particles, self.p_threshold, self.p_final, self.p_seeds = P, float(threshold), bool(final), self.frame.seeds
        f32, i32 = dict(dtype=torch.float32, device=self.dev), dict(dtype=torch.int32, device=self.dev)
        self.p_lw, self.p_wn, self.p_anc = torch.empty(M, **f32), torch.empty(M, **f32), torch.empty(M, **i32)
        self.p_evidence, self.p_pending, self.p_ess = (torch.empty(G, **f32) for _ in range(3))
        self.p_flag = torch.empty(1, **i32)
        self.p_hist_anc, self.p_hist_wn = torch.empty(codes, M, **i32), torch.empty(codes, M, **f32)
        self.p_hist_ess = torch.empty(codes, G, **f32)

    def _clear_particles(self):
        """The filter before its first code (a warm-up step of a capture writes into these buffers, so a run clears them again)."""
        if self.particles is None:
            return
        P, nan = self.particles, float('nan')
        for rows, value in ((self.p_lw, 0.0), (self.p_wn, 1.0 / P), (self.p_evidence, 0.0), (self.p_pending, 0.0),
                            (self.p_ess, float(P)), (self.p_flag, 0), (self.p_hist_anc, -1), (self.p_hist_wn, nan),
                            (self.p_hist_ess, nan)):
            rows.fill_(value)
        self.p_anc.copy_(torch.arange(self.M, dtype=torch.int32))

    def particle_results(self):
        """After a run: the final normalised weights (G, P), the log-evidence (G,) -- the resampled codes' increments plus the
        last weights' mx + log(s / P), which a final forced resampling has added already --, and the per-code histories."""
        G, P = self.M // self.particles, self.particles
        evidence = self.p_evidence if self.p_final else self.p_evidence + self.p_pending
        return {'weights': self.p_wn.view(G, P).clone(), 'log_evidence': evidence.clone(), 'ancestors': self.p_hist_anc,
                'wn': self.p_hist_wn, 'ess': self.p_hist_ess}

    # ---- one step ----------------------------------------------------------------------------------------------------
    def _ln(self, s, norm, out):
        hip.call('vqcpc_add_layernorm_fwd', s, self.d, None, norm.weight, norm.bias, out, self.mean, self.rstd, self.M, self.d,
                 1e-5, 0.0, 0)

    def _linear(self, x, w, b, out, res=None, relu=0):
        N, K = w.shape
        hip.call('vqcpc_decode_linear', x, x.shape[1], None, w, b, res, out.shape[1] if res is not None else 0, out,
                 out.shape[1], self.M, N, K, relu)

    def _no_cross(self, li, lay):
        """The step's cross hook of layer li: reads `h1`, returns the rows the FFN reads."""
        return self.h1

    def step(self):
        M, d, W, H, hd = self.M, self.d, self.W, self.H, self.hd
        cross = self._cross
        hin = self.x
        for li, lay in enumerate(self.layers):
            sa = lay.self_attn
            hout = self.hb[li % 2]
            self._linear(hin, sa.in_proj_weight, sa.in_proj_bias, self.qkv)
            q0 = self.qkv.data_ptr()
            slot = self._attn_slot.get(li)
            if slot is None:
                hip.call('vqcpc_decode_attn', self.qkv, 3 * d, self.kcache[li], self.vcache[li], d, q0 + 4 * d, q0 + 8 * d, 3 * d,
                         sa.attn_bias.e1, sa.attn_bias.e2, self.att, d, self.pos, M, W, 1, H, hd, ops.MASK_CAUSAL)
            else:                                         # a recorded layer: the same kernel body, which also stores its row
                hip.call('vqcpc_decode_attn_probs', self.qkv, 3 * d, self.kcache[li], self.vcache[li], d, q0 + 4 * d, q0 + 8 * d,
                         3 * d, sa.attn_bias.e1, sa.attn_bias.e2, self.att, d, self.pos, M, W, 1, H, hd, ops.MASK_CAUSAL,
                         self.self_probs[slot], W, self.frame.width, self.frame.win, self.frame.stride)
            self._linear(self.att, sa.out_proj.weight, sa.out_proj.bias, self.s, res=hin)
            self._ln(self.s, lay.norm1, self.h1)
            h = cross(self, li, lay)
            self._linear(h, lay.linear1.weight, lay.linear1.bias, self.f, relu=1)
            self._linear(self.f, lay.linear2.weight, lay.linear2.bias, self.s, res=h)
            self._ln(self.s, self.last_norms[li], hout)
            hin = hout
        self._linear(hin, self.head_w, self.head_b, self.logits)
        self._sample()

    # ---- the prefix of a moved window ----------------------------------------------------------------------------------
    def _prefix_ln(self, x, r, norm):
        y = torch.empty_like(x)
        n = x.shape[0]
        hip.call('vqcpc_add_layernorm_fwd', x, self.d, r, norm.weight, norm.bias, y, self._pmean[:n], self._prstd[:n], n, self.d,
                 1e-5, 0.0, 0)
        return y

    def _no_prefix_cross(self, li, lay, h1, att, P):
        """The prefix's cross hook of layer li on the (M * P, d) rows h1 (att: (M * P, d), free here): returns the rows the
        FFN reads."""
        return h1

    def _input_rows(self, idx):
        """The input rows of the table-row indices idx: a lookup in `table` (a subclass whose inputs are not one table overrides
        it)."""
        return ops.EmbeddingFn.apply(self.table, idx)

    def prefill_prefix(self, P):
        """The stack, teacher-forced over prefix rows [0, P) of every sequence (inputs: table rows `prefix_rows`): fills
        every layer's K/V cache rows [0, P)."""
        if P == 0:
            return
        M, d, W, H, hd = self.M, self.d, self.W, self.H, self.hd
        h = self._input_rows(self.prefix_rows[:M * P])                                # (M * P, d), row b * P + i
        last = len(self.layers) - 1
        for li, lay in enumerate(self.layers):
            sa = lay.self_attn
            qkv = ops.gemm_nt(h, sa.in_proj_weight, bias=sa.in_proj_bias)
            att = torch.empty(M * P, d, dtype=torch.float32, device=self.dev) if li < last else None
            hip.call('vqcpc_decode_prefill_attn', qkv, 3 * d, qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d, 3 * d,
                     self.kcache[li], self.vcache[li], d, sa.attn_bias.e1, sa.attn_bias.e2, att, d, M, P, W, 1, H, hd,
                     ops.MASK_CAUSAL)
            if li == last:
                break                                     # nothing reads the last layer's prefix outputs
            h1 = self._prefix_ln(h, ops.gemm_nt(att, sa.out_proj.weight, bias=sa.out_proj.bias), lay.norm1)
            h2 = self._prefix_cross(self, li, lay, h1, att, P)
            f = ops.gemm_nt(h2, lay.linear1.weight, bias=lay.linear1.bias, act=1)
            h = self._prefix_ln(h2, ops.gemm_nt(f, lay.linear2.weight, bias=lay.linear2.bias), self.last_norms[li])

    # ---- graphs --------------------------------------------------------------------------------------------------------
    def capture(self, fn):
        """fn's launches as a captured graph.  The caller has run them eagerly once already: first launches (module
        loading, workspace and buffer allocation) stay outside the capture."""
        torch.cuda.synchronize(self.dev)
        graph = torch.cuda.CUDAGraph()
        # no cyclic garbage collection while the stream captures: a collection that starts inside fn() runs the finalizers of
        # whatever dead cycles earlier generations left (graphs, events, tensors), and a runtime call of theirs that is not
        # allowed during a thread-local capture aborts the process.  The collector only waits: nothing is collected here.
        collecting = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                fn()
        finally:
            if collecting:
                gc.enable()
        return graph
