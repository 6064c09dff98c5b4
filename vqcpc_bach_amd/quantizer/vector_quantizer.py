"""ProductVectorQuantizer (reference: VQCPCB/quantizer/vector_quantizer.py:27-159).

Codebooks stay `nn.Parameter`s trained by Adam through the q_latent term (:44-48, :72-83) -- the reference has NO EMA
update; `EMAProductVectorQuantizer` below is this package's opt-in extension (quantizer_type 'ema').  Nearest-code search, straight-through output and loss are one kernel (vqcpc_vq_fwd) that never materialises
the (rows, K, D) difference tensor; the codebook gradient is a deterministic segment-sum (vqcpc_vq_bwd)."""
import torch
from torch import nn

from .. import ops


class VectorQuantizer(nn.Module):
    def __init__(self, **kwargs):
        super().__init__()

    def forward(self, inputs, **kwargs):
        raise NotImplementedError


class NoQuantization(VectorQuantizer):
    def __init__(self, codebook_dim):
        super().__init__()
        self.codebook_dim = codebook_dim

    def forward(self, inputs, **kwargs):
        return inputs, None, torch.zeros(inputs.shape[:-1], dtype=inputs.dtype, device=inputs.device)


class ProductVectorQuantizer(VectorQuantizer):
    def __init__(self, codebook_size, codebook_dim, commitment_cost, num_codebooks, use_batch_norm, initialize,
                 squared_l2_norm):
        super().__init__()
        if use_batch_norm:
            raise NotImplementedError('use_batch_norm=True is not used by any encoder config (SURVEY.md section 5): '
                                      'out of scope')
        self.num_codebooks = num_codebooks
        self.codebook_dim = codebook_dim
        self.codebook_size = codebook_size
        self._commitment_cost = commitment_cost
        assert self.codebook_dim % self.num_codebooks == 0
        self.embeddings = nn.ParameterList([
            nn.Parameter(torch.randn(self.codebook_size, self.codebook_dim // num_codebooks) * 4)
            for _ in range(num_codebooks)])
        self.initialize = initialize
        self.squared_l2_norm = squared_l2_norm
        self.use_batch_norm = use_batch_norm
        self.init_broadcast = None       # set by the DP helper: rank 0's data-initialised codebooks go to every rank

    def _initialize(self, flat_input):
        """First-call codebook init from a random permutation of the batch rows (:57-70)."""
        assert flat_input.size(-1) == self.codebook_dim
        assert flat_input.size(0) >= self.codebook_size, \
            'not enough elements in a batch to initialise the clusters. You need to increase the batch dimension.'
        with torch.no_grad():
            for k, embedding in enumerate(self.embeddings):
                # drawn from the global CPU generator like the reference's `torch.randperm(flat_input.size(0))` (:65),
                # so `torch.manual_seed(s)` before the first batch selects the same rows as it does there
                perm = torch.randperm(flat_input.size(0))[:embedding.size(0)].to(flat_input.device)
                dsub = embedding.size(1)
                embedding.copy_(flat_input[perm, k * dsub:(k + 1) * dsub])    # in place: parameters may be flat views
            if self.init_broadcast is not None:
                self.init_broadcast(list(self.embeddings))
        self.initialize = False

    def forward(self, inputs, corrupt_labels=False, init_rows=None, corrupt_rows=None, **kwargs):
        """inputs (..., codebook_dim) -> quantized_sg (..., D), encoding_indices (..., num_codebooks) int64,
        quantization_loss (...).  `init_rows` / `corrupt_rows` (slices over the flattened rows) restrict the data
        initialisation / label corruption to a sub-range when several encoder calls are merged into one."""
        shape = inputs.shape
        flat = inputs.reshape(-1, self.codebook_dim)
        if self.initialize:
            self._initialize(flat.detach()[init_rows] if init_rows is not None else flat.detach())
        codebooks = torch.stack(list(self.embeddings), dim=0)
        given = None
        if self.training and corrupt_labels:                                      # :119-132
            with torch.no_grad():
                idx = ops.vq_assign(flat.detach(), codebooks.detach())     # index-only search; the pass below is a lookup
                rnd = torch.randint_like(idx, low=0, high=self.codebook_size)
                keep = torch.rand(idx.shape, device=idx.device) > 0.05
                if corrupt_rows is not None:
                    only = torch.zeros(idx.shape[0], 1, dtype=torch.bool, device=idx.device)
                    only[corrupt_rows] = True
                    keep = keep | ~only
                given = torch.where(keep, idx, rnd)
        zq, idx, loss = ops.VQFn.apply(flat, codebooks, self._commitment_cost, self.squared_l2_norm, given)
        return zq.view(shape), idx.view(*shape[:-1], self.num_codebooks), loss.view(shape[:-1])


class EMAProductVectorQuantizer(VectorQuantizer):
    """Product quantiser whose codebooks follow exponential moving averages of the rows assigned to them (van den Oord et al.
    2017, appendix A.1) instead of a gradient: no counterpart in the reference, selected by quantizer_type 'ema'.

    Per codebook and training step, with n_k / s_k the count / sum of the rows whose nearest code is k (summed over ranks):
        N_k <- g N_k + h n_k ;  m_k <- g m_k + h s_k ;  T = sum_k N_k ;  Nt_k = (N_k + eps) / (T + K eps) * T ;  e_k <- m_k / Nt_k
    g = float32(decay), h = float32(1 - decay).  Initial state N = 1, m = e, so that e = m / Nt holds before the first update.
    The loss is the commitment term alone (beta * l), the output the straight-through z + (q - z).  `embeddings` (ncb, K, dsub),
    `ema_cluster_size` (ncb, K), `ema_sum` (ncb, K, dsub) and the per-step `stats` (ncb, K, 1 + dsub) are BUFFERS: they never
    enter the flat parameter / gradient buffers, Adam or the clip norm.  forward() in training mode (with gradients enabled)
    leaves the step's statistics in `stats`; `apply_update()` folds them in (the trainer calls it after Adam, after the
    statistics were sum-reduced over the ranks).

    Dead-code restarts (`restart_threshold`, default None = off; 0 is off too, a negative value raises ValueError): after the
    update every code whose N_k is below the threshold (strict, fp32) becomes a row of THIS step's quantiser input -- sub-vector
    c of the row a keyed hash of (restart_seed, step, c, k) names among the rows of all ranks -- with m_k = e_k and N_k = 1, the
    initial-state convention above.  N is an average of rows per step: with decay 0.99 a code that receives no row falls from 1
    to 0.5 in 69 steps (0.99^69 = 0.4998), one that receives a row per step stays near 1, so 0.5 reads "no row for about 70
    steps" and a restarted code gets the same 70 steps of grace.  A threshold of 1 or more restarts every code that misses a
    single step right after the initialisation: accepted, and almost never what is wanted.  Two dead codes may draw the same
    row; the later index then loses every tie, stays dead and draws again on a later step.  The option adds two non-persistent
    buffers (`restart_rows`, `restarts`: the per-codebook count since it was last zeroed) and two launches per step; the
    state_dict keys are the same with and without it."""

    def __init__(self, codebook_size, codebook_dim, commitment_cost, num_codebooks, initialize, squared_l2_norm, decay=0.99,
                 epsilon=1e-5, restart_threshold=None, restart_seed=0):
        super().__init__()
        assert codebook_dim % num_codebooks == 0
        assert 0.0 < decay < 1.0 and epsilon > 0.0
        restart_threshold = 0.0 if restart_threshold is None else float(restart_threshold)
        if not restart_threshold >= 0.0:
            raise ValueError(f'restart_threshold must be None or >= 0, got {restart_threshold}')
        self.restart_threshold, self.restart_seed = restart_threshold, int(restart_seed)
        self.num_codebooks = num_codebooks
        self.codebook_dim = codebook_dim
        self.codebook_size = codebook_size
        self._commitment_cost = commitment_cost
        self.decay, self.epsilon = float(decay), float(epsilon)
        dsub = codebook_dim // num_codebooks
        # iterating `embeddings` gives the (K, dsub) codebooks, as the ParameterList of ProductVectorQuantizer does
        self.register_buffer('embeddings', torch.randn(num_codebooks, codebook_size, dsub) * 4)
        self.register_buffer('ema_cluster_size', torch.ones(num_codebooks, codebook_size))
        self.register_buffer('ema_sum', self.embeddings.clone())
        self.register_buffer('stats', torch.zeros(num_codebooks, codebook_size, dsub + 1), persistent=False)
        self.initialize = initialize
        self.squared_l2_norm = squared_l2_norm
        self.use_batch_norm = False
        self.init_broadcast = None
        # (step, step_dev, rank, world) of the step being enqueued, set by the trainer (its optimiser owns the step count);
        # without one, a quantiser used on its own counts its own apply_update() calls and is the only rank
        self.restart_context = None
        self._updates = 0
        if self.restarting:
            self.register_buffer('restart_rows', torch.zeros(num_codebooks, codebook_size, dsub), persistent=False)
            self.register_buffer('restarts', torch.zeros(num_codebooks, dtype=torch.int32), persistent=False)

    @property
    def restarting(self):
        return self.restart_threshold > 0.0

    def ema_buffers(self):
        return [self.embeddings, self.ema_cluster_size, self.ema_sum]

    def reset_ema(self):
        """m <- e, N <- 1: the state in which e = m / Nt holds exactly (Nt = 1 when every N is 1)."""
        with torch.no_grad():
            self.ema_sum.copy_(self.embeddings)
            self.ema_cluster_size.fill_(1.0)

    def _initialize(self, flat_input):
        """First-call codebook init as ProductVectorQuantizer._initialize, then the EMA state restarts from it."""
        assert flat_input.size(-1) == self.codebook_dim
        assert flat_input.size(0) >= self.codebook_size, \
            'not enough elements in a batch to initialise the clusters. You need to increase the batch dimension.'
        with torch.no_grad():
            dsub = self.embeddings.size(2)
            for k in range(self.num_codebooks):
                perm = torch.randperm(flat_input.size(0))[:self.codebook_size].to(flat_input.device)
                self.embeddings[k].copy_(flat_input[perm, k * dsub:(k + 1) * dsub])
            if self.init_broadcast is not None:
                self.init_broadcast([self.embeddings])
        self.reset_ema()
        self.initialize = False

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """Also accepts a ProductVectorQuantizer checkpoint (keys `embeddings.<c>`): a codebook trained by Adam continues under
        EMA from m = e, N = 1."""
        keys = [f'{prefix}embeddings.{c}' for c in range(self.num_codebooks)]
        if f'{prefix}embeddings' not in state_dict and all(k in state_dict for k in keys):
            e = torch.stack([state_dict.pop(k) for k in keys], dim=0)
            state_dict[f'{prefix}embeddings'] = e
            state_dict[f'{prefix}ema_sum'] = e.clone()
            state_dict[f'{prefix}ema_cluster_size'] = torch.ones(e.shape[:2], dtype=e.dtype, device=e.device)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def apply_update(self):
        """Enqueues the EMA update on the statistics of the last training forward, then (restart_threshold > 0) the restart of
        the codes it left below the threshold from the candidates of that same forward."""
        ops.vq_ema_update(self.stats, self.ema_cluster_size, self.ema_sum, self.embeddings, self.decay, self.epsilon)
        if self.restarting:
            ops.vq_ema_restart(self.restart_rows, self.ema_cluster_size, self.ema_sum, self.embeddings, self.restart_threshold,
                               self.restarts)
            self._updates += 1

    def codebook_perplexity(self):
        """(ncb,) exp(-sum_k p_k log p_k) with p = N / sum N: the effective number of codes in use per codebook."""
        p = self.ema_cluster_size / self.ema_cluster_size.sum(-1, keepdim=True)
        return torch.exp(-(p * torch.log(p.clamp_min(torch.finfo(p.dtype).tiny))).sum(-1))

    def forward(self, inputs, corrupt_labels=False, init_rows=None, corrupt_rows=None, **kwargs):
        """As ProductVectorQuantizer.forward; the loss is commitment_cost * l.  In training mode with gradients enabled the
        step's statistics (always of the UNCORRUPTED nearest-code assignment) are left in `self.stats`."""
        shape = inputs.shape
        flat = inputs.reshape(-1, self.codebook_dim)
        if self.initialize:
            self._initialize(flat.detach()[init_rows] if init_rows is not None else flat.detach())
        given = nearest = None
        if self.training and corrupt_labels:
            with torch.no_grad():
                nearest = ops.vq_assign(flat.detach(), self.embeddings)
                rnd = torch.randint_like(nearest, low=0, high=self.codebook_size)
                keep = torch.rand(nearest.shape, device=nearest.device) > 0.05
                if corrupt_rows is not None:
                    only = torch.zeros(nearest.shape[0], 1, dtype=torch.bool, device=nearest.device)
                    only[corrupt_rows] = True
                    keep = keep | ~only
                given = torch.where(keep, nearest, rnd)
        stats = self.stats if (self.training and torch.is_grad_enabled()) else None
        restart = None
        if stats is not None and self.restarting:
            ctx = self.restart_context() if self.restart_context is not None else (self._updates + 1, None, 0, 1)
            restart = (self.restart_rows, self.restart_seed) + tuple(ctx)
        zq, idx, loss = ops.VQEmaFn.apply(flat, self.embeddings, self._commitment_cost, self.squared_l2_norm, given, stats,
                                          nearest, restart)
        return zq.view(shape), idx.view(*shape[:-1], self.num_codebooks), loss.view(shape[:-1])
