"""LstmDownscaler (reference: VQCPCB/downscalers/lstm_downscaler.py:9-94): one or two independent GRU stacks over the tokens
of a block (the second reads the block flipped), last step of each, concatenation, output_linear.

`g_enc_fwd` / `g_enc_bwd` are kept as `torch.nn.GRU` parameter containers (the reference's state_dict keys and shapes); the
recurrences run on this library.  Hot path = forward_tokens(): the first layer's input is a per-voice embedding lookup with
no positional term (bach_cpc_data_processor.py:24-28), so its input projection is computed on the stacked embedding tables
(n_voices * vmax rows) and the step kernels look their rows up by token (ops.GRUTokLayerFn); the upper layers are
ops.GRULayerFn as in the context network."""
import torch
from torch import nn

from .. import ops
from ..utils import SEEDS
from .relative_transformer_downscaler import Downscaler


class LstmDownscaler(Downscaler):
    def __init__(self, input_dim, output_dim, num_channels, downscale_factors, hidden_size, num_layers, dropout, bidirectional):
        super().__init__(downscale_factors)
        assert len(downscale_factors) == 1
        self.output_dim = output_dim
        self.num_channels = num_channels
        self.sequence_length = int(downscale_factors[0])
        self.hidden_size = hidden_size
        self.num_layers = num_layers
        self.p = dropout
        self.g_enc_fwd = nn.GRU(input_size=input_dim, hidden_size=hidden_size, num_layers=num_layers, bias=True,
                                batch_first=True, dropout=dropout, bidirectional=False)
        if bidirectional:
            self.g_enc_bwd = nn.GRU(input_size=input_dim, hidden_size=hidden_size, num_layers=num_layers, bias=True,
                                    batch_first=True, dropout=dropout, bidirectional=False)
        else:
            self.g_enc_bwd = None
        self.output_linear = nn.Linear(hidden_size * (2 if bidirectional else 1), output_dim, bias=True)

    # use the first layer's gi table when tokens >= ratio * (n_voices * vmax) table rows; tests force either path (0 / inf)
    table_lookup_min_ratio = 4

    def _stacks(self):
        return [(self.g_enc_fwd, False)] + ([(self.g_enc_bwd, True)] if self.g_enc_bwd is not None else [])

    def _upper_layers(self, g, x, T, first):
        """Layers first .. num_layers - 1 of one stack on time-major rows x (T R, in) -> last step (R, H)."""
        p = self.p if self.training else 0.0
        for l in range(first, self.num_layers):
            last = l == self.num_layers - 1
            x = ops.GRULayerFn.apply(x, getattr(g, f'weight_ih_l{l}'), getattr(g, f'weight_hh_l{l}'),
                                     getattr(g, f'bias_ih_l{l}'), getattr(g, f'bias_hh_l{l}'), T, p,
                                     SEEDS.next() if (p > 0 and not last) else 0, last)
        return x

    def _head(self, lasts, lead):
        z_bi = torch.cat(lasts, dim=1) if len(lasts) > 1 else lasts[0]
        return ops.linear(z_bi, self.output_linear.weight, self.output_linear.bias).view(*lead, self.output_dim)

    # ---- hot path ---------------------------------------------------------------------------------------------
    def forward_tokens(self, tokens, data_processor):
        """tokens (..., num_blocks, sequence_length) int64 on the device -> (..., num_blocks, output_dim)."""
        lead = tokens.shape[:-1]
        L = self.sequence_length
        assert tokens.shape[-1] == L
        flat = tokens.reshape(-1, L).contiguous()
        tables = data_processor.stacked_tables()                                     # (nv, vmax, emb)
        nv, vmax = tables.shape[0], tables.shape[1]
        assert nv == self.num_channels
        if flat.numel() < self.table_lookup_min_ratio * nv * vmax:                  # tiny inputs: the plain projection
            x = data_processor.embed(flat)                                           # (R, L, emb)
            return self._from_embedded(x, lead)
        p = self.p if self.training else 0.0
        lasts = []
        for g, reverse in self._stacks():
            only = self.num_layers == 1
            gi_table = ops.linear(tables, g.weight_ih_l0, g.bias_ih_l0)              # (nv, vmax, 3H): lookup(E) W^T + b == lookup(E W^T + b)
            x = ops.GRUTokLayerFn.apply(flat, gi_table, g.weight_hh_l0, g.bias_hh_l0, L, reverse, p,
                                        SEEDS.next() if (p > 0 and not only) else 0, only)
            lasts.append(x if only else self._upper_layers(g, x, L, 1))
        return self._head(lasts, lead)

    # ---- API-compatible path ----------------------------------------------------------------------------------
    def _from_embedded(self, x, lead):
        """x (R, L, input_dim) -> (*lead, output_dim), every layer through ops.GRULayerFn."""
        R, L, dim = x.shape
        lasts = []
        for g, reverse in self._stacks():
            xs = x.flip(dims=[1]) if reverse else x
            rows = xs.transpose(0, 1).reshape(L * R, dim)                            # time-major rows
            lasts.append(self._upper_layers(g, rows, L, 0))
        return self._head(lasts, lead)

    def forward(self, embedded_seq):
        """(batch, seq_len, input_dim) embeddings -> (batch, seq_len // sequence_length, output_dim)."""
        batch_size, seq_len, dim = embedded_seq.shape
        L = self.sequence_length
        assert seq_len % L == 0
        return self._from_embedded(embedded_seq.reshape(batch_size * (seq_len // L), L, dim), (batch_size, seq_len // L))
