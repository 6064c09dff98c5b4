"""Embedding of the merged codes of a product quantiser as a sum of per-codebook rows (this package's extension: the reference
embeds the merged code as one symbol of a vocabulary of K**ncb, decoders/decoder.py:230, priors/prior_relative.py:61).

A merged code is `sum_j c_j * K**j` (Encoder.merge_codes); its embedding is `weight[0][c_0] + ... + weight[ncb-1][c_{ncb-1}]`,
added left to right in fp32 (ops.ProductEmbeddingFn, vqcpc_product_gather).  ncb * K rows instead of K**ncb: a code that never
occurred in training is decoded from rows that did, and the table, its gradient and both Adam moments shrink by K**(ncb-1) / ncb.
"""
import torch
from torch import nn

from .. import ops


class ProductEmbedding(nn.Module):
    def __init__(self, num_codebooks, codebook_size, dim):
        super().__init__()
        ops.check_product_shape(num_codebooks, codebook_size)
        if dim < 1:
            raise ValueError(f'ProductEmbedding: rows of {dim} floats')
        self.num_codebooks, self.codebook_size, self.dim = int(num_codebooks), int(codebook_size), int(dim)
        # the sum of ncb rows has the unit variance of an nn.Embedding row
        self.weight = nn.Parameter(torch.randn(self.num_codebooks, self.codebook_size, self.dim) / self.num_codebooks ** 0.5)

    @property
    def num_codes(self):
        return self.codebook_size ** self.num_codebooks

    def forward(self, codes, nj=None, res=None):
        """codes (...) merged int64 < K**ncb -> (codes.numel(), dim) rows: the sum of the first nj (default: all) digits' rows,
        on top of res (codes.numel(), dim) when given.  dim must be a multiple of 4 here (ValueError otherwise); a module that
        only holds rows for a projection, as the prior's `embedding`, may have any dim."""
        return ops.ProductEmbeddingFn.apply(self.weight, None, codes.reshape(-1), nj, res)

    @torch.no_grad()
    def merged_table(self):
        """The (K**ncb, dim) table of all sums, bit for bit what `forward` returns for every code: for tests and for exporting to
        a merged-format model.  Small K**ncb only (it allocates the table this module exists to avoid)."""
        return self.forward(torch.arange(self.num_codes, device=self.weight.device))

    def extra_repr(self):
        return f'{self.num_codebooks} x {self.codebook_size}, dim {self.dim}'
