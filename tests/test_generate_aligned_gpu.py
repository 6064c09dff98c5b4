"""Generation with the aligned ('diagonal') decoder (decoders/generation.py: C = cross_attn(memory) per layer at prefill,
vqcpc_decode_aligned_add in the step, vqcpc_aligned_expand in the re-prefill) against
  (1) fixtures of the reference's own greedy generate loop and generate_from_code_long on the diagonal tiny decoder
      (tests/golden/generate_greedy_tiny_diagonal.npz, generate_long_tiny_S3_diagonal.npz),
  (2) the full forward of this package, at the criterion of tests/test_generate_gpu.py / test_generate_long_gpu.py:
      max |incremental logits - forward logits| < 1e-5 rms(forward logits),
  (3) row invariance."""
import json
import types

import pytest
import torch

from conftest import load_golden, sub_state
from oracle import decoder_oracle as D
from test_decoder_gpu import build_decoder, seeded_decoder
from test_generate_gpu import _golden_decoder, _random_inputs, _teacher_forced_error
from test_generate_long_gpu import _prefill_errors

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _decoder(name):
    if name == 'DEC':
        return seeded_decoder(D.make_cfg('DEC', B=2, cross_attn='diagonal'), 5)[0], 2      # d 512, 8 heads, 3 + 3 layers, T 384, S 24
    return _golden_decoder(name)[0], 3


def test_greedy_generation_equals_the_reference():
    g = load_golden('generate_greedy_tiny_diagonal')
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    assert cfg['cross_attn'] == 'diagonal'
    dec = build_decoder(cfg, sub_state(g, 'sd'))
    codes = T(g['codes']).cuda()
    for use_graph in (True, False):
        tokens = dec.generate_from_codes(codes, top_k=1, seed=0, use_graph=use_graph)
        assert torch.equal(tokens.cpu(), T(g['tokens'])), use_graph


def test_greedy_long_generation_equals_the_reference():
    g = load_golden('generate_long_tiny_S3_diagonal')
    cfg = D.make_cfg(**json.loads(str(g['cfg_json'])))
    assert cfg['cross_attn'] == 'diagonal'
    dec = build_decoder(cfg, sub_state(g, 'sd'))
    dec.dataloader_generator = types.SimpleNamespace(dataset=types.SimpleNamespace(
        note2index_dicts=[{'START': int(s), 'END': int(e), 'XX': int(p)} for s, e, p in zip(g['start'], g['end'], g['pad'])]))
    codes = T(g['codes']).cuda()
    for use_graph in (True, False):
        tokens = dec.generate_from_code_long(codes, temperature=1.0, top_k=1, num_decodings=int(g['num_decodings']),
                                             code_index_start=int(g['code_index_start']),
                                             code_index_end=int(g['code_index_end']), seed=0, use_graph=use_graph)
        assert torch.equal(tokens.cpu(), T(g['tokens'])), use_graph


@pytest.mark.parametrize('name', ['decoder_tiny_diagonal', 'DEC'])
def test_incremental_step_equals_full_forward(name):
    """Teacher-forced: the logits handed to the sampler at position t equal forward(codes, x)[t % nc][:, t // nc]."""
    dec, B = _decoder(name)
    assert dec.cross_attention_type == 'diagonal'
    err = _teacher_forced_error(dec, B, seed=11)
    print(f'{name} diagonal: max |incremental - forward| / rms = {err:.2e}')
    assert err < 1e-5, err


@pytest.mark.parametrize('name', ['decoder_tiny_diagonal', 'DEC'])
def test_reprefill_equals_full_forward(name):
    """After a re-prefill of P tokens (vqcpc_aligned_expand on P rows per sequence) every teacher-forced step's logits equal
    the full forward's and the K/V cache rows [0, P) equal those of P incremental steps, both within 1e-5 of their rms."""
    dec, B = _decoder(name)
    U, S, Tt = dec.total_upscaling, dec.num_tokens_source, dec.num_tokens_target
    for P in sorted({0, U, (S // 2) * U, Tt - U}) if name != 'DEC' else [(S // 2) * U]:
        err, cache = _prefill_errors(dec, B, P, seed=11 + P)
        print(f'{name} diagonal P = {P}: logits {err:.2e}, caches {cache:.2e} (relative to rms)')
        assert cache < 1e-5 and err < 1e-5, (P, err, cache)


def test_a_rows_tokens_do_not_depend_on_the_other_rows():
    dec, _ = _decoder('decoder_tiny_diagonal')
    codes, _ = _random_inputs(dec, 4, seed=21)
    seeds = torch.tensor([11, 22, 33, 44], dtype=torch.int64)
    four = dec.generate_from_codes(codes, seed=seeds)
    assert torch.equal(four, dec.generate_from_codes(codes, seed=seeds, use_graph=False))
    for r in (0, 2):
        assert torch.equal(four[r], dec.generate_from_codes(codes[r:r + 1], seed=seeds[r:r + 1])[0])
    pair = dec.generate_from_codes(codes[[3, 1]], seed=seeds[[3, 1]])
    assert torch.equal(pair[0], four[3]) and torch.equal(pair[1], four[1])
    nb = dec.num_tokens_source + 2
    g = torch.Generator().manual_seed(5)
    long_codes = torch.randint(0, dec.source_embeddings.weight.shape[0], (3, nb), generator=g).cuda()
    vocab = [int(v) for v in dec.num_tokens_per_channel]
    kw = dict(temperature=1.0, pad=[v - 1 for v in vocab], start=[v - 3 for v in vocab], code_index_start=1)
    three = dec.generate_from_code_long(long_codes, seed=seeds[:3], **kw)
    assert torch.equal(three[1], dec.generate_from_code_long(long_codes[1:2], seed=seeds[1:2], **kw)[0])
