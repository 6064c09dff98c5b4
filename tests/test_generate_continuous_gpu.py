"""Generation with the decoder on continuous latents (decoders/generation.py: vqcpc_decode_source_rows as the first launch of
the prefill and of every window move) against
  (1) fixtures of the reference's own greedy generate loop and generate_from_code_long on the diagonal tiny decoder with a
      NoQuantization encoder (tests/golden/generate_greedy_tiny_continuous_diagonal.npz,
      generate_long_tiny_S3_continuous_diagonal.npz; tools/gen_golden_decoder_continuous.py),
  (2) the full forward of this package, at the criterion of tests/test_generate_gpu.py:
      max |incremental logits - forward logits| < 1e-5 rms(forward logits)."""
import glob
import os
import types

import pytest
import torch

from continuous_helpers import golden_continuous_decoder, random_inputs, stub_dataset

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def test_greedy_generation_equals_the_reference():
    dec, cfg, g = golden_continuous_decoder('generate_greedy_tiny_continuous_diagonal')
    assert cfg['cross_attn'] == 'diagonal' and float(g['min_gap']) >= 1e-3
    z = T(g['codes']).cuda()
    for use_graph in (True, False):
        tokens = dec.generate_from_codes(z, top_k=1, seed=0, use_graph=use_graph)
        assert torch.equal(tokens.cpu(), T(g['tokens'])), use_graph
    assert torch.equal(dec.generate_from_codes(dec.encode(T(g['x'])), top_k=1, seed=0).cpu(), T(g['tokens']))


def test_greedy_long_generation_equals_the_reference():
    """use_graph True / False and captured / eager slides: the same tokens, the reference's."""
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    dec, cfg, g = golden_continuous_decoder('generate_long_tiny_S3_continuous_diagonal')
    assert cfg['cross_attn'] == 'diagonal' and float(g['min_gap']) >= 1e-3
    dec.dataloader_generator = stub_dataset(g)
    z = T(g['codes']).cuda()
    start, end = int(g['code_index_start']), int(g['code_index_end'])
    kw = dict(temperature=1.0, top_k=1, num_decodings=int(g['num_decodings']), code_index_start=start, code_index_end=end, seed=0)
    for use_graph in (True, False):
        tokens = dec.generate_from_code_long(z, use_graph=use_graph, **kw)
        assert torch.equal(tokens.cpu(), T(g['tokens'])), use_graph
    # the step captured, the slides eager -- and the reverse
    nb, U, nc, epc = z.shape[1], dec.total_upscaling, dec.num_channels, dec.num_events_per_code
    chorale = dec.init_generation_chorale(num_events=nb * epc, start_index=start * epc)
    dec.eval()
    for use_graph, graph_slides in ((True, False), (False, True)):
        with torch.no_grad():
            inc = IncrementalDecoder(dec, z.shape[0])
            inc.start_long(z, chorale.reshape(1, -1).expand(z.shape[0], -1), seeds=0, temperature=1.0, top_k=1)
            out = inc.run_long(start, end, use_graph=use_graph, graph_slides=graph_slides)
        out = out.view(z.shape[0], nb * epc, nc)[:, start * epc:end * epc]
        assert torch.equal(out.cpu(), T(g['tokens'])), (use_graph, graph_slides)


def test_alla_mano_takes_latent_parts():
    dec, cfg, g = golden_continuous_decoder('generate_long_tiny_S3_continuous_diagonal')
    dec.dataloader_generator = stub_dataset(g)
    z = T(g['codes'])[0]
    start, end = int(g['code_index_start']), int(g['code_index_end'])
    out = dec.generate_alla_mano(start_codes=z[:start], body_codes=z[start:end], end_codes=z[end:], temperature=1.0, top_k=1,
                                 num_decodings=1, seed=0)
    assert torch.equal(out.cpu()[0], T(g['tokens'])[0])


def _teacher_forced_error(dec, B, seed):
    """tests/test_generate_gpu.py:_teacher_forced_error on latents: max |incremental - forward| / rms(forward logits)."""
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.utils import flatten
    dec.eval()
    z, x = random_inputs(dec, B, seed)
    nc = dec.num_channels
    with torch.no_grad():
        full = dec.forward(z, x)['weights_per_category']
        inc = IncrementalDecoder(dec, B)
        inc.prefill(z)
        inc.start(teacher=flatten(x))
        worst = 0.0
        for t in range(dec.num_tokens_target):
            inc.step()
            c = t % nc
            worst = max(worst, float((inc.logits[:, inc.offsets[c]:inc.offsets[c + 1]] - full[c][:, t // nc]).abs().max()))
        rms = float(torch.cat([f.reshape(-1) for f in full]).pow(2).mean().sqrt())
        assert torch.equal(inc.tokens, flatten(x))
    return worst / rms


@pytest.mark.parametrize('name', ['decoder_tiny_continuous_diagonal', 'decoder_tiny_continuous'])
def test_incremental_step_equals_full_forward(name):
    """gemm mode 0.  Measured on the MI355X, max |difference| / rms(logits): 9.2e-7 (diagonal), 1.1e-6 ('transformer_relative')."""
    from vqcpc_bach_amd import hip
    hip.load()
    assert hip.get_gemm_mode() == 0
    dec, cfg, _ = golden_continuous_decoder(name)
    assert dec.cross_attention_type == ('diagonal' if name.endswith('diagonal') else 'anticausal')
    err = _teacher_forced_error(dec, 3, seed=11)
    print(f'{name}: max |incremental - forward| / rms = {err:.2e}')
    assert err < 1e-5, err


def test_a_rows_tokens_do_not_depend_on_the_other_rows():
    dec, _, _ = golden_continuous_decoder('decoder_tiny_continuous_diagonal')
    z, _ = random_inputs(dec, 4, seed=21)
    seeds = torch.tensor([11, 22, 33, 44], dtype=torch.int64)
    four = dec.generate_from_codes(z, seed=seeds)
    for r in (0, 2):
        assert torch.equal(four[r], dec.generate_from_codes(z[r:r + 1], seed=seeds[r:r + 1])[0])
    two = dec.generate_from_codes(z[:2], seed=seeds[:2].repeat_interleave(2), num_decodings=2)
    assert torch.equal(two[0], four[0]) and two.shape[0] == 4


def test_generate_returns_latents_and_writes_no_file(tmp_path):
    dec, cfg, g = golden_continuous_decoder('decoder_tiny_continuous_diagonal')
    x = T(g['batch/x'])[:1]

    class Stream:
        def dataloaders(self, batch_size, shuffle_val=False, **kw):
            return iter([{'x': x}]), iter([{'x': x}]), None

    dec.dataloader_generator = Stream()
    dec.model_dir = str(tmp_path)
    out = dec.generate(temperature=1.0, batch_size=2, top_k=1, seed_set='val', seed=0)
    assert out['recoding'] is None
    assert out['codes'].dtype == torch.float32 and tuple(out['codes'].shape) == (2, dec.num_tokens_source, dec.source_dim)
    assert torch.equal(out['codes'], dec.encode(x.repeat(2, 1, 1)))
    assert tuple(out['generation'].shape) == (2, cfg['events'], len(cfg['vocab']))
    assert not glob.glob(os.path.join(str(tmp_path), '**', '*.txt'), recursive=True)


def test_prior_on_a_continuous_encoder_still_raises():
    from vqcpc_bach_amd.priors.prior_relative import PriorRelative
    dec, _, _ = golden_continuous_decoder('decoder_tiny_continuous_diagonal')
    with pytest.raises(NotImplementedError, match='continuous'):
        PriorRelative(model_dir='/tmp/vqcpc_test_prior_continuous', dataloader_generator=None, encoder=dec.encoder, d_model=32,
                      num_layers=1, n_head=2, dim_feedforward=64, embedding_size=8, num_channels=1, num_events=3, dropout=0.0)
