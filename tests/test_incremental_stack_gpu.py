"""The launches of one incremental step (transformer/incremental.py: IncrementalStack.step with the decoder's and the
prior's hooks), recorded around `hip.call`: the launch counts the module docstrings state and "the prior's step is the
decoder's without the cross-attention" as a checked statement about the kernel-name sequence."""
import pytest
import torch

from test_generate_gpu import _golden_decoder, _random_inputs
from test_prior_gpu import _golden_prior

pytestmark = pytest.mark.gpu

SELF = ['vqcpc_decode_linear', 'vqcpc_decode_attn', 'vqcpc_decode_linear', 'vqcpc_add_layernorm_fwd']     # -> norm1
FFN = ['vqcpc_decode_linear', 'vqcpc_decode_linear', 'vqcpc_add_layernorm_fwd']                            # -> last norm
CROSS = {'full': ['vqcpc_decode_linear', 'vqcpc_decode_attn', 'vqcpc_decode_linear'], 'diagonal': ['vqcpc_decode_aligned_add']}


def _record_step(monkeypatch, inc):
    """Kernel names of ONE eager step(), in launch order; `hip.call` is restored afterwards."""
    from vqcpc_bach_amd import hip
    names, real = [], hip.call

    def recorder(name, *args):
        names.append(name)
        return real(name, *args)
    with monkeypatch.context() as m:
        m.setattr(hip, 'call', recorder)
        inc.step()
    torch.cuda.synchronize()
    assert hip.call is real
    return names


def _decoder_step(monkeypatch, name):
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    dec = _golden_decoder(name)[0].eval()
    with torch.no_grad():
        inc = IncrementalDecoder(dec, 2)
        inc.prefill(_random_inputs(dec, 2, seed=3)[0])
        inc.start(seeds=1)
        return _record_step(monkeypatch, inc), len(inc.layers)


def _prior_step(monkeypatch):
    from vqcpc_bach_amd.priors.generation import IncrementalPrior
    prior = _golden_prior('v32')[0].eval()
    with torch.no_grad():
        inc = IncrementalPrior(prior, 2)
        inc.start(prior.num_tokens, seeds=1)
        return _record_step(monkeypatch, inc), len(inc.layers)


def _layers(names, L):
    """The step's per-layer blocks and its tail (head + sampler)."""
    per = (len(names) - 2) // L
    assert len(names) == per * L + 2
    return [names[i * per:(i + 1) * per] for i in range(L)], names[L * per:]


@pytest.mark.parametrize('name, kind, per_layer', [('decoder_tiny', 'full', 11), ('decoder_tiny_diagonal', 'diagonal', 9)])
def test_decoder_step_launches(monkeypatch, name, kind, per_layer):
    names, L = _decoder_step(monkeypatch, name)
    assert len(names) == per_layer * L + 2, (len(names), L)
    blocks, tail = _layers(names, L)
    for block in blocks:
        assert block == SELF + CROSS[kind] + ['vqcpc_add_layernorm_fwd'] + FFN, block
    assert tail == ['vqcpc_decode_linear', 'vqcpc_decode_sample']


def test_prior_step_is_the_decoders_without_the_cross_block(monkeypatch):
    """The prior's kernel-name sequence equals the decoder's with the cross block removed, layer for layer: the cross
    launches and, of the decoder's three LayerNorms, the one that closes the cross block.  (The three LayerNorm launches
    share a name; dropping the one after the FFN instead would leave two LayerNorms back to back, which is not the
    prior's layer.)  What is left is a layer of two norms, the prior's norm2 standing where the decoder's third stands.
    Then the head and each model's own sampler."""
    names, L = _prior_step(monkeypatch)
    assert len(names) == 7 * L + 2, (len(names), L)
    assert names[-2:] == ['vqcpc_decode_linear', 'vqcpc_prior_sample']
    for dec_name, kind in (('decoder_tiny', 'full'), ('decoder_tiny_diagonal', 'diagonal')):
        dec_names, dec_L = _decoder_step(monkeypatch, dec_name)
        dec_blocks, dec_tail = _layers(dec_names, dec_L)
        n = len(CROSS[kind])
        assert dec_blocks[0][4:4 + n + 1] == CROSS[kind] + ['vqcpc_add_layernorm_fwd']
        without = dec_blocks[0][:4] + dec_blocks[0][4 + n + 1:]
        assert sum(k == 'vqcpc_add_layernorm_fwd' for k in without) == 2
        assert without * L + [dec_tail[0], 'vqcpc_prior_sample'] == names, (kind, without, names)
