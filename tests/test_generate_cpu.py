"""CPU-side checks of decoder generation: the fixtures' internal consistency and the host-side argument validation of the
vqcpc_decode_* entry points (rejected before any HIP call, so no GPU is needed)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import load_golden


def test_filter_fixture_is_consistent():
    g = load_golden('generate_filter')
    logits, widths, keep = g['logits'], g['widths'], g['keep']
    assert keep.shape[:4] == (len(widths), len(g['top_k']), len(g['top_p']), len(g['temperature']))
    assert 11 <= widths.min() and widths.max() <= logits.shape[1]
    for r, V in enumerate(widths):
        assert len(np.unique(logits[r, :V])) == V                     # no ties
        assert not keep[r, ..., V:].any()
        sizes = keep[r, ..., :V].sum(axis=-1)                           # (top_k, top_p, temperature)
        assert (sizes >= 1).all()
        for a, k in enumerate(g['top_k']):
            if k > 0:
                assert (sizes[a] <= k).all()
            if k == 1:
                assert (sizes[a] == 1).all()
                assert keep[r, a, :, :, int(np.argmax(logits[r, :V]))].all()
        # top_k 0, top_p 1: everything, except tail tokens whose fp32 cumulative sum rounds above 1.0 in the reference
        # (the documented deviation: the kernels treat top_p >= 1 as "keep all"); those carry less than 1e-7
        for c, temp in enumerate(g['temperature']):
            dropped = ~keep[r, 0, -1, c, :V]
            if dropped.any():
                z = logits[r, :V].astype(np.float64) / temp
                pz = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
                assert pz[dropped].sum() < 1e-7
        assert (np.diff(sizes, axis=1) >= 0).all()                      # larger top_p keeps more
        for a in range(len(g['top_k'])):                                # kept entries are the largest logits
            for b in range(len(g['top_p'])):
                for c in range(len(g['temperature'])):
                    m = keep[r, a, b, c, :V]
                    assert logits[r, :V][m].min() > logits[r, :V][~m].max() if (~m).any() else True


def test_greedy_fixture_is_consistent():
    import json
    g = load_golden('generate_greedy_tiny')
    cfg = json.loads(str(g['cfg_json']))
    B, E, nc = g['tokens'].shape
    assert (B, E, nc) == (cfg['B'], cfg['events'], len(cfg['vocab']))
    assert g['codes'].shape == (B, E * nc // 16)
    for c, v in enumerate(cfg['vocab']):
        assert (g['tokens'][:, :, c] < v).all() and (g['tokens'] >= 0).all()
    assert g['gaps'].shape == (B, E * nc) and g['gaps'].min() > 1e-3


@pytest.fixture(scope='module')
def lib():
    import torch  # noqa: F401  (loads the process-wide libamdhip64.so.7 first)
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    return hip.load()


def test_decode_entry_points_reject_bad_arguments(lib):
    P, Q = 4096, 8192                     # 16-byte aligned stand-ins: nothing is dereferenced before the checks fail
    # decode_linear: M > 64
    rc = lib.vqcpc_decode_linear(P, 64, None, Q, None, None, 0, P + Q, 64, 65, 64, 64, 0, None)
    assert rc == -1 and b'decode_linear' in lib.vqcpc_last_error()
    rc = lib.vqcpc_decode_linear(P, 64, None, Q, None, None, 0, P + Q, 64, 8, 64, 6, 0, None)        # K % 4
    assert rc == -1 and b'decode_linear' in lib.vqcpc_last_error()
    # decode_attn: head dim 48, M > 64
    rc = lib.vqcpc_decode_attn(P, 96, P, P, 96, None, None, 0, Q, Q, P, 96, P, 2, 16, 1, 2, 48, 0, None)
    assert rc == -1 and b'hd' in lib.vqcpc_last_error()
    rc = lib.vqcpc_decode_attn(P, 128, P, P, 128, None, None, 0, Q, Q, P, 128, P, 65, 16, 1, 2, 64, 0, None)
    assert rc == -1 and b'decode_attn' in lib.vqcpc_last_error()
    # decode_sample: V_c > 256, M > 64
    offs = (ctypes.c_int32 * 3)(0, 40, 40 + 257)
    rc = lib.vqcpc_decode_sample(P, 297, offs, 2, 4, 1.0, 0, 1.0, None, Q, None, 0, P, 8, 8, Q, 257 * 16 + 1, 32, 16, P,
                                 32, None, 0, P, None)
    assert rc == -1 and b'256' in lib.vqcpc_last_error()
    offs = (ctypes.c_int32 * 2)(0, 40)
    rc = lib.vqcpc_decode_sample(P, 40, offs, 1, 65, 1.0, 0, 1.0, None, Q, None, 0, P, 8, 8, Q, 40 * 16 + 1, 32, 16, P,
                                 32, None, 0, P, None)
    assert rc == -1 and b'decode_sample' in lib.vqcpc_last_error()
    rc = lib.vqcpc_decode_sample(P, 40, offs, 1, 4, 0.0, 0, 1.0, None, Q, None, 0, P, 8, 8, Q, 40 * 16 + 1, 32, 16, P,
                                 32, None, 0, P, None)                                               # temperature 0
    assert rc == -1 and b'temperature' in lib.vqcpc_last_error()


def test_generation_host_helpers():
    import torch
    from vqcpc_bach_amd.decoders.generation import row_seeds
    a, b = row_seeds(5, 6), row_seeds(5, 6)
    assert torch.equal(a, b) and len(set(a.tolist())) == 6
    assert not torch.equal(a, row_seeds(6, 6))
    s = torch.tensor([1, 2, 3], dtype=torch.int64)
    assert torch.equal(row_seeds(s, 3), s)
    with pytest.raises(ValueError):
        row_seeds(s, 4)
