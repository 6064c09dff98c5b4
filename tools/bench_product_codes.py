"""What product codes cost and save downstream of the encoder (profiles/product_codes_perf_log.md): the decoder's
`source_embedding` and the prior's `code_model`, 'merged' against 'product'.

    python tools/bench_product_codes.py                         # everything below, one JSON line per section
    python tools/bench_product_codes.py --sections dec,kernels
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_product_codes.py --sections kernels --reps 5

Every comparison runs in ONE process, the arms in alternating windows between two device synchronisations (one warm-up of each arm
first); per arm the median, minimum and maximum over `--reps` windows are printed.  Wherever 'merged' is an arm it is there TWICE
('merged', 'merged_again': two identically built models): the difference between those two legs is the run-to-run spread a
difference between arms has to exceed, and the figure to hold against the parent commit's for the default paths.

  dec       DEC shape (configs.make_decoder_config) on a 2 x 512 encoder, source_embedding merged / product: the replayed training
            step at batch 32 under what train_model() selects, one cached generation step at 8 rows, parameter + optimiser bytes
  pri       PRI shape (configs.make_prior_config) on a 2 x 64 encoder (V = 4096, the largest the merged prior samples), code_model
            merged / product: the replayed training step at batch 32, codes / s of generate_codes (96 codes) at B = 1 / 8 / 32
  pri512    the same for 'product' alone on 2 x 512, which has no merged counterpart
  kernels   the new kernels alone: vqcpc_product_gather / _bwd at the DEC step's rows (768 x 512), one sampler stage at K = 512
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _window_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternating(arms, reps, per=1.0):
    """arms: {name: fn}.  One warm-up of each, then `reps` rounds of one window per arm in turn -> {name: median / min / max}."""
    for fn in arms.values():
        fn()
    samples = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            samples[k].append(_window_ms(fn) / per)
    return {k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in samples.items()}


def encoder_config(K, ncb):
    from vqcpc_bach_amd import configs
    enc = configs.make_decoder_config()['config_encoder']
    enc['quantizer_kwargs'].update(num_codebooks=ncb, codebook_size=K, codebook_dim=4 * ncb, initialize=False)
    return enc


def build_decoder(K, ncb, source_embedding, seed):
    from vqcpc_bach_amd import configs, getters
    torch.manual_seed(seed)
    config = configs.make_decoder_config(source_embedding=source_embedding, config_encoder=encoder_config(K, ncb))
    enc_cfg = config['config_encoder']
    dlg = getters.get_dataloader_generator(config['dataset'], config['training_method'],
                                           dict(config['dataloader_generator_kwargs'], seed=7, device='cuda'))
    enc_dlg = getters.get_dataloader_generator(enc_cfg['dataset'], enc_cfg['training_method'],
                                               dict(enc_cfg['dataloader_generator_kwargs'], seed=7, device='cuda'))
    encoder = getters.get_encoder('/tmp/vqcpc_bench_product', enc_dlg, enc_cfg)
    dp = getters.get_data_processor(dlg, config['data_processor_type'], config['data_processor_kwargs'])
    dec = getters.get_decoder('/tmp/vqcpc_bench_product', dlg, dp, encoder, config['decoder_type'], config['decoder_kwargs'])
    dec.cuda()
    dec.use_training_defaults()
    dec.init_optimizers(lr=config['lr'], schedule_lr=config['schedule_lr'])
    return dec, dlg.dataloaders(batch_size=config['batch_size'])[0]


def build_prior(K, ncb, code_model, seed):
    from vqcpc_bach_amd import configs, getters
    torch.manual_seed(seed)
    config = configs.make_prior_config(code_model=code_model, config_encoder=encoder_config(K, ncb))
    enc_cfg = config['config_encoder']
    dlg = getters.get_dataloader_generator(config['dataset'], config['training_method'],
                                           dict(config['dataloader_generator_kwargs'], seed=7, device='cuda'))
    enc_dlg = getters.get_dataloader_generator(enc_cfg['dataset'], enc_cfg['training_method'],
                                               dict(enc_cfg['dataloader_generator_kwargs'], seed=7, device='cuda'))
    encoder = getters.get_encoder('/tmp/vqcpc_bench_product', enc_dlg, enc_cfg)
    prior = getters.get_prior('/tmp/vqcpc_bench_product', dlg, encoder, config['prior_type'], config['prior_kwargs'])
    prior.cuda()
    prior.use_training_defaults()
    prior.init_optimizers(lr=config['lr'])
    return prior, dlg.dataloaders(batch_size=config['batch_size'])[0]


def train_arms(models, steps, warmup=6):
    """{name: (trainer, loader)} -> {name: fn running `steps` replayed training steps} (after eager steps, capture, replays)."""
    arms = {}
    for name, (tr, loader) in models.items():
        tr.train()
        tr.enable_step_graph(True)
        for _ in range(warmup):
            tr.train_step(next(loader), train=True)

        def fn(tr=tr, loader=loader):
            for _ in range(steps):
                tr.train_step(next(loader), train=True)
        arms[name] = fn
    return arms


def trainable_bytes(model):
    n = model.flat.numel
    return dict(parameters=4 * n, gradient=4 * n, adam_moments=8 * n, total=16 * n)


def section_dec(args):
    from vqcpc_bach_amd.decoders.generation import IncrementalDecoder
    from vqcpc_bach_amd.utils import STEP_LOCK
    models = {'merged': build_decoder(512, 2, None, 1), 'product': build_decoder(512, 2, 'product', 1),
              'merged_again': build_decoder(512, 2, None, 1)}
    out = {'section': 'dec', 'encoder': '2 x 512', 'bytes': {k: trainable_bytes(m) for k, (m, _) in models.items() if k != 'merged_again'}}
    out['train_step_replayed_ms'] = alternating(train_arms(models, args.steps), args.reps, per=args.steps)
    for m, _ in models.values():
        m.enable_step_graph(False)
        m.eval()
    B, arms = 8, {}
    with STEP_LOCK, torch.no_grad():
        for name, (dec, _) in models.items():
            inc = IncrementalDecoder(dec, B)
            codes = torch.randint(0, 512 ** 2, (B, dec.num_tokens_source), generator=torch.Generator().manual_seed(2)).cuda()
            inc.prefill(codes)
            inc.start(seeds=1)
            inc.step()
            graph = inc.capture(inc.step)

            def fn(inc=inc, graph=graph, T=dec.num_tokens_target):
                inc.pos.zero_()
                for _ in range(T):
                    graph.replay()
            arms[name] = fn
        T = models['merged'][0].num_tokens_target
        out['generation_step_replayed_us_8_rows'] = alternating(arms, args.reps, per=T / 1e3)
        # the source rows are looked up once per window: the prefill, where the two lookups differ
        pre = {}
        for name, (dec, _) in models.items():
            inc = IncrementalDecoder(dec, B)
            pre[name] = lambda inc=inc, codes=codes: [inc.prefill(codes) for _ in range(20)]
        out['prefill_ms_8_rows'] = alternating(pre, args.reps, per=20)
    return out


def _prior_section(tag, K, ncb, kinds, args):
    models = {name: build_prior(K, ncb, cm, 1) for name, cm in kinds.items()}
    out = {'section': tag, 'encoder': f'{ncb} x {K}', 'bytes': {k: trainable_bytes(m) for k, (m, _) in models.items() if k != 'merged_again'}}
    out['train_step_replayed_ms'] = alternating(train_arms(models, args.steps), args.reps, per=args.steps)
    for m, _ in models.values():
        m.enable_step_graph(False)
        m.eval()
    nt = 96
    for B in (1, 8, 32):
        ms = alternating({k: (lambda p=p, B=B: p.generate_codes(nt, num_generated_codes=B, seed=1)) for k, (p, _) in models.items()},
                         args.reps)
        out[f'generate_96_codes_B{B}'] = {k: dict(ms=v, codes_per_s=round(B * nt / v['median'] * 1e3)) for k, v in ms.items()}
    return out


def section_pri(args):
    return _prior_section('pri', 64, 2, {'merged': None, 'product': 'product', 'merged_again': None}, args)


def section_pri512(args):
    return _prior_section('pri512', 512, 2, {'product': 'product'}, args)


def section_kernels(args):
    from vqcpc_bach_amd import hip, ops
    hip.load()
    g = torch.Generator().manual_seed(0)
    ncb, K, C, M = 2, 512, 512, 768
    tables = torch.randn(ncb, K, C, generator=g).cuda().requires_grad_(True)
    merged = torch.randn(4096, C, generator=g).cuda().requires_grad_(True)       # as many rows as fit: timing does not depend on V
    idx = torch.randint(0, K ** ncb, (M,), generator=g).cuda()
    go = torch.randn(M, C, generator=g).cuda()
    R = 200

    def fwd_product():
        for _ in range(R):
            ops.ProductEmbeddingFn.apply(tables, None, idx)

    def fwd_merged():
        for _ in range(R):
            ops.EmbeddingFn.apply(merged, idx % 4096)

    def fb(fn_table, apply):
        def fn():
            for _ in range(R):
                fn_table.grad = None
                apply().backward(go)
        return fn
    out = {'section': 'kernels', 'rows': M, 'width': C, 'note': 'us per call, host launch path included (eager calls)'}
    out['gather_us'] = alternating({'product_gather': fwd_product, 'block_table_gather': fwd_merged}, args.reps, per=R / 1e3)
    out['gather_forward_backward_us'] = alternating(
        {'product': fb(tables, lambda: ops.ProductEmbeddingFn.apply(tables, None, idx)),
         'merged_4096_rows': fb(merged, lambda: ops.EmbeddingFn.apply(merged, idx % 4096))}, args.reps, per=R / 1e3)
    # one sampler stage at K = 512, 32 rows, against the merged sampler at V = 4096
    Mr, d, N = 32, 512, 24
    lg = torch.randn(2, Mr, 4096, generator=g).cuda()
    seeds = torch.arange(Mr, dtype=torch.int64).cuda()
    codes = torch.zeros(Mr, N, dtype=torch.int64).cuda()
    t2, dt = torch.randn(2, 512, d, generator=g).cuda(), torch.randn(1, 512, d, generator=g).cuda()
    tm = torch.randn(4097, d, generator=g).cuda()
    h, hn, x = (torch.randn(Mr, d, generator=g).cuda() for _ in range(3))
    pos, ticket = torch.zeros(1, dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    digits, acc = torch.zeros(Mr, 2, dtype=torch.int32).cuda(), torch.zeros(Mr).cuda()

    def product_tail():
        for _ in range(R):
            pos.zero_()
            hip.call('vqcpc_prior_sample_product', lg[0], 4096, 512, 2, 0, Mr, 1.0, 0, 1.0, seeds, None, N, None, N, None, N, None,
                     digits, acc, h, d, dt, hn, d, codes, N, N, t2, d, x, d, None, 512, pos, ticket)
            hip.call('vqcpc_prior_sample_product', lg[1], 4096, 512, 2, 1, Mr, 1.0, 0, 1.0, seeds, None, N, None, N, None, N, None,
                     digits, acc, None, d, None, None, d, codes, N, N, t2, d, x, d, None, 512, pos, ticket)

    def merged_tail():
        for _ in range(R):
            pos.zero_()
            hip.call('vqcpc_prior_sample', lg[0], 4096, 4096, Mr, 1.0, 0, 1.0, seeds, None, N, codes, N, N, tm, 4097, d, x, d, None,
                     4096, pos, ticket)
    out['sampler_us_32_rows'] = alternating({'two_stages_K512': product_tail, 'merged_V4096': merged_tail}, args.reps, per=R / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sections', default='dec,pri,pri512,kernels')
    ap.add_argument('--steps', type=int, default=20, help='training steps per window')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert args.reps >= 5, 'medians of at least 5 windows'
    assert torch.cuda.is_available(), 'bench_product_codes needs the GPU'
    out = []
    for name in args.sections.split(','):
        res = {'dec': section_dec, 'pri': section_pri, 'pri512': section_pri512, 'kernels': section_kernels}[name](args)
        out.append(res)
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
