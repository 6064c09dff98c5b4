"""The GRU block downscaler at the SAMESEQ shape (configs.make_config('SAMESEQ'): embedding 32, hidden 512, 2 layers,
bidirectional, L = 16; 1 x 32 codes of dim 3): in ONE process, the legs of every comparison interleaved sample by sample,
  (a) ms of one VQCPCEncoderTrainer training step at --batch, eager and replayed from the step graph;
  (b) the first GRU layer of one stack, forward + backward, on R rows (R = the blocks of one step at --batch): by the gi table
      (ops.linear on the stacked tables + ops.GRUTokLayerFn) against the plain projection (embedding rows -> ops.GRULayerFn,
      existing code: the baseline), with the peak memory of each;
  (c) one step of the recurrence, forward (+ backward), over R in --rows: the fused vqcpc_gru_tok_step_* launch against
      vqcpc_gemm_nt + vqcpc_gru_tok_cell_* (the baseline).
Device-synchronised host clocks, a warm-up per leg, medians of --reps >= 5 samples; the relative spread (max - min) / median
of the samples is printed next to every median.  Prints one JSON object at the end (and writes it to --json).

    python tools/bench_lstm_downscaler.py [--batch 16] [--rows 256,1632,26112] [--reps 7] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _interleaved(legs, reps, inner):
    """legs: {name: fn}.  One warm-up each, then `reps` rounds in which every leg is timed once (`inner` calls per sample)."""
    samples = {k: [] for k in legs}
    for fn in legs.values():
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            samples[k].append((time.perf_counter() - t0) / inner * 1e3)
    return {k: dict(median_ms=statistics.median(v), spread=(max(v) - min(v)) / statistics.median(v)) for k, v in samples.items()}


def _peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bench_step(batch, reps):
    from vqcpc_bach_amd import configs, getters
    config = configs.make_config('SAMESEQ')
    dlg = getters.get_dataloader_generator('bach', 'vqcpc', dict(config['dataloader_generator_kwargs'], device='cuda'))
    enc = getters.get_encoder('/tmp/vqcpc_bench_lstm', dlg, config)
    tr = getters.get_encoder_trainer('/tmp/vqcpc_bench_lstm', dlg, 'vqcpc', enc, config['auxiliary_networks_kwargs'])
    tr.to('cuda')
    tr.init_optimizers(lr=config['lr'], schedule_lr=False)
    tr.use_training_defaults()
    tr.train()
    loader, _, _ = dlg.dataloaders(batch_size=batch)
    batches = [next(loader) for _ in range(4)]
    rows = sum(v.numel() // 16 for v in batches[0].values())
    out = {'batch': batch, 'blocks_per_step': rows}
    i = [0]

    def step():
        tr.train_step(batches[i[0] % len(batches)], train=True)
        i[0] += 1
    inner = 8
    for name, graph in (('eager', False), ('replayed', True)):
        tr.enable_step_graph(graph)
        for _ in range(tr.graph_warmup_steps + 2):
            step()
        out[name] = _interleaved({name: step}, reps, inner)[name]
        if graph:
            out['replays'] = tr._graph.replays if tr._graph is not None else 0
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    out['step_peak_allocated_mb'] = torch.cuda.max_memory_allocated() / 2 ** 20
    tr.enable_step_graph(False)
    return out


def bench_layer0(R, reps, H=512, emb=32, L=16, nv=4, vmax=57):
    from vqcpc_bach_amd import ops
    g = torch.Generator().manual_seed(R)
    tables = torch.randn(nv, vmax, emb, generator=g).cuda().requires_grad_(True)
    w_ih = (torch.randn(3 * H, emb, generator=g) / emb ** 0.5).cuda().requires_grad_(True)
    w_hh = (torch.randn(3 * H, H, generator=g) / H ** 0.5).cuda().requires_grad_(True)
    b_ih, b_hh = (torch.randn(3 * H, generator=g).cuda().requires_grad_(True) for _ in range(2))
    tokens = torch.randint(0, vmax - 1, (R, L), generator=g).cuda()
    cot = torch.randn(L * R, H, generator=g).cuda()
    voice = (torch.arange(L) % nv).cuda()

    def table():
        gi_table = ops.linear(tables, w_ih, b_ih)
        y = ops.GRUTokLayerFn.apply(tokens, gi_table, w_hh, b_hh, L, False, 0.1, 5, False)
        torch.autograd.grad((y * cot).sum(), [tables, w_ih, w_hh, b_ih, b_hh])

    def plain():
        x = tables[voice.unsqueeze(0).expand(R, L), tokens]                        # (R, L, emb): the embedding lookup
        rows = x.transpose(0, 1).reshape(L * R, emb)
        y = ops.GRULayerFn.apply(rows, w_ih, w_hh, b_ih, b_hh, L, 0.1, 5, False)
        torch.autograd.grad((y * cot).sum(), [tables, w_ih, w_hh, b_ih, b_hh])

    inner = 4 if R <= 4096 else 1
    res = _interleaved({'table': table, 'plain': plain}, reps, inner)
    res['table']['peak_mb'], res['plain']['peak_mb'] = _peak_mb(table), _peak_mb(plain)
    return dict(R=R, **res)


def bench_step_forms(R, reps, H=512, L=16, nv=4, vmax=57):
    """One recurrence step forward and one backward at R rows, the fused launch against gemm_nt + cell."""
    from vqcpc_bach_amd import hip, ops
    g = torch.Generator().manual_seed(R + 1)
    table = torch.randn(nv * vmax, 3 * H, generator=g).cuda()
    tokens = torch.randint(0, vmax, (R, L), generator=g).cuda()
    w = (torch.randn(3 * H, H, generator=g) / H ** 0.5).cuda()
    wt = w.t().contiguous()
    b = torch.randn(3 * H, generator=g).cuda()
    hp = torch.randn(R, H, generator=g).cuda()
    dgh_next = torch.randn(R, 3 * H, generator=g).cuda()
    d_y = torch.randn(R, H, generator=g).cuda()
    gh, h, y = torch.empty(R, 3 * H).cuda(), torch.empty(R, H).cuda(), torch.empty(R, H).cuda()
    dgi, dgh, dhp = torch.empty(R, 3 * H).cuda(), torch.empty(R, 3 * H).cuda(), torch.zeros(R, H).cuda()
    p = 5

    def fused_fwd():
        hip.call('vqcpc_gru_tok_step_fwd', table, tokens, L, p, nv, vmax, w, b, hp, gh, h, y, R, H, 0.1, 5, 0)

    def split_fwd():
        ops.gemm_nt(hp, w, bias=b, out=gh)
        hip.call('vqcpc_gru_tok_cell_fwd', table, tokens, L, p, nv, vmax, gh, hp, h, y, R, H, 0.1, 5, 0)

    def fused_bwd():
        hip.call('vqcpc_gru_tok_step_bwd', dgh_next, wt, dhp, table, tokens, L, p, nv, vmax, gh, hp, d_y, dgi, dgh, R, H, 0.1, 5, 0)

    def split_bwd():
        dh = ops.gemm_nt(dgh_next, wt, add=dhp)
        hip.call('vqcpc_gru_tok_cell_bwd', table, tokens, L, p, nv, vmax, gh, hp, d_y, dh, dgi, dgh, dhp, R, H, 0.1, 5, 0)

    split_fwd()
    inner = 64 if R <= 4096 else 16
    res = _interleaved({'fused_fwd': fused_fwd, 'split_fwd': split_fwd, 'fused_bwd': fused_bwd, 'split_bwd': split_bwd}, reps, inner)
    return dict(R=R, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--rows', default='256,1632,26112')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--gemm-mode', type=int, default=1)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert args.reps >= 5, 'medians of at least 5 samples'
    assert torch.cuda.is_available(), 'bench_lstm_downscaler needs the GPU'
    from vqcpc_bach_amd import hip, ops
    hip.load()
    hip.set_gemm_mode(args.gemm_mode)
    out = {'gemm_mode': args.gemm_mode, 'fused_max_rows': ops.GRU_TOK_FUSED_MAX_ROWS, 'step_forms': [], 'layer0': []}
    for R in [int(r) for r in args.rows.split(',') if r]:
        out['step_forms'].append(bench_step_forms(R, args.reps))
        print(json.dumps(out['step_forms'][-1]), flush=True)
    if not args.skip_step:
        out['step'] = bench_step(args.batch, args.reps)
        print(json.dumps(out['step']), flush=True)
        for R in sorted({out['step']['blocks_per_step'], 16 * 102 * args.batch // 16}):
            out['layer0'].append(bench_layer0(R, args.reps))
            print(json.dumps(out['layer0'][-1]), flush=True)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
