"""Weight-gradient (TN) GEMM at the C1 step's shapes in the bf16x6 mode (the 256-tile ping-pong kernel).    python tools/bench_tn.py"""
import os, sys, statistics, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from vqcpc_bach_amd import hip, ops
hip.load()
for M, N, K in [(557056, 1024, 256), (557056, 256, 1024), (557056, 512, 256), (557056, 256, 256), (139264, 1024, 256),
                (139264, 256, 1024), (139264, 768, 256), (139264, 256, 256), (34816, 1024, 256)]:
    a = torch.randn(M, N, device='cuda'); b = torch.randn(M, K, device='cuda')
    hip.set_gemm_mode(1)
    ts = []
    for r in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            dw, db = ops.gemm_tn(a, b)
        e1.record(); torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1) / 10 * 1e3)
    t = statistics.median(ts)
    print(f'M={M} N={N} K={K}: {t:.1f} us ({2.0*M*N*K/t/1e6:.0f} TFLOP/s incl. reduction)', flush=True)
hip.set_gemm_mode(0)
