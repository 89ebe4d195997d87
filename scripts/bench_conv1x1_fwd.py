"""A/B of the weight-stationary streaming 1x1 forward (csrc/kernels/conv1x1_fwd.hip) against
the igemm path on the ResNet-50 conv3 shapes, statistics on: graph-timed interleaved rounds in
one process.  Every arm cycles through three sets of x / y buffers so that no call finds its
operands in the 256 MB last-level cache.  Prints one JSON line per shape.

    python scripts/bench_conv1x1_fwd.py [--batch 512] [--rounds 7] [--iters 12]
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, '.')
from mlcomp_amd.ops import functional as Fn  # noqa: E402

SHAPES = [(28, 128, 512), (14, 256, 1024)]   # H = W, Cin, Cout


def graph_of(fn, sets, iters):
    for s in sets:
        fn(*s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(iters):
            fn(*sets[i % len(sets)])
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=12)
    a = ap.parse_args()
    for H, Ci, Co in SHAPES:
        w = (torch.randn(Co, 1, 1, Ci, device='cuda') * Ci ** -0.5).to(torch.bfloat16)
        s1, s2 = Fn.stat_buffers(Co, 'cuda')
        sets = [(torch.randn(a.batch, H, H, Ci, device='cuda').to(torch.bfloat16),
                 torch.empty(a.batch, H, H, Co, device='cuda', dtype=torch.bfloat16)) for _ in range(3)]
        arms = {'igemm': lambda x, y: Fn.conv2d_fwd(x, w, 1, 0, stats=(s1, s2), out=y),
                'stream': lambda x, y: Fn.conv1x1_fwd(x, w, (s1, s2), out=y)}
        graphs = {k: graph_of(f, sets, a.iters) for k, f in arms.items()}
        us = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                s1.zero_()
                s2.zero_()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                g.replay()
                e.record()
                torch.cuda.synchronize()
                us[k].append(s.elapsed_time(e) * 1e3 / a.iters)
        rows = a.batch * H * H
        gb = rows * (Ci + Co) * 2 / 1e9
        out = {'shape': f'{a.batch}x{H}x{H} {Ci}>{Co}', 'rows': rows, 'MB': round(gb * 1e3, 1)}
        for k, v in us.items():
            med = statistics.median(v)
            out[k] = {'us_min': round(min(v), 1), 'us_median': round(med, 1), 'us_max': round(max(v), 1),
                      'GBps_median': round(gb / (med * 1e-6), 0)}
        out['stream_wins'] = out['stream']['us_median'] < out['igemm']['us_min']
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
