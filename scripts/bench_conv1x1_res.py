"""A/B of the streaming 1x1 kernel's inference form (csrc/kernels/conv1x1_fwd.hip,
``Fn.conv1x1_fwd_res``) against the igemm path (``Fn.conv2d_fwd_res``) on the ResNet-50 conv3
shapes of layers 2 and 3, with bias, shortcut addend and ReLU: the timing method of
bench_conv1x1_fwd.py - graph-timed interleaved rounds in one process, every arm cycling through
three sets of x / addend buffers so that no call finds its operands in the 256 MB last-level
cache.  Prints one JSON line per (shape, batch); ``margin_over_3_spreads`` is the rule of
docs/kernels.md for a dispatch threshold: the streaming median below igemm's minimum by more than
three times the spread (max - min) of the igemm rounds.

    python scripts/bench_conv1x1_res.py [--batches 32,64,128,256] [--rounds 7] [--iters 12]
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, '.')
from mlcomp_amd.ops import functional as Fn  # noqa: E402
from bench_conv1x1_fwd import SHAPES, graph_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='32,64,128,256')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=12)
    a = ap.parse_args()
    for H, Ci, Co in SHAPES:
        w = (torch.randn(Co, 1, 1, Ci, device='cuda') * Ci ** -0.5).to(torch.bfloat16)
        b = torch.randn(Co, device='cuda')
        for B in [int(v) for v in a.batches.split(',')]:
            sets = [(torch.randn(B, H, H, Ci, device='cuda').to(torch.bfloat16),
                     torch.randn(B, H, H, Co, device='cuda').to(torch.bfloat16)) for _ in range(3)]
            arms = {'igemm': lambda x, r: Fn.conv2d_fwd_res(x, w, b, r, 3),
                    'stream': lambda x, r: Fn.conv1x1_fwd_res(x, w, b, r, 3)}
            graphs = {k: graph_of(f, sets, a.iters) for k, f in arms.items()}
            us = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, g in graphs.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    g.replay()
                    e.record()
                    torch.cuda.synchronize()
                    us[k].append(s.elapsed_time(e) * 1e3 / a.iters)
            rows = B * H * H
            gb = rows * (Ci + 2 * Co) * 2 / 1e9
            out = {'shape': f'{B}x{H}x{H} {Ci}>{Co}', 'rows': rows, 'MB': round(gb * 1e3, 1)}
            for k, v in us.items():
                med = statistics.median(v)
                out[k] = {'us_min': round(min(v), 1), 'us_median': round(med, 1), 'us_max': round(max(v), 1),
                          'GBps_median': round(gb / (med * 1e-6), 0)}
            spread = max(us['igemm']) - min(us['igemm'])
            margin = min(us['igemm']) - statistics.median(us['stream'])
            out['margin_us'] = round(margin, 1)
            out['igemm_spread_us'] = round(spread, 1)
            out['margin_over_3_spreads'] = margin > 3 * spread
            print(json.dumps(out), flush=True)
            del graphs, sets


if __name__ == '__main__':
    main()
