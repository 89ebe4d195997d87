"""ResNet-50 eval forward, four arms interleaved in one process (MI355X):

  a  NativeInference, folded units, HIP graph
  b  NativeInference, folded units, eager
  c  the existing unfolded native eval path (conv -> y, then bn_apply), eager
  d  TorchScript under bf16 autocast, channels-last (utils.torch_infer's path)

    python scripts/bench_native_infer.py --batch 256 --rounds 3 --iters 20 --out profiles/native_infer/b256.jsonl
    rocprofv3 --kernel-trace --stats -d out -- python scripts/bench_native_infer.py --batch 256 --arms a --rounds 1

Inputs are device-resident (NHWC bf16 for the native arms, fp32 channels-last for d), so no arm
pays a host copy.  Each round times ``iters`` calls of every arm between device synchronises;
images/s per round, the median and the spread (max - min) per arm go to stdout and ``--out``.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlcomp_amd.models import build_model  # noqa: E402
from mlcomp_amd.ops import functional as Fn  # noqa: E402
from mlcomp_amd.train.native_infer import NativeInference  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--arms', default='abcd')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda')
    torch.manual_seed(0)
    model = build_model('resnet50', num_classes=1000).eval()
    x = torch.randn(args.batch, 3, args.size, args.size, generator=torch.Generator().manual_seed(1))
    x_nhwc = Fn.nchw_to_nhwc(x.to(dev), pad_to=8)
    calls = {}
    if 'a' in args.arms:
        ea = NativeInference(model, args.batch, args.size, device=dev, use_graph=True)
        calls['a'] = lambda: ea.predict(x_nhwc)
    if 'b' in args.arms:
        eb = NativeInference(model, args.batch, args.size, device=dev, use_graph=False)
        calls['b'] = lambda: eb.predict(x_nhwc)
    if 'c' in args.arms:
        ec = NativeInference(model, args.batch, args.size, device=dev, use_graph=False)
        ec.net.ctx.deploy = False
        calls['c'] = lambda: ec.predict(x_nhwc)
    if 'd' in args.arms:
        gm = build_model('resnet50', num_classes=1000).eval()
        gm.load_state_dict(model.state_dict())
        gm = gm.to(dev)
        x_cl = x.to(dev).contiguous(memory_format=torch.channels_last)
        traced = torch.jit.trace(gm, x_cl[:2], check_trace=False)

        def arm_d():
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                return traced(x_cl).float()
        calls['d'] = arm_d
    for name, f in calls.items():              # warm-up: lazy init, graph capture, library tuning
        for _ in range(4):
            f()
    torch.cuda.synchronize()
    rates = {k: [] for k in calls}
    for _ in range(args.rounds):
        for name, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                f()
            torch.cuda.synchronize()
            rates[name].append(args.batch * args.iters / (time.perf_counter() - t0))
    lines = []
    for name, r in rates.items():
        s = sorted(r)
        lines.append({'arm': name, 'batch': args.batch, 'size': args.size, 'iters': args.iters,
                      'images_per_s': [round(v, 1) for v in r], 'median': round(s[len(s) // 2], 1),
                      'spread': round(s[-1] - s[0], 1)})
    if 'a' in rates and 'c' in rates:
        ma, mc = (sorted(rates[k])[len(rates[k]) // 2] for k in 'ac')
        sp = max(max(rates[k]) - min(rates[k]) for k in 'ac')
        lines.append({'a_minus_c': round(ma - mc, 1), 'three_spreads': round(3 * sp, 1),
                      'outside': abs(ma - mc) > 3 * sp})
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.writelines(json.dumps(ln) + '\n' for ln in lines)


if __name__ == '__main__':
    main()
