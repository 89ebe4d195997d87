#!/usr/bin/env python
"""The video clip record pipeline on one GPU, one process.  Prints JSON lines.

  (a) ``kernel``   ``mlc_augment_clip`` alone on a resident uint8 batch, both layouts, at
                   16 clips x 8 frames of 128x171 -> 112x112 and 32 x 16 of 256x256 -> 224x224,
                   against what the tree could do before it: ``mlc_augment`` (nchw) over the
                   B*T frames, then a torch permute to contiguous NCTHW.  Device events around
                   ``--iters`` launches; the variants are interleaved, ``--rounds`` rounds.
  (b) ``loader``   the CUDA ClipRecordLoader alone (file of ``--records`` clips of
                   ``--stored-frames`` frames 128x171, clips of 8 frames -> 112x112), clips/s;
  (c) ``step``     the generic native engine's training step of ResNeXt3D-18 and R(2+1)D-18
                   at 16 x 8 x 112x112: fed from the clip file (``load_batch`` of the loader's
                   bf16 channels_last_3d batch, then the step) against the same step on its
                   resident batch, interleaved, ``--rounds`` rounds.

(b) and (c) follow bench.py's discipline: warm-up steps, a device synchronise, a host clock
around ``--steps`` steps that ends in a synchronise.  Run it under ``timeout``; it needs a
GPU and does not fall back.

  timeout -k 10 900 python scripts/bench_clip_records.py --out profiles/clip_records/bench_clip_records.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlcomp_amd.train.records import (CLIP_LAYOUTS, IMAGENET_MEAN, IMAGENET_STD, LAYOUTS,  # noqa: E402
                                      ClipRecordLoader, write_clip_records)

VIDEO = {   # scripts/bench_generic.py's configs of the reference's video models
    'r2plus1d_18': dict(residual_transformation_type='basic_r2plus1d_transformation', stem_name='r2plus1d_stem',
                        num_blocks=(2, 2, 2, 2), stage_planes=64, in_plane=512),
    'resnext3d_18': dict(residual_transformation_type='basic_transformation', num_blocks=(2, 2, 2, 2),
                         stage_planes=64, in_plane=512),
}
KERNEL_SHAPES = [(16, 8, 128, 171, 112), (32, 16, 256, 256, 224)]    # B, T, H, W, out


def endless(loader):
    while True:
        yield from loader


def timed(fn, warmup, steps, batch):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {'clips_per_s': round(batch * steps / dt, 1), 'ms_per_step': round(dt * 1000 / steps, 3)}


def device_us(fn, warmup, iters):
    """Mean device time of one fn() in microseconds: events around ``iters`` calls."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1000 / iters, 2)


def bench_kernel(args, emit):
    from mlcomp_amd.ops import _lib
    ms = [0.0] * 8
    for c in range(3):
        ms[c], ms[4 + c] = IMAGENET_MEAN[c] * 255.0, 1.0 / (IMAGENET_STD[c] * 255.0)
    dms = torch.tensor(ms, device='cuda')
    g = torch.Generator().manual_seed(0)
    for B, T, H, W, S in KERNEL_SHAPES:
        src = torch.randint(0, 256, (B, T, H, W, 3), dtype=torch.uint8, generator=g).cuda()
        box = torch.tensor([[H // 8, W // 8, (3 * H) // 4, (3 * W) // 4]]).repeat(B, 1)
        flip = (torch.arange(B) % 2)[:, None]
        par8 = torch.cat([box, flip, torch.zeros(B, 1, dtype=torch.long), torch.ones(B, 1, dtype=torch.long),
                          torch.zeros(B, 1, dtype=torch.long)], 1).int().cuda()
        par5 = par8[:, :5].repeat_interleave(T, dim=0).contiguous()
        out32 = torch.empty(B, 3, T, S, S, device='cuda')
        out16 = torch.empty(B, T, S, S, 3, dtype=torch.bfloat16, device='cuda')
        frames = torch.empty(B * T, 3, S, S, device='cuda')

        def clip(layout, out):
            _lib.call('mlc_augment_clip', _lib.ptr(src), _lib.ptr(par8), _lib.ptr(dms), _lib.ptr(out), B, T, H, W, 3,
                      S, S, CLIP_LAYOUTS[layout], _lib.stream())

        def baseline():
            _lib.call('mlc_augment', _lib.ptr(src), _lib.ptr(par5), _lib.ptr(dms), _lib.ptr(frames), B * T, H, W, 3,
                      S, S, LAYOUTS['nchw'], _lib.stream())
            out32.copy_(frames.view(B, T, 3, S, S).transpose(1, 2))
        variants = [('mlc_augment+permute', baseline), ('mlc_augment_clip ncthw', lambda: clip('ncthw', out32)),
                    ('mlc_augment_clip nthwc', lambda: clip('nthwc', out16))]
        # bytes the job needs at least: every source byte of the boxes once, every output element once
        src_bytes = B * T * ((3 * H) // 4) * ((3 * W) // 4) * 3
        for r in range(args.rounds):
            for name, fn in variants:
                us = device_us(fn, args.warmup, args.iters)
                out_bytes = B * T * S * S * 3 * (2 if name.endswith('nthwc') else 4)
                emit('kernel', variant=name, round=r, B=B, T=T, H=H, W=W, out=S, us=us,
                     min_gbytes_per_s=round((src_bytes + out_bytes) / us / 1e3, 1))


def clip_file(args):
    path = os.path.join(os.environ.get('TMPDIR', '/tmp'), f'mlc_bench_clip_{os.getpid()}.mlrec')
    rng = np.random.default_rng(0)
    write_clip_records(path, (rng.integers(0, 256, (args.stored_frames, 128, 171, 3), dtype=np.uint8)
                              for _ in range(args.records)), (i % 10 for i in range(args.records)))
    return path


def bench_loader(args, emit, path):
    for layout in ('nthwc', 'ncthw'):
        loader = ClipRecordLoader(path, args.batch, clip_len=args.frames, out_size=args.size, layout=layout,
                                  threads=args.threads, depth=4, device='cuda')
        feed = endless(loader)
        for r in range(args.rounds):
            emit('loader', layout=layout, threads=args.threads, round=r,
                 **timed(lambda: next(feed), args.warmup, args.steps, args.batch))
        feed.close()
        loader.close()


def bench_steps(args, emit, path):
    from mlcomp_amd.contrib.video import ResNeXt3D
    from mlcomp_amd.train.native_generic_step import NativeGenericStep
    for name in args.models.split(','):
        torch.manual_seed(0)
        loader = ClipRecordLoader(path, args.batch, clip_len=args.frames, out_size=args.size, layout='nthwc',
                                  threads=args.threads, depth=4, device='cuda')
        feed = endless(loader)
        first = next(feed)
        step = NativeGenericStep(ResNeXt3D(num_classes=10, **VIDEO[name]), first['features'], first['targets'],
                                 device='cuda', criterion=torch.nn.CrossEntropyLoss(), optimizer='SGD', lr=0.01,
                                 momentum=0.9, weight_decay=1e-4)

        def fed():
            bt = next(feed)
            step.load_batch(bt['features'], bt['targets'])
            step()

        def resident():
            step()
        for r in range(args.rounds):
            emit('step+records', model=name, round=r, **timed(fed, args.warmup, args.steps, args.batch))
            emit('step+resident', model=name, round=r, **timed(resident, args.warmup, args.steps, args.batch))
        feed.close()
        loader.close()
        del step


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parts', default='kernel,loader,step')
    p.add_argument('--models', default='resnext3d_18,r2plus1d_18')
    p.add_argument('--steps', type=int, default=60)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--iters', type=int, default=200, help='launches per kernel timing')
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--frames', type=int, default=8)
    p.add_argument('--size', type=int, default=112)
    p.add_argument('--stored-frames', type=int, default=16)
    p.add_argument('--records', type=int, default=256)
    p.add_argument('--threads', type=int, default=8)
    p.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = p.parse_args()
    if not torch.cuda.is_available():
        print('bench_clip_records: no GPU', file=sys.stderr)
        sys.exit(2)
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, 'a')

    def emit(what, **kw):
        line = json.dumps(dict({'what': what}, **kw))
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()
    parts = args.parts.split(',')
    if 'kernel' in parts:
        bench_kernel(args, emit)
    if 'loader' in parts or 'step' in parts:
        path = clip_file(args)
        try:
            if 'loader' in parts:
                bench_loader(args, emit, path)
            if 'step' in parts:
                bench_steps(args, emit, path)
        finally:
            os.remove(path)
    if out:
        out.close()


if __name__ == '__main__':
    main()
