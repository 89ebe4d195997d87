#!/usr/bin/env python
"""The segmentation record pipeline against the U-Net step it feeds, on one GPU, one process.

Prints JSON lines (images/s, bench.py's discipline: warm-up steps, a device synchronise,
a host clock around ``--steps`` steps that ends in a synchronise):

  (a) ``loader``          the CUDA SegRecordLoader alone: batch 32, 256x256 crops of 288x288
                          records, s2d images + pixel-order masks, no model;
  (b) ``step+records``    the native U-Net / ResNet-34 step fed by (a) through
                          ``load_batch(..., pixel_order=True)``;
  (c) ``step+resident``   the same step on its resident synthetic batch, what
                          ``bench.py --model unet`` times;
  (d) ``step+dataloader`` the same step fed by a python ``DataLoader`` over the same file:
                          per-sample host transforms (crop, bilinear / nearest resize, flips,
                          normalise) to fp32 NCHW images and float masks, then today's
                          ``load_batch`` (nchw_to_nhwc, stem_s2d, mask permute).

(b) and (c) are interleaved, ``--pairs`` pairs, so drift of the machine shows in both.
Run it under ``timeout``; it needs a GPU and does not fall back.

  timeout -k 10 900 python scripts/bench_seg_records.py --out profiles/seg_records/bench_seg_records.jsonl
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlcomp_amd.train.records import (IMAGENET_MEAN, IMAGENET_STD, SegRecordFile, SegRecordLoader,  # noqa: E402
                                      write_seg_records)


class HostSegDataset(torch.utils.data.Dataset):
    """The python path: one record -> RandomResizedCrop(scale (0.5, 1), ratio (3/4, 4/3)) with
    bilinear / nearest resize, hflip / vflip / transpose coins, normalise; fp32 CHW + float mask."""

    def __init__(self, path, size):
        self.path, self.size, self.f = path, size, None
        self.n = len(SegRecordFile(path))
        self.mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1) * 255
        self.std = torch.tensor(IMAGENET_STD).view(3, 1, 1) * 255

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if self.f is None:
            self.f = SegRecordFile(self.path)
        H, W, _ = self.f.shape
        g = np.random.default_rng()
        a = H * W * g.uniform(0.5, 1.0)
        r = np.exp(g.uniform(np.log(3 / 4), np.log(4 / 3)))
        w, h = min(W, int(round(np.sqrt(a * r)))), min(H, int(round(np.sqrt(a / r))))
        y0, x0 = g.integers(0, H - h + 1), g.integers(0, W - w + 1)
        img = torch.from_numpy(self.f.image(i)[y0:y0 + h, x0:x0 + w].copy()).permute(2, 0, 1).float()[None]
        msk = torch.from_numpy(self.f.mask(i)[y0:y0 + h, x0:x0 + w].copy()).permute(2, 0, 1).float()[None]
        img = torch.nn.functional.interpolate(img, size=(self.size, self.size), mode='bilinear', align_corners=False)[0]
        msk = torch.nn.functional.interpolate(msk, size=(self.size, self.size), mode='nearest')[0]
        if g.integers(2):
            img, msk = img.flip(-1), msk.flip(-1)
        if g.integers(2):
            img, msk = img.flip(-2), msk.flip(-2)
        if g.integers(2):
            img, msk = img.transpose(-1, -2), msk.transpose(-1, -2)
        return {'features': ((img - self.mean) / self.std).contiguous(), 'targets': (msk != 0).float().contiguous()}


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
    return {'images_per_s': round(batch * steps / dt, 1), 'ms_per_step': round(dt * 1000 / steps, 3)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--steps', type=int, default=60)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--pairs', type=int, default=3)
    p.add_argument('--batch', type=int, default=32)
    p.add_argument('--size', type=int, default=256)
    p.add_argument('--stored', type=int, default=288)
    p.add_argument('--records', type=int, default=1024)
    p.add_argument('--threads', type=int, default=8)
    p.add_argument('--workers', type=int, default=8)
    p.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = p.parse_args()

    path = os.path.join(os.environ.get('TMPDIR', '/tmp'), f'mlc_bench_seg_{os.getpid()}.mlrec')
    rng = np.random.default_rng(0)

    def pairs():
        for _ in range(args.records):
            im = rng.integers(0, 256, (args.stored, args.stored, 3), dtype=np.uint8)
            yield im, (im[..., :1] > 127).astype(np.uint8)
    a, b = itertools.tee(pairs())
    write_seg_records(path, (q[0] for q in a), (q[1] for q in b))

    # the DataLoader's worker processes start before this process touches the GPU
    dl = torch.utils.data.DataLoader(HostSegDataset(path, args.size), batch_size=args.batch, shuffle=True,
                                     num_workers=args.workers, drop_last=True, pin_memory=True,
                                     persistent_workers=True, prefetch_factor=4)
    host_feed = endless(dl)
    first_host = next(host_feed)

    if not torch.cuda.is_available():
        print('bench_seg_records: no GPU', file=sys.stderr)
        del host_feed, dl
        os.remove(path)
        sys.exit(2)
    from mlcomp_amd.train.native_seg_step import NativeSegmentationStep
    lines = []

    def emit(what, **kw):
        line = dict({'what': what, 'batch': args.batch, 'size': args.size, 'stored': args.stored,
                     'steps': args.steps, 'warmup': args.warmup}, **kw)
        lines.append(line)
        print(json.dumps(line), flush=True)

    step = NativeSegmentationStep('resnet34', batch=args.batch, image_size=args.size, classes=1, use_graph=True)
    layout = 's2d' if step.x.shape[-1] == 16 else 'nhwc8'
    loader = SegRecordLoader(path, args.batch, out_size=args.size, layout=layout, mask_order='pixel',
                             threads=args.threads, depth=4, device='cuda')
    feed = endless(loader)
    synth_x, synth_t = step.x.clone(), step.t.clone()

    emit('loader', layout=layout, threads=args.threads, **timed(lambda: next(feed), args.warmup, args.steps, args.batch))

    def fed():
        bt = next(feed)
        step.load_batch(bt['features'], bt['targets'], pixel_order=True)
        step()

    def resident():
        step()

    for i in range(args.pairs):
        emit('step+records', pair=i, **timed(fed, args.warmup, args.steps, args.batch))
        step.x.copy_(synth_x)
        step.t.copy_(synth_t)
        emit('step+resident', pair=i, **timed(resident, args.warmup, args.steps, args.batch))

    pending = [first_host]

    def host_fed():
        bt = pending.pop() if pending else next(host_feed)
        step.load_batch(bt['features'], bt['targets'])
        step()
    emit('step+dataloader', workers=args.workers, **timed(host_fed, args.warmup, args.steps, args.batch))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')
    feed.close()          # hands its slot back before the loader goes
    loader.close()
    del host_feed, dl
    os.remove(path)


if __name__ == '__main__':
    main()
