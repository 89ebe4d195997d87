"""Video clip record files on the CPU (`mlcomp_amd/train/records.py`,
`csrc/runtime/records.cpp`): the ``MLVID001`` format next to the two image formats, which
frames of a record reach a slot, the first-frame draw, the box and flip shared with the image
loader, the thread-count independent stream, sharding, the PyTorch twin of
``mlc_augment_clip``, the CPU loader, the runner, the packing CLI and the sanitizer
self-tests of the new C entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from mlcomp_amd.train.records import (ClipRecordFile, ClipRecordLoader, RecordFile, RecordLoader, SegRecordFile,
                                      SegRecordLoader, augment_clip_reference, augment_reference, runtime,
                                      write_clip_records, write_records, write_seg_records)

MS = [123.7, 116.3, 103.5, 0.0, 1 / 58.4, 1 / 57.1, 1 / 57.4, 0.0]
RAW = dict(mean=(0, 0, 0), std=(1 / 255,) * 3)      # features are the interpolated bytes


def _coded_clips(n, F, H, W, Cc):
    """Clips whose every byte tells its record and frame: channel 0 is the record index,
    every other channel (channel 0 too for C = 1: 16*record + frame) the frame index."""
    a = np.zeros((n, F, H, W, Cc), np.uint8)
    rec, fr = np.arange(n)[:, None, None, None], np.arange(F)[None, :, None, None]
    if Cc == 1:
        a[..., 0] = rec * 16 + fr
    else:
        a[..., 0] = rec
        a[..., 1:] = fr[..., None]
    return a


def _clip_file(tmp_path, n=24, F=7, H=20, W=28, Cc=3, name='v.mlrec', random=False, seed=0):
    if random:
        clips = np.random.default_rng(seed).integers(0, 256, (n, F, H, W, Cc), dtype=np.uint8)
    else:
        clips = _coded_clips(n, F, H, W, Cc)
    path = str(tmp_path / name)
    assert write_clip_records(path, clips, [100 + i for i in range(n)]) == n
    return path, clips


def _slots(loader):
    """(batches, [(frames, labels, params) of every batch as the C++ workers filled the slot])
    of the next epoch; see test_seg_records_cpu._params for why the slot is still intact."""
    seen = []
    orig = loader._augment_cpu

    def spy(slot):
        seen.append(tuple(t.clone() for t in slot))
        return orig(slot)
    loader._augment_cpu = spy
    try:
        batches = list(loader)
    finally:
        loader._augment_cpu = orig
    return batches, seen


# ------------------------------------------------------------------------- 1. format
@pytest.mark.parametrize('Cc', [1, 3])
@pytest.mark.parametrize('F', [1, 5])
def test_clip_round_trip(tmp_path, Cc, F):
    path, clips = _clip_file(tmp_path, n=6, F=F, H=10, W=12, Cc=Cc, random=True)
    assert not os.path.exists(path + '.tmp')
    f = ClipRecordFile(path)
    assert len(f) == 6 and f.shape == (10, 12, Cc) and f.frames == F
    for i in (0, 3, 5):
        assert f.clip(i).shape == (F, 10, 12, Cc) and np.array_equal(f.clip(i), clips[i]) and f.label(i) == 100 + i
    rt = runtime()
    h = rt.mlr_clip_open(path.encode())
    assert h
    shp = (C.c_uint64 * 5)()
    rt.mlr_clip_shape(h, shp)
    rt.mlr_close(h)
    assert [int(v) for v in shp] == [6, 10, 12, Cc, F]


def test_partial_write_is_cleaned_up_and_bad_shapes_are_refused(tmp_path):
    out = str(tmp_path / 'b.mlrec')
    good = np.zeros((3, 6, 7, 3), np.uint8)

    def broken():
        yield good
        raise RuntimeError('decoder died')
    with pytest.raises(RuntimeError):
        write_clip_records(out, broken(), [0, 1])
    assert not os.path.exists(out) and not os.path.exists(out + '.tmp')
    for clips in ([good, np.zeros((4, 6, 7, 3), np.uint8)],      # another frame count
                  [good, np.zeros((3, 6, 8, 3), np.uint8)],      # another width
                  [np.zeros((3, 6, 7, 5), np.uint8)],            # five channels
                  [np.zeros((6, 7, 3), np.uint8)],               # an image, not a clip
                  []):                                           # nothing
        with pytest.raises(ValueError):
            write_clip_records(out, clips, [0, 1])
        assert not os.path.exists(out) and not os.path.exists(out + '.tmp')
    with pytest.raises(ValueError):                              # fewer labels than clips
        write_clip_records(out, [good, good], [0])
    assert not os.path.exists(out) and not os.path.exists(out + '.tmp')


def test_each_of_the_three_readers_refuses_the_other_two_kinds(tmp_path):
    """One image shape for all three, a one-frame clip (record = image + label, the size of a
    classification record) and a mask the size of a label: only the header tells them apart."""
    rng = np.random.default_rng(2)
    imgs = rng.integers(0, 256, (4, 2, 2, 3), dtype=np.uint8)
    cls, seg, vid = (str(tmp_path / n) for n in ('c.mlrec', 's.mlrec', 'v.mlrec'))
    write_records(cls, imgs, list(range(4)))
    write_seg_records(seg, imgs, np.ones((4, 2, 2, 1), np.uint8))
    write_clip_records(vid, imgs[:, None], list(range(4)))
    assert os.path.getsize(cls) == os.path.getsize(seg) == os.path.getsize(vid)
    readers = {cls: (RecordFile, lambda p: RecordLoader(p, 2, out_size=2, device='cpu', layout='nchw')),
               seg: (SegRecordFile, lambda p: SegRecordLoader(p, 2, out_size=2, device='cpu')),
               vid: (ClipRecordFile, lambda p: ClipRecordLoader(p, 2, clip_len=1, out_size=2, device='cpu'))}
    rt = runtime()
    opens = {cls: rt.mlr_open, seg: rt.mlr_seg_open, vid: rt.mlr_clip_open}
    for path in readers:
        for other, (view, loader) in readers.items():
            if other == path:
                assert len(view(path)) == 4 and len(loader(path)) == 2
                h = opens[other](path.encode())
                assert h
                rt.mlr_close(h)
                continue
            with pytest.raises(ValueError):
                view(path)
            with pytest.raises(ValueError):
                loader(path)
            assert not opens[other](path.encode())


# ------------------------------------------------------------------------- 2. draws
F, T, S = 7, 3, 2          # span 5: t0 in {0, 1, 2}
SEED = 3


def _frames_in(slot_img, Cc=3):
    """(record, frame) of every [b, k] frame of a slot's image buffer, from the coded bytes."""
    if Cc == 1:
        v = slot_img[:, :, 0, 0, 0].long()
        return v // 16, v % 16
    return slot_img[:, :, 0, 0, 0].long(), slot_img[:, :, 0, 0, 1].long()


@pytest.mark.parametrize('Cc', [1, 3])
def test_train_slots_hold_exactly_the_frames_t0_plus_k_stride(tmp_path, Cc):
    n = 12 if Cc == 1 else 24          # 16*record + frame has to fit a byte
    path, clips = _clip_file(tmp_path, n=n, Cc=Cc)
    L = ClipRecordLoader(path, 4, clip_len=T, frame_stride=S, out_size=16, device='cpu', seed=SEED, **RAW)
    t0s = set()
    for epoch in range(4):
        batches, slots = _slots(L)
        assert len(batches) == n // 4
        recs = []
        for b, (img, lab, par) in zip(batches, slots):
            assert img.shape == (4, T, 20, 28, Cc) and par.shape == (4, 8) and par.dtype == torch.int32
            rec, fr = _frames_in(img, Cc)
            t0 = par[:, 5].long()
            assert bool(((t0 >= 0) & (t0 <= F - ((T - 1) * S + 1))).all())
            assert torch.equal(par[:, 6], torch.full((4,), S, dtype=torch.int32)) and not par[:, 7].any()
            assert torch.equal(fr, t0[:, None] + S * torch.arange(T)[None, :])
            assert torch.equal(rec, rec[:, :1].expand(4, T))
            assert torch.equal(lab, 100 + rec[:, 0]) and torch.equal(b['targets'], lab)
            assert b['targets'].dtype == torch.int64 and b['targets'].shape == (4,)
            # the whole frame was copied, not only its first pixel
            for i in range(4):
                for k in range(T):
                    assert np.array_equal(img[i, k].numpy(), clips[int(rec[i, 0]), int(fr[i, k])])
            # the box lies in the image and every frame of a clip got the same one: constant frames
            # come out constant, with the frame index in channel 1
            assert bool((par[:, 0] >= 0).all() and (par[:, 0] + par[:, 2] <= 20).all())
            assert bool((par[:, 1] >= 0).all() and (par[:, 1] + par[:, 3] <= 28).all())
            if Cc == 3:
                assert torch.equal(b['features'][:, 1, :, 0, 0].round().long(), fr)
            t0s |= set(t0.tolist())
            recs += rec[:, 0].tolist()
        assert sorted(recs) == list(range(n))           # an epoch is a permutation of the file
    assert t0s == {0, 1, 2}                             # both extremes of t0 occur


def test_eval_takes_the_centre_frames_and_the_centre_crop_in_file_order(tmp_path):
    path, _ = _clip_file(tmp_path)
    L = ClipRecordLoader(path, 4, clip_len=T, frame_stride=S, out_size=(16, 18), train=False, device='cpu', **RAW)
    batches, slots = _slots(L)
    assert len(batches) == 6
    for k, (b, (img, lab, par)) in enumerate(zip(batches, slots)):
        assert par.tolist() == [[2, 5, 16, 18, 0, 1, S, 0]] * 4         # t0 = (7 - 5) // 2
        rec, fr = _frames_in(img)
        assert rec[:, 0].tolist() == [4 * k + i for i in range(4)] and fr.tolist() == [[1, 3, 5]] * 4
        assert b['features'].shape == (4, 3, T, 16, 18) and b['targets'].tolist() == [100 + 4 * k + i for i in range(4)]


@pytest.mark.parametrize('scale,ratio', [((0.3, 1.0), (3 / 4, 4 / 3)), ((0.08, 0.5), (0.5, 2.0))])
def test_box_and_flip_are_the_image_loader_draws(tmp_path, scale, ratio):
    """Same (seed, epoch, sample, scale, ratio, H, W): par[:, :5] is what RecordLoader draws.
    Both loaders shuffle with the same epoch RNG, so batch k holds the same sample indices."""
    path, _ = _clip_file(tmp_path)
    ipath = str(tmp_path / 'i.mlrec')
    write_records(ipath, np.zeros((24, 20, 28, 3), np.uint8), [100 + i for i in range(24)])
    kw = dict(out_size=16, device='cpu', seed=11, scale=scale, ratio=ratio, threads=2)
    a = ClipRecordLoader(path, 8, clip_len=T, frame_stride=S, **kw)
    b = RecordLoader(ipath, 8, layout='nchw', **kw)
    for epoch in (0, 1, 5):
        a.set_epoch(epoch)
        b.set_epoch(epoch)
        (_, sa), (_, sb) = _slots(a), _slots(b)
        assert len(sa) == len(sb) == 3
        for (_, la, pa), (_, lb, pb) in zip(sa, sb):
            assert torch.equal(la, lb)                  # the same samples ...
            assert pb.shape == (8, 5) and torch.equal(pa[:, :5], pb)   # ... the same box and flip
    assert len({tuple(p) for _, _, pa in sa for p in pa[:, :4].tolist()}) > 1


def test_stream_is_independent_of_threads_and_chunk(tmp_path):
    path, _ = _clip_file(tmp_path, random=True)
    kw = dict(clip_len=T, frame_stride=S, out_size=16, device='cpu', seed=SEED)
    a = ClipRecordLoader(path, 8, threads=1, **kw)
    b = ClipRecordLoader(path, 8, threads=8, chunk=3, **kw)
    c = ClipRecordLoader(path, 8, threads=8, chunk=16, **kw)
    for _ in range(2):
        (ba, sa), (bb, sb), (bc, sc) = _slots(a), _slots(b), _slots(c)
        assert len(ba) == len(bb) == len(bc) == 3
        for other_b, other_s in ((bb, sb), (bc, sc)):
            for x, y, p, q in zip(ba, other_b, sa, other_s):
                assert torch.equal(x['features'], y['features']) and torch.equal(x['targets'], y['targets'])
                assert all(torch.equal(u, v) for u, v in zip(p, q))


def test_two_ranks_cover_every_record_once_plus_the_padding(tmp_path):
    n = 23                                               # odd: one wrap-around sample pads the shards
    path, _ = _clip_file(tmp_path, n=n)
    seen = []
    for rank in (0, 1):
        L = ClipRecordLoader(path, 4, clip_len=T, frame_stride=S, out_size=16, device='cpu', seed=SEED, rank=rank,
                             world_size=2, drop_last=False)
        assert len(L) == 3 and [L.real_rows(k) for k in range(3)] == [4, 4, 4]
        got = [int(t) - 100 for b in L for t in b['targets']]
        assert len(got) == 12
        seen.append(got)
    both = seen[0] + seen[1]
    assert set(both) == set(range(n)) and len(both) == n + 1
    L = ClipRecordLoader(path, 5, clip_len=T, frame_stride=S, out_size=16, device='cpu', train=False)
    assert len(L) == 5 and L.real_rows(4) == 3 and [len(b['targets']) for b in L] == [5, 5, 5, 5, 3]


def test_a_span_longer_than_the_record_is_refused(tmp_path):
    path, _ = _clip_file(tmp_path, n=4)
    ClipRecordLoader(path, 2, clip_len=7, frame_stride=1, out_size=16, device='cpu')     # the longest that fits
    ClipRecordLoader(path, 2, clip_len=4, frame_stride=2, out_size=16, device='cpu')
    with pytest.raises(ValueError) as e:
        ClipRecordLoader(path, 2, clip_len=4, frame_stride=3, out_size=16, device='cpu')
    assert 'F=7' in str(e.value) and 'T=4' in str(e.value) and 's=3' in str(e.value)
    with pytest.raises(ValueError):
        ClipRecordLoader(path, 2, clip_len=8, out_size=16, device='cpu')
    with pytest.raises(ValueError):
        ClipRecordLoader(path, 2, clip_len=0, out_size=16, device='cpu')
    with pytest.raises(ValueError):
        ClipRecordLoader(path, 2, clip_len=2, out_size=16, device='cpu', layout='nchw')
    rt = runtime()
    h = rt.mlr_clip_open(path.encode())
    args = (0, 0.3, 1.0, 0.75, 1.333, 0, 0, 1, 0, 0, 1, 4)
    assert not rt.mlr_clip_loader_create(h, 2, 16, 16, 4, 3, *args)
    ok = rt.mlr_clip_loader_create(h, 2, 16, 16, 4, 2, *args)
    assert ok
    rt.mlr_loader_destroy(ok)
    rt.mlr_close(h)


# ------------------------------------------------------------------------- 3. twin
def _hand_pars(H, W):
    """1x1 box, the full image, a box touching the bottom-right corner, an inner box."""
    return [[H - 1, W - 1, 1, 1], [0, 0, H, W], [H - 17, W - 13, 17, 13], [3, 5, 20, 17]]


def test_twin_is_augment_reference_on_every_frame():
    torch.manual_seed(0)
    H, W, oh, ow = 40, 36, 24, 20
    boxes = _hand_pars(H, W)
    B = len(boxes)
    for flip in (0, 1):
        par = torch.tensor([b + [flip, 2, 1, 0] for b in boxes], dtype=torch.int32)
        one = torch.randint(0, 256, (B, 1, H, W, 3), dtype=torch.uint8)
        x1 = augment_clip_reference(one, par, oh, ow, MS, 'ncthw')
        assert x1.shape == (B, 3, 1, oh, ow) and x1.dtype == torch.float32 and x1.is_contiguous()
        assert torch.equal(x1[:, :, 0], augment_reference(one[:, 0], par[:, :5], oh, ow, MS, 'nchw'))
        clips = torch.randint(0, 256, (B, 3, H, W, 3), dtype=torch.uint8)
        x = augment_clip_reference(clips, par, oh, ow, MS, 'ncthw')
        assert x.shape == (B, 3, 3, oh, ow)
        for t in range(3):
            assert torch.equal(x[:, :, t], augment_reference(clips[:, t], par[:, :5], oh, ow, MS, 'nchw'))
        assert torch.equal(x[0], x[0, :, :, :1, :1].expand(3, 3, oh, ow))       # a 1x1 box is one pixel a frame
        y = augment_clip_reference(clips, par, oh, ow, MS, 'nthwc')
        assert y.shape == (B, 3, 3, oh, ow) and y.dtype == torch.bfloat16
        assert y.is_contiguous(memory_format=torch.channels_last_3d)
        assert y.permute(0, 2, 3, 4, 1).is_contiguous()
        assert torch.equal(y, x.to(torch.bfloat16))
    # a box past the image is clamped into it, as the kernel clamps it
    clips = torch.randint(0, 256, (2, 2, H, W, 3), dtype=torch.uint8)
    wild = torch.tensor([[H - 10, W - 8, 30, 30, 0, 0, 1, 0], [-4, -3, 12, 0, 1, 0, 1, 0]], dtype=torch.int32)
    tame = torch.tensor([[H - 10, W - 8, 10, 8, 0, 0, 1, 0], [0, 0, 12, 1, 1, 0, 1, 0]], dtype=torch.int32)
    assert torch.equal(augment_clip_reference(clips, wild, oh, ow, MS), augment_clip_reference(clips, tame, oh, ow, MS))
    with pytest.raises(ValueError):
        augment_clip_reference(clips, tame, oh, ow, MS, 'nchw')


@pytest.mark.parametrize('layout', ['ncthw', 'nthwc'])
def test_cpu_loader_batches_are_the_twin_of_the_slot(tmp_path, layout):
    path, _ = _clip_file(tmp_path, random=True)
    L = ClipRecordLoader(path, 8, clip_len=T, frame_stride=S, out_size=(16, 12), device='cpu', seed=SEED, layout=layout)
    batches, slots = _slots(L)
    assert len(batches) == 3
    for b, (img, lab, par) in zip(batches, slots):
        want = augment_clip_reference(img, par, 16, 12, L.mean_istd, layout)
        assert b['features'].shape == (8, 3, T, 16, 12) and b['features'].dtype == want.dtype
        assert b['features'].stride() == want.stride() and torch.equal(b['features'], want)
        assert torch.equal(b['targets'], lab)


# ------------------------------------------------------------------------- 4. runner
R2PLUS1D = dict(model='ResNeXt3D', residual_transformation_type='basic_r2plus1d_transformation',
                stem_name='r2plus1d_stem', stem_maxpool=True, num_blocks=(1, 1), stage_planes=8, stem_planes=8,
                in_plane=16, num_classes=5, stage_temporal_kernel_basis=([3], [3]),
                temporal_conv_1x1=(False, False), stage_temporal_stride=(1, 2), stage_spatial_stride=(1, 2))


@pytest.mark.parametrize('say_kind', [True, False])
def test_runner_trains_a_video_stage_from_record_files(tmp_path, say_kind):
    from mlcomp_amd.train.experiment import ConfigExperiment
    from mlcomp_amd.train.runner import Runner
    rng = np.random.default_rng(5)
    for name, n in (('tr', 8), ('va', 4)):
        write_clip_records(str(tmp_path / f'{name}.mlrec'), rng.integers(0, 256, (n, 6, 24, 28, 3), dtype=np.uint8),
                           rng.integers(0, 5, n))
    dp = {'dataset': 'records', 'path': str(tmp_path / 'tr.mlrec'), 'valid_path': str(tmp_path / 'va.mlrec'),
          'clip_length': 4, 'frame_stride': 1, 'image_size': [16, 20], 'batch_size': 4, 'num_workers': 2,
          'scale': [0.5, 1.0], 'ratio': [0.9, 1.1], 'seed': 2}
    if say_kind:
        dp['kind'] = 'video'
    cfg = {'model_params': dict(R2PLUS1D),
           'args': {'logdir': str(tmp_path / 'log'), 'engine': 'torch'},
           'stages': {'data_params': dp, 'state_params': {'num_epochs': 1},
                      'criterion_params': {'criterion': 'CrossEntropyLoss'},
                      'optimizer_params': {'optimizer': 'SGD', 'lr': 0.01},
                      'callbacks_params': {'loss': {'callback': 'CriterionCallback'},
                                           'opt': {'callback': 'OptimizerCallback'}},
                      'stage1': {}}}
    runner = Runner(ConfigExperiment(cfg), device='cpu')
    st = runner.run_experiment()
    assert set(runner.loaders) == {'train', 'valid'}
    assert all(isinstance(v, ClipRecordLoader) for v in runner.loaders.values())
    tr, va = runner.loaders['train'], runner.loaders['valid']
    assert tr.train and not va.train and tr.layout == va.layout == 'ncthw'
    assert (tr.clip_len, tr.frame_stride) == (4, 1)
    assert len(tr) == 2 and len(va) == 1                 # two training steps
    b = next(iter(tr))
    assert b['features'].shape == (4, 3, 4, 16, 20) and b['features'].dtype == torch.float32
    assert b['targets'].shape == (4,) and b['targets'].dtype == torch.int64
    m = st.epoch_metrics
    assert np.isfinite(m['train_loss']) and np.isfinite(m['valid_loss'])


# ------------------------------------------------------------------------- 5. CLI
def _frame_tree(root, videos):
    """class/video/frame files; frame k of a video is the constant image of value 10*k + id."""
    from PIL import Image
    for vid, (cls, name, count, hw) in enumerate(videos):
        d = root / cls / name
        d.mkdir(parents=True)
        for k in range(count):
            Image.fromarray(np.full(hw + (3,), 10 * k + vid, np.uint8)).save(d / f'f{k:03d}.png')


def test_contrib_pack_clip_records_cli(tmp_path):
    from click.testing import CliRunner
    from mlcomp_amd.contrib.__main__ import main
    root = tmp_path / 'videos'
    _frame_tree(root, [('cat', 'a', 9, (30, 40)), ('cat', 'b', 6, (24, 24)), ('dog', 'c', 12, (40, 26))])
    out = str(tmp_path / 'x.mlrec')
    r = CliRunner().invoke(main, ['pack-clip-records', '--video-path', str(root), '--out', out, '--frames', '3',
                                  '--size', '24', '--frame-step', '2'])
    assert r.exit_code == 0, r.output
    f = ClipRecordFile(out)
    assert len(f) == 3 and f.shape == (24, 24, 3) and f.frames == 3
    assert [f.label(i) for i in range(3)] == [0, 0, 1]
    assert open(out + '.classes').read().split() == ['cat', 'dog']
    # span 5, centred: folder a (9 frames) starts at 2, b (6) at 0, c (12) at 3
    for i, off in enumerate((2, 0, 3)):
        assert [int(f.clip(i)[k, 0, 0, 0]) for k in range(3)] == [10 * (off + 2 * k) + i for k in range(3)]
        assert len(np.unique(f.clip(i)[0])) == 1
    # a folder with too few frames: an error that names it, nothing written ...
    short = str(tmp_path / 'y.mlrec')
    r = CliRunner().invoke(main, ['pack-clip-records', '--video-path', str(root), '--out', short, '--frames', '8'])
    assert r.exit_code != 0 and os.path.join('cat', 'b') in r.output
    assert not os.path.exists(short) and not os.path.exists(short + '.tmp')
    # ... unless --pad-short repeats its last frame
    r = CliRunner().invoke(main, ['pack-clip-records', '--video-path', str(root), '--out', short, '--frames', '8',
                                  '--size', '24', '--pad-short'])
    assert r.exit_code == 0, r.output
    f = ClipRecordFile(short)
    assert f.frames == 8 and [int(f.clip(1)[k, 0, 0, 0]) for k in range(8)] == [1, 11, 21, 31, 41, 51, 51, 51]
    assert [int(f.clip(0)[k, 0, 0, 0]) for k in range(8)] == [10 * k for k in range(8)]
    # fold.csv rows, as VideoDataset reads them
    csv = tmp_path / 'fold.csv'
    csv.write_text('video,label,fold\ncat/a,cat,0\ncat/b,cat,1\ndog/c,dog,0\n')
    for extra, want in (([], [0, 1]), (['--exclude-fold'], [0])):
        o = str(tmp_path / f'f{len(extra)}.mlrec')
        r = CliRunner().invoke(main, ['pack-clip-records', '--video-path', str(root), '--out', o, '--frames', '2',
                                      '--size', '24', '--fold-csv', str(csv), '--fold', '0'] + extra)
        assert r.exit_code == 0, r.output
        f = ClipRecordFile(o)
        assert [f.label(i) for i in range(len(f))] == want


# ------------------------------------------------------------------------- 6. sanitizers
@pytest.mark.parametrize('san', ['tsan', 'asan'])
def test_clip_loader_sanitizer_selftest(san, tmp_path):
    """ThreadSanitizer / AddressSanitizer+UBSan builds of the C++ runtime under a
    stand-alone driver of the clip entry points, run as a child process."""
    from mlcomp_amd.build import build_runtime_selftest
    binary = build_runtime_selftest(san, main='records_clip_selftest.cpp')
    assert os.path.basename(binary) == f'mlcomp-records-clip-selftest-{san}'
    assert os.path.basename(build_runtime_selftest(san)) == f'mlcomp-records-selftest-{san}'   # the two
    assert os.path.basename(build_runtime_selftest(san, main='records_seg_selftest.cpp')) == \
        f'mlcomp-records-seg-selftest-{san}'                                                    # existing names
    r = subprocess.run([binary, str(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TSAN_OPTIONS='halt_on_error=1', ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'records clip selftest ok' in r.stdout
    assert 'WARNING: ThreadSanitizer' not in r.stderr and 'ERROR: AddressSanitizer' not in r.stderr
