"""Image + mask record files on the CPU (`mlcomp_amd/train/records.py`,
`csrc/runtime/records.cpp`): the file format next to the classification one, the
thread-count independent stream with its eight symmetries, image / mask alignment under
every symmetry, the PyTorch twin of ``mlc_augment_seg`` on hand-written boxes, the
sanitizer self-tests of the new C entry points, the runner and the packing CLI."""
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

from mlcomp_amd.train.records import (RecordFile, RecordLoader, SegRecordFile, SegRecordLoader, augment_reference,
                                      augment_seg_reference, write_records, write_seg_records)

MS = [123.7, 116.3, 103.5, 0.0, 1 / 58.4, 1 / 57.1, 1 / 57.4, 0.0]
FLAGS = list(itertools.product((0, 1), repeat=3))    # (hflip, vflip, transpose)


def _seg_file(tmp_path, n=40, shape=(20, 28, 3), K=1, kind='planes', seed=0, name='s.mlrec'):
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (n,) + shape, dtype=np.uint8)
    if kind == 'index':
        masks = rng.integers(0, 5, (n,) + shape[:2] + (1,), dtype=np.uint8)
    else:
        masks = (rng.integers(0, 3, (n,) + shape[:2] + (K,), dtype=np.uint8) > 1) * rng.integers(
            1, 256, (n,) + shape[:2] + (K,), dtype=np.uint8)
    path = str(tmp_path / name)
    assert write_seg_records(path, imgs, masks, kind=kind) == n
    return path, imgs, masks.astype(np.uint8)


# ------------------------------------------------------------------------- 1. format
@pytest.mark.parametrize('K,kind', [(1, 'planes'), (3, 'planes'), (1, 'index')])
def test_seg_round_trip(tmp_path, K, kind):
    path, imgs, masks = _seg_file(tmp_path, n=12, K=K, kind=kind)
    assert not os.path.exists(path + '.tmp')
    f = SegRecordFile(path)
    assert len(f) == 12 and f.shape == (20, 28, 3) and f.planes == K and f.kind == kind
    for i in (0, 5, 11):
        assert np.array_equal(f.image(i), imgs[i]) and np.array_equal(f.mask(i), masks[i])
    L = SegRecordLoader(path, 4, out_size=(20, 28), train=False, device='cpu', mean=(0, 0, 0), std=(1 / 255,) * 3)
    b = next(iter(L))
    assert torch.equal(b['features'].permute(0, 2, 3, 1).round().to(torch.uint8), torch.from_numpy(imgs[:4]))
    if kind == 'index':
        assert b['targets'].dtype == torch.int64 and torch.equal(b['targets'], torch.from_numpy(masks[:4, ..., 0]).long())
    else:
        assert b['targets'].dtype == torch.float32 and b['targets'].shape == (4, K, 20, 28)
        assert torch.equal(b['targets'], torch.from_numpy(masks[:4] != 0).float().permute(0, 3, 1, 2))


def test_two_dimensional_masks_and_bad_input(tmp_path):
    rng = np.random.default_rng(1)
    imgs = rng.integers(0, 256, (3, 6, 7, 3), dtype=np.uint8)
    m2 = rng.integers(0, 2, (3, 6, 7), dtype=np.uint8)
    path = str(tmp_path / 'a.mlrec')
    write_seg_records(path, imgs, m2)
    assert np.array_equal(SegRecordFile(path).mask(2)[..., 0], m2[2])
    with pytest.raises(ValueError):
        write_seg_records(str(tmp_path / 'b.mlrec'), imgs, np.zeros((3, 6, 7, 2), np.uint8), kind='index')
    with pytest.raises(ValueError):
        write_seg_records(str(tmp_path / 'b.mlrec'), imgs, np.zeros((3, 6, 7, 5), np.uint8))
    with pytest.raises(ValueError):
        write_seg_records(str(tmp_path / 'b.mlrec'), imgs, np.zeros((3, 6, 6, 1), np.uint8))
    assert not os.path.exists(str(tmp_path / 'b.mlrec')) and not os.path.exists(str(tmp_path / 'b.mlrec.tmp'))


def test_each_reader_refuses_the_other_kind(tmp_path):
    seg, _, _ = _seg_file(tmp_path, n=8)
    cls = str(tmp_path / 'c.mlrec')
    rng = np.random.default_rng(2)
    imgs = rng.integers(0, 256, (8, 20, 28, 3), dtype=np.uint8)
    write_records(cls, imgs, list(range(8)))
    f = RecordFile(cls)                       # a classification file reads as before
    assert len(f) == 8 and np.array_equal(f.image(3), imgs[3]) and f.label(3) == 3
    assert [int(b['targets'][0]) for b in RecordLoader(cls, 4, out_size=16, train=False, layout='nchw',
                                                       device='cpu')] == [0, 4]
    with pytest.raises(ValueError):
        RecordFile(seg)
    with pytest.raises(ValueError):
        RecordLoader(seg, 4, out_size=16, device='cpu')
    with pytest.raises(ValueError):
        SegRecordFile(cls)
    with pytest.raises(ValueError):
        SegRecordLoader(cls, 4, out_size=16, device='cpu')


def test_mask_the_size_of_a_label_is_still_refused(tmp_path):
    """2x2x1 masks are 4 bytes, the size of a label: the magic keeps the readers apart."""
    path = str(tmp_path / 't.mlrec')
    write_seg_records(path, np.zeros((2, 2, 2, 3), np.uint8), np.ones((2, 2, 2, 1), np.uint8))
    with pytest.raises(ValueError):
        RecordFile(path)
    with pytest.raises(ValueError):
        RecordLoader(path, 1, out_size=2, device='cpu', layout='nchw')


# ------------------------------------------------------------------------- 2. determinism
SEED = 3


def _params(loader):
    """The params of every batch of the next epoch, read from the ring slots as the C++
    workers fill them (the CPU path releases a slot right after the twin ran, and nothing
    refills it before the next batch is asked for when the ring is deeper than the epoch)."""
    pars = []
    orig = loader._augment_cpu

    def spy(slot):
        pars.append(slot[2].clone())
        return orig(slot)
    loader._augment_cpu = spy
    try:
        batches = list(loader)
    finally:
        loader._augment_cpu = orig
    return batches, pars


def test_stream_is_independent_of_threads_and_chunk(tmp_path):
    path, _, _ = _seg_file(tmp_path)
    a = SegRecordLoader(path, 8, out_size=16, threads=1, device='cpu', seed=SEED)
    b = SegRecordLoader(path, 8, out_size=16, threads=6, device='cpu', seed=SEED, chunk=3)
    combos = set()
    for _ in range(2):
        (ba, pa), (bb, pb) = _params(a), _params(b)
        assert len(ba) == len(bb) == 5
        for x, y, p, q in zip(ba, bb, pa, pb):
            assert torch.equal(x['features'], y['features']) and torch.equal(x['targets'], y['targets'])
            assert torch.equal(p, q) and p.shape == (8, 8) and not p[:, 7].any()
            combos |= {tuple(r) for r in p[:, 4:7].tolist()}
    assert combos == set(FLAGS)           # SEED is chosen so that two epochs show all eight


# ------------------------------------------------------------------------- 3. alignment
def test_mask_stays_on_its_image_under_every_symmetry(tmp_path):
    """Masks are ``image[..., 0] > 127``; with the output the stored size and the whole
    image as the box the resize is the identity, so the transformed mask must be the
    threshold of the transformed image, exactly, for every sample and symmetry."""
    rng = np.random.default_rng(4)
    imgs = rng.integers(0, 256, (40, 20, 20, 3), dtype=np.uint8)
    path = str(tmp_path / 'al.mlrec')
    write_seg_records(path, imgs, (imgs[..., :1] > 127).astype(np.uint8))
    L = SegRecordLoader(path, 8, out_size=20, scale=(1, 1), ratio=(1, 1), device='cpu', seed=SEED,
                        mean=(0, 0, 0), std=(1 / 255,) * 3)
    combos = set()
    for _ in range(2):
        batches, pars = _params(L)
        for b, p in zip(batches, pars):
            assert p[:, :4].tolist() == [[0, 0, 20, 20]] * 8
            combos |= {tuple(r) for r in p[:, 4:7].tolist()}
            assert torch.equal(b['targets'][:, 0], (b['features'][:, 0] > 127).float())
    assert combos == set(FLAGS)
    # the same on the twin alone, non-square, one sample per symmetry, against numpy
    img = torch.from_numpy(rng.integers(0, 256, (8, 12, 18, 3), dtype=np.uint8))
    par = torch.tensor([[0, 0, 12, 18, h, v, 0, 0] for h, v, _ in FLAGS], dtype=torch.int32)
    x, m = augment_seg_reference(img, (img[..., :1] > 127).to(torch.uint8), par, 12, 18, [0.0] * 4 + [1.0] * 4)
    for i, (h, v, _) in enumerate(FLAGS):
        want = img[i].numpy()
        want = want[:, ::-1] if h else want
        want = want[::-1] if v else want
        assert np.array_equal(x[i].permute(1, 2, 0).numpy(), want.astype(np.float32))
        assert np.array_equal(m[i, ..., 0].numpy(), (want[..., 0] > 127).astype(np.float32))


# ------------------------------------------------------------------------- 4. twin
def _hand_pars(H, W):
    """1x1 box, the full image, a box touching the bottom-right corner, an inner box."""
    return [[H - 1, W - 1, 1, 1], [0, 0, H, W], [H - 17, W - 13, 17, 13], [3, 5, 20, 17]]


def _integer_mask(mask, p, oh, ow):
    y0, x0, h, w, hf, vf, tr = p[:7]
    out = np.zeros((oh, ow, mask.shape[-1]), np.uint8)
    for oy in range(oh):
        for ox in range(ow):
            u, v, gh, gw = (ox, oy, ow, oh) if tr else (oy, ox, oh, ow)
            v = gw - 1 - v if hf else v
            u = gh - 1 - u if vf else u
            out[oy, ox] = mask[y0 + ((2 * u + 1) * h) // (2 * gh), x0 + ((2 * v + 1) * w) // (2 * gw)]
    return out


def test_twin_on_hand_written_boxes():
    torch.manual_seed(0)
    H, W, oh, ow = 40, 36, 24, 20
    boxes = _hand_pars(H, W)
    B = len(boxes)
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8)
    mask = torch.randint(0, 2, (B, H, W, 3), dtype=torch.uint8) * torch.randint(1, 256, (B, H, W, 3), dtype=torch.uint8)
    par0 = torch.tensor([b + [0, 0, 0, 0] for b in boxes], dtype=torch.int32)
    x, m = augment_seg_reference(img, mask, par0, oh, ow, MS, 'nchw')
    assert x.shape == (B, 3, oh, ow) and m.shape == (B, oh, ow, 3) and m.dtype == torch.float32
    # no flags: the image is augment_reference's
    assert torch.equal(x, augment_reference(img, par0[:, :5], oh, ow, MS, 'nchw'))
    assert torch.equal(x[0], x[0, :, :1, :1].expand(3, oh, ow))          # a 1x1 box is one pixel
    for hf, vf, tr in FLAGS:
        par = par0.clone()
        par[:, 4], par[:, 5], par[:, 6] = hf, vf, tr
        xf, mf = augment_seg_reference(img, mask, par, oh, ow, MS, 'nchw')
        _, mi = augment_seg_reference(img, mask[..., :1], par, oh, ow, MS, 'nchw', 'index')
        assert mi.dtype == torch.int64 and mi.shape == (B, oh, ow)
        for b in range(B):
            want = _integer_mask(mask[b].numpy(), par[b].tolist(), oh, ow)
            assert np.array_equal(mf[b].numpy(), (want != 0).astype(np.float32))
            assert np.array_equal(mi[b].numpy(), want[..., 0].astype(np.int64))
        if not tr:      # flips of the untransposed output are flips of the tensor
            dims = [d for d, f in ((-1, hf), (-2, vf)) if f]
            assert torch.equal(xf, x.flip(dims) if dims else x)
    # layouts carry the same image
    nhwc, _ = augment_seg_reference(img, mask, par0, oh, ow, MS, 'nhwc8')
    s2d, _ = augment_seg_reference(img, mask, par0, oh, ow, MS, 's2d')
    assert nhwc.shape == (B, oh, ow, 8) and s2d.shape == (B, (oh + 6) // 2, (ow + 6) // 2, 16)
    assert torch.allclose(nhwc[..., :3].float(), x.permute(0, 2, 3, 1), rtol=1e-2, atol=1e-2)


def test_transpose_of_a_transpose_is_the_identity():
    torch.manual_seed(1)
    S = 16
    img = torch.randint(0, 256, (2, 30, 26, 3), dtype=torch.uint8)
    mask = torch.randint(0, 2, (2, 30, 26, 2), dtype=torch.uint8)
    one = [0.0] * 4 + [1.0] * 4
    par = torch.tensor([[2, 3, 22, 19, 0, 0, 1, 0], [0, 0, 30, 26, 0, 0, 1, 0]], dtype=torch.int32)
    full = torch.tensor([[0, 0, S, S, 0, 0, 1, 0]] * 2, dtype=torch.int32)
    plain = par.clone()
    plain[:, 6] = 0
    x0, m0 = augment_seg_reference(img, mask, plain, S, S, one)
    x1, m1 = augment_seg_reference(img, mask, par, S, S, one)
    # transposing is swapping the output axes ...
    assert torch.equal(x1, x0.transpose(2, 3)) and torch.equal(m1, m0.transpose(1, 2))
    # ... and an identity-size transpose of the transposed result gives the first back
    back_m = augment_seg_reference(img[:, :S, :S], m1.to(torch.uint8), full, S, S, one)[1]
    assert torch.equal(back_m, m0)
    x1u8 = x1.permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8)
    x0u8 = x0.permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8)
    back_x = augment_seg_reference(x1u8, m1.to(torch.uint8), full, S, S, one)[0]
    assert torch.equal(back_x.permute(0, 2, 3, 1).to(torch.uint8), x0u8)


# ------------------------------------------------------------------------- 5. sanitizers
@pytest.mark.parametrize('san', ['tsan', 'asan'])
def test_seg_loader_sanitizer_selftest(san, tmp_path):
    """ThreadSanitizer / AddressSanitizer+UBSan builds of the C++ runtime under a
    stand-alone driver of the segmentation entry points, run as a child process."""
    from mlcomp_amd.build import build_runtime_selftest
    binary = build_runtime_selftest(san, main='records_seg_selftest.cpp')
    assert os.path.basename(binary) == f'mlcomp-records-seg-selftest-{san}'
    assert os.path.basename(build_runtime_selftest(san)) == f'mlcomp-records-selftest-{san}'   # default kept
    r = subprocess.run([binary, str(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TSAN_OPTIONS='halt_on_error=1', ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'records seg selftest ok' in r.stdout
    assert 'WARNING: ThreadSanitizer' not in r.stderr and 'ERROR: AddressSanitizer' not in r.stderr


# ------------------------------------------------------------------------- 6. runner
@pytest.mark.parametrize('kind', ['planes', 'index'])
def test_runner_trains_a_segmentation_stage_from_record_files(tmp_path, kind):
    from mlcomp_amd.train.experiment import ConfigExperiment
    from mlcomp_amd.train.runner import Runner
    tr, _, _ = _seg_file(tmp_path, n=16, shape=(40, 40, 3), kind=kind, name='tr.mlrec')
    va, _, _ = _seg_file(tmp_path, n=8, shape=(40, 40, 3), kind=kind, seed=1, name='va.mlrec')
    classes = 1 if kind == 'planes' else 5
    cfg = {'model_params': {'model': 'Unet', 'encoder_name': 'resnet18', 'classes': classes,
                            'encoder_weights': None},
           'args': {'logdir': str(tmp_path / 'log'), 'engine': 'torch'},
           'stages': {'data_params': {'dataset': 'records', 'kind': 'segmentation', 'path': tr, 'valid_path': va,
                                      'image_size': 32, 'batch_size': 4, 'num_workers': 2, 'scale': [0.6, 1.0],
                                      'ratio': [0.9, 1.1]},
                      'state_params': {'num_epochs': 1},
                      'criterion_params': {'criterion': 'BCEWithLogitsLoss' if kind == 'planes'
                                           else 'CrossEntropyLoss'},
                      'optimizer_params': {'optimizer': 'Adam', 'lr': 0.001},
                      'callbacks_params': {'loss': {'callback': 'CriterionCallback'},
                                           'opt': {'callback': 'OptimizerCallback'}},
                      'stage1': {}}}
    runner = Runner(ConfigExperiment(cfg), device='cpu')
    st = runner.run_experiment()
    assert set(runner.loaders) == {'train', 'valid'}
    assert all(isinstance(v, SegRecordLoader) for v in runner.loaders.values())
    assert runner.loaders['train'].train and not runner.loaders['valid'].train
    for name, n in (('train', 4), ('valid', 2)):
        batches = list(runner.loaders[name])
        assert len(batches) == n
        b = batches[0]
        assert b['features'].shape == (4, 3, 32, 32) and b['features'].dtype == torch.float32
        if kind == 'planes':
            assert b['targets'].shape == (4, 1, 32, 32) and b['targets'].dtype == torch.float32
        else:
            assert b['targets'].shape == (4, 32, 32) and b['targets'].dtype == torch.int64
    m = st.epoch_metrics
    assert np.isfinite(m['train_loss']) and np.isfinite(m['valid_loss'])


def test_runner_tells_the_kind_from_the_file_header(tmp_path):
    from mlcomp_amd.train.experiment import ConfigExperiment
    from mlcomp_amd.train.runner import Runner
    tr, _, _ = _seg_file(tmp_path, n=8, shape=(24, 24, 3), name='tr.mlrec')
    cfg = {'model_params': {'model': 'SimpleCNN', 'num_classes': 2, 'width': 8},
           'args': {'logdir': str(tmp_path / 'log'), 'engine': 'torch'}, 'stages': {'stage1': {}}}
    r = Runner(ConfigExperiment(cfg), device='cpu')
    loaders = r._record_loaders({'dataset': 'records', 'path': tr, 'image_size': [16, 20], 'num_workers': 1}, 4)
    assert isinstance(loaders['train'], SegRecordLoader) and list(loaders) == ['train']
    b = next(iter(loaders['train']))
    assert b['features'].shape == (4, 3, 16, 20) and b['targets'].shape == (4, 1, 16, 20)


# ------------------------------------------------------------------------- 7. CLI
def test_contrib_pack_seg_records_cli(tmp_path):
    from click.testing import CliRunner
    from PIL import Image
    from mlcomp_amd.contrib.__main__ import main
    rng = np.random.default_rng(3)
    (tmp_path / 'img').mkdir()
    (tmp_path / 'mask').mkdir()
    for i in range(6):
        if i < 5:    # a horizontal ramp: the resized image and the nearest-sampled mask share one edge
            a = np.broadcast_to((np.arange(40) * 6).astype(np.uint8)[None, :, None], (30 + i, 40, 3))
        else:        # already the stored size: packed as it is
            a = rng.integers(0, 256, (24, 24, 3), dtype=np.uint8)
        Image.fromarray(np.ascontiguousarray(a)).save(tmp_path / 'img' / f'{i}.png')
        Image.fromarray(((a[..., 0] > 127) * 255).astype(np.uint8)).save(tmp_path / 'mask' / f'{i}.png')
    out = str(tmp_path / 'x.mlrec')
    r = CliRunner().invoke(main, ['pack-seg-records', str(tmp_path / 'img'), str(tmp_path / 'mask'), out,
                                  '--size', '24'])
    assert r.exit_code == 0, r.output
    f = SegRecordFile(out)
    assert len(f) == 6 and f.shape == (24, 24, 3) and f.planes == 1 and f.kind == 'planes'
    assert set(np.unique(f.mask(0))) <= {0, 255}
    assert np.array_equal(f.image(5)[..., 0] > 127, f.mask(5)[..., 0] > 0)
    for i in range(5):   # same geometry for both: they disagree in the edge column at most
        assert np.sum((f.image(i)[..., 0] > 127) != (f.mask(i)[..., 0] > 0)) <= 24
    r = CliRunner().invoke(main, ['pack-seg-records', str(tmp_path / 'img'), str(tmp_path / 'mask'),
                                  str(tmp_path / 'i.mlrec'), '--size', '24', '--kind', 'index'])
    assert r.exit_code == 0 and SegRecordFile(str(tmp_path / 'i.mlrec')).kind == 'index'
    os.rename(tmp_path / 'mask' / '5.png', tmp_path / 'mask' / '7.png')
    r = CliRunner().invoke(main, ['pack-seg-records', str(tmp_path / 'img'), str(tmp_path / 'mask'),
                                  str(tmp_path / 'y.mlrec'), '--size', '24'])
    assert r.exit_code != 0 and 'pair' in r.output and not os.path.exists(str(tmp_path / 'y.mlrec'))
