"""The GPU half of the segmentation input pipeline: ``mlc_augment_seg``
(csrc/kernels/augment.hip) against its PyTorch twin for every output layout and mask kind
and against ``mlc_augment`` where the two must agree bit for bit, the CUDA SegRecordLoader
against the CPU one on the same stream, and a loader batch fed to the native U-Net step
through ``load_batch(..., pixel_order=True)`` against today's NCHW / NKHW path."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MS = [123.7, 116.3, 103.5, 0.0, 1 / 58.4, 1 / 57.1, 1 / 57.4, 0.0]
H, W = 40, 36
FULL, ONE, CORNER = [0, 0, H, W], [H - 1, W - 1, 1, 1], [H - 17, W - 13, 17, 13]
INNER = [[3, 5, 20, 17], [10, 2, 30, 30], [0, 20, 9, 16]]
# two batches of five: every (hflip, vflip, transpose) once, the 1x1, full and corner boxes with
# and without flags
BOXES = [FULL, INNER[0], CORNER, INNER[1], ONE, INNER[2], FULL, CORNER, ONE, CORNER]
FLAGS = list(itertools.product((0, 1), repeat=3)) + [(0, 0, 0), (1, 1, 1)]
PARS = torch.tensor([b + list(f) + [0] for b, f in zip(BOXES, FLAGS)], dtype=torch.int32)
KINDS = [('planes', 1), ('planes', 3), ('planes', 4), ('index', 1)]


@pytest.fixture(scope='module')
def source():
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (5, H, W, 3), dtype=torch.uint8, generator=g)
    mask = torch.randint(0, 2, (5, H, W, 4), dtype=torch.uint8, generator=g) \
        * torch.randint(1, 256, (5, H, W, 4), dtype=torch.uint8, generator=g)
    index = torch.randint(0, 7, (5, H, W, 1), dtype=torch.uint8, generator=g)
    return img, mask, index


def _run(img, mask, par, oh, ow, layout, kind):
    from mlcomp_amd.ops import _lib
    from mlcomp_amd.train.records import LAYOUTS, MASK_KINDS, augment_seg_reference
    ref_x, ref_m = augment_seg_reference(img, mask, par, oh, ow, MS, layout, kind)
    B, K = img.shape[0], mask.shape[-1]
    dimg, dmask, dpar = img.cuda(), mask.contiguous().cuda(), par.cuda()
    dms = torch.tensor(MS, device='cuda')
    out = torch.empty(ref_x.shape, dtype=ref_x.dtype, device='cuda')
    om = torch.full(ref_m.shape, -1, dtype=ref_m.dtype, device='cuda')
    _lib.call('mlc_augment_seg', _lib.ptr(dimg), _lib.ptr(dmask), _lib.ptr(dpar), _lib.ptr(dms), _lib.ptr(out),
              _lib.ptr(om), B, H, W, 3, K, oh, ow, LAYOUTS[layout], MASK_KINDS[kind], _lib.stream())
    torch.cuda.synchronize()
    return out, om, ref_x, ref_m


@pytest.mark.parametrize('kind,K', KINDS)
@pytest.mark.parametrize('layout', ['s2d', 'nhwc8', 'nchw'])
def test_augment_seg_kernel_matches_reference(source, layout, kind, K):
    img, mask, index = source
    m = index if kind == 'index' else mask[..., :K].contiguous()
    oh, ow = (24, 24) if layout == 's2d' else (24, 20)
    tol = 1e-4 if layout == 'nchw' else 2e-2
    for part in (PARS[:5], PARS[5:]):
        out, om, ref_x, ref_m = _run(img, m, part, oh, ow, layout, kind)
        assert om.dtype == (torch.int64 if kind == 'index' else torch.float32)
        assert torch.equal(om.cpu(), ref_m)
        assert torch.allclose(out.cpu().float(), ref_x.float(), atol=tol, rtol=tol)


@pytest.mark.parametrize('layout', ['s2d', 'nhwc8', 'nchw'])
def test_without_flags_the_image_is_mlc_augment_bit_for_bit(source, layout):
    from mlcomp_amd.ops import _lib
    from mlcomp_amd.train.records import LAYOUTS
    img, mask, _ = source
    par = torch.tensor([b + [0, 0, 0, 0] for b in (FULL, INNER[0], CORNER, INNER[1], ONE)], dtype=torch.int32)
    oh, ow = (24, 24) if layout == 's2d' else (24, 20)
    out, _, _, _ = _run(img, mask[..., :1].contiguous(), par, oh, ow, layout, 'planes')
    old = torch.empty_like(out)
    dimg, dpar5, dms = img.cuda(), par[:, :5].contiguous().cuda(), torch.tensor(MS, device='cuda')
    _lib.call('mlc_augment', _lib.ptr(dimg), _lib.ptr(dpar5), _lib.ptr(dms), _lib.ptr(old), 5, H, W, 3, oh, ow,
              LAYOUTS[layout], _lib.stream())
    torch.cuda.synchronize()
    bits = torch.int16 if out.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(out.view(bits), old.view(bits))


def test_launcher_refuses_arguments_out_of_range(source):
    from mlcomp_amd.ops import _lib
    img, mask, _ = source
    d = [t.cuda() for t in (img, mask, PARS[:5], torch.tensor(MS))]
    out = torch.empty(5 * 32 * 32 * 16, device='cuda')
    om = torch.empty(5 * 32 * 32 * 4, dtype=torch.int64, device='cuda')
    fn = _lib.load().mlc_augment_seg

    def rc(C=3, K=4, oh=24, ow=24, layout=0, kind=0, B=5):
        return fn(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), _lib.ptr(out), _lib.ptr(om),
                  B, H, W, C, K, oh, ow, layout, kind, _lib.stream())
    assert rc() == 0
    for bad in (dict(C=0), dict(C=5), dict(K=0), dict(K=5), dict(layout=3), dict(layout=-1), dict(kind=2),
                dict(kind=1, K=3), dict(oh=23), dict(ow=23), dict(C=4, layout=0), dict(B=0), dict(oh=0)):
        assert rc(**bad) == -1, bad
    torch.cuda.synchronize()


@pytest.mark.parametrize('layout,out_size,shape', [('s2d', 24, (8, 15, 15, 16)), ('nhwc8', (24, 20), (8, 24, 20, 8)),
                                                   ('nchw', (24, 20), (8, 3, 24, 20))])
def test_cuda_seg_loader_matches_cpu(tmp_path, layout, out_size, shape):
    from mlcomp_amd.train.records import SegRecordLoader, write_seg_records
    rng = np.random.default_rng(2)
    path = str(tmp_path / 's.mlrec')
    write_seg_records(path, rng.integers(0, 256, (40, 32, 32, 3), dtype=np.uint8),
                      rng.integers(0, 2, (40, 32, 32, 2), dtype=np.uint8))
    kw = dict(out_size=out_size, layout=layout, seed=5, mask_order='pixel' if layout != 'nchw' else 'nkhw')
    g = SegRecordLoader(path, 8, threads=4, device='cuda', **kw)
    c = SegRecordLoader(path, 8, threads=2, device='cpu', **kw)
    oh, ow = (out_size, out_size) if isinstance(out_size, int) else out_size
    tol = 1e-4 if layout == 'nchw' else 2e-2
    for _ in range(2):   # two epochs
        gb, cb = list(g), list(c)
        assert len(gb) == len(cb) == 5
        for a, b in zip(gb, cb):
            assert a['features'].is_cuda and a['targets'].is_cuda and a['features'].shape == shape
            assert a['targets'].shape == ((8, 2, oh, ow) if layout == 'nchw' else (8, oh, ow, 2))
            assert torch.equal(a['targets'].cpu(), b['targets'])
            assert torch.allclose(a['features'].cpu().float(), b['features'].float(), atol=tol, rtol=tol)


def test_loader_batch_feeds_the_native_step(tmp_path):
    from mlcomp_amd.train.native_seg_step import NativeSegmentationStep
    from mlcomp_amd.train.records import SegRecordLoader, write_seg_records
    rng = np.random.default_rng(7)
    imgs = rng.integers(0, 256, (8, 72, 72, 3), dtype=np.uint8)
    path = str(tmp_path / 'n.mlrec')
    write_seg_records(path, imgs, (imgs[..., :1] > 127).astype(np.uint8))
    step = NativeSegmentationStep(arch='unet', encoder='resnet34', batch=4, image_size=64, classes=1,
                                  use_graph=False)
    layout = 's2d' if step.x.shape[-1] == 16 else 'nhwc8'
    new = next(iter(SegRecordLoader(path, 4, out_size=64, layout=layout, mask_order='pixel', seed=1, device='cuda')))
    # the same samples on today's path: the twin's NCHW fp32 images and [N, K, H, W] masks
    old = next(iter(SegRecordLoader(path, 4, out_size=64, layout='nchw', mask_order='nkhw', seed=1, device='cpu')))
    assert new['features'].shape == step.x.shape and new['targets'].shape == (4, 64, 64, 1)
    assert old['features'].shape == (4, 3, 64, 64) and old['targets'].shape == (4, 1, 64, 64)
    step.load_batch(old['features'], old['targets'])
    x_old, t_old = step.x.clone(), step.t.clone()
    step.load_batch(new['features'], new['targets'], pixel_order=True)
    assert torch.equal(step.t, t_old)
    assert torch.allclose(step.x.float(), x_old.float(), atol=2e-2, rtol=2e-2)
    with pytest.raises(ValueError):
        step.load_batch(new['features'][:2], new['targets'][:2], pixel_order=True)
    losses = []
    for _ in range(3):
        step()
        losses.append(step.last_loss())
    print('losses on the repeated batch:', losses)
    assert all(np.isfinite(v) for v in losses)
    assert losses[0] >= losses[1] >= losses[2]


def test_native_segmentation_stage_trains_from_record_files(tmp_path):
    """``dataset: records`` with mask files on the native engine: training batches arrive
    in pixel order and go through ``load_batch(pixel_order=True)``, validation batches
    through the native eval path."""
    from mlcomp_amd.train.experiment import ConfigExperiment
    from mlcomp_amd.train.records import SegRecordLoader, write_seg_records
    from mlcomp_amd.train.runner import Runner
    rng = np.random.default_rng(8)
    for name, n in (('tr', 16), ('va', 6)):
        imgs = rng.integers(0, 256, (n, 72, 72, 3), dtype=np.uint8)
        write_seg_records(str(tmp_path / f'{name}.mlrec'), imgs, (imgs[..., :1] > 127).astype(np.uint8))
    cfg = {'model_params': {'model': 'Unet', 'encoder_name': 'resnet34', 'classes': 1},
           'args': {'logdir': str(tmp_path / 'log'), 'engine': 'native', 'graph': False},
           'stages': {'data_params': {'dataset': 'records', 'path': str(tmp_path / 'tr.mlrec'),
                                      'valid_path': str(tmp_path / 'va.mlrec'), 'image_size': 64, 'batch_size': 4,
                                      'num_workers': 2},
                      'state_params': {'num_epochs': 1, 'main_metric': 'dice', 'minimize_metric': False},
                      'criterion_params': {'criterion': 'BCEDiceLoss'},
                      'optimizer_params': {'optimizer': 'Adam', 'lr': 3e-4},
                      'callbacks_params': {'loss': {'callback': 'CriterionCallback'},
                                           'opt': {'callback': 'OptimizerCallback'},
                                           'dice': {'callback': 'DiceCallback'}},
                      'stage1': {}}}
    r = Runner(ConfigExperiment(cfg), device='cuda')
    calls = []
    st = None
    orig = None

    def spy(images, masks, pixel_order=False):
        calls.append((tuple(images.shape), tuple(masks.shape), pixel_order))
        return orig(images, masks, pixel_order=pixel_order)
    build = r._build_native

    def build_and_spy(stage, batch):
        nonlocal orig
        build(stage, batch)
        orig = r.native_step.load_batch
        r.native_step.load_batch = spy
    r._build_native = build_and_spy
    st = r.run_experiment()
    assert st.native and r.native_kind == 'unet'
    tr, va = r.loaders['train'], r.loaders['valid']
    assert isinstance(tr, SegRecordLoader) and tr.mask_order == 'pixel' and tr.layout in ('s2d', 'nhwc8')
    assert isinstance(va, SegRecordLoader) and va.mask_order == 'nkhw' and va.layout == tr.layout
    assert len(calls) == 4 and all(c == (tuple(r.native_step.x.shape), (4, 64, 64, 1), True) for c in calls)
    m = st.epoch_metrics
    assert np.isfinite(m['train_loss']) and np.isfinite(m['valid_loss']) and 0.0 <= m['valid_dice'] <= 1.0
