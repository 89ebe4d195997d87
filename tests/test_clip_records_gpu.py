"""The GPU half of the video input pipeline: ``mlc_augment_clip`` (csrc/kernels/augment.hip)
against its PyTorch twin in both layouts, against ``mlc_augment`` frame by frame and between
its two layouts bit for bit, its guard band and its launcher checks, the CUDA
ClipRecordLoader against the CPU one on the same stream, a loader batch through a training
step of the generic native engine in both layouts, and a video stage through the runner."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MS = [123.7, 116.3, 103.5, 0.0, 1 / 58.4, 1 / 57.1, 1 / 57.4, 0.0]
B, T, H, W = 3, 3, 40, 36
FULL, ONE, CORNER, INNER = [0, 0, H, W], [H - 1, W - 1, 1, 1], [H - 17, W - 13, 17, 13], [3, 5, 20, 17]
# runs past the image on both axes.  Always sample 0 of its launch: without the kernel's clamp
# its reads land in the frames behind it, inside the batch, and the comparison fails - no fault
WILD = [H - 10, W - 8, 30, 30]
TAIL = [6, 1, 0]            # t0, frame stride, 0: carried, not read by the kernel
# three launches of three clips: every box with flip 0 and with flip 1
GROUPS = [torch.tensor([b + [f] + TAIL for b, f in g], dtype=torch.int32) for g in (
    [(WILD, 0), (FULL, 0), (ONE, 1)], [(CORNER, 0), (INNER, 1), (FULL, 1)], [(ONE, 0), (CORNER, 1), (INNER, 0)])]
SIZES = [(24, 20), (23, 19)]        # the second: oh*ow odd, the paired 3-channel store has a tail
GUARD = 4096


@pytest.fixture(scope='module')
def source():
    g = torch.Generator().manual_seed(0)
    return torch.randint(0, 256, (B, T, H, W, 3), dtype=torch.uint8, generator=g)


def _clips(source, Cc):
    return source if Cc == 3 else source[..., :Cc].contiguous()


_twins = {}


def _twin(source, Cc, gi, size, layout):
    """The twin's result, computed once per case and shared."""
    from mlcomp_amd.train.records import augment_clip_reference
    key = (Cc, gi, size, layout)
    if key not in _twins:
        _twins[key] = augment_clip_reference(_clips(source, Cc), GROUPS[gi], size[0], size[1], MS, layout)
    return _twins[key]


def _launch(clips, par, oh, ow, layout):
    """(out as the logical [B, C, T, oh, ow] tensor, guard band intact): out is the front of
    a buffer whose last GUARD elements hold a sentinel."""
    from mlcomp_amd.ops import _lib
    from mlcomp_amd.train.records import CLIP_LAYOUTS
    Bn, Tn, Cc = clips.shape[0], clips.shape[1], clips.shape[-1]
    n = Bn * Tn * oh * ow * Cc
    dt = torch.float32 if layout == 'ncthw' else torch.bfloat16
    buf = torch.full((n + GUARD,), 12352.0, dtype=dt, device='cuda')
    dclips, dpar, dms = clips.cuda(), par.cuda(), torch.tensor(MS, device='cuda')
    _lib.call('mlc_augment_clip', _lib.ptr(dclips), _lib.ptr(dpar), _lib.ptr(dms), _lib.ptr(buf), Bn, Tn, H, W, Cc,
              oh, ow, CLIP_LAYOUTS[layout], _lib.stream())
    torch.cuda.synchronize()
    intact = bool((buf[n:] == 12352.0).all())
    if layout == 'ncthw':
        return buf[:n].view(Bn, Cc, Tn, oh, ow), intact
    return buf[:n].view(Bn, Tn, oh, ow, Cc).permute(0, 4, 1, 2, 3), intact


def _bits(x):
    """Integer view of a logical [B, C, T, oh, ow] tensor in [B, T, oh, ow, C] order."""
    return x.permute(0, 2, 3, 4, 1).contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize('Cc', [3, 1])
@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('layout', ['ncthw', 'nthwc'])
def test_augment_clip_kernel_matches_reference(source, layout, size, Cc):
    tol = 1e-4 if layout == 'ncthw' else 2e-2
    for gi, par in enumerate(GROUPS):
        out, _ = _launch(_clips(source, Cc), par, size[0], size[1], layout)
        ref = _twin(source, Cc, gi, size, layout)
        assert out.shape == ref.shape == (B, Cc, T, size[0], size[1]) and out.dtype == ref.dtype
        err = float((out.cpu().float() - ref.float()).abs().max())
        print(f'{layout} C={Cc} {size} launch {gi}: max abs err {err:.3g}')
        assert torch.allclose(out.cpu().float(), ref.float(), atol=tol, rtol=tol)


def _clamped5(par):
    p = par[:, :5].clone().long()
    p[:, 0].clamp_(0, H - 1)
    p[:, 1].clamp_(0, W - 1)
    p[:, 2] = torch.minimum(p[:, 2].clamp(min=1), H - p[:, 0])
    p[:, 3] = torch.minimum(p[:, 3].clamp(min=1), W - p[:, 1])
    return p.int()


@pytest.mark.parametrize('Cc', [3, 1])
@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('frames', [T, 1])
def test_every_frame_is_mlc_augment_bit_for_bit(source, frames, size, Cc):
    """``out[b, :, t]`` of ncthw against ``mlc_augment`` (nchw) over the B*T frames with each
    clip's box repeated (the out-of-range box as the kernel clamps it: ``mlc_augment`` does not
    clamp and must not see it)."""
    from mlcomp_amd.ops import _lib
    from mlcomp_amd.train.records import LAYOUTS
    oh, ow = size
    clips = _clips(source, Cc)[:, :frames].contiguous()
    for par in GROUPS:
        out, _ = _launch(clips, par, oh, ow, 'ncthw')
        dimg = clips.view(B * frames, H, W, Cc).cuda()
        dpar5 = _clamped5(par).repeat_interleave(frames, dim=0).contiguous().cuda()
        dms = torch.tensor(MS, device='cuda')
        old = torch.empty(B * frames, Cc, oh, ow, device='cuda')
        _lib.call('mlc_augment', _lib.ptr(dimg), _lib.ptr(dpar5), _lib.ptr(dms), _lib.ptr(old), B * frames, H, W, Cc,
                  oh, ow, LAYOUTS['nchw'], _lib.stream())
        torch.cuda.synchronize()
        old = old.view(B, frames, Cc, oh, ow).transpose(1, 2)
        assert torch.equal(out.contiguous().view(torch.int32), old.contiguous().view(torch.int32))


@pytest.mark.parametrize('Cc', [3, 1])
@pytest.mark.parametrize('size', SIZES)
def test_the_two_layouts_hold_the_same_bits(source, size, Cc):
    """nthwc is ncthw rounded to bf16 by torch and permuted, exactly (the kernel packs with
    the hardware's round-to-nearest-even conversion, torch's rounding)."""
    for par in GROUPS:
        a, _ = _launch(_clips(source, Cc), par, size[0], size[1], 'ncthw')
        b, _ = _launch(_clips(source, Cc), par, size[0], size[1], 'nthwc')
        want, got = _bits(a.to(torch.bfloat16)), _bits(b)
        print(f'C={Cc} {size}: {int((want != got).sum())} of {want.numel()} bf16 elements differ')
        assert torch.equal(want, got)


@pytest.mark.parametrize('Cc', [3, 1, 2, 4])
@pytest.mark.parametrize('layout', ['ncthw', 'nthwc'])
def test_nothing_is_written_behind_the_output(source, layout, Cc):
    g = torch.Generator().manual_seed(Cc)
    clips = torch.randint(0, 256, (B, T, H, W, Cc), dtype=torch.uint8, generator=g)
    for size in SIZES + [(1, 1)]:
        for par in GROUPS[:2]:
            out, intact = _launch(clips, par, size[0], size[1], layout)
            assert intact, (layout, Cc, size)
            assert bool((out != 12352.0).all())          # and everything in front of it is


def test_launcher_refuses_arguments_out_of_range(source):
    from mlcomp_amd.ops import _lib
    d = [t.cuda() for t in (source, GROUPS[0], torch.tensor(MS))]
    out = torch.full((B * T * 24 * 20 * 4,), 7.0, device='cuda')
    fn = _lib.load().mlc_augment_clip
    ptrs = dict(src=_lib.ptr(d[0]), par=_lib.ptr(d[1]), ms=_lib.ptr(d[2]), out=_lib.ptr(out))

    def rc(Cc=3, Bn=B, Tn=T, h=H, w=W, oh=24, ow=20, layout=0, **null):
        p = dict(ptrs, **{k: None for k in null})
        return fn(p['src'], p['par'], p['ms'], p['out'], Bn, Tn, h, w, Cc, oh, ow, layout, _lib.stream())
    for bad in (dict(Cc=0), dict(Cc=5), dict(Bn=0), dict(Bn=-1), dict(Tn=0), dict(h=0), dict(w=-3), dict(oh=0),
                dict(ow=0), dict(layout=2), dict(layout=-1), dict(src=1), dict(par=1), dict(ms=1), dict(out=1)):
        assert rc(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                      # nothing was launched
    assert rc() == 0 and rc(layout=1) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize('layout', ['ncthw', 'nthwc'])
def test_cuda_clip_loader_matches_cpu(tmp_path, layout):
    from mlcomp_amd.train.records import ClipRecordLoader, write_clip_records
    rng = np.random.default_rng(2)
    path = str(tmp_path / 'v.mlrec')
    write_clip_records(path, rng.integers(0, 256, (20, 7, 32, 36, 3), dtype=np.uint8), rng.integers(0, 9, 20))
    kw = dict(clip_len=3, frame_stride=2, out_size=(24, 20), layout=layout, seed=5)
    g = ClipRecordLoader(path, 4, threads=4, device='cuda', **kw)
    c = ClipRecordLoader(path, 4, threads=2, device='cpu', **kw)
    tol = 1e-4 if layout == 'ncthw' else 2e-2
    for _ in range(2):   # two epochs
        gb, cb = list(g), list(c)
        assert len(gb) == len(cb) == 5
        for a, b in zip(gb, cb):
            assert a['features'].is_cuda and a['targets'].is_cuda and a['features'].shape == (4, 3, 3, 24, 20)
            assert a['features'].dtype == b['features'].dtype and a['features'].stride() == b['features'].stride()
            assert a['targets'].dtype == torch.int64 and torch.equal(a['targets'].cpu(), b['targets'])
            assert torch.allclose(a['features'].cpu().float(), b['features'].float(), atol=tol, rtol=tol)


@pytest.mark.parametrize('name', ['r2plus1d', 'resnext3d'])
def test_loader_batch_trains_the_generic_engine_in_both_layouts(tmp_path, name):
    """One training step of the tiny video models of test_generic_gpu on the generic native
    engine, fed the loader's bf16 channels_last_3d batch and the same batch as NCTHW fp32:
    loss and updated parameters agree within that file's tolerance for these models (loss
    2e-2 relative + 1e-3, as its graph / eager comparison; relative error 2e-2)."""
    from test_generic_gpu import _models, _no_stochastic
    from mlcomp_amd.train.native_generic_step import NativeGenericStep
    from mlcomp_amd.train.records import ClipRecordLoader, write_clip_records
    make, shape, ncls = _models()[name]
    N, Cc, frames, size, _ = shape
    rng = np.random.default_rng(4)
    path = str(tmp_path / 'v.mlrec')
    write_clip_records(path, rng.integers(0, 256, (2 * N, frames + 2, 40, 40, Cc), dtype=np.uint8),
                       rng.integers(0, ncls, 2 * N))
    batches = {layout: next(iter(ClipRecordLoader(path, N, clip_len=frames, out_size=size, layout=layout, seed=1,
                                                  device='cuda')))
               for layout in ('nthwc', 'ncthw')}
    new, old = batches['nthwc'], batches['ncthw']
    assert new['features'].shape == old['features'].shape == shape
    assert new['features'].dtype == torch.bfloat16 and old['features'].dtype == torch.float32
    assert new['features'].permute(0, 2, 3, 4, 1).is_contiguous() and old['features'].is_contiguous()
    assert torch.equal(new['targets'], old['targets'])
    torch.manual_seed(0)
    ms = [_no_stochastic(make()) for _ in range(2)]
    ms[1].load_state_dict(ms[0].state_dict())
    losses, params = [], []
    for m, b in zip(ms, (new, old)):
        step = NativeGenericStep(m, b['features'], b['targets'], device='cuda', use_graph=False, optimizer='SGD',
                                 lr=0.05, momentum=0.9)
        assert step.x.dtype == b['features'].dtype and step.x.stride() == b['features'].stride()
        step()
        losses.append(step.last_loss())
        params.append(torch.cat([a.master for a in step.net.arena.arenas()]).float().cpu())
    err = float((params[0] - params[1]).norm() / params[1].norm())
    print(f'{name}: loss {losses[0]:.6f} (nthwc bf16) / {losses[1]:.6f} (ncthw fp32), parameters rel err {err:.3g}')
    assert all(np.isfinite(v) for v in losses)
    assert abs(losses[0] - losses[1]) <= 2e-2 * abs(losses[1]) + 1e-3
    assert err <= 2e-2


def test_video_stage_trains_from_record_files_on_the_generic_engine(tmp_path):
    """``dataset: records`` with clip files through the runner on the GPU: the generic native
    engine gets the bf16 channels_last_3d clips, validation included."""
    from mlcomp_amd.train.experiment import ConfigExperiment
    from mlcomp_amd.train.records import ClipRecordLoader, write_clip_records
    from mlcomp_amd.train.runner import Runner
    rng = np.random.default_rng(8)
    for name, n in (('tr', 16), ('va', 4)):
        write_clip_records(str(tmp_path / f'{name}.mlrec'), rng.integers(0, 256, (n, 10, 40, 40, 3), dtype=np.uint8),
                           rng.integers(0, 5, n))
    cfg = {'model_params': dict(model='ResNeXt3D', residual_transformation_type='basic_r2plus1d_transformation',
                                stem_name='r2plus1d_stem', stem_maxpool=True, num_blocks=(1, 1), stage_planes=32,
                                stem_planes=32, in_plane=64, num_classes=5, stage_temporal_kernel_basis=([3], [3]),
                                temporal_conv_1x1=(False, False), stage_temporal_stride=(1, 2),
                                stage_spatial_stride=(1, 2)),
           'args': {'logdir': str(tmp_path / 'log'), 'engine': 'native', 'graph': False},
           'stages': {'data_params': {'dataset': 'records', 'path': str(tmp_path / 'tr.mlrec'),
                                      'valid_path': str(tmp_path / 'va.mlrec'), 'clip_length': 8, 'image_size': 32,
                                      'batch_size': 4, 'num_workers': 2},
                      'state_params': {'num_epochs': 1},
                      'criterion_params': {'criterion': 'CrossEntropyLoss'},
                      'optimizer_params': {'optimizer': 'SGD', 'lr': 0.01, 'momentum': 0.9},
                      'callbacks_params': {'loss': {'callback': 'CriterionCallback'},
                                           'opt': {'callback': 'OptimizerCallback'}},
                      'stage1': {}}}
    r = Runner(ConfigExperiment(cfg), device='cuda')
    st = r.run_experiment()
    assert st.native and r.native_kind == 'generic'
    tr, va = r.loaders['train'], r.loaders['valid']
    assert isinstance(tr, ClipRecordLoader) and isinstance(va, ClipRecordLoader)
    assert tr.layout == va.layout == 'nthwc' and len(tr) == 4
    assert r.native_step.x.dtype == torch.bfloat16 and r.native_step.x.shape == (4, 3, 8, 32, 32)
    m = st.epoch_metrics
    print('video stage metrics:', {k: v for k, v in m.items() if 'loss' in k})
    assert np.isfinite(m['train_loss']) and np.isfinite(m['valid_loss'])
