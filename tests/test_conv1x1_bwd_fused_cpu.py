"""The fused 1x1 ConvBN backward (MLC_FUSE_1X1_BWD) is a GPU path: on the CPU ``ConvBN.bwd``
must give identical results with the knob on and off, and never reach the fused op."""
import torch

from mlcomp_amd.models import build_model
from mlcomp_amd.ops import functional as Fn
from mlcomp_amd.train.native_step import NativeClassifierStep


def _grads(monkeypatch, on):
    monkeypatch.setattr(Fn, 'FUSE_1X1_BWD', on)

    def boom(*a, **k):
        raise AssertionError('the fused 1x1 backward must not run on the CPU')
    monkeypatch.setattr(Fn, 'conv1x1_bn_bwd', boom)
    torch.manual_seed(0)
    tm = build_model('resnet50', num_classes=16)
    step = NativeClassifierStep(torch_model=tm, batch=4, image_size=32, device='cpu', num_classes=16,
                                lr=0.1, momentum=0.0, weight_decay=0.0, use_graph=False)
    step()
    arena = step.net.arena
    return step.last_loss(), {n: s.grad.clone() for n, s in arena.by_name.items()}


def test_cpu_unaffected_by_knob(monkeypatch):
    l1, g1 = _grads(monkeypatch, True)
    l0, g0 = _grads(monkeypatch, False)
    assert l1 == l0
    assert 'layer1.0.cb3.conv.weight' in g1     # a (64, 256) 1x1 unit the GPU path would fuse
    assert tuple(g1['layer1.0.cb3.conv.weight'].shape) == (256, 1, 1, 64)
    assert g1.keys() == g0.keys()
    for n in g1:
        assert torch.equal(g1[n], g0[n]), n
