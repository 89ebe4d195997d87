"""The streaming 1x1 forward (MLC_CONV1X1_FWD) is a GPU path: on the CPU ``ConvBN.fwd`` never
reaches ``Fn.conv1x1_fwd`` and gives identical results with the knob on and off; with the knob
off the layer does not reach it for a device tensor either."""
import torch

from mlcomp_amd.models import build_model
from mlcomp_amd.ops import functional as Fn
from mlcomp_amd.train.native_step import NativeClassifierStep


def _boom(*a, **k):
    raise AssertionError('the streaming 1x1 forward must not run here')


def _step(monkeypatch, on):
    monkeypatch.setattr(Fn, 'CONV1X1_FWD', on)
    monkeypatch.setattr(Fn, 'conv1x1_fwd', _boom)
    torch.manual_seed(0)
    tm = build_model('resnet50', num_classes=16)
    step = NativeClassifierStep(torch_model=tm, batch=4, image_size=32, device='cpu', num_classes=16,
                                lr=0.1, momentum=0.0, weight_decay=0.0, use_graph=False)
    step()
    arena = step.net.arena
    return step, step.last_loss(), {n: s.grad.clone() for n, s in arena.by_name.items()}


def test_cpu_unaffected_by_knob(monkeypatch):
    _, l1, g1 = _step(monkeypatch, True)
    _, l0, g0 = _step(monkeypatch, False)
    assert l1 == l0
    assert tuple(g1['layer2.0.cb3.conv.weight'].shape) == (512, 1, 1, 128)   # a unit the GPU path would take
    assert g1.keys() == g0.keys()
    for n in g1:
        assert torch.equal(g1[n], g0[n]), n


def test_knob_off_never_selects_it(monkeypatch):
    """The selection itself, asked about a (128 -> 512) unit and a tensor that claims to be on the
    device: off means no, before the kernel library is even consulted."""
    step, _, _ = _step(monkeypatch, False)
    monkeypatch.setattr(Fn, 'conv1x1_fwd_available', _boom)
    units = [u for u in _units(step.net) if (u.cin_p, u.Co) == (128, 512) and u.k == (1, 1) and u.stride == 1]
    assert len(units) == 4    # conv3 of the four layer2 bottlenecks

    class OnDevice:
        is_cuda = True
        shape = (4, 4, 4, 128)
    for u in units:
        assert u._conv1x1_fwd_ok(OnDevice()) is False


def _units(net):
    from mlcomp_amd.ops.layers import ConvBN
    seen, out, todo = set(), [], [net]
    while todo:
        o = todo.pop()
        if id(o) in seen:
            continue
        seen.add(id(o))
        if isinstance(o, ConvBN):
            out.append(o)
        elif isinstance(o, (list, tuple)):
            todo.extend(o)
        elif hasattr(o, '__dict__') and type(o).__module__.startswith('mlcomp_amd'):
            todo.extend(v for v in vars(o).values() if not isinstance(v, (torch.Tensor, str, int, float)))
    return out
