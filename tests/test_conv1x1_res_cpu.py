"""The streaming kernel's inference form (MLC_CONV1X1_RES) is a GPU path: on CPU tensors
``Fn.conv1x1_fwd_res`` is ``Fn.conv2d_fwd_res``, a CPU ``NativeInference`` forward never reaches
the kernel library and gives identical logits with the knob on and off, and with the knob off or
too few rows the layer does not select it for a device tensor either."""
import pytest
import torch

from mlcomp_amd.models import build_model
from mlcomp_amd.ops import _lib
from mlcomp_amd.ops import functional as Fn
from mlcomp_amd.ops.layers import ConvBN
from mlcomp_amd.train.native_infer import NativeInference


def _boom(*a, **k):
    raise AssertionError('the kernel library must not be reached here')


@pytest.mark.parametrize('act', [0, 3])
@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('with_bias', [False, True])
def test_cpu_tensors_take_conv2d_fwd_res(monkeypatch, with_bias, with_add, act):
    monkeypatch.setattr(_lib, 'call', _boom)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 7, 128, generator=g).to(torch.bfloat16)
    w = (torch.randn(512, 1, 1, 128, generator=g) * 128 ** -0.5).to(torch.bfloat16)
    b = torch.randn(512, generator=g) if with_bias else None
    add = torch.randn(2, 5, 7, 512, generator=g).to(torch.bfloat16) if with_add else None
    want = Fn.conv2d_fwd_res(x, w, b, add, act)
    got = Fn.conv1x1_fwd_res(x, w, b, add, act)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)
    out = torch.empty_like(want)
    assert Fn.conv1x1_fwd_res(x, w, b, add, act, out=out) is out and torch.equal(out, want)


def _engine(monkeypatch, on):
    monkeypatch.setattr(Fn, 'CONV1X1_RES', on)
    monkeypatch.setattr(Fn, 'CONV1X1_RES_MIN_ROWS', 0)
    monkeypatch.setattr(_lib, 'call', _boom)
    torch.manual_seed(0)
    model = build_model('resnet50', num_classes=16).eval()
    return NativeInference(model, batch=2, image_size=32, device='cpu', use_graph=False)


def test_cpu_engine_unaffected_by_knob(monkeypatch):
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    on = _engine(monkeypatch, True).predict(x)
    off = _engine(monkeypatch, False).predict(x)
    assert on.shape == (2, 16) and torch.isfinite(on).all()
    assert torch.equal(on, off)


class OnDevice:
    """Stand-in for a device tensor of 64 rows of 128 channels."""
    is_cuda = True
    shape = (4, 4, 4, 128)


def _units128(eng):
    units = [u for u in _units(eng.net) if (u.cin_p, u.Co) == (128, 512) and u.k == (1, 1) and u.stride == 1]
    assert len(units) == 4    # conv3 of the four layer2 bottlenecks
    return units


def test_knob_off_never_selects_it(monkeypatch):
    """Off means no, before the kernel library is even consulted."""
    eng = _engine(monkeypatch, False)
    monkeypatch.setattr(Fn, 'conv1x1_fwd_res_available', _boom)
    for u in _units128(eng):
        assert u._conv1x1_res_ok(OnDevice()) is False


def test_too_few_rows_never_select_it(monkeypatch):
    eng = _engine(monkeypatch, True)
    units = _units128(eng)
    monkeypatch.setattr(Fn, 'conv1x1_fwd_res_available', _boom)
    monkeypatch.setattr(Fn, 'CONV1X1_RES_MIN_ROWS', 65)
    for u in units:
        assert u._conv1x1_res_ok(OnDevice()) is False
    # at the threshold the question does go to the library
    monkeypatch.setattr(Fn, 'CONV1X1_RES_MIN_ROWS', 64)
    monkeypatch.setattr(Fn, 'conv1x1_fwd_res_available', lambda ci, co: (ci, co) == (128, 512))
    for u in units:
        assert u._conv1x1_res_ok(OnDevice()) is True


def test_default_thresholds_only_name_instantiated_pairs():
    assert Fn.CONV1X1_RES_MIN_ROWS is None or isinstance(Fn.CONV1X1_RES_MIN_ROWS, int)
    assert set(Fn.CONV1X1_RES_MIN_ROWS_DEFAULT) <= {(128, 512), (256, 1024)}
    assert Fn.conv1x1_res_min_rows(64, 256) is None or Fn.CONV1X1_RES_MIN_ROWS is not None


def _units(net):
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
