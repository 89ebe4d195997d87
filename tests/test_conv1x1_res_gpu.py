"""Inference form of the weight-stationary streaming 1x1 kernel (csrc/kernels/conv1x1_fwd.hip,
``Fn.conv1x1_fwd_res``) against the igemm path it replaces (``Fn.conv2d_fwd_res``): z equal
element for element with and without bias, addend and ReLU, nothing written outside z, an addend
with wider rows never read past its channels, and the ResNet-50 engine dispatching its ten
channel-expanding conv3 units to it with unchanged logits.

Shapes as in test_conv1x1_fwd_gpu.py (rows = N * H * W; 64-row tiles, one 256-channel chunk per
block): 126 rows (no multiple of the tile), 1 row, 507 rows, 6272 rows (98 whole tiles) and
``full`` = (2 * groups - 1) * 64 + 1 rows with groups = CUs / (Co / 256), the smallest row count
at which every block of a full grid gets two tiles and the last tile is partial."""
import pytest
import torch
import torch.nn.functional as F

from mlcomp_amd.models import build_model
from mlcomp_amd.ops import _lib
from mlcomp_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu

DEV = 'cuda'
PAIRS = [(128, 512), (256, 1024)]
SHAPES = {'126': (2, 7, 9), '1': (1, 1, 1), '507': (3, 13, 13), '6272': (8, 28, 28), 'full': None}
BM, CHUNK = 64, 256
_cache = {}


def _shape(name, Co):
    if SHAPES[name] is not None:
        return SHAPES[name]
    groups = torch.cuda.get_device_properties(0).multi_processor_count // (Co // CHUNK)
    return (1, 1, (2 * groups - 1) * BM + 1)


def _case(Ci, Co, name):
    """Operands, computed once per (pair, shape) and left unchanged; the igemm results are added
    per (addend, act, bias) combination as they are first asked for."""
    key = (Ci, Co, name)
    if key not in _cache:
        N, H, W = _shape(name, Co)
        g = torch.Generator().manual_seed(Ci + 7 * N * H * W)
        x = torch.randn(N, H, W, Ci, generator=g).to(torch.bfloat16).to(DEV)
        w = (torch.randn(Co, 1, 1, Ci, generator=g) * Ci ** -0.5).to(torch.bfloat16).to(DEV)
        b = torch.randn(Co, generator=g).to(DEV)
        add = torch.randn(N, H, W, Co, generator=g).to(torch.bfloat16).to(DEV)
        conv = F.conv2d(x.permute(0, 3, 1, 2).float(), w.permute(0, 3, 1, 2).float()).permute(0, 2, 3, 1)
        _cache[key] = dict(x=x, w=w, b=b, add=add, conv=conv, igemm={})
    return _cache[key]


def _operands(c, with_add, with_bias):
    return (c['b'] if with_bias else None), (c['add'] if with_add else None)


def _igemm(c, with_add, act, with_bias):
    key = (with_add, act, with_bias)
    if key not in c['igemm']:
        b, add = _operands(c, with_add, with_bias)
        c['igemm'][key] = Fn.conv2d_fwd_res(c['x'], c['w'], b, add, act)
        torch.cuda.synchronize()
    return c['igemm'][key]


def _check(Ci, Co, name, with_add=True, act=3, with_bias=True):
    c = _case(Ci, Co, name)
    want = _igemm(c, with_add, act, with_bias)
    b, add = _operands(c, with_add, with_bias)
    rows = want.numel() // Co
    buf = torch.full(((rows + BM) * Co,), -7.0, device=DEV, dtype=torch.bfloat16)   # one tile of slack
    z = Fn.conv1x1_fwd_res(c['x'], c['w'], b, add, act, out=buf[:rows * Co].view(want.shape))
    torch.cuda.synchronize()
    # value equality: the two zeros compare equal and, the operands being finite, nothing else
    assert torch.isfinite(z.float()).all()
    assert torch.equal(z, want)
    assert torch.all(buf[rows * Co:] == -7.0)
    ref = c['conv']
    if with_bias:
        ref = ref + c['b']
    if with_add:
        ref = ref + c['add'].float()
    if act == 3:
        ref = ref.clamp_min(0)
    err = ((z.float() - ref).norm() / (ref.norm() + 1e-12)).item()
    print(f'conv1x1_fwd_res {Ci}>{Co} rows {rows} addend={with_add} act={act} bias={with_bias}: rel {err:.3e}')
    assert err < 1e-2
    return z


@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('act', [0, 3])
@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('name', list(SHAPES))
@pytest.mark.parametrize('Ci,Co', PAIRS)
def test_equals_igemm(Ci, Co, name, with_add, act, with_bias):
    """Also the tail writes: the output lies in a buffer with one tile of slack filled with -7,
    which is untouched afterwards."""
    _check(Ci, Co, name, with_add, act, with_bias)


@pytest.mark.parametrize('Ci,Co', PAIRS)
def test_addend_with_wider_rows(Ci, Co):
    """The addend is the leading Co channels of a [rows, Co + 64] buffer that ends with its last
    row; the other columns hold 1e4 and must never reach the sum."""
    c = _case(Ci, Co, '507')
    dense = _check(Ci, Co, '507')
    wide = torch.full((*c['add'].shape[:-1], Co + 64), 1e4, device=DEV, dtype=torch.bfloat16)
    wide[..., :Co] = c['add']
    z = Fn.conv1x1_fwd_res(c['x'], c['w'], c['b'], wide[..., :Co], 3)
    torch.cuda.synchronize()
    assert torch.equal(z, dense)


@pytest.mark.parametrize('Ci,Co', PAIRS)
def test_few_blocks_walk_many_tiles(Ci, Co):
    """Grid capped to 3 blocks (whole row groups: one block per 256-channel chunk at the least),
    so one block walks all 98 tiles of the 6272 rows."""
    lib = _lib.load()
    old = lib.mlc_conv1x1_fwd_get_set(0, 3)
    try:
        _check(Ci, Co, '6272')
    finally:
        lib.mlc_conv1x1_fwd_get_set(0, old)


def test_ok_reports_instantiations():
    lib = _lib.load()
    for Ci, Co in PAIRS:
        assert Fn.conv1x1_fwd_res_available(Ci, Co)
    for Ci, Co in [(64, 64), (512, 2048), (128, 500)]:
        assert not Fn.conv1x1_fwd_res_available(Ci, Co)
    # nothing in the kernel is unordered: deterministic mode keeps it, unlike the training form
    was, copies = lib.mlc_get_deterministic(), lib.mlc_get_stat_copies()
    lib.mlc_set_deterministic(1, max(copies, 1))
    try:
        assert lib.mlc_get_deterministic() == 1
        assert not lib.mlc_conv1x1_fwd_ok(128, 512)
        for Ci, Co in PAIRS:
            assert Fn.conv1x1_fwd_res_available(Ci, Co)
        _check(128, 512, '126')
    finally:
        lib.mlc_set_deterministic(was, copies)
    assert lib.mlc_get_deterministic() == was and lib.mlc_get_stat_copies() == copies


def _randomize_bn(model, seed=3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.3)
    return model


def test_engine_dispatches_ten_units(monkeypatch):
    """ResNet-50 at 4 x 64^2: with the knob on and no row threshold, conv3 of layer 2's four and
    layer 3's six bottlenecks run the streaming kernel, and the logits are those of the igemm
    path, eager and replayed from the graph."""
    from mlcomp_amd.train.native_infer import NativeInference
    torch.manual_seed(0)
    model = _randomize_bn(build_model('resnet50', num_classes=16)).eval()
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    calls = []
    real = Fn.conv1x1_fwd_res

    def spy(x, w, *a, **k):
        calls.append((w.shape[-1], w.shape[0]))
        return real(x, w, *a, **k)
    monkeypatch.setattr(Fn, 'conv1x1_fwd_res', spy)

    monkeypatch.setattr(Fn, 'CONV1X1_RES', False)
    off = NativeInference(model, batch=4, image_size=64, device=DEV, use_graph=False)
    want = off.predict(x).cpu()
    assert calls == []

    monkeypatch.setattr(Fn, 'CONV1X1_RES', True)
    monkeypatch.setattr(Fn, 'CONV1X1_RES_MIN_ROWS', 0)
    eager = NativeInference(model, batch=4, image_size=64, device=DEV, use_graph=False)
    got = eager.predict(x).cpu()
    assert sorted(calls) == [(128, 512)] * 4 + [(256, 1024)] * 6
    assert torch.isfinite(got).all() and torch.equal(got, want)

    graphed = NativeInference(model, batch=4, image_size=64, device=DEV, use_graph=True)
    outs = [graphed.predict(x).cpu() for _ in range(3)]   # eager warm-up, capture + replay, replay
    assert graphed.graph is not None, graphed.capture_error
    for o in outs:
        assert torch.equal(o, want)
