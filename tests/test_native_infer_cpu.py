"""The native inference engine on the CPU reference paths: the residual conv epilogue's twin,
BatchNorm folding, NativeInference's static-buffer protocol and the ``engine`` keyword of the
inference helpers."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from mlcomp_amd.models import build_model
from mlcomp_amd.ops import functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cos(a, b):
    a, b = a.flatten().float(), b.flatten().float()
    return (a @ b / (a.norm() * b.norm() + 1e-12)).item()


def _randomize_bn(model, seed=3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.3)
    return model


@pytest.mark.parametrize('act', [0, 3])
@pytest.mark.parametrize('with_addend', [False, True])
@pytest.mark.parametrize('k,s,p', [(3, 1, 1), (1, 1, 0), (3, 2, 1)])
def test_conv2d_fwd_res_twin_is_fp32_rounded_once(k, s, p, act, with_addend):
    g = torch.Generator().manual_seed(k * 10 + s)
    x = torch.randn(2, 9, 9, 16, generator=g).to(torch.bfloat16)
    w = (torch.randn(24, k, k, 16, generator=g) * 0.2).to(torch.bfloat16)
    b = torch.randn(24, generator=g)
    Ho, Wo = Fn.conv_out_hw(9, 9, k, k, s, p, 1)
    add = torch.randn(2, Ho, Wo, 24, generator=g).to(torch.bfloat16) if with_addend else None
    z = Fn.conv2d_fwd_res(x, w, b, add, act, s, p, 1)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), b, s, p).permute(0, 2, 3, 1)
    if add is not None:
        ref = ref + add.float()
    if act == 3:
        ref = torch.relu(ref)
    assert z.dtype == torch.bfloat16 and z.shape == (2, Ho, Wo, 24)
    assert torch.equal(z, ref.to(torch.bfloat16))


def test_convbn_fold_reproduces_eval_bn_of_conv():
    """w_fold / b_fold against the fp32 torch modules in eval mode.  No per-unit ConvBN eval test
    exists to borrow a tolerance from (the eval tests bound whole models by a cosine), so the
    bounds come from the number formats: w_fold is w * scale rounded to bf16 once (relative
    error <= 2^-8 per element, half an ulp of 7 mantissa bits), b_fold is fp32 (1e-6 relative;
    dropping eps = 1e-5 at variances of 0.5-1.5 moves it by 3e-6 or more), and bn(conv(x)) on the
    folded operands in fp32 differs from the modules' only by the rounding of w_fold."""
    from mlcomp_amd.ops.layers import ConvBN, NativeContext
    torch.manual_seed(0)
    conv = nn.Conv2d(16, 40, 3, 1, 1, bias=False)
    bn = _randomize_bn(nn.BatchNorm2d(40)).eval()
    ctx = NativeContext()
    unit = ConvBN(ctx, 'u', conv, bn, act=False)
    ctx.finalize('cpu')
    unit.load_from_torch()
    ctx.arena.decay.refresh_mirror()
    ctx.training, ctx.deploy = False, True
    x = torch.randn(2, 11, 11, 16).to(torch.bfloat16)
    z, _ = unit.fwd(x)
    w_fold, b_fold = unit._fold
    assert w_fold.dtype == torch.bfloat16 and b_fold.dtype == torch.float32
    with torch.no_grad():
        scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        w_want = conv.weight.double().permute(0, 2, 3, 1) * scale.view(-1, 1, 1, 1)
        b_want = bn.bias.double() - bn.running_mean.double() * scale
        assert ((w_fold.double() - w_want).abs() <= 2.0 ** -8 * w_want.abs() + 1e-30).all()
        assert ((b_fold.double() - b_want).abs() <= 1e-6 * (b_want.abs() + (bn.running_mean.double() * scale).abs())).all()
        want = bn(conv(x.float().permute(0, 3, 1, 2))).permute(0, 2, 3, 1)
        folded = F.conv2d(x.float().permute(0, 3, 1, 2), w_fold.float().permute(0, 3, 1, 2), b_fold, 1, 1)
        folded = folded.permute(0, 2, 3, 1)
    assert ((folded - want).norm() / want.norm()).item() < 2.0 ** -8
    # the unit's own output: that fp32 result rounded to bf16 once more (2^-8 + 2^-8)
    assert ((z.float() - want).norm() / want.norm()).item() < 2.0 ** -7
    # deferred residuals and loader transforms are training constructs
    with pytest.raises(AssertionError):
        unit.fwd(x, res=(z, b_fold, b_fold))


@pytest.fixture(scope='module')
def engine():
    from mlcomp_amd.train.native_infer import NativeInference
    torch.manual_seed(0)
    model = _randomize_bn(build_model('resnet18', num_classes=10)).eval()
    return NativeInference(model, batch=2, image_size=32, device='cpu')


def test_native_inference_rows_are_independent(engine):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 32, 32, generator=g)
    full = engine.predict(x)
    assert full.shape == (2, 10) and full.dtype == torch.float32
    engine.predict(torch.randn(2, 3, 32, 32, generator=g))      # leaves other rows behind
    one = engine.predict(x[:1])                                  # row 1 of the buffer is stale
    assert torch.equal(one, full[:1])
    with torch.no_grad():
        want = engine.torch_model(x)
    assert _cos(full, want) > 0.999
    with pytest.raises(ValueError):
        engine.predict(torch.randn(3, 3, 32, 32))


def test_native_inference_refold_after_load_state_dict(engine):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 32, 32, generator=g)
    before = engine.predict(x)
    folds = [u._fold[0].clone() for u in engine.net._units() if u._fold is not None]
    assert folds, 'no unit was folded'
    other = _randomize_bn(build_model('resnet18', num_classes=10), seed=11)
    engine.load_state_dict({'model_state_dict': other.state_dict()})
    after = engine.predict(x)
    now = [u._fold[0] for u in engine.net._units() if u._fold is not None]
    assert any(not torch.equal(a, b) for a, b in zip(folds, now))     # a stale cache would be equal
    assert not torch.equal(before, after)
    with torch.no_grad():
        want = other.eval()(x)
    assert _cos(after, want) > 0.999


_PLAIN_EVAL = """
import sys, torch
sys.path.insert(0, {root!r})
from mlcomp_amd.models import build_model
from mlcomp_amd.models.native_resnet import NativeResNet
from mlcomp_amd.ops import functional as Fn
torch.manual_seed(0)
net = NativeResNet(build_model('resnet18', num_classes=10), 'cpu').eval()
x = Fn.nchw_to_nhwc(torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(7)), pad_to=8)
with torch.no_grad():
    out = net.logits(x).float()
assert 'mlcomp_amd.train.native_infer' not in sys.modules
torch.save(out, {out!r})
"""


def test_deploy_off_leaves_eval_logits_bitwise(tmp_path):
    """NativeResNet's eval logits with the engine module imported (deploy off) equal, bit for
    bit, what a process that never imported it computes."""
    import mlcomp_amd.train.native_infer  # noqa: F401
    from mlcomp_amd.models.native_resnet import NativeResNet
    out = str(tmp_path / 'plain.pt')
    subprocess.run([sys.executable, '-c', _PLAIN_EVAL.format(root=ROOT, out=out)], check=True, timeout=300)
    torch.manual_seed(0)
    net = NativeResNet(build_model('resnet18', num_classes=10), 'cpu').eval()
    assert net.ctx.deploy is False
    x = Fn.nchw_to_nhwc(torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(7)), pad_to=8)
    with torch.no_grad():
        got = net.logits(x).float()
    assert torch.equal(got, torch.load(out))
    assert all(u._fold is None for u in net._units())


class _Arr(torch.utils.data.Dataset):
    def __init__(self, x):
        self.x = x

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return {'features': self.x[i]}


def test_torch_infer_engine_keyword(tmp_path, monkeypatch):
    from mlcomp_amd.utils import torch_infer
    from mlcomp_amd.utils.torch_infer import infer
    monkeypatch.setattr(torch_infer, '_device', lambda: torch.device('cpu'))     # the CPU paths, wherever this runs
    torch.manual_seed(0)
    m = build_model('SimpleCNN', num_classes=3, width=4).eval()
    path = str(tmp_path / 'net.pth')
    torch.jit.save(torch.jit.trace(m, torch.randn(1, 3, 8, 8)), path)
    X = torch.randn(10, 3, 8, 8)
    with torch.no_grad():
        want = torch.softmax(m(X), 1).numpy()
    default = infer(_Arr(X), path, batch_size=4, activation='softmax')
    named = infer(_Arr(X), path, batch_size=4, activation='softmax', engine='torch')
    assert default.shape == (10, 3)
    assert (default == named).all()
    assert abs(default - want).max() < 1e-6
    with pytest.raises(RuntimeError, match='no HIP device'):
        infer(_Arr(X), path, batch_size=4, engine='native', model=build_model('resnet18', num_classes=3))
    # auto falls back to the TorchScript path
    assert (infer(_Arr(X), path, batch_size=4, activation='softmax', engine='auto') == default).all()
    with pytest.raises(ValueError):
        infer(_Arr(X), path, engine='fast')


def test_native_inference_names_what_it_cannot_lower():
    from mlcomp_amd.train.native_infer import NativeInference
    from mlcomp_amd.train.native_spec import NativeUnsupported
    with pytest.raises(NativeUnsupported, match='SimpleCNN'):
        NativeInference(build_model('SimpleCNN', num_classes=3, width=4), 2, 8, device='cpu')


def test_classifier_step_predict_is_the_unfolded_eval_path():
    from mlcomp_amd.train.native_step import NativeClassifierStep
    step = NativeClassifierStep(model_name='resnet18', batch=2, image_size=32, device='cpu', num_classes=10,
                                use_graph=False)
    x = torch.randn(2, 3, 32, 32)
    got = step.predict(x)
    step.net.eval()
    with torch.no_grad():
        want = step.net.logits(step._prep(Fn.nchw_to_nhwc(x, pad_to=8))).float()
    step.net.train()
    assert torch.equal(got, want) and got.dtype == torch.float32
    assert step.net.ctx.training and not step.net.ctx.deploy


def _executor_from_yaml(tmp_path, text):
    """An equation executor built the way a DAG builds it: YAML -> Executor.from_config."""
    import yaml
    from mlcomp_amd.worker.executors import Executor
    from mlcomp_amd.worker.executors.valid import Valid

    @Executor.register
    class ValidYamlProbe(Valid):
        def score(self, preds):
            return 0

        def score_final(self):
            return 0

    cfg = yaml.safe_load(text)
    return Executor.from_config(executor='valid', config=cfg, additional_info={}, session=None, logger=None,
                                logger_db=None)


def test_equation_executor_engine_keys_from_yaml(tmp_path, monkeypatch, capsys):
    """engine / model_spec / checkpoint reach the executor from the YAML and are no equations;
    the checkpoint resolves through the model folder; engine: auto goes back to the traced file
    with the reason when the checkpoint is missing or there is no device, engine: native raises."""
    monkeypatch.setenv('MLCOMP_ROOT', str(tmp_path / 'mlcomp'))
    from mlcomp_amd import config
    config.reset()
    folder = config.get().MODEL_FOLDER
    os.makedirs(folder, exist_ok=True)
    torch.manual_seed(0)
    m = build_model('resnet18', num_classes=10).eval()
    torch.jit.save(torch.jit.trace(m, torch.randn(1, 3, 32, 32), check_trace=False), os.path.join(folder, 'net.pth'))
    X = torch.randn(6, 3, 32, 32)
    with torch.no_grad():
        want = m(X).numpy()
    yml = """
info: {{name: d, project: p}}
executors:
  valid:
    type: valid_yaml_probe
    y: torch(x, file='net.pth', batch_size=4)
    engine: {engine}
    model_spec: {{name: resnet18, num_classes: 10}}
    {extra}
    depends: train
"""
    ex = _executor_from_yaml(tmp_path, yml.format(engine='auto', extra=''))
    assert ex.engine == 'auto' and ex.model_spec == {'name': 'resnet18', 'num_classes': 10} and ex.checkpoint is None
    assert set(ex.equations) == {'y'}
    ex.x = _Arr(X)
    # no net_weight.pth: auto falls back and says why
    got = ex.solve('y', (0, 6))
    assert 'engine: auto runs the torch path' in capsys.readouterr().out
    if not torch.cuda.is_available():
        assert abs(got - want).max() < 1e-5
    # native with the same missing checkpoint raises, naming the file
    ex = _executor_from_yaml(tmp_path, yml.format(engine='native', extra=''))
    ex.x = _Arr(X)
    with pytest.raises(RuntimeError, match='net_weight.pth'):
        ex.solve('y', (0, 6))
    # an explicit checkpoint in the model folder resolves; without a device auto still falls back
    torch.save({'model_state_dict': m.state_dict()}, os.path.join(folder, 'best.pth'))
    ex = _executor_from_yaml(tmp_path, yml.format(engine='auto', extra='checkpoint: best.pth'))
    assert ex.checkpoint == 'best.pth'
    assert ex.resolve_model_file(ex.checkpoint) == os.path.join(folder, 'best.pth')
    ex.x = _Arr(X)
    got = ex.solve('y', (0, 6))
    if not torch.cuda.is_available():
        assert 'no HIP device' in capsys.readouterr().out
        assert abs(got - want).max() < 1e-5
        ex = _executor_from_yaml(tmp_path, yml.format(engine='native', extra='checkpoint: best.pth'))
        ex.x = _Arr(X)
        with pytest.raises(RuntimeError, match='no HIP device'):
            ex.solve('y', (0, 6))
    config.reset()


def test_torch_infer_native_declines_before_the_first_batch(monkeypatch):
    """What the native path can decline is decided inside infer(), not while the caller iterates:
    batch_mode returns a generator, and auto must already have fallen back by then."""
    from mlcomp_amd.utils import torch_infer
    from mlcomp_amd.train.native_spec import NativeUnsupported
    monkeypatch.setattr(torch_infer, '_native_model', lambda model, *a: model)    # as if a device were there
    monkeypatch.setattr(torch_infer, '_device', lambda: torch.device('cpu'))
    m = build_model('resnet18', num_classes=3).eval()
    flat = _Arr(torch.randn(4, 12))                       # not NCHW images
    with pytest.raises(RuntimeError, match='engine: native cannot run'):
        torch_infer.infer(flat, None, batch_size=2, engine='native', model=m, batch_mode=True)

    def boom(*a, **k):
        raise NativeUnsupported('engine construction failed')
    monkeypatch.setattr(torch_infer, '_native_engine', boom)
    X = torch.randn(4, 3, 32, 32)
    out = torch_infer.infer(_Arr(X), None, batch_size=2, engine='auto', model=m)      # falls back, runs
    with torch.no_grad():
        assert abs(out - m(X).numpy()).max() < 1e-5
