"""The native inference engine on the MI355X: the residual conv epilogue against the fp32
reference, ``mlc_conv_fwd_ex`` against bytes recorded from the library before the residual
epilogue existed, NativeInference's graph / short-batch protocol, and the folded model's
logits error against the two existing inference paths."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from mlcomp_amd.models import build_model
from mlcomp_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_fwd_ex_parent.npz')
# test_generic_gpu's bound for mlc_conv_fwd_ex against its CPU twin (the fp32 result rounded to
# bf16 once): what is left is accumulation order flipping a last bit here and there
KERNEL_REL = 8e-3


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _bf(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


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


# 3x3 with an M tail and Co no tile multiple; the 1x1 fast path with an M tail; a strided 3x3
SHAPES = [(2, 9, 9, 16, 72, 3, 1, 1), (3, 14, 14, 64, 256, 1, 1, 0), (2, 15, 15, 32, 40, 3, 2, 1)]


@pytest.mark.parametrize('act', [0, 3])
@pytest.mark.parametrize('with_addend', [False, True])
@pytest.mark.parametrize('N,H,W,C,Co,k,s,p', SHAPES)
def test_conv_res_kernel_vs_fp32(N, H, W, C, Co, k, s, p, with_addend, act):
    g = torch.Generator().manual_seed(N * 100 + Co)
    x, w, b = _bf(g, N, H, W, C), _bf(g, Co, k, k, C, scale=0.2), torch.randn(Co, generator=g)
    Ho, Wo = Fn.conv_out_hw(H, W, k, k, s, p, 1)
    add = _bf(g, N, Ho, Wo, Co) if with_addend else None
    ref = Fn.conv2d_fwd_res(x, w, b, add, act, s, p, 1)         # fp32 math, one bf16 rounding
    z = Fn.conv2d_fwd_res(x.to(DEV), w.to(DEV), b.to(DEV), add.to(DEV) if with_addend else None, act, s, p, 1)
    torch.cuda.synchronize()
    err = rel(z, ref)
    print(f'conv_res {(N, H, W, C, Co, k, s, p)} addend={with_addend} act={act}: rel {err:.3e}')
    assert z.shape == ref.shape and err < KERNEL_REL
    if act == 3:
        assert (z.float() >= 0).all()


def test_conv_res_kernel_addend_with_wider_rows():
    """lda > Co: the addend is the leading channels of a wider buffer; the columns behind it hold
    large values that must never be read into the sum."""
    g = torch.Generator().manual_seed(9)
    N, H, W, C, Co = 2, 9, 9, 16, 72
    x, w, b = _bf(g, N, H, W, C), _bf(g, Co, 3, 3, C, scale=0.2), torch.randn(Co, generator=g)
    wide = _bf(g, N, H, W, Co + 24)
    wide[..., Co:] = 1000.0
    ref = Fn.conv2d_fwd_res(x, w, b, wide[..., :Co], 3, 1, 1, 1)
    z = Fn.conv2d_fwd_res(x.to(DEV), w.to(DEV), b.to(DEV), wide.to(DEV)[..., :Co], 3, 1, 1, 1)
    torch.cuda.synchronize()
    assert rel(z, ref) < KERNEL_REL


def test_conv_fwd_ex_bytes_unchanged():
    """mlc_conv_fwd_ex on two shapes (general path with bias + ReLU, 1x1 fast path with bias):
    bitwise the output recorded from the kernel library built before mlc_conv_fwd_res was added
    (inputs and outputs in tests/golden/conv_fwd_ex_parent.npz, bf16 as int16)."""
    rec = np.load(GOLDEN)
    for tag, act, k, s, p in (('a', 3, 3, 1, 1), ('b', 0, 1, 1, 0)):
        x = torch.from_numpy(rec[f'{tag}_x']).view(torch.bfloat16).to(DEV)
        w = torch.from_numpy(rec[f'{tag}_w']).view(torch.bfloat16).to(DEV)
        b = torch.from_numpy(rec[f'{tag}_b']).to(DEV)
        y = Fn.conv2d_fwd_ex(x, w, b, act, s, p, 1)
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().view(torch.int16).numpy(), rec[f'{tag}_y']), tag


@pytest.fixture(scope='module')
def engines():
    from mlcomp_amd.train.native_infer import NativeInference
    torch.manual_seed(0)
    model = _randomize_bn(build_model('resnet18', num_classes=10)).eval()
    graphed = NativeInference(model, batch=4, image_size=64, device=DEV, use_graph=True)
    eager = NativeInference(model, batch=4, image_size=64, device=DEV, use_graph=False)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(4, 3, 64, 64, generator=g) for _ in range(3)]
    with torch.no_grad():
        refs = [model(x) for x in xs]
    return graphed, eager, xs, refs


def test_native_inference_graph_replay_equals_eager(engines):
    graphed, eager, xs, refs = engines
    outs = [graphed.predict(x).cpu() for x in xs]          # eager warm-up, capture + replay, replay
    assert graphed.graph is not None, graphed.capture_error
    for x, out, ref in zip(xs, outs, refs):
        assert torch.equal(out, eager.predict(x).cpu())
        # ~20 conv units of 2-3 bf16 roundings each (2^-9 relative, rms ~1.1e-3) adding up at
        # random: sqrt(60) * 1.1e-3 ~ 9e-3, times three for the spread between inputs
        assert rel(out, ref) < 3e-2
    # different inputs gave different outputs: the static buffer is refreshed on every call
    assert not torch.equal(outs[1], outs[2])


def test_native_inference_short_batch(engines):
    graphed, eager, xs, refs = engines
    full = graphed.predict(xs[0]).cpu()
    graphed.predict(xs[1])
    short = graphed.predict(xs[0][:3]).cpu()               # row 3 of the buffer is stale
    assert short.shape == (3, 10) and torch.equal(short, full[:3])


@pytest.fixture(scope='module')
def numerics():
    """Relative logits error against fp32 PyTorch eval, ResNet-50 at 4 x 64^2, same weights and
    input: (a) folded, (b) the existing unfolded native eval path, (c) TorchScript under bf16
    autocast.  Measured once per run and shared."""
    from mlcomp_amd.train.native_infer import NativeInference
    torch.manual_seed(0)
    model = _randomize_bn(build_model('resnet50', num_classes=100)).eval()
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        ref = model(x)
    eng = NativeInference(model, batch=4, image_size=64, device=DEV, use_graph=False)
    a = rel(eng.predict(x), ref)
    eng.net.ctx.deploy = False                              # the existing unfolded eval path
    b = rel(eng.predict(x), ref)
    traced = torch.jit.trace(model.to(DEV), x.to(DEV), check_trace=False)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        c = rel(traced(x.to(DEV).contiguous(memory_format=torch.channels_last)).float(), ref)
    model.cpu()
    return a, b, c


def test_folded_model_numerics_vs_existing_paths(numerics):
    """The folded path's error may exceed the larger of the two existing paths' by at most 25 %.
    TorchScript autocast measures ten times the native paths' error here, so that bound alone
    would let the folded path be far worse than the unfolded one it replaces: it is also held
    to 25 % over the unfolded native path by itself (the same margin: folding trades the
    rounding of y for one of w * scale, two roundings of the same pass)."""
    a, b, c = numerics
    text = (f'resnet50 4x64^2 relative logits error vs fp32 eval: folded {a:.4e}  unfolded native {b:.4e}  '
            f'torchscript bf16 autocast {c:.4e}')
    print(text)
    if os.environ.get('MLC_NUMERICS_OUT'):
        with open(os.environ['MLC_NUMERICS_OUT'], 'w') as f:
            f.write(text + '\n')
    assert a <= 1.25 * max(b, c), text
    assert a <= 1.25 * b, text


def test_torch_infer_native_follows_the_modules_weights():
    """infer(model=m, engine='native') folds m's weights as they are at the call: after the
    caller changes them, the next call predicts from the new ones."""
    from mlcomp_amd.utils.torch_infer import infer

    class DS(torch.utils.data.Dataset):
        x = torch.randn(6, 3, 64, 64, generator=torch.Generator().manual_seed(8))

        def __len__(self):
            return 6

        def __getitem__(self, i):
            return {'features': self.x[i]}

    torch.manual_seed(0)
    m = _randomize_bn(build_model('resnet18', num_classes=10)).eval()
    first = infer(DS(), None, batch_size=4, model=m, engine='native')
    m.load_state_dict(_randomize_bn(build_model('resnet18', num_classes=10), seed=12).state_dict())
    second = infer(DS(), None, batch_size=4, model=m, engine='native')
    with torch.no_grad():
        want = m(DS.x)
    assert not np.array_equal(first, second)
    assert rel(torch.from_numpy(second), want) < 3e-2       # the bound of the graph test above


def test_equation_executor_engine_native_agrees_with_torch(tmp_path, numerics):
    """A ``valid`` equation executor with ``engine: native`` (model_spec + the checkpoint beside
    the traced file) against the same executor on the default torch engine: same argmax on every
    row whose fp32 top-2 margin (relative to the row's norm) is at least the model-numerics error
    this run measured for the folded path (the ``numerics`` fixture; the smallest of its three
    figures, so the fewest rows are let off); at most 2 % of the rows may fall under that margin."""
    from mlcomp_amd.worker.executors.valid import Valid

    class V(Valid):
        def score(self, preds):
            return 0

        def score_final(self):
            return 0

    torch.manual_seed(0)
    m = _randomize_bn(build_model('resnet18', num_classes=10)).eval()
    with torch.no_grad():
        m.fc.weight.mul_(8.0)                               # spread the logits
    net = str(tmp_path / 'net.pth')
    torch.jit.save(torch.jit.trace(m, torch.randn(1, 3, 64, 64), check_trace=False), net)
    torch.save({'model_state_dict': m.state_dict()}, str(tmp_path / 'net_weight.pth'))
    X = torch.randn(96, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref = m(X)

    class DS(torch.utils.data.Dataset):
        def __init__(self, a=0, b=len(X)):
            self.a, self.b = a, b

        def __len__(self):
            return self.b - self.a

        def __getitem__(self, i):
            return {'features': X[self.a + i]}

    def run(**kw):
        eq = V(y=f'torch(x, file={net!r}, batch_size=40)', part_size=48, **kw)
        eq.x = DS()
        outs = []
        for part in eq.parts():
            eq.begin_part(part)
            eq.x = DS(*part)
            outs.append(eq.solve('y', part))
        return np.concatenate(outs)

    p_torch = run()
    p_native = run(engine='native', model_spec={'name': 'resnet18', 'num_classes': 10})
    top2 = ref.topk(2, dim=1).values
    keep = (((top2[:, 0] - top2[:, 1]) / ref.norm(dim=1)) >= numerics[0]).numpy()
    print(f'excluded {int((~keep).sum())} of {len(X)} rows; disagreements '
          f'{int((p_torch.argmax(1) != p_native.argmax(1)).sum())}')
    assert (~keep).mean() <= 0.02
    assert (p_torch.argmax(1)[keep] == ref.argmax(1).numpy()[keep]).all()
    assert (p_native.argmax(1)[keep] == p_torch.argmax(1)[keep]).all()
