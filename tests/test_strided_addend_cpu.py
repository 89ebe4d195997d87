"""CPU path of ``Fn.conv2d_dgrad(..., strided_addend=(t, S))``: the compact [N, Ho, Wo, C]
addend scatter-added at ``dx[:, ::S, ::S]`` must give what the same values give as a
full-resolution ``addend`` with zeros in between: the same dx (``torch.equal``; a -0 that
is no longer added to +0 compares equal) and, with a fused BN-backward reduction, the same
sums, on the shapes and the three reduction modes tests/test_strided_addend_gpu.py uses."""
import pytest
import torch

from mlcomp_amd.ops import functional as Fn

SHAPES = [(2, 7, 7, 2), (1, 6, 10, 2), (2, 7, 7, 3)]
CHANNELS = [(24, 16), (256, 64)]
MODES = ['plain', 'one_y', 'two_y']


def make_inputs(N, H, W, S, C, Co, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    Hs, Ws = (H - 1) // S + 1, (W - 1) // S + 1
    t = {'dy': r(N, H, W, Co).to(torch.bfloat16), 'w': (r(Co, 1, 1, C) * 0.2).to(torch.bfloat16),
         'sadd': r(N, Hs, Ws, C).to(torch.bfloat16)}
    full = torch.zeros(N, H, W, C, dtype=torch.bfloat16)
    full[:, ::S, ::S, :] = t['sadd']
    t['full'] = full
    for k in (0, 1):
        t[f'y{k}'] = r(N, H, W, C).to(torch.bfloat16)
        t[f'mean{k}'] = t[f'y{k}'].float().reshape(-1, C).mean(0)
        t[f'sc{k}'] = 0.5 + torch.rand(C, generator=g)
        t[f'sh{k}'] = r(C) * 0.3
    return t


def make_spec(t, mode, dev):
    """(BnBwdSpec or None, its sums buffers) for a reduction mode."""
    if mode == 'plain':
        return None, []
    C = t['y0'].shape[-1]
    ks = (0,) if mode == 'one_y' else (0, 1)
    sums = [torch.zeros(Fn.NSTAT * 2 * C, device=dev) for _ in ks]
    ys = [(t[f'y{k}'].to(dev), t[f'mean{k}'].to(dev), sums[i]) for i, k in enumerate(ks)]
    aff = [(t[f'sc{k}'].to(dev), t[f'sh{k}'].to(dev)) for k in ks]
    return Fn.BnBwdSpec(None, ys, affine=aff), sums


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('C,Co', CHANNELS)
@pytest.mark.parametrize('N,H,W,S', SHAPES)
def test_cpu_strided_addend_equals_expanded_addend(N, H, W, S, C, Co, mode):
    t = make_inputs(N, H, W, S, C, Co)
    for wt in (None, Fn.wt_flip_transpose(t['w'])):
        bn_a, sums_a = make_spec(t, mode, 'cpu')
        bn_b, sums_b = make_spec(t, mode, 'cpu')
        a = Fn.conv2d_dgrad(t['dy'], t['w'], (N, H, W, C), bn=bn_a, wt=wt, strided_addend=(t['sadd'], S))
        b = Fn.conv2d_dgrad(t['dy'], t['w'], (N, H, W, C), bn=bn_b, wt=wt, addend=t['full'])
        assert a.dtype == torch.bfloat16 and a.shape == (N, H, W, C)
        assert torch.equal(a, b)
        for sa, sb in zip(sums_a, sums_b):
            assert torch.equal(sa, sb)
    if mode == 'plain':   # the addend really is in, and only at the strided pixels
        d = a.float() - Fn.conv2d_dgrad(t['dy'], t['w'], (N, H, W, C)).float()
        assert d[:, ::S, ::S].abs().sum() > 0
        d[:, ::S, ::S] = 0
        assert d.abs().sum() == 0


def test_cpu_strided_addend_on_a_strided_3x3_dgrad():
    """A basic block's first unit (3x3 / stride 2 / pad 1) beside a 1x1 / stride-2 shortcut."""
    N, H, W, S, C, Co = 2, 9, 9, 2, 24, 16
    t = make_inputs(N, H, W, S, C, Co)
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(Co, 3, 3, C, generator=g) * 0.1).to(torch.bfloat16)
    dy = torch.randn(N, 5, 5, Co, generator=g).to(torch.bfloat16)
    for wt in (None, Fn.wt_flip_transpose(w)):
        bn_a, sums_a = make_spec(t, 'two_y', 'cpu')
        bn_b, sums_b = make_spec(t, 'two_y', 'cpu')
        a = Fn.conv2d_dgrad(dy, w, (N, H, W, C), 2, 1, 1, bn=bn_a, wt=wt, strided_addend=(t['sadd'], S))
        b = Fn.conv2d_dgrad(dy, w, (N, H, W, C), 2, 1, 1, bn=bn_b, wt=wt, addend=t['full'])
        assert torch.equal(a, b) and a.abs().sum() > 0
        for sa, sb in zip(sums_a, sums_b):
            assert torch.equal(sa, sb)


def test_cpu_strided_addend_argument_checks():
    t = make_inputs(2, 7, 7, 2, 24, 16)
    with pytest.raises(AssertionError):
        Fn.conv2d_dgrad(t['dy'], t['w'], (2, 7, 7, 24), addend=t['full'], strided_addend=(t['sadd'], 2))
    with pytest.raises(AssertionError):
        Fn.conv2d_dgrad(t['dy'], t['w'], (2, 7, 7, 24), strided_addend=(t['sadd'], 3))   # shape of S = 2
