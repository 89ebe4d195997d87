"""The compact strided addend of the dgrad epilogue (``mlc_conv_dgrad_sadd`` /
``mlc_conv_dgrad_t_sadd``, EpiBF16 under a StridedAddRows row map, csrc/kernels/igemm.hip)
against the existing exports given the same values zero-expanded to dx's resolution.

A 1x1 / stride-1 dgrad, both filter layouts, three epilogue modes (no BN reduction, the
single-y affine one, the two-y one).  dx must be equal as numbers (``torch.equal``: the
only bit difference allowed is a -0 where the old path added +0).  The BN sums, summed over
their copies, may differ by the order of the fp32 atomics only:
|delta| <= 1.2e-5 * sum|terms|, i.e. 200 additions at 2^-24 relative each (the largest shape
has 98 rows), with sum|terms| taken in float64 from the stored dx and y.

Shapes: 2x7x7 / S=2 (odd size, Ho = 4, 98 rows: a tail tile), 1x6x10 / S=2, 2x7x7 / S=3;
channels 24 <- 16 (column tail) and 256 <- 64 (two column tiles)."""
import ctypes

import pytest
import torch

from mlcomp_amd.ops import _lib, functional as Fn

pytestmark = pytest.mark.gpu

SHAPES = [(2, 7, 7, 2), (1, 6, 10, 2), (2, 7, 7, 3)]
CHANNELS = [(24, 16), (256, 64)]
MODES = ['plain', 'one_y', 'two_y']
SUM_BOUND = 1.2e-5
DEV = 'cuda'


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
    return {k: v.to(DEV) for k, v in t.items()}


def make_spec(t, mode):
    if mode == 'plain':
        return None, []
    C = t['y0'].shape[-1]
    ks = (0,) if mode == 'one_y' else (0, 1)
    sums = [torch.zeros(Fn.NSTAT * 2 * C, device=DEV) for _ in ks]
    ys = [(t[f'y{k}'], t[f'mean{k}'], sums[i]) for i, k in enumerate(ks)]
    return Fn.BnBwdSpec(None, ys, affine=[(t[f'sc{k}'], t[f'sh{k}']) for k in ks]), sums


@pytest.mark.parametrize('transposed', [False, True], ids=['dgrad_sadd', 'dgrad_t_sadd'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('C,Co', CHANNELS)
@pytest.mark.parametrize('N,H,W,S', SHAPES)
def test_strided_addend_equals_expanded_addend(N, H, W, S, C, Co, mode, transposed):
    t = make_inputs(N, H, W, S, C, Co)
    wt = Fn.wt_flip_transpose(t['w']) if transposed else None
    bn_a, sums_a = make_spec(t, mode)
    bn_b, sums_b = make_spec(t, mode)
    out = torch.full((N, H, W, C), float('nan'), device=DEV, dtype=torch.bfloat16)
    a = Fn.conv2d_dgrad(t['dy'], t['w'], (N, H, W, C), bn=bn_a, wt=wt, out=out, strided_addend=(t['sadd'], S))
    b = Fn.conv2d_dgrad(t['dy'], t['w'], (N, H, W, C), bn=bn_b, wt=wt, addend=t['full'])
    torch.cuda.synchronize()
    assert a.data_ptr() == out.data_ptr() and not torch.isnan(a.float()).any()
    assert torch.equal(a, b)
    if mode == 'plain':   # the addend is in, and only at the strided pixels
        d = a.float() - Fn.conv2d_dgrad(t['dy'], t['w'], (N, H, W, C), wt=wt).float()
        assert d[:, ::S, ::S].abs().sum().item() > 0
        d[:, ::S, ::S] = 0
        assert d.abs().sum().item() == 0
    dx = b.double().reshape(-1, C)
    for i, (sa, sb) in enumerate(zip(sums_a, sums_b)):
        got, want = sa.view(Fn.NSTAT, 2, C).sum(0).double(), sb.view(Fn.NSTAT, 2, C).sum(0).double()
        yc = t[f'y{i}'].double().reshape(-1, C) - t[f'mean{i}'].double()
        terms = torch.stack([dx.abs().sum(0), (dx * yc).abs().sum(0)])
        worst = ((got - want).abs() / terms.clamp_min(1e-30)).max().item()
        print(f'sums{i}: worst |delta| / sum|terms| = {worst:.3e} (bound {SUM_BOUND:.1e})')
        assert ((got - want).abs() <= SUM_BOUND * terms).all(), worst
        assert want.abs().sum().item() > 0


@pytest.mark.parametrize('name', ['mlc_conv_dgrad_sadd', 'mlc_conv_dgrad_t_sadd'])
def test_strided_addend_argument_checks(name):
    """S < 1, rows that are no multiple of 8 elements (the addend's rows are dx's: C), and both
    addend forms at once are refused before anything is launched."""
    fn = getattr(_lib.load(), name)

    def rc(C, S, both):
        N, H, W, Co = 1, 4, 4, 16
        dy = torch.zeros(N, H, W, Co, device=DEV, dtype=torch.bfloat16)
        w = torch.zeros(Co * C, device=DEV, dtype=torch.bfloat16)
        dx = torch.zeros(N, H, W, C, device=DEV, dtype=torch.bfloat16)
        sadd = torch.zeros(N, H, W, C, device=DEV, dtype=torch.bfloat16)   # large enough for any S >= 1
        none = [None] * 11
        r = fn(_lib.ptr(dy), _lib.ptr(w), _lib.ptr(dx), _lib.ptr(dx) if both else None, _lib.ptr(sadd),
               ctypes.c_int(S), N, H, W, C, Co, 1, 1, 1, 0, 1, H, W, *none, _lib.stream())
        torch.cuda.synchronize()
        return r

    assert rc(16, 2, False) == 0
    assert rc(16, 1, False) == 0
    assert rc(16, 0, False) != 0
    assert rc(16, -2, False) != 0
    assert rc(12, 2, False) != 0
    assert rc(16, 2, True) != 0
