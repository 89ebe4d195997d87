"""Fused backward of a narrow-in / wide-out 1x1 ConvBN unit (csrc/kernels/conv1x1_bwd.hip,
``Fn.conv1x1_bn_bwd``) against the three-kernel path it replaces.

For every output the error of
  (a) the fused op
against
  (c) an fp32 reference of the same formula with dy NOT rounded to bf16
must not exceed the error of
  (b) Fn.bn_bwd -> Fn.conv2d_dgrad -> Fn.conv2d_wgrad on the same inputs
against (c) by more than a margin.  Errors are max-abs over the reference's RMS.  Margins
(from the number formats, not from what the kernel gives):
  * fp32 outputs (dW, dgamma, dbeta, the previous BN's sums): (a) and (b) add the same bf16
    products in a different order (per-block register accumulators and atomics); a worst-case
    linear fp32 accumulation bound over n <= 1024 rows is n * 2^-24 < 1e-4, far below the
    error both share from rounding dy to bf16 (~2^-9 per term);
  * dx (bf16): one bf16 ulp of the largest reference element, 2^-8 * max|ref| / rms(ref).
(d) is (c) with dy rounded to bf16; it only decides which dx elements are compared when the
previous BN's ReLU mask is applied: an element is excluded where (b)'s stored dx is zero /
non-zero differently from (d)'s (the mask sign, or a value that rounds across zero), and
the excluded share must stay under MASK_CAP.  On the CPU, before any GPU work, the same
share is checked between the two ways the mask pre-activation can round (fused
multiply-add or separate multiply and add).
"""
import itertools

import pytest
import torch

from mlcomp_amd.ops import _lib, functional as Fn

pytestmark = pytest.mark.gpu

CI, CO = 64, 256
MARGIN_F32 = 1e-4
MASK_CAP = 2e-3


def _inputs(nhw, seed):
    g = torch.Generator().manual_seed(seed)
    N, H, W = nhw
    rows = N * H * W
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = {}
    t['dz'] = r(N, H, W, CO).to(torch.bfloat16)
    t['y'] = (r(N, H, W, CO) * 1.5 + 0.3).to(torch.bfloat16)
    t['x'] = r(N, H, W, CI).abs().to(torch.bfloat16)
    t['w'] = (r(CO, 1, 1, CI) * 0.1).to(torch.bfloat16)
    yf = t['y'].float().reshape(rows, CO)
    t['mean'] = yf.mean(0)
    t['invstd'] = (yf.var(0, unbiased=False) + 1e-5).rsqrt()
    t['gamma'] = 0.5 + torch.rand(CO, generator=g)
    # sums as a producer (a dgrad epilogue) leaves them: row chunks spread over the NSTAT copies
    d = t['dz'].float().reshape(rows, CO)
    sums = torch.zeros(Fn.NSTAT, 2, CO)
    for k, idx in enumerate(torch.arange(rows).chunk(min(Fn.NSTAT, rows))):
        sums[k, 0] = d[idx].sum(0)
        sums[k, 1] = (d[idx] * (yf[idx] - t['mean'])).sum(0)
    t['sums'] = sums.reshape(-1)
    t['addend'] = r(N, H, W, CI).to(torch.bfloat16)
    # previous BN: z_prev = relu(y_prev * psc + psh)
    t['py'] = r(N, H, W, CI).to(torch.bfloat16)
    t['pmean'] = t['py'].float().reshape(rows, CI).mean(0)
    t['psc'] = 0.5 + torch.rand(CI, generator=g)
    t['psh'] = r(CI) * 0.3
    t['dw0'] = r(CO, 1, 1, CI)
    return t


def _reference(t, use_addend, use_bn, dw_init, round_dy):
    """(c) (round_dy False) or (d) (True) in fp32 on the CPU."""
    rows = t['y'].numel() // CO
    d = t['dz'].float().reshape(rows, CO)
    sv = t['sums'].view(Fn.NSTAT, 2, CO).sum(0)
    S1, S2 = sv[0], sv[1]
    k1 = t['gamma'] * t['invstd']
    dy = k1 * d - k1 * S1 / rows - k1 * t['invstd'] ** 2 * S2 / rows * (t['y'].float().reshape(rows, CO) - t['mean'])
    if round_dy:
        dy = dy.to(torch.bfloat16).float()
    xf = t['x'].float().reshape(rows, CI)
    dx = dy @ t['w'].float().reshape(CO, CI)
    if round_dy:
        dx = dx.to(torch.bfloat16).float()      # the GEMM epilogues stage the tile as bf16
    if use_addend:
        dx = dx + t['addend'].float().reshape(rows, CI)
    out = {'dgamma': S2 * t['invstd'], 'dbeta': S1,
           'dw': (dy.t() @ xf).reshape(CO, 1, 1, CI) + (t['dw0'] if dw_init else 0)}
    if use_bn:
        pyf = t['py'].float().reshape(rows, CI)
        mask = pyf * t['psc'] + t['psh'] > 0
        dx = dx * mask
        out['mask'] = mask
        out['psums'] = torch.stack([dx.sum(0), (dx * (pyf - t['pmean'])).sum(0)])
    out['dx'] = dx
    return out


def _run(t, dev, fused, use_addend, use_out, use_bn, dw_init, alias=False):
    """(a) (fused True) or (b) on the GPU; returns CPU fp32 tensors."""
    c = {k: v.to(dev) for k, v in t.items()}
    dgamma, dbeta = torch.zeros(CO, device=dev), torch.zeros(CO, device=dev)
    dw = c['dw0'].clone() if dw_init else torch.zeros(CO, 1, 1, CI, device=dev)
    psums = torch.zeros(Fn.NSTAT * 2 * CI, device=dev)
    bn = Fn.BnBwdSpec(None, [(c['py'], c['pmean'], psums)], affine=[(c['psc'], c['psh'])]) if use_bn else None
    addend = c['addend'].clone() if use_addend else None
    out = (addend if alias else torch.full_like(c['x'], float('nan'))) if use_out else None
    if fused:
        dx = Fn.conv1x1_bn_bwd(c['dz'], c['y'], c['x'], c['w'], c['mean'], c['invstd'], c['gamma'], c['sums'],
                               dgamma, dbeta, dw, addend=addend, out=out, bn=bn)
    else:
        dy, _ = Fn.bn_bwd(c['dz'], None, c['y'], c['mean'], c['invstd'], c['gamma'], dgamma=dgamma, dbeta=dbeta,
                          sums=c['sums'], zero_sums=False, prereduced=True)
        dx = Fn.conv2d_dgrad(dy, c['w'], c['x'].shape, addend=addend, out=out, bn=bn)
        Fn.conv2d_wgrad(dy, c['x'], c['w'].shape, out=dw, accumulate=True, slab=False)
    if use_out:
        assert dx.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    res = {'dx': dx.float().cpu().reshape(-1, CI), 'dw': dw.cpu(), 'dgamma': dgamma.cpu(), 'dbeta': dbeta.cpu()}
    if use_bn:
        res['psums'] = psums.cpu().view(Fn.NSTAT, 2, CI).sum(0)
    return res


def _err(got, ref, keep=None):
    e = (got - ref).abs()
    if keep is not None:
        e = e[keep]
    return (e.max() / ref.pow(2).mean().sqrt()).item()


def _check(t, dev, use_addend=False, use_out=False, use_bn=False, dw_init=False, alias=False, tag=''):
    c = _reference(t, use_addend, use_bn, dw_init, round_dy=False)
    a = _run(t, dev, True, use_addend, use_out, use_bn, dw_init, alias)
    b = _run(t, dev, False, use_addend, use_out, use_bn, dw_init, alias)
    keep = None
    if use_bn:
        d = _reference(t, use_addend, use_bn, dw_init, round_dy=True)
        nz_d = d['dx'].to(torch.bfloat16) != 0
        keep = (b['dx'] != 0) == nz_d
        excluded = 1.0 - keep.float().mean().item()
        print(f'{tag} excluded share {excluded:.2e}')
        assert excluded <= MASK_CAP, excluded
        # where (b) and (d) agree, the fused op must have masked the same elements
        assert torch.equal((a['dx'] != 0)[keep], nz_d[keep])
    for name in ('dx', 'dw', 'dgamma', 'dbeta') + (('psums',) if use_bn else ()):
        ref = c[name].reshape(a[name].shape)
        k = keep if name == 'dx' else None
        ea, eb = _err(a[name], ref, k), _err(b[name], ref, k)
        margin = MARGIN_F32
        if name == 'dx':
            margin = 2.0 ** -8 * (ref.abs().max() / ref.pow(2).mean().sqrt()).item()
        print(f'{tag} {name}: fused {ea:.3e} three-kernel {eb:.3e} margin {margin:.1e}')
        assert ea <= eb + margin, (name, ea, eb, margin)


@pytest.fixture(scope='module')
def dev():
    assert Fn.conv1x1_bn_bwd_available(CI, CO)
    return torch.device('cuda')


@pytest.fixture(scope='module')
def t243():
    return _inputs((3, 9, 9), 1)


def test_mask_share_cpu(t243):
    """The mask pre-activation y*sc + sh may round once (fma, emulated in fp64) or twice: the
    two signs differ on far fewer elements than MASK_CAP for these inputs."""
    py = t243['py'].float().reshape(-1, CI)
    two = py * t243['psc'] + t243['psh'] > 0
    one = (py.double() * t243['psc'].double() + t243['psh'].double()).float() > 0
    assert (two != one).float().mean().item() <= MASK_CAP


@pytest.mark.parametrize('nhw', [(2, 7, 7), (3, 9, 9)])
def test_ragged_tail(dev, nhw):
    _check(_inputs(nhw, 2), dev, use_addend=True, use_bn=True, tag=f'ragged{nhw}')


def test_two_blocks_two_tiles_each(dev):
    """544 rows = 9 tiles (the last ragged) over 2 blocks: cross-block atomics on dW and the
    previous BN's sums, accumulators carried over >= 4 tiles per block."""
    lib = _lib.load()
    old = lib.mlc_conv1x1_bwd_get_set(0, 2)
    try:
        _check(_inputs((2, 16, 17), 3), dev, use_addend=True, use_bn=True, dw_init=True, tag='2blocks')
    finally:
        lib.mlc_conv1x1_bwd_get_set(0, old)


def test_epilogue_options(dev, t243):
    for add, out, bn in itertools.product((False, True), repeat=3):
        _check(t243, dev, use_addend=add, use_out=out, use_bn=bn, tag=f'add{int(add)} out{int(out)} bn{int(bn)}')
    # the block-input gradient of a residual block: dx written over its own addend
    _check(t243, dev, use_addend=True, use_out=True, use_bn=True, alias=True, tag='alias')


@pytest.mark.parametrize('dw_init', [False, True])
def test_accumulates_into_gradient_slot(dev, t243, dw_init):
    _check(t243, dev, dw_init=dw_init, tag=f'dw_init{int(dw_init)}')
