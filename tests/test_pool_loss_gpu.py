"""`csrc/kernels/pool_loss.hip` per element: mlc_softmax_ce, mlc_maxpool_*, mlc_avgpool_*, mlc_colsum.

References are fp64 torch on the CPU from the same bits.  bf16 outputs are compared element by
element with the fp64 value rounded to bf16, exactly where the kernel's arithmetic is exact
(max pool) and within one bf16 ulp elsewhere; outputs that must not be written sit inside
sentinel-filled storage.  Measured maxima on an MI355X are in the tests' docstrings.
"""
import pytest
import torch
import torch.nn.functional as F

from mlcomp_amd.ops import _lib
from mlcomp_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS32 = 2.0 ** -23
SENT = -7.5
SENT16 = 0x4243


def _bits(t):
    return t.contiguous().view(torch.int16)


def _bf16_ulp(r):
    """spacing of bf16 (8 significand bits) at |r|, for fp64 r"""
    e = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def _ulps_off(got, ref64):
    """|got - bf16(ref64)| in bf16 ulps of the rounded reference, per element (fp64)"""
    rb = ref64.float().to(torch.bfloat16).double()
    return (got.double() - rb).abs() / _bf16_ulp(rb)


# ------------------------------------------------------------------ softmax cross-entropy
def _ce_ref(logits, labels, V, scale, smoothing):
    """fp64: summed loss, #correct, dlogits [B, V]"""
    lf = logits[:, :V].double()
    lse = torch.logsumexp(lf, 1)
    nll = lse - lf.gather(1, labels[:, None])[:, 0]
    loss = ((1 - smoothing) * nll + smoothing * (lse - lf.mean(1))).sum().item()
    correct = (lf.argmax(1) == labels).sum().item()
    tgt = torch.full_like(lf, smoothing / V)
    tgt[torch.arange(lf.shape[0]), labels] += 1 - smoothing
    return loss, correct, (torch.softmax(lf, 1) - tgt) * scale


def _ce_run(logits, labels, V, scale, smoothing, want_grad=True, with_correct=True):
    B, ld = logits.shape
    loss = torch.full((2,), 2.5, device=DEV)             # pre-loaded: the kernel accumulates
    corr = torch.full((2,), 3.0, device=DEV) if with_correct else None
    d = Fn.softmax_ce(logits.to(DEV), labels.to(DEV), loss, corr, scale=scale, smoothing=smoothing,
                      want_grad=want_grad, num_classes=V)
    torch.cuda.synchronize()
    assert loss[1].item() == 2.5 and (corr is None or corr[1].item() == 3.0)
    return loss[0].item() - 2.5, (corr[0].item() - 3.0 if with_correct else None), (d.cpu() if d is not None else None)


def _ce_check(logits, labels, V, scale, smoothing, tag):
    B, ld = logits.shape
    sc = (1.0 / B) if scale is None else scale
    rl, rc, rd = _ce_ref(logits, labels, V, sc, smoothing)
    gl, gc, gd = _ce_run(logits, labels, V, scale, smoothing)
    off = _ulps_off(gd[:, :V], rd)
    # near zero (softmax minus target cancelling): an absolute bound instead of the ulp
    near0 = (rd.abs() <= 2.0 ** -9 * sc) & ((gd[:, :V].double() - rd).abs() <= 2.0 ** -9 * sc)
    worst = off[~near0].max().item() if bool((~near0).any()) else 0.0
    print(f'GPU_MAXIMA_CE {tag}: loss rel {abs(gl - rl) / rl:.3e}, dlogits worst {worst:.2f} ulp, '
          f'max abs {(gd[:, :V].double() - rd).abs().max().item():.3e}')
    assert abs(gl - rl) / rl < 1e-4, (gl, rl)
    assert gc == rc, (gc, rc)
    assert bool(((off <= 1.0) | near0).all()), worst
    assert bool((_bits(gd[:, V:]) == 0).all())           # padding columns: exactly +0
    return rl, rc, rd


@pytest.mark.parametrize('scale', [None, 0.25])
@pytest.mark.parametrize('smoothing', [0.0, 0.1])
@pytest.mark.parametrize('B,V,ld', [(5, 10, 10), (3, 10, 16), (4, 100, 104), (2, 257, 264), (3, 1000, 1000),
                                    (2, 1000, 1008)])
def test_softmax_ce_per_element(B, V, ld, smoothing, scale):
    """V < 256 (idle lanes), V % 64 != 0, V = 257 (one element in a second pass) and the padded
    form ld > V, whose padding logits are set to 1e30 so that reading them cannot go unseen.
    Measured on an MI355X: loss within 1.0e-7 relative in every case (2.1e-7 in the ties case;
    the fp32 accumulator's own rounding), every dlogits element equal to the rounded fp64 value
    (0 ulp), the near-zero rule never needed."""
    gen = torch.Generator().manual_seed(B * 1000 + V)
    logits = torch.full((B, ld), 1e30)
    logits[:, :V] = torch.randn(B, V, generator=gen) * 3
    labels = torch.randint(0, V, (B,), generator=gen)
    labels[0] = logits[0, :V].argmax()                    # at least one counted row
    _ce_check(logits, labels, V, scale, smoothing, f'{B}x{V}/{ld} s={smoothing} scale={scale}')


def test_softmax_ce_large_magnitude():
    """logits of magnitude 80: exp(80) overflows nothing only because the row maximum is
    subtracted first; the loss must match the fp64 logsumexp."""
    gen = torch.Generator().manual_seed(80)
    B, V, ld = 3, 100, 104
    logits = torch.zeros(B, ld)
    logits[:, :V] = 80.0 * (torch.randint(0, 2, (B, V), generator=gen).float() * 2 - 1) + torch.randn(B, V, generator=gen)
    labels = torch.randint(0, V, (B,), generator=gen)
    _ce_check(logits, labels, V, None, 0.1, 'magnitude 80')


def test_softmax_ce_argmax_ties_take_the_lower_index():
    """Two equal maxima: torch's argmax returns the first and so must the kernel, whether the
    two sit in different waves (70, 200), in one thread's two passes (5, 261) or in one wave
    (3, 40).  With the label on the higher index the row is not counted."""
    B, V = 3, 300
    gen = torch.Generator().manual_seed(3)
    logits = torch.randn(B, V, generator=gen)
    for r, (a, b) in enumerate([(70, 200), (5, 261), (3, 40)]):
        logits[r, a] = logits[r, b] = 9.0
    labels = torch.tensor([200, 261, 3])
    _, rc, _ = _ce_check(logits, labels, V, None, 0.0, 'ties')
    assert rc == 1


def test_softmax_ce_without_grad_and_without_correct():
    gen = torch.Generator().manual_seed(11)
    B, V, ld = 4, 100, 104
    logits = torch.zeros(B, ld)
    logits[:, :V] = torch.randn(B, V, generator=gen) * 3
    labels = logits[:, :V].argmax(1)
    labels[1] = (labels[1] + 1) % V
    rl, rc, rd = _ce_ref(logits, labels, V, 1.0 / B, 0.1)
    gl, gc, gd = _ce_run(logits, labels, V, None, 0.1, want_grad=False)
    assert gd is None and gc == rc == 3 and abs(gl - rl) / rl < 1e-4
    gl, gc, gd = _ce_run(logits, labels, V, None, 0.1, with_correct=False)
    off = _ulps_off(gd[:, :V], rd)
    assert abs(gl - rl) / rl < 1e-4
    near0 = (rd.abs() <= 2.0 ** -9 / B) & ((gd[:, :V].double() - rd).abs() <= 2.0 ** -9 / B)
    assert bool(((off <= 1.0) | near0).all())
    assert bool((_bits(gd[:, V:]) == 0).all())


# ------------------------------------------------------------------ max pool
def _pool_input(kind, shape, gen):
    if kind == 'random':
        x = torch.randn(shape, generator=gen)
    elif kind == 'relu':            # post-ReLU: more than half exact zeros, most windows tie
        x = torch.relu(torch.randn(shape, generator=gen) - 0.3)
    else:                           # all negative: a window overlapping the padding must not give 0
        x = -(torch.rand(shape, generator=gen) + 0.5)
    return x.to(torch.bfloat16)


@pytest.mark.parametrize('kind', ['random', 'relu', 'negative'])
@pytest.mark.parametrize('N,H,W,C,k,s,p', [(2, 12, 12, 64, 3, 2, 1), (1, 7, 9, 8, 3, 2, 1), (2, 13, 13, 16, 3, 2, 0),
                                           (1, 5, 5, 24, 2, 2, 0), (1, 6, 6, 8, 3, 1, 1)])
def test_maxpool_per_element(N, H, W, C, k, s, p, kind):
    """y bit-equal to F.max_pool2d; the window position idx decodes to torch's flat argmax (the
    first maximum in scan order, also among equal zeros); the backward from the GPU's own idx
    equals the fp64 scatter-add rounded once to bf16.  dy holds multiples of 1/64 up to 4, so the
    fp32 sum of the up to k*k contributions of overlapping windows is exact and the comparison
    is element for element."""
    gen = torch.Generator().manual_seed(H * 100 + C)
    x = _pool_input(kind, (N, H, W, C), gen)
    if kind == 'relu':
        assert (x == 0).float().mean().item() > 0.5
    yr, ir = F.max_pool2d(x.permute(0, 3, 1, 2).double(), k, s, p, return_indices=True)
    y, idx = Fn.maxpool_fwd(x.to(DEV), k, s, p)
    torch.cuda.synchronize()
    Ho, Wo = yr.shape[2:]
    assert tuple(y.shape) == (N, Ho, Wo, C)
    assert torch.equal(_bits(y.cpu()), _bits(yr.permute(0, 2, 3, 1).to(torch.bfloat16)))
    if kind == 'negative':
        assert bool((y.cpu().float() < 0).all())
    pos = idx.cpu().long()                                                   # [N, Ho, Wo, C]
    hi = torch.arange(Ho)[None, :, None, None] * s - p + pos // k
    wi = torch.arange(Wo)[None, None, :, None] * s - p + pos % k
    assert bool((pos < k * k).all()) and bool((hi >= 0).all() & (hi < H).all() & (wi >= 0).all() & (wi < W).all())
    flat = hi * W + wi
    assert torch.equal(flat, ir.permute(0, 2, 3, 1))
    dy = (torch.randint(-256, 257, (N, Ho, Wo, C), generator=gen).float() / 64).to(torch.bfloat16)
    dx = Fn.maxpool_bwd(dy.to(DEV), idx, (N, H, W, C), k, s, p)
    torch.cuda.synchronize()
    ref = torch.zeros(N, C, H * W, dtype=torch.float64)
    ref.scatter_add_(2, flat.permute(0, 3, 1, 2).reshape(N, C, -1), dy.double().permute(0, 3, 1, 2).reshape(N, C, -1))
    ref = ref.reshape(N, C, H, W).permute(0, 2, 3, 1).float().to(torch.bfloat16)
    assert torch.equal(dx.cpu().float(), ref.float())      # value for value (a cancelled sum is +0 or -0)
    assert bool((dx.cpu().float() != 0).any())


# ------------------------------------------------------------------ global average pool
@pytest.mark.parametrize('N,HW,C', [(3, 49, 2048), (2, 49, 192), (2, 1, 64), (1, 50, 8), (2, 9, 2056), (1, 4, 4096)])
def test_avgpool_per_element(N, HW, C):
    """C = 192 is 24 channel groups, which does not divide the block (threads past lanes*G idle);
    C = 2056 puts one group into a second slab; HW = 1; the backward with and without addend,
    into a dx inside sentinel-filled storage.  Measured on an MI355X: forward and both backwards
    equal the rounded fp64 value in every element (0 ulp)."""
    gen = torch.Generator().manual_seed(HW * 10000 + C)
    x = torch.randn(N, HW, 1, C, generator=gen).to(torch.bfloat16)
    y = Fn.avgpool_fwd(x.to(DEV))
    torch.cuda.synchronize()
    off = _ulps_off(y.cpu(), x.double().mean(dim=(1, 2)))
    assert off.max().item() <= 1.0, off.max().item()
    dy = torch.randn(N, C, generator=gen).to(torch.bfloat16)
    add = torch.randn(N, HW, 1, C, generator=gen).to(torch.bfloat16)
    worst = [off.max().item()]
    for addend in (None, add):
        lead, numel = 8, N * HW * C
        store = torch.full((lead + numel + 8,), SENT16, dtype=torch.int16, device=DEV)
        dx = store[lead:lead + numel].view(torch.bfloat16)
        dy_d, add_d = dy.to(DEV), (addend.to(DEV) if addend is not None else None)
        _lib.call('mlc_avgpool_bwd', _lib.ptr(dy_d), _lib.ptr(add_d), _lib.ptr(dx), N, HW, C, _lib.stream())
        torch.cuda.synchronize()
        ref = (dy.double() / HW)[:, None, None, :].expand(N, HW, 1, C)
        if addend is not None:
            ref = ref + addend.double()
        off = _ulps_off(dx.cpu().view(N, HW, 1, C), ref)
        worst.append(off.max().item())
        assert off.max().item() <= 1.0, off.max().item()
        assert bool((store[:lead] == SENT16).all()) and bool((store[lead + numel:] == SENT16).all())
        # the library wrapper passes the same arguments
        same = Fn.avgpool_bwd(dy_d, (N, HW, 1, C), addend=add_d)
        assert torch.equal(_bits(same.cpu()).flatten(), _bits(dx.cpu()))
    print(f'GPU_MAXIMA_AVGPOOL {N}x{HW}x{C}: fwd / bwd / bwd+addend worst ulp', ['%.2f' % w for w in worst])


# ------------------------------------------------------------------ column sums
@pytest.mark.parametrize('R,C', [(1, 1), (7, 10), (33, 255), (40, 256), (16, 1000)])
def test_colsum_per_element(R, C):
    """fp32 column sums of a bf16 matrix within the fp32 summation bound R * eps32 * sum|g| of
    the fp64 sum, per column; the elements of ``out`` past C keep their sentinel.  Measured on an
    MI355X: at most 2.4e-7 abs (33 x 255), exact in the other cases."""
    gen = torch.Generator().manual_seed(R * 1000 + C)
    g = torch.randn(R, C, generator=gen).to(torch.bfloat16)
    out = torch.full((C + 8,), SENT, device=DEV)
    Fn.colsum(g.to(DEV), out)
    torch.cuda.synchronize()
    ref = g.double().sum(0)
    tol = R * EPS32 * g.double().abs().sum(0)
    err = (out[:C].cpu().double() - ref).abs()
    print(f'GPU_MAXIMA_COLSUM {R}x{C}: max err {err.max().item():.3e}, min slack {(tol - err).min().item():.3e}')
    assert bool((err <= tol).all()), (err.max().item())
    assert bool((out[C:] == SENT).all())
