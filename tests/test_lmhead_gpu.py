"""`csrc/kernels/lmhead.hip` per element: mlc_lmhead_lse and mlc_lmhead_dlogits against a reference
written out in torch fp64 from the bf16 inputs widened to fp64, on guarded storage
(tests/test_transformer_pointwise_gpu.py).  Bounds, with Ez[row] = K 2^-24 max_v sum_k |h[row,k] w[v,k]|
(the worst-case error of an fp32 dot product summed in any order) and e32 = max |fp32 run - fp64 run|
of the same reference:

  lse   |got - ref| <= Ez + 4 e32
  nll   |got - ref| <= 2 Ez + 4 e32
  dl    |got - ref| <= ulp_bf16(ref) + |dnll| p 3 Ez + 4 e32
  ignored rows: nll and dl exactly zero

and `lm_head_loss` / `lm_loss_bwd` on the GPU against their CPU twins."""
import pytest
import torch

from mlcomp_amd.ops import _lib
from mlcomp_amd.ops import transformer as Tx
from test_transformer_pointwise_gpu import BF, DEV, F32, Guarded, _bf, _bits, ulp_bf16

pytestmark = pytest.mark.gpu
F64, IGN = torch.float64, -100


def ref(h, w, lab, dnll, dt):
    """lab, dnll [R, T]: lse [T], nll [R, T], p [T, V], g [R, T, V]"""
    z = h.to(dt) @ w.to(dt).t()
    lse, ign = z.logsumexp(1), lab == IGN
    lc = lab.clamp(0)
    nll = torch.where(ign, torch.zeros((), dtype=dt), lse - z.gather(1, lc.t()).t())
    p = (z - lse[:, None]).exp()
    g = (p - torch.nn.functional.one_hot(lc, w.shape[0]).to(dt)) * torch.where(ign, torch.zeros((), dtype=dt), dnll.to(dt))[..., None]
    return lse, nll, p, g


def check(name, got, want, twin, bound):
    e32 = (twin.double() - want).abs().max().item()
    err = (got.double().cpu().reshape(want.shape) - want).abs()
    tol = bound + 4 * e32
    print(f'LMHEAD {name}: max err/bound {(err / tol).max().item():.3f}, e32 {e32:.3e}, {err.numel()} elements')
    assert bool((err <= tol).all()), (name, int((err > tol).sum()), e32)     # a NaN fails too


@pytest.mark.parametrize('splits', [1, 3])
@pytest.mark.parametrize('K', [64, 192])
@pytest.mark.parametrize('V', [8, 136, 392])
@pytest.mark.parametrize('T', [1, 129])
def test_lmhead_per_element(T, V, K, splits):
    gen = torch.Generator().manual_seed(T * V + K)
    h, w = _bf(T, K, gen=gen), _bf(V, K, gen=gen, scale=4.0 * K ** -0.5)          # logits: std ~ 4
    big = V // 2                       # one vocabulary row whose logits pass 100 in magnitude for half the rows
    w[big] = (w[big].double() * 110.0 / (h.double() @ w[big].double()).abs().median()).to(BF)
    # labels at the first / last column and both sides of the first tile edge; row 0 of repetition 0
    # has its label (V - 1) in the last split and, where its logit is positive, its maximum at `big`;
    # repetition 1 starts the cycle one step on, so the single row of T = 1 is ignored there
    cyc = [c for c in (V - 1, IGN, 0, 127, 128, big) if c < V]
    lab = torch.tensor([[cyc[(t + r) % len(cyc)] for t in range(T)] for r in range(2)])
    R, dnll = 2, torch.randn(2, T, generator=gen)
    (lse64, nll64, p64, g64), (lse32, nll32, _, g32) = ref(h, w, lab, dnll, F64), ref(h, w, lab, dnll, F32)
    Ez = K * 2.0 ** -24 * (h.double().abs() @ w.double().abs().t()).max(1).values
    assert (h.double() @ w[big].double()).abs().max() > 100 and bool((lab == IGN).any())

    sp = min(splits, -(-V // 128))
    assert _lib.load().mlc_lmhead_splits(T, V, splits) == sp
    H, W = Guarded(1, T * K, BF, 8, data=h), Guarded(1, V * K, BF, 8, data=w)
    LAB = Guarded(R, 2 * T, F32, 2, data=lab.view(F32))                      # int64 labels, 8 bytes in
    LSE_IN, DN = Guarded(1, T, F32, 1, data=lse64.float()), Guarded(R, T, F32, 1, data=dnll)
    PART, LSE, NLL = Guarded(R, (2 * sp + 1) * T, F32, 1), Guarded(R, T, F32, 1), Guarded(R, T, F32, 1)
    DL = Guarded(R, T * V, BF, 8)
    for r in range(R):
        _lib.call('mlc_lmhead_lse', H.ptr(), W.ptr(), LAB.ptr(r), PART.ptr(r), LSE.ptr(r), NLL.ptr(r), T, V, K, splits,
                  IGN, _lib.stream())
        _lib.call('mlc_lmhead_dlogits', H.ptr(), W.ptr(), LAB.ptr(r), LSE_IN.ptr(), DN.ptr(r), DL.ptr(r), T, V, K,
                  splits, IGN, _lib.stream())
    torch.cuda.synchronize()
    for name, arr in (('h', H), ('w', W), ('labels', LAB), ('lse in', LSE_IN), ('dnll', DN)):
        arr.untouched(name)
    for name, arr in (('partials', PART), ('lse', LSE), ('nll', NLL), ('dl', DL)):
        arr.written(name)
    check('lse', LSE.cpu(T), lse64.expand(R, T), lse32, Ez)
    check('nll', NLL.cpu(T), nll64, nll32, 2 * Ez)
    check('dl', DL.cpu(T, V), g64, g32, ulp_bf16(g64) + (dnll.double().abs() * 3 * Ez)[..., None] * p64)
    ign = lab == IGN
    assert not NLL.cpu(T)[ign].any() and not _bits(DL.cpu(T, V)[ign]).any(), 'an ignored row is not exactly zero'


def rel(a, b):                         # the comparison of tests/test_transformer_gpu.py
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
def test_lm_head_loss_matches_the_cpu_twin(reduction):
    """T = 160 in chunks of 128 (the second short), dw accumulated onto a non-zero start; dgrad outputs
    within 1e-2, fp32 weight gradients within 1e-3, fp32 sums within 1e-4, as in test_transformer_gpu.py"""
    T, V, K = 160, 136, 64
    gen = torch.Generator().manual_seed(5)
    h, w = _bf(2, T // 2, K, gen=gen), torch.randn(V, K, generator=gen) * 0.5     # fp32 master weight
    lab = torch.randint(0, V, (2, T // 2), generator=gen)
    lab[0, 3] = lab[1, 7] = IGN
    dw0 = torch.randn(V, K, generator=gen)
    out = {}
    for dev in ('cpu', DEV):
        hd, wd = h.detach().to(dev).requires_grad_(), w.detach().to(dev).requires_grad_()
        loss = Tx.lm_head_loss(hd, wd, lab.to(dev), reduction=reduction)
        loss.backward()
        hb, wb, lb = hd.detach().view(T, K), wd.detach().to(BF), lab.to(dev).view(T)
        nll, lse = Tx.lm_loss_fwd(hb, wb, lb)
        dnll = torch.full((T,), 1.0 / (T - 2) if reduction == 'mean' else 1.0, device=dev)
        dw = dw0.clone().to(dev)
        dh = Tx.lm_loss_bwd(hb, wb, lb, lse, dnll, dw, chunk_rows=128)
        assert loss.dtype == F32 and loss.dim() == 0 and hd.grad.shape == h.shape and wd.grad.dtype == F32
        assert rel(hd.grad.view(T, K), dh) < 1e-2, 'autograd and the chunked call differ in dh'
        out[dev] = (loss.detach(), nll.sum(), dh, dw, wd.grad)
    (l_r, n_r, dh_r, dw_r, wg_r), (l_g, n_g, dh_g, dw_g, wg_g) = out['cpu'], out[DEV]
    assert rel(l_g, l_r) < 1e-4 and rel(n_g, n_r) < 1e-4
    assert rel(dh_g, dh_r) < 1e-2 and rel(dw_g, dw_r) < 1e-3 and rel(wg_g, wg_r) < 1e-3
    assert rel(dw_r - dw0, wg_r) < 1e-3, 'dw was not accumulated onto its start'
