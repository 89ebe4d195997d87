"""The fp32 CPU twins of `lm_loss_fwd` / `lm_loss_bwd` and `lm_head_loss` against
`F.cross_entropy` under torch autograd in fp64, and the shape check of the native path."""
import pytest
import torch
import torch.nn.functional as F

from mlcomp_amd.ops import transformer as Tx

T, V, K = 9, 16, 64


def _case():
    gen = torch.Generator().manual_seed(11)
    h = torch.randn(T, K, generator=gen).to(torch.bfloat16)
    w = (torch.randn(V, K, generator=gen) * 0.5).to(torch.bfloat16)
    lab = torch.randint(0, V, (T,), generator=gen)
    lab[2] = lab[6] = -100
    return h, w, lab


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
def test_twins_match_cross_entropy_autograd(reduction):
    h, w, lab = _case()
    h64, w64 = h.double().requires_grad_(), w.double().requires_grad_()
    ref = F.cross_entropy(h64 @ w64.t(), lab, ignore_index=-100, reduction=reduction)
    ref.backward()
    # the op wrappers, dw accumulated onto a non-zero start over chunks of 4 rows
    nll, lse = Tx.lm_loss_fwd(h, w, lab)
    scale = 1.0 / (T - 2) if reduction == 'mean' else 1.0
    dw0 = torch.randn(V, K)
    dw = dw0.clone()
    dh = Tx.lm_loss_bwd(h, w, lab, lse, torch.full((T,), scale), dw, chunk_rows=4)
    assert nll[2] == 0 and nll[6] == 0 and not dh[2].any() and not dh[6].any()
    torch.testing.assert_close(nll.sum().double() * scale, ref.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(lse.double(), (h64 @ w64.t()).logsumexp(1).detach(), rtol=1e-5, atol=1e-5)
    # dlogits and dh are rounded to bf16 once each: 2^-8 relative, twice
    torch.testing.assert_close(dh.double(), h64.grad, rtol=2.0 ** -7, atol=2.0 ** -7 * h64.grad.abs().max().item())
    torch.testing.assert_close((dw - dw0).double(), w64.grad, rtol=2.0 ** -7, atol=2.0 ** -7 * w64.grad.abs().max().item())
    # the autograd entry: fp32 master weight, hidden with a leading shape
    hid, wm = h.view(3, 3, K).clone().requires_grad_(), w.float().requires_grad_()
    loss = Tx.lm_head_loss(hid, wm, lab.view(3, 3), reduction=reduction)
    loss.backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and hid.grad.shape == hid.shape and wm.grad.dtype == torch.float32
    torch.testing.assert_close(loss.double(), ref.detach(), rtol=1e-5, atol=1e-6)
    assert torch.equal(hid.grad.view(T, K), Tx.lm_loss_bwd(h, w, lab, lse, torch.full((T,), scale), dw0.clone()))
    torch.testing.assert_close(wm.grad.double(), w64.grad, rtol=2.0 ** -7, atol=2.0 ** -7 * w64.grad.abs().max().item())


def test_bad_shapes_raise():
    h, w, lab = _case()
    with pytest.raises(ValueError, match='V % 8 == 0'):
        Tx.lm_loss_fwd(h, w[:12].contiguous(), lab)
    with pytest.raises(ValueError, match='K % 64 == 0'):
        Tx.lm_loss_bwd(h[:, :32].contiguous(), w[:, :32].contiguous(), lab, torch.zeros(T), torch.ones(T), torch.zeros(V, 32))
    with pytest.raises(ValueError, match='reduction'):
        Tx.lm_head_loss(h, w, lab, reduction='none')
