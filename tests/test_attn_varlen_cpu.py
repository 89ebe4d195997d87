"""Packed variable-length attention, CPU side: the fp32 twin of ``attn_fwd_varlen`` /
``attn_bwd_varlen`` against ``F.scaled_dot_product_attention`` per sequence (forward and
autograd), against the padded twin with a -inf key bias under dropout (same dropped
elements), the wrapper's validation of ``cu_seqlens``, and the zero rows of empty slots and
of the unused tail."""
import math

import pytest
import torch
import torch.nn.functional as F

from mlcomp_amd.ops import transformer as Tx

NEG = float('-inf')


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return float(a @ b / (a.norm() * b.norm() + 1e-20))


def _inputs(T, H, D, seed=3):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(T, 3 * H * D, generator=g) * 0.5).to(torch.bfloat16)
    dctx = torch.randn(T, H * D, generator=g).to(torch.bfloat16)
    return qkv, dctx


def _cu(lengths):
    return torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32)


def _twin(qkv, dctx, cu, max_len, H, D, p=0.0, causal=False, seed=None):
    scale = 1.0 / math.sqrt(D)
    ctx, lse = Tx.attn_fwd_varlen(qkv, cu, max_len, H, scale, p, seed, 9, head_dim=D, causal=causal)
    dqkv = Tx.attn_bwd_varlen(qkv, cu, max_len, dctx, lse, H, scale, p, seed, 9, head_dim=D, ctx=ctx, causal=causal)
    return ctx, lse, dqkv


@pytest.mark.parametrize('causal', [False, True])
def test_twin_matches_sdpa_per_sequence(causal):
    lengths, H, D = [45, 1, 0, 70, 17], 3, 64
    T = sum(lengths) + 4
    qkv, dctx = _inputs(T, H, D)
    cu = _cu(lengths)
    ctx, lse, dqkv = _twin(qkv, dctx, cu, max(lengths), H, D, causal=causal)
    assert torch.isfinite(lse).all()
    for c0, c1 in zip(cu[:-1].tolist(), cu[1:].tolist()):
        L = c1 - c0
        if not L:
            continue
        x = qkv[c0:c1].float().requires_grad_(True)
        q, k, v = x.view(1, L, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
        o = F.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(1, 2).reshape(L, H * D)
        o.backward(dctx[c0:c1].float())
        # the bounds tests/test_attn_mask_cpu.py holds the padded twin to against SDPA
        assert (ctx[c0:c1].float() - o.detach()).abs().max().item() < 2e-2
        if L > 1:
            assert _cos(dqkv[c0:c1], x.grad) > 0.999
        else:   # one key: dQ = dK = 0, dV = dO
            assert _cos(dqkv[c0:c1, 2 * H * D:], x.grad[:, 2 * H * D:]) > 0.999
            assert dqkv[c0:c1, :2 * H * D].abs().max().item() == 0


@pytest.mark.parametrize('causal', [False, True])
def test_twin_with_dropout_equals_the_padded_twin(causal):
    """p = 0.1: the packed call drops exactly the elements the padded call over the same
    sequences at S = max_len drops, so the real rows agree."""
    lengths, H, D, S = [20, 0, 7, 1, 33], 2, 64, 40
    T, B = sum(lengths) + 3, len(lengths)
    qkv, dctx = _inputs(T, H, D, seed=5)
    cu = _cu(lengths)
    seed = torch.tensor([77], dtype=torch.int32)
    ctx, lse, dqkv = _twin(qkv, dctx, cu, S, H, D, p=0.1, causal=causal, seed=seed)
    pq, pd, kb = torch.zeros(B, S, 3 * H * D, dtype=torch.bfloat16), torch.zeros(B, S, H * D, dtype=torch.bfloat16), \
        torch.zeros(B, S)
    for b, n in enumerate(lengths):
        c0 = int(cu[b])
        pq[b, :n], pd[b, :n] = qkv[c0:c0 + n], dctx[c0:c0 + n]
        kb[b, n:] = NEG
    scale = 1.0 / math.sqrt(D)
    pq, pd = pq.view(B * S, -1), pd.view(B * S, -1)
    pctx, plse = Tx.attn_fwd(pq, kb, B, S, H, scale, 0.1, seed, 9, head_dim=D, causal=causal)
    pdq = Tx.attn_bwd(pq, kb, pd, plse, B, S, H, scale, 0.1, seed, 9, head_dim=D, ctx=pctx, causal=causal)
    dropped = 0
    for b, n in enumerate(lengths):
        if not n:
            continue
        c0 = int(cu[b])
        assert torch.allclose(ctx[c0:c0 + n].float(), pctx.view(B, S, -1)[b, :n].float(), atol=1e-6, rtol=1e-5)
        assert torch.allclose(dqkv[c0:c0 + n].float(), pdq.view(B, S, -1)[b, :n].float(), atol=1e-6, rtol=1e-5)
        assert torch.allclose(lse.view(H, T)[:, c0:c0 + n], plse.view(B, H, S)[b, :, :n], atol=1e-6, rtol=1e-5)
        dropped += int((~Tx._seq_keep(b, H, n, S, 0.1, seed, 9)).sum())
    assert dropped > 0      # the mask did drop something


def test_wrapper_validates_cu_seqlens():
    H, D, T = 2, 64, 32
    qkv, dctx = _inputs(T, H, D)
    ok = _cu([10, 0, 12])
    Tx.attn_fwd_varlen(qkv, ok, 12, H, 0.125, head_dim=D)
    bad = {'non-decreasing': torch.tensor([0, 12, 10, 20], dtype=torch.int32),
           'past': _cu([10, 12, 11]),
           'max_len': _cu([10, 13])}
    for match, cu in bad.items():
        with pytest.raises(ValueError, match=match):
            Tx.attn_fwd_varlen(qkv, cu, 12, H, 0.125, head_dim=D)
        with pytest.raises(ValueError, match=match):
            Tx.attn_bwd_varlen(qkv, cu, 12, dctx, torch.zeros(H * T), H, 0.125, head_dim=D, ctx=dctx)
    with pytest.raises(ValueError, match='start at 0'):
        Tx.attn_fwd_varlen(qkv, torch.tensor([2, 12], dtype=torch.int32), 12, H, 0.125, head_dim=D)
    for kw in ({'key_bias': torch.zeros(3, 12)}, {'attn_bias': torch.zeros(12, 12)}):
        with pytest.raises(ValueError, match='key_bias / attn_bias'):
            Tx.attn_fwd_varlen(qkv, ok, 12, H, 0.125, head_dim=D, **kw)
        with pytest.raises(ValueError, match='key_bias / attn_bias'):
            Tx.attn_bwd_varlen(qkv, ok, 12, dctx, torch.zeros(H * T), H, 0.125, head_dim=D, ctx=dctx, **kw)


def test_empty_slots_and_tail_rows_are_zero():
    lengths, H, D = [0, 9, 0, 0, 14, 0], 2, 64
    T = sum(lengths) + 9
    qkv, dctx = _inputs(T, H, D, seed=8)
    ctx, lse, dqkv = _twin(qkv, dctx, _cu(lengths), 16, H, D)
    assert ctx[23:].abs().max().item() == 0 and dqkv[23:].abs().max().item() == 0
    assert lse.view(H, T)[:, 23:].abs().max().item() == 0 and torch.isfinite(lse).all()
    assert ctx[:23].abs().min(1)[0].max().item() > 0 and dqkv[:23].abs().sum().item() > 0
    # an all-empty batch: nothing but zeros
    ctx, lse, dqkv = _twin(qkv, dctx, _cu([0, 0]), 16, H, D)
    assert ctx.abs().max().item() == 0 and dqkv.abs().max().item() == 0 and lse.abs().max().item() == 0
