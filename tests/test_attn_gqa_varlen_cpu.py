"""Packed grouped-query attention on the CPU: the twins against fp64 attention per sequence."""
import functools
import math

import pytest
import torch

from mlcomp_amd.ops import transformer as Tx

from test_attn_mask_gpu import _bf, rel

SALT = 33
MODES = {'none': (False, 0.0), 'causal': (True, 0.0), 'causal+dropout': (True, 0.1)}


@functools.lru_cache(maxsize=None)
def packed_case(lengths, T, max_len, heads, mode):
    """Inputs of one case and the fp64 per-sequence reference's (ctx, lse, dqkv), computed once."""
    (H, Hkv, D), (causal, p) = heads, MODES[mode]
    qkv, dctx = _bf(T, (H + 2 * Hkv) * D, seed=16, scale=0.7), _bf(T, H * D, seed=17)
    cu = torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32)
    seed = torch.tensor([29], dtype=torch.int32)
    x = qkv.double().requires_grad_(True)
    ctx, lse = torch.zeros(T, H * D, dtype=torch.float64), torch.zeros(H, T, dtype=torch.float64)
    for b, c0, c1 in Tx._seq_slices(cu):
        L = c1 - c0
        q, k, v = x[c0:c1].view(L, H + 2 * Hkv, D).transpose(0, 1).split([H, Hkv, Hkv])
        s = q @ k.repeat_interleave(H // Hkv, 0).transpose(-1, -2) / math.sqrt(D)
        if causal:
            s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float('-inf'))
        P = torch.softmax(s, -1)
        if p > 0:
            P = torch.where(Tx._seq_keep(b, H, L, max_len, p, seed, SALT), P / (1 - p), torch.zeros_like(P))
        ctx[c0:c1] = (P @ v.repeat_interleave(H // Hkv, 0)).transpose(0, 1).reshape(L, H * D)
        lse[:, c0:c1] = torch.logsumexp(s, -1).detach()
    ctx.backward(dctx.double())
    return qkv, dctx, cu, seed, (ctx.detach(), lse.reshape(-1), x.grad)


def packed_run(lengths, T, max_len, heads, mode, dev, dq_bound=2e-2):
    """One case on ``dev`` against the fp64 reference, with ``gqa_run``'s bounds."""
    (H, Hkv, D), (causal, p) = heads, MODES[mode]
    qkv, dctx, cu, seed, (ctx_r, lse_r, dq_r) = packed_case(lengths, T, max_len, heads, mode)
    a = (H, Hkv, 1.0 / math.sqrt(D), p, seed.to(dev), SALT)
    ctx, lse = Tx.attn_fwd_gqa_varlen(qkv.to(dev), cu, max_len, *a, head_dim=D, causal=causal)
    dq = Tx.attn_bwd_gqa_varlen(qkv.to(dev), cu, max_len, dctx.to(dev), lse, *a, head_dim=D, ctx=ctx, causal=causal)
    cols = [H * D, Hkv * D, Hkv * D]
    figures = [rel(ctx, ctx_r), rel(lse, lse_r)] + [rel(g, w) for g, w in zip(dq.split(cols, 1), dq_r.split(cols, 1))]
    print(lengths, heads, mode, dev, 'rel ctx / lse / dQ / dK / dV:', ' '.join(f'{v:.2e}' for v in figures))
    assert torch.isfinite(dq.float()).all() and torch.isfinite(lse).all()
    assert figures[0] < 1e-2 and figures[1] < 1e-4 and max(figures[2:]) < dq_bound, figures
    # a length-1 sequence has dQ = dK = 0 exactly: gqa_run's rounding bound for what the kernels leave there
    zero_tol = (H // Hkv) * D * D * 2.0 ** -23 / math.sqrt(D) * dctx.float().abs().max() * qkv.float().abs().max() ** 2
    for b, c0, c1 in Tx._seq_slices(cu):
        if c1 - c0 == 1:
            assert dq_r[c0, :(H + Hkv) * D].abs().max() == 0 and dq[c0, :(H + Hkv) * D].float().abs().max() <= zero_tol
    end = int(cu[-1])   # rows of no sequence: exact zeros
    assert not ctx[end:].any() and not dq[end:].any() and not lse.view(H, T)[:, end:].any()
    return ctx, lse, dq


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('lengths,T,max_len,heads', [((1, 0, 45, 70), 120, 70, (4, 2, 64)), ((33, 20), 53, 40, (6, 2, 32))])
def test_twin_matches_fp64_reference(lengths, T, max_len, heads, mode):
    packed_run(lengths, T, max_len, heads, mode, 'cpu')


def test_twin_backward_is_autograd_of_the_plain_composition():
    """The reference gradient is torch.autograd's through repeat_interleave + softmax; the fp32 twin differs
    from it by its one rounding to bf16, half an ulp = 2^-9 relative per element: 2^-8 on the norms."""
    packed_run((1, 0, 45, 70), 120, 70, (4, 2, 64), 'causal+dropout', 'cpu', dq_bound=2.0 ** -8)


def test_refusals():
    qkv, cu = torch.zeros(8, (4 + 2 * 2) * 64, dtype=torch.bfloat16), torch.tensor([0, 8], dtype=torch.int32)
    for bad in (dict(Hkv=3), dict(key_bias=torch.zeros(1, 8)), dict(attn_bias=torch.zeros(8, 8)),
                dict(cu=torch.tensor([0, 9], dtype=torch.int32)), dict(cu=torch.tensor([0, 5, 3], dtype=torch.int32))):
        kw = {k: v for k, v in bad.items() if k.endswith('bias')}
        with pytest.raises(ValueError):
            Tx.attn_fwd_gqa_varlen(qkv, bad.get('cu', cu), 8, 4, bad.get('Hkv', 2), 0.125, **kw)
        with pytest.raises(ValueError):
            Tx.attn_bwd_gqa_varlen(qkv, bad.get('cu', cu), 8, qkv[:, :256], torch.zeros(32), 4, bad.get('Hkv', 2),
                                   0.125, **kw)
