"""Grouped-query attention on the CPU: twins against a plain fp64 reference, fx node, lowering, preset."""
import functools
import math

import pytest
import torch
import torch.nn as nn

from mlcomp_amd.models import build_model
from mlcomp_amd.models.native_generic import lower_or_none
from mlcomp_amd.ops import transformer as Tx
from mlcomp_amd.ops.gtransformer import grouped_query_attention

from test_attn_mask_cpu import B_SITE, S_SITE, _check, _site_x
from test_attn_mask_gpu import NEG, _bf, _bias, rel

SALT = 33


@functools.lru_cache(maxsize=None)
def gqa_case(shape, mode):
    """Inputs of one (B, S, H, Hkv, D) case and the fp64 reference's (ctx, lse, dqkv), computed once."""
    B, S, H, Hkv, D = shape
    qkv = _bf(B * S, (H + 2 * Hkv) * D, seed=16, scale=0.7)
    dctx = _bf(B * S, H * D, seed=17)
    kw = dict(key_bias=None, p=0.0, causal='causal' in mode, attn_bias=_bias((B, H, S, S)) if mode == 'bias4d' else None)
    if 'keybias' in mode:
        kw.update(key_bias=torch.zeros(B, S), p=0.1)
        kw['key_bias'][0, S - 37:] = NEG       # right padding: key 0 stays visible to every query
        kw['key_bias'][-1, 1:5] = -2.5         # a finite bias too
    seed = torch.tensor([29], dtype=torch.int32)
    x = qkv.double().requires_grad_(True)
    q, k, v = x.view(B, S, H + 2 * Hkv, D).permute(0, 2, 1, 3).split([H, Hkv, Hkv], 1)
    k, v = k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
    s = q @ k.transpose(-1, -2) / math.sqrt(D)
    if kw['key_bias'] is not None:
        s = s + kw['key_bias'].double()[:, None, None, :]
    if kw['attn_bias'] is not None:
        s = s + kw['attn_bias'].double()
    if kw['causal']:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), NEG)
    P = torch.softmax(s, -1).nan_to_num(0.0)
    if kw['p'] > 0:
        P = torch.where(Tx.keep_mask((B, H, S, S), kw['p'], int(seed), SALT), P / (1 - kw['p']), torch.zeros_like(P))
    ctx = (P @ v).permute(0, 2, 1, 3).reshape(B * S, H * D)
    ctx.backward(dctx.double())
    return qkv, dctx, seed, kw, (ctx.detach(), torch.logsumexp(s, -1).detach().reshape(-1), x.grad)


def gqa_run(shape, mode, dev):
    """One case on ``dev`` against the fp64 reference, with tests/test_attn_mask_gpu.py's bounds."""
    B, S, H, Hkv, D = shape
    qkv, dctx, seed, kw, (ctx_r, lse_r, dq_r) = gqa_case(shape, mode)
    to = lambda t: None if t is None else t.to(dev)
    a = (B, S, H, Hkv, 1.0 / math.sqrt(D), kw['p'], to(seed), SALT)
    m = dict(head_dim=D, causal=kw['causal'], attn_bias=to(kw['attn_bias']))
    ctx, lse = Tx.attn_fwd_gqa(to(qkv), to(kw['key_bias']), *a, **m)
    dq = Tx.attn_bwd_gqa(to(qkv), to(kw['key_bias']), to(dctx), lse, *a, ctx=ctx, **m)
    parts = [(a.float().cpu(), b) for a, b in zip(dq.split([H * D, Hkv * D, Hkv * D], 1), dq_r.split([H * D, Hkv * D, Hkv * D], 1))]
    figures = [rel(ctx, ctx_r), rel(lse, lse_r)] + [rel(got, want) for got, want in parts]
    print(shape, mode, dev, 'rel ctx / lse / dQ / dK / dV:', ' '.join(f'{v:.2e}' for v in figures))
    assert torch.isfinite(dq.float()).all() and torch.isfinite(lse).all()
    assert figures[0] < 1e-2 and figures[1] < 1e-4
    # S = 1: P = 1 and dS = P (dP - sum P dP) = 0, so dQ and dK are exactly zero and have no relative
    # error.  The kernels form dP and sum P dP as two fp32 sums of D products, each within
    # D * 2^-24 * D max|dO| max|v| of the exact value; times scale, max|q or k| and the G heads summed.
    zero_tol = (H // Hkv) * D * D * 2.0 ** -23 / math.sqrt(D) * dctx.float().abs().max() * qkv.float().abs().max() ** 2
    for part, (got, want) in enumerate(parts):   # dQ, dK, dV separately
        if want.abs().max() == 0:
            assert S == 1 and got.abs().max() <= zero_tol, part
        else:
            assert figures[2 + part] < 2e-2, part
    return ctx, lse, dq


@pytest.mark.parametrize('mode', ['none', 'causal', 'bias4d', 'causal+keybias+dropout'])
@pytest.mark.parametrize('shape', [(2, 45, 4, 2, 64), (1, 70, 6, 2, 32)])
def test_twin_matches_fp64_reference(shape, mode):
    gqa_run(shape, mode, 'cpu')


def test_heads_must_divide():
    qkv = torch.zeros(8, (4 + 2 * 3) * 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='no multiple'):
        Tx.attn_fwd_gqa(qkv, None, 1, 8, 4, 3, 0.125)


class GQANet(nn.Module):
    """q / k / v projections (heads 4 / 2), one causal call and one with a float [1, H, S, S] mask."""

    def __init__(self):
        super().__init__()
        # no key bias: softmax is invariant to it, so its gradient is rounding noise around zero
        self.q, self.k, self.v = nn.Linear(16, 64), nn.Linear(16, 32, bias=False), nn.Linear(16, 32)
        self.register_buffer('bias', torch.randn(1, 4, S_SITE, S_SITE, generator=torch.Generator().manual_seed(12)))
        self.head = nn.Linear(64, 3)

    def forward(self, x):
        B, S, _ = x.shape
        sp = lambda t, h: t.reshape(B, S, h, -1).transpose(1, 2)
        q, k, v = sp(self.q(x), 4), sp(self.k(x), 2), sp(self.v(x), 2)
        b = grouped_query_attention(grouped_query_attention(q, k, v, is_causal=True), k, v, attn_mask=self.bias)
        return self.head(b.transpose(1, 2).reshape(B, S, -1).mean(1))


def test_gqa_net_lowers_and_matches_autograd():
    assert lower_or_none(GQANet()) is None
    _check(GQANet, _site_x, {'GQASite': 2})


def test_traces_as_one_node_when_imported_by_name():
    class M(nn.Module):
        def forward(self, q, k, v):
            return grouped_query_attention(q, k, v, is_causal=True)
    gm = torch.fx.symbolic_trace(M())
    assert [n.target for n in gm.graph.nodes if n.op == 'call_function'] == [grouped_query_attention]
    q, k = torch.randn(B_SITE, 4, S_SITE, 16), torch.randn(B_SITE, 2, S_SITE, 16)
    assert torch.equal(gm(q, k, k), M()(q, k, k))


def test_gqa_preset_builds_and_lowers():
    m = build_model('transformer-gqa-tiny', num_classes=4)
    assert m.blocks[0].attn.qkv.out_features == (4 + 2 * 2) * 64
    assert lower_or_none(m) is None
