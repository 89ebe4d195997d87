"""Causal and additive attention masks, CPU path: the fp32 twins of ``attn_fwd`` / ``attn_bwd``
against fp32 ``F.scaled_dot_product_attention`` and its autograd, and the lowering of
GPT-style ``is_causal=True`` attention, SDPA with ``attn_mask=`` and ``nn.MultiheadAttention``
with ``attn_mask`` + ``key_padding_mask`` onto the native sites (forward and every parameter
gradient against the fp32 PyTorch model).

Bool-mask polarity follows torch: SDPA takes part where True, MultiheadAttention masks out
where True.  Masks are constants (no gradient)."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from mlcomp_amd.models import build_model
from mlcomp_amd.models.native_generic import GenericNet, lower_or_none
from mlcomp_amd.ops import gtransformer as GT
from mlcomp_amd.ops import transformer as Tx

from test_gtransformer_cpu import _CausalNet, _check, _cos

NEG = float('-inf')


# ---------------------------------------------------------------------------- op layer
def _inputs(B, S, H, D, seed=3):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * S, 3 * H * D, generator=g) * 0.5).to(torch.bfloat16)
    dctx = torch.randn(B * S, H * D, generator=g).to(torch.bfloat16)
    return qkv, dctx


def _sdpa_reference(qkv, dctx, B, S, H, D, mask, causal):
    """fp32 torch SDPA + autograd on the same bf16-rounded inputs: (ctx [B*S, E], dqkv)."""
    x = qkv.float().requires_grad_(True)
    q, k, v = x.view(B, S, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, is_causal=causal)
    o = o.transpose(1, 2).reshape(B * S, H * D)
    o.backward(dctx.float())
    return o.detach(), x.grad


def _twin(qkv, dctx, kb, B, S, H, D, **masks):
    scale = 1.0 / math.sqrt(D)
    ctx, lse = Tx.attn_fwd(qkv, kb, B, S, H, scale, head_dim=D, **masks)
    dqkv = Tx.attn_bwd(qkv, kb, dctx, lse, B, S, H, scale, head_dim=D, ctx=ctx, **masks)
    return ctx, lse, dqkv


def _assert_close(ctx, dqkv, want_ctx, want_grad):
    # the bounds tests/test_bert_cpu.py holds the unmasked twin to
    assert (ctx.float() - want_ctx).abs().max().item() < 2e-2
    assert _cos(dqkv, want_grad) > 0.999


def test_twin_causal_matches_sdpa():
    B, S, H, D = 2, 70, 3, 64
    qkv, dctx = _inputs(B, S, H, D)
    ctx, lse, dqkv = _twin(qkv, dctx, None, B, S, H, D, causal=True)
    _assert_close(ctx, dqkv, *_sdpa_reference(qkv, dctx, B, S, H, D, None, True))
    assert torch.isfinite(lse).all()


def test_twin_float_bias_2d_matches_sdpa():
    B, S, H, D = 2, 45, 2, 64
    qkv, dctx = _inputs(B, S, H, D, seed=4)
    bias = torch.randn(S, S, generator=torch.Generator().manual_seed(5))
    ctx, _, dqkv = _twin(qkv, dctx, None, B, S, H, D, attn_bias=bias)
    _assert_close(ctx, dqkv, *_sdpa_reference(qkv, dctx, B, S, H, D, bias, False))


@pytest.mark.parametrize('shape', ['BHSS', 'B1SS', '1HSS', 'flat'])
def test_twin_4d_bias_with_inf_matches_sdpa(shape):
    B, S, H, D = 2, 33, 3, 32
    qkv, dctx = _inputs(B, S, H, D, seed=6)
    g = torch.Generator().manual_seed(7)
    b, h = {'BHSS': (B, H), 'B1SS': (B, 1), '1HSS': (1, H), 'flat': (B, H)}[shape]
    bias = torch.randn(b, h, S, S, generator=g)
    drop = torch.rand(b, h, S, S, generator=g) < 0.3
    drop &= ~torch.eye(S, dtype=torch.bool)          # every row keeps its diagonal: none fully masked
    bias = bias.masked_fill(drop, NEG)
    given = bias.reshape(B * H, S, S) if shape == 'flat' else bias
    ctx, _, dqkv = _twin(qkv, dctx, None, B, S, H, D, attn_bias=given)
    _assert_close(ctx, dqkv, *_sdpa_reference(qkv, dctx, B, S, H, D, bias, False))


def test_twin_causal_with_right_padding_matches_sdpa():
    B, S, H, D = 3, 50, 2, 64
    qkv, dctx = _inputs(B, S, H, D, seed=8)
    kb = torch.zeros(B, S)
    kb[0, 40:] = NEG                                 # right padding: key 0 is always visible
    kb[2, 7:] = NEG
    ctx, _, dqkv = _twin(qkv, dctx, kb, B, S, H, D, causal=True)
    full = torch.zeros(S, S).masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), NEG) + kb[:, None, None, :]
    _assert_close(ctx, dqkv, *_sdpa_reference(qkv, dctx, B, S, H, D, full, False))


def test_twin_fully_masked_row_is_zero():
    B, S, H, D = 1, 20, 2, 64
    qkv, dctx = _inputs(B, S, H, D, seed=9)
    bias = torch.zeros(S, S)
    bias[5] = NEG
    ctx, lse, dqkv = _twin(qkv, dctx, None, B, S, H, D, attn_bias=bias)
    assert ctx.view(B, S, H * D)[0, 5].abs().max().item() == 0
    assert (lse.view(B, H, S)[:, :, 5] == float('inf')).all() and torch.isfinite(lse.view(B, H, S)[:, :, 4]).all()
    assert torch.isfinite(dqkv.float()).all()
    assert dqkv.view(B, S, 3, H * D)[0, 5, 0].abs().max().item() == 0      # its dQ row


def test_defaults_are_the_unmasked_twin():
    B, S, H, D = 2, 24, 2, 64
    qkv, dctx = _inputs(B, S, H, D, seed=10)
    kb = torch.zeros(B, S)
    kb[1, 20:] = NEG
    a = _twin(qkv, dctx, kb, B, S, H, D)
    b = _twin(qkv, dctx, kb, B, S, H, D, causal=False, attn_bias=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match='attn_bias shape'):
        Tx.attn_fwd(qkv, None, B, S, H, 0.125, attn_bias=torch.zeros(3, S, S))


# ---------------------------------------------------------------------------- lowering
def _tiny_causal():
    return build_model('transformer-causal-tiny', num_classes=3, dropout=0.0)


def _tiny_ids():
    return torch.randint(0, 1024, (3, 24), generator=torch.Generator().manual_seed(1))


S_SITE, B_SITE = 12, 3


def _nonsym_mask(S=S_SITE):
    """A bool [S, S] pattern that is not its own transpose and whose column 0 and diagonal are
    False, so either polarity reading leaves every row something to attend to."""
    g = torch.Generator().manual_seed(11)
    m = torch.rand(S, S, generator=g) < 0.4
    m |= torch.ones(S, S, dtype=torch.bool).triu(S // 2)
    m[:, 0] = False
    m &= ~torch.eye(S, dtype=torch.bool)
    m[1:, -1] |= True
    m[-1, -1] = False
    assert not torch.equal(m, m.t())
    return m


class _SDPAMaskNet(nn.Module):
    """q/k/v projections + SDPA with ``attn_mask`` (a buffer: bool True = takes part, or float),
    then a second SDPA with a float [1, H, S, S] mask."""

    def __init__(self, mask=None, heads=2, dim=64):
        super().__init__()
        self.heads = heads
        # no key bias: softmax is invariant to it, so its gradient is rounding noise around zero
        self.q, self.k, self.v = nn.Linear(16, dim), nn.Linear(16, dim, bias=False), nn.Linear(16, dim)
        self.register_buffer('mask', ~_nonsym_mask() if mask is None else mask)
        g = torch.Generator().manual_seed(12)
        self.register_buffer('bias', torch.randn(1, heads, S_SITE, S_SITE, generator=g))
        self.head = nn.Linear(dim, 3)

    def forward(self, x):
        B, S, _ = x.shape
        sp = lambda t: t.reshape(B, S, self.heads, -1).transpose(1, 2)
        q, k, v = sp(self.q(x)), sp(self.k(x)), sp(self.v(x))
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=self.mask)
        b = F.scaled_dot_product_attention(a, k, v, attn_mask=self.bias)
        return self.head(b.transpose(1, 2).reshape(B, S, -1).mean(1))


class _MHAMaskNet(nn.Module):
    """nn.MultiheadAttention (batch-first) with a 2-D ``attn_mask`` (bool True = masked out, or
    float) and a right-padding ``key_padding_mask``."""

    def __init__(self, mask=None):
        super().__init__()
        self.inp = nn.Linear(16, 64)
        self.attn = nn.MultiheadAttention(64, 2, batch_first=True)
        self.register_buffer('mask', _nonsym_mask() if mask is None else mask)
        pad = torch.zeros(B_SITE, S_SITE, dtype=torch.bool)
        pad[1, 9:] = True
        pad[2, 4:] = True
        self.register_buffer('pad', pad)
        self.head = nn.Linear(64, 3)

    def forward(self, x):
        h = self.inp(x)
        a = self.attn(h, h, h, key_padding_mask=self.pad, attn_mask=self.mask, need_weights=False)[0]
        return self.head((h + a).mean(1))


def _site_x():
    return torch.randn(B_SITE, S_SITE, 16, generator=torch.Generator().manual_seed(2))


def test_gpt_style_block_lowers_and_matches_autograd():
    assert lower_or_none(_tiny_causal()) is None
    net = _check(_tiny_causal, _tiny_ids, {'SDPASite': 2})
    sites = [s for s in net.train_gm.modules() if isinstance(s, GT.SDPASite)]
    assert all(s.causal and s.heads == 2 and not s.has_mask for s in sites)     # packed-qkv zero-copy form


def test_sdpa_with_masks_lowers_and_matches_autograd():
    assert lower_or_none(_SDPAMaskNet()) is None
    net = _check(_SDPAMaskNet, _site_x, {'SDPASite': 2})
    assert all(s.has_mask and not s.causal for s in net.train_gm.modules() if isinstance(s, GT.SDPASite))


def test_mha_with_attn_mask_and_padding_lowers_and_matches_autograd():
    assert lower_or_none(_MHAMaskNet()) is None
    net = _check(_MHAMaskNet, _site_x, {'MHASite': 1})
    assert all(s.has_mask for s in net.train_gm.modules() if isinstance(s, GT.MHASite))


def _out(make):
    torch.manual_seed(0)
    net = GenericNet(make(), 'cpu')
    net.eval()
    return net(_site_x()).detach()


def test_bool_mask_polarity_sdpa_takes_part_mha_masks_out():
    m = _nonsym_mask()
    additive = torch.zeros(S_SITE, S_SITE).masked_fill(m, NEG)          # -inf where m is True
    # MultiheadAttention: True = masked out
    assert torch.equal(GT.additive_mask(m, true_masks_out=True), additive)
    assert torch.equal(_out(lambda: _MHAMaskNet(m)), _out(lambda: _MHAMaskNet(additive)))
    assert not torch.equal(_out(lambda: _MHAMaskNet(m)), _out(lambda: _MHAMaskNet(~m)))
    # scaled_dot_product_attention: True = takes part, so ~m is the same additive mask
    assert torch.equal(GT.additive_mask(~m, true_masks_out=False), additive)
    assert torch.equal(_out(lambda: _SDPAMaskNet(~m)), _out(lambda: _SDPAMaskNet(additive)))
    assert not torch.equal(_out(lambda: _SDPAMaskNet(~m)), _out(lambda: _SDPAMaskNet(m)))
    assert not torch.equal(_out(lambda: _SDPAMaskNet(~m)), _out(lambda: _SDPAMaskNet((~m).t().contiguous())))


class _KeyMaskSDPA(nn.Module):
    """SDPA with a [B, 1, 1, S] bool mask: the key-padding form."""

    def __init__(self, shape=(B_SITE, 1, 1, S_SITE)):
        super().__init__()
        self.qkv = nn.Linear(16, 3 * 64)
        keep = torch.ones(shape, dtype=torch.bool)
        keep[-1, ..., 5:] = False
        self.register_buffer('keep', keep)

    def forward(self, x):
        B, S, _ = x.shape
        q, k, v = self.qkv(x).reshape(B, S, 3, 2, 32).permute(2, 0, 3, 1, 4).unbind(0)
        return F.scaled_dot_product_attention(q, k, v, attn_mask=self.keep).transpose(1, 2).reshape(B, S, 64).mean(1)


def test_sdpa_key_mask_maps_to_key_bias_and_other_shapes_are_named():
    _check(_KeyMaskSDPA, _site_x, {'SDPASite': 1})
    bad = GenericNet(_KeyMaskSDPA(shape=(B_SITE, 1, S_SITE, 1)), 'cpu')
    with pytest.raises(ValueError, match=r'\(3, 1, 12, 1\)'):
        bad(_site_x())


class _GQA(nn.Module):
    def forward(self, q, k, v):
        return F.scaled_dot_product_attention(q, k, v, enable_gqa=True)


def test_gqa_and_encoder_masks_stay_rejected():
    assert 'gqa' in lower_or_none(_GQA()).lower()
    assert 'mask' in lower_or_none(_CausalNet())


def test_causal_presets_are_registered():
    from mlcomp_amd.models.transformers import CausalTransformerClassifier
    from mlcomp_amd.train.generic import is_text
    m = build_model('transformer-causal-tiny', num_classes=4)
    assert isinstance(m, CausalTransformerClassifier) and m.word.num_embeddings == 1024
    assert len(m.blocks) == 2 and all(b.attn.causal for b in m.blocks)
    assert is_text('transformer-causal-base')
