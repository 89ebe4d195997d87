"""Causal and additive attention masks on the GPU: the masked flash kernels
(``mlc_flash_fwd_masked`` / ``mlc_flash_bwd_masked``) against the fp32 CPU twin, exact
causality (bit-identical rows under perturbation of the future), fully masked rows, the
unmasked entry points against the masked ones in "no mask" mode, the lowered sites against the
fp32 PyTorch models, and ``transformer-causal-tiny`` training under graph capture."""
import functools
import math

import pytest
import torch

from mlcomp_amd.ops import transformer as Tx

from test_attn_mask_cpu import _MHAMaskNet, _SDPAMaskNet, _site_x, _tiny_causal, _tiny_ids
from test_gtransformer_gpu import _gpu_check

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NEG = float('-inf')

SHAPES = [(1, 1, 2, 64),        # S = 1
          (3, 45, 3, 128),      # one partial tile, S % 4 != 0 (scalar bias loads)
          (2, 64, 2, 64),       # a single full tile
          (2, 100, 2, 64),      # partial second tile
          (3, 128, 4, 64),      # the shape the fused 128 pair owns when unmasked
          (2, 192, 3, 64),      # second query block half empty, dkv starts at tile 2
          (2, 200, 2, 32),      # zero-padded head dim
          (2, 77, 2, 80),       # zero-padded head dim, odd S
          (1, 320, 2, 128)]     # three blocks at D = 128
BIAS4 = [(3, 45, 3, 128), (2, 192, 3, 64)]
CASES = [(s, 'causal') for s in SHAPES] + [(s, 'bias2d') for s in SHAPES] + [(s, 'bias4d') for s in BIAS4] \
    + [(s, 'causal+keybias+dropout') for s in SHAPES if s[1] >= 100] \
    + [(s, 'causal+bias4d+keybias+dropout') for s in BIAS4]          # every operand at once


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _bf(*s, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*s, generator=g) * scale).to(torch.bfloat16)


def _bias(shape, seed=41):
    """Random finite bias with ~25 % of the entries -inf; the diagonal stays finite, so no row
    is fully masked."""
    g = torch.Generator().manual_seed(seed)
    S = shape[-1]
    b = torch.randn(shape, generator=g)
    drop = (torch.rand(shape, generator=g) < 0.25) & ~torch.eye(S, dtype=torch.bool)
    return b.masked_fill(drop, NEG)


@functools.lru_cache(maxsize=None)
def _case(shape, mode):
    """Inputs and the CPU twin's results of one case, computed once and left unchanged."""
    B, S, H, D = shape
    qkv = _bf(B * S, 3 * H * D, seed=16, scale=0.7)
    dctx = _bf(B * S, H * D, seed=17)
    kw = dict(kb=None, p=0.0, causal=False, attn_bias=None)
    if mode == 'causal':
        kw['causal'] = True
    elif mode == 'bias2d':
        kw['attn_bias'] = _bias((S, S))
    elif mode == 'bias4d':
        kw['attn_bias'] = _bias((B, H, S, S))
    else:
        kb = torch.zeros(B, S)
        kb[0, S - 37:] = NEG              # right padding: key 0 stays visible to every query
        kb[-1, 1:5] = -2.5                # a finite bias too
        kw.update(causal=True, kb=kb, p=0.1)
        if 'bias4d' in mode:
            kw['attn_bias'] = _bias((B, H, S, S))
    seed = torch.tensor([29], dtype=torch.int32)
    ctx, lse, dq = _run(qkv, dctx, seed, shape, 'cpu', **kw)
    return qkv, dctx, seed, kw, ctx, lse, dq


def _run(qkv, dctx, seed, shape, dev, kb, p, causal, attn_bias):
    B, S, H, D = shape
    scale = 1.0 / math.sqrt(D)
    to = lambda t: None if t is None else t.to(dev)
    qkv, dctx, seed, kb, attn_bias = to(qkv), to(dctx), to(seed), to(kb), to(attn_bias)
    ctx, lse = Tx.attn_fwd(qkv, kb, B, S, H, scale, p, seed, 33, head_dim=D, causal=causal, attn_bias=attn_bias)
    dq = Tx.attn_bwd(qkv, kb, dctx, lse, B, S, H, scale, p, seed, 33, head_dim=D, ctx=ctx, causal=causal,
                     attn_bias=attn_bias)
    return ctx, lse, dq


@pytest.mark.parametrize('shape,mode', CASES, ids=[f'{"x".join(map(str, s))}-{m}' for s, m in CASES])
def test_masked_flash_attention_fwd_bwd(shape, mode, monkeypatch):
    """The bounds of test_flash_attention_fwd_bwd, on the masked kernels."""
    monkeypatch.setattr(Tx, '_FLASH_ONLY', True)
    qkv, dctx, seed, kw, ctx_r, lse_r, dq_r = _case(shape, mode)
    ctx_g, lse_g, dq_g = _run(qkv, dctx, seed, shape, DEV, **kw)
    torch.cuda.synchronize()
    E = shape[2] * shape[3]
    figures = [rel(ctx_g, ctx_r), rel(lse_g, lse_r)] + [rel(dq_g[:, i * E:(i + 1) * E], dq_r[:, i * E:(i + 1) * E])
                                                        for i in range(3)]
    print(shape, mode, 'rel ctx / lse / dQ / dK / dV:', ' '.join(f'{v:.2e}' for v in figures))
    assert torch.isfinite(dq_g.float()).all() and torch.isfinite(lse_g).all()
    assert figures[0] < 1e-2
    assert figures[1] < 1e-4
    for part in range(3):   # dQ, dK, dV separately
        assert figures[2 + part] < 2e-2, part


@pytest.mark.parametrize('shape,j', [((2, 192, 3, 64), 100), ((2, 192, 3, 64), 63), ((1, 320, 2, 128), 127),
                                     ((2, 77, 2, 80), 31)])
def test_causal_is_exact(shape, j):
    """Nothing after position j reaches positions <= j: with K and V rows > j perturbed, the
    context rows <= j are bit-identical, and so are the dQ rows <= j; an upstream gradient
    that lives on rows <= j leaves dK / dV rows > j exactly zero.  An off-by-one on the
    diagonal fails here where a norm bound could hide it."""
    B, S, H, D = shape
    E = H * D
    scale = 1.0 / math.sqrt(D)
    qkv = _bf(B * S, 3 * E, seed=51, scale=0.7).to(DEV)
    dctx = _bf(B * S, E, seed=52).to(DEV)
    other = qkv.clone().view(B, S, 3 * E)
    other[:, j + 1:, E:] = _bf(B, S - j - 1, 2 * E, seed=53, scale=2.0).to(DEV)
    other = other.view(B * S, 3 * E).contiguous()

    def run(x, d):
        ctx, lse = Tx.attn_fwd(x, None, B, S, H, scale, head_dim=D, causal=True)
        return ctx, Tx.attn_bwd(x, None, d, lse, B, S, H, scale, head_dim=D, ctx=ctx, causal=True)

    past = dctx.clone().view(B, S, E)
    past[:, j + 1:] = 0                   # upstream gradient on rows <= j only
    past = past.view(B * S, E).contiguous()
    future = (dctx.view(B, S, E) - past.view(B, S, E)).view(B * S, E).contiguous()   # on rows > j only
    ctx_a, dq_a = run(qkv, past)
    ctx_b, dq_b = run(other, past)
    _, dq_f = run(other, future)
    torch.cuda.synchronize()
    v = lambda t: t.view(B, S, -1)
    assert torch.equal(v(ctx_a)[:, :j + 1], v(ctx_b)[:, :j + 1])
    assert not torch.equal(v(ctx_a)[:, j + 1:], v(ctx_b)[:, j + 1:])
    assert torch.equal(v(dq_a)[:, :j + 1, :E], v(dq_b)[:, :j + 1, :E])          # dQ rows <= j unchanged
    assert v(dq_a)[:, :j + 1, :E].abs().max().item() > 0
    for g in (dq_a, dq_b):
        assert v(g)[:, j + 1:, E:].abs().max().item() == 0                      # dK, dV rows > j: exactly zero
        assert v(g)[:, j + 1:, :E].abs().max().item() == 0                      # their queries got no gradient
    # upstream gradient zero on rows <= j: everything stays finite, dQ rows <= j are zero in both
    assert torch.isfinite(dq_f.float()).all()
    assert v(dq_f)[:, :j + 1, :E].abs().max().item() == 0
    assert v(dq_f)[:, j + 1:, E:].abs().max().item() > 0


@pytest.mark.parametrize('shape', [(2, 100, 2, 64), (1, 45, 2, 128)])
def test_fully_masked_bias_rows(shape):
    """A bias row that is all -inf: zero context, lse = +inf, zero dQ for that row and no
    contribution to dK / dV (the rest still matches the CPU twin)."""
    B, S, H, D = shape
    E = H * D
    rows = [0, S // 2, S - 1]
    bias = _bias((S, S), seed=61)
    bias[rows] = NEG
    qkv, dctx = _bf(B * S, 3 * E, seed=62, scale=0.7), _bf(B * S, E, seed=63)
    seed = torch.tensor([5], dtype=torch.int32)
    kw = dict(kb=None, p=0.0, causal=False, attn_bias=bias)
    ctx_r, lse_r, dq_r = _run(qkv, dctx, seed, shape, 'cpu', **kw)
    ctx, lse, dq = _run(qkv, dctx, seed, shape, DEV, **kw)
    torch.cuda.synchronize()
    assert ctx.view(B, S, E)[:, rows].abs().max().item() == 0
    assert (lse.view(B, H, S)[:, :, rows] == float('inf')).all()
    live = [s for s in range(S) if s not in rows]
    assert torch.isfinite(lse.view(B, H, S)[:, :, live]).all()
    assert torch.isfinite(dq.float()).all()
    assert dq.view(B, S, 3 * E)[:, rows, :E].abs().max().item() == 0
    assert rel(ctx, ctx_r) < 1e-2
    for part in range(3):
        assert rel(dq[:, part * E:(part + 1) * E], dq_r[:, part * E:(part + 1) * E]) < 2e-2, part


def test_unmasked_entry_points_equal_masked_ones_in_no_mask_mode(monkeypatch):
    """attn_fwd / attn_bwd with default arguments (mlc_flash_fwd / mlc_flash_bwd) and the
    masked entry points called with causal = 0 and a null bias: bit for bit the same."""
    from mlcomp_amd.ops import _lib
    monkeypatch.setattr(Tx, '_FLASH_ONLY', True)
    B, S, H, D = 2, 192, 3, 64
    scale, p, salt = 1.0 / math.sqrt(D), 0.1, 33
    qkv, dctx = _bf(B * S, 3 * H * D, seed=16, scale=0.7).to(DEV), _bf(B * S, H * D, seed=17).to(DEV)
    kb = torch.zeros(B, S, device=DEV)
    kb[0, S - 37:] = NEG
    seed = torch.tensor([29], dtype=torch.int32, device=DEV)
    ctx, lse = Tx.attn_fwd(qkv, kb, B, S, H, scale, p, seed, salt, head_dim=D)
    dq = Tx.attn_bwd(qkv, kb, dctx, lse, B, S, H, scale, p, seed, salt, head_dim=D, ctx=ctx)
    ctx2, lse2, dq2 = torch.empty_like(ctx), torch.empty_like(lse), torch.empty_like(dq)
    dot = torch.empty_like(lse)
    P = _lib.ptr
    _lib.call('mlc_flash_fwd_masked', P(qkv), P(kb), P(ctx2), P(lse2), B, S, H, D, scale, p, P(seed), salt, 0, None,
              0, 0, _lib.stream())
    _lib.call('mlc_flash_bwd_masked', P(qkv), P(kb), P(ctx2), P(dctx), P(lse2), P(dot), P(dq2), B, S, H, D, scale, p,
              P(seed), salt, 0, None, 0, 0, _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(ctx, ctx2) and torch.equal(lse, lse2) and torch.equal(dq, dq2)


def test_gpt_style_model_on_kernels():
    _gpu_check(_tiny_causal, _tiny_ids)


def test_sdpa_with_masks_on_kernels():
    _gpu_check(_SDPAMaskNet, _site_x)


def test_mha_with_attn_mask_and_padding_on_kernels():
    _gpu_check(_MHAMaskNet, _site_x)


def test_causal_transformer_step_trains_with_graphs():
    from mlcomp_amd.ops import _lib
    from mlcomp_amd.train.generic import build_generic_step
    step = build_generic_step('transformer-causal-tiny', batch=8, seq_len=32, image_size=32,
                              device=torch.device('cuda'), num_classes=4, lr=1e-3)
    losses = []
    for _ in range(8):
        step()
        losses.append(step.last_loss())
    assert step.graph is not None, step.capture_error
    assert all(math.isfinite(v) for v in losses), losses
    assert _lib.load() is not None
