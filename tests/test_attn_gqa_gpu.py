"""Grouped-query attention kernels: fp64 reference, bit-equality with the multi-head kernels, lowering."""
import math

import pytest
import torch

from mlcomp_amd.ops import _lib, transformer as Tx

from test_attn_gqa_cpu import SALT, GQANet, gqa_case, gqa_run
from test_attn_mask_cpu import _site_x
from test_attn_mask_gpu import NEG, _bf
from test_gtransformer_gpu import _gpu_check

pytestmark = pytest.mark.gpu
DEV = 'cuda'

SHAPES = [(1, 1, 2, 1, 64),        # S = 1
          (2, 100, 4, 2, 64),      # G = 2, partial second tile
          (2, 192, 6, 2, 64),      # G = 3, three tiles: an odd tile count per head (3, causal 3 / 1): buffer parity
          (1, 320, 4, 1, 128),     # multi-query, three blocks, D = 128
          (2, 77, 4, 2, 80),       # zero-padded head dim, S % 4 != 0
          (2, 45, 3, 3, 128)]      # G = 1 through the new entry
CASES = [(s, m) for s in SHAPES for m in ('none', 'causal', 'bias4d')] \
    + [(s, 'causal+keybias+dropout') for s in SHAPES if s[1] >= 100]
EXACT = [(2, 192, 6, 2, 64), (1, 320, 4, 1, 128)]


@pytest.mark.parametrize('shape,mode', CASES, ids=[f'{"x".join(map(str, s))}-{m}' for s, m in CASES])
def test_gqa_kernels_match_fp64_reference(shape, mode):
    gqa_run(shape, mode, DEV)


def _both(shape, p, dctx):
    """(ctx, lse, dqkv) of the grouped call and of the multi-head call on expanded K / V, causal."""
    B, S, H, Hkv, D = shape
    qkv, _, seed, _, _ = gqa_case(shape, 'causal')
    qkv, seed, scale = qkv.to(DEV), seed.to(DEV), 1.0 / math.sqrt(D)
    ctx, lse = Tx.attn_fwd_gqa(qkv, None, B, S, H, Hkv, scale, p, seed, SALT, head_dim=D, causal=True)
    dq = Tx.attn_bwd_gqa(qkv, None, dctx, lse, B, S, H, Hkv, scale, p, seed, SALT, head_dim=D, ctx=ctx, causal=True)
    q, k, v = qkv.view(B * S, H + 2 * Hkv, D).split([H, Hkv, Hkv], 1)
    wide = torch.cat([q, k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)], 1).reshape(B * S, -1)
    ctx_m, lse_m = Tx.attn_fwd(wide, None, B, S, H, scale, p, seed, SALT, head_dim=D, causal=True)
    dq_m = Tx.attn_bwd(wide, None, dctx, lse_m, B, S, H, scale, p, seed, SALT, head_dim=D, ctx=ctx_m, causal=True)
    torch.cuda.synchronize()
    return (ctx, lse, dq), (ctx_m, lse_m, dq_m)


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('shape', EXACT)
def test_ctx_lse_dq_equal_multi_head_on_expanded_kv(shape, p):
    """The same bits, element by element: pins the head map and the dropout index."""
    E = shape[2] * shape[4]
    (ctx, lse, dq), (ctx_m, lse_m, dq_m) = _both(shape, p, gqa_case(shape, 'causal')[1].to(DEV))
    assert torch.equal(ctx, ctx_m) and torch.equal(lse, lse_m) and torch.equal(dq[:, :E], dq_m[:, :E])
    assert dq[:, :E].abs().max().item() > 0


@pytest.mark.parametrize('shape,g', [(s, g) for s in EXACT for g in range(s[2] // s[3])])
def test_dkv_of_one_group_member_equals_multi_head(shape, g):
    """dout on member g of every group only: dK / dV equal the multi-head call's of head j*G + g."""
    (B, S, H, Hkv, D), G = shape, shape[2] // shape[3]
    dctx = gqa_case(shape, 'causal')[1].to(DEV).view(B * S, Hkv, G, D).clone()
    dctx[:, :, [i for i in range(G) if i != g]] = 0
    (_, _, dq), (_, _, dq_m) = _both(shape, 0.0, dctx.view(B * S, H * D))
    for part in (1, 2):   # dK, dV
        got = dq[:, (H + (part - 1) * Hkv) * D:(H + part * Hkv) * D].view(B * S, Hkv, D)
        want = dq_m[:, part * H * D:(part + 1) * H * D].view(B * S, Hkv, G, D)[:, :, g]
        assert torch.equal(got, want), part
        assert got.abs().max().item() > 0


def test_g1_equals_masked_entry_points():
    """Hkv == H is today's layout: bit for bit mlc_flash_fwd_masked / mlc_flash_bwd_masked."""
    B, S, H, D, scale, p = 2, 192, 3, 64, 0.125, 0.1
    qkv, dctx = _bf(B * S, 3 * H * D, seed=16, scale=0.7).to(DEV), _bf(B * S, H * D, seed=17).to(DEV)
    kb = torch.zeros(B, S, device=DEV)
    kb[0, S - 37:] = NEG
    seed = torch.tensor([29], dtype=torch.int32, device=DEV)
    P, st, res = _lib.ptr, _lib.stream(), []
    for name, heads in (('gqa', (H, H)), ('masked', (H,))):
        ctx, dq = torch.empty(B * S, H * D, device=DEV, dtype=torch.bfloat16), torch.empty_like(qkv)
        lse, dot = torch.empty(B * H * S, device=DEV), torch.empty(B * H * S, device=DEV)
        _lib.call(f'mlc_flash_fwd_{name}', P(qkv), P(kb), P(ctx), P(lse), B, S, *heads, D, scale, p, P(seed), SALT, 1,
                  None, 0, 0, st)
        _lib.call(f'mlc_flash_bwd_{name}', P(qkv), P(kb), P(ctx), P(dctx), P(lse), P(dot), P(dq), B, S, *heads, D,
                  scale, p, P(seed), SALT, 1, None, 0, 0, st)
        res.append((ctx, lse, dq))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*res))


@pytest.mark.parametrize('H,Hkv', [(4, 3), (4, 0)])
def test_bad_head_counts_are_rejected_without_a_launch(H, Hkv):
    B, S, D = 1, 64, 64
    qkv = _bf(B * S, (H + 2 * max(Hkv, 1)) * D, seed=1).to(DEV)
    ctx = torch.full((B * S, H * D), 7.0, device=DEV, dtype=torch.bfloat16)
    lse, dot = torch.full((B * H * S,), 7.0, device=DEV), torch.full((B * H * S,), 7.0, device=DEV)
    dq = torch.full_like(qkv, 7.0)
    P, lib = _lib.ptr, _lib.load()
    assert lib.mlc_flash_fwd_gqa(P(qkv), None, P(ctx), P(lse), B, S, H, Hkv, D, 0.125, 0.0, None, 0, 0, None, 0, 0,
                                 _lib.stream()) == -1
    assert lib.mlc_flash_bwd_gqa(P(qkv), None, P(ctx), P(ctx), P(lse), P(dot), P(dq), B, S, H, Hkv, D, 0.125, 0.0,
                                 None, 0, 0, None, 0, 0, _lib.stream()) == -1
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in (ctx, lse, dot, dq))


def test_gqa_net_on_kernels():
    _gpu_check(GQANet, _site_x)


def test_gqa_transformer_step_trains_with_graphs():
    from mlcomp_amd.train.generic import build_generic_step
    step = build_generic_step('transformer-gqa-tiny', batch=8, seq_len=32, image_size=32,
                              device=torch.device('cuda'), num_classes=4, lr=1e-3)
    losses = [(step(), step.last_loss())[1] for _ in range(8)]
    assert step.graph is not None, step.capture_error
    assert all(math.isfinite(v) for v in losses), losses
