"""The fp32 CPU twins of `attn_decode_gqa` and `kv_append_` against a torch fp64 softmax written out
here, and the shape errors of both."""
import math

import pytest
import torch

from mlcomp_amd.ops import transformer as Tx

BF = torch.bfloat16


def ref64(q, cache, lens, H, Hkv, D, scale):
    """one query head at a time: (ctx [B, H*D], lse [B, H]) in fp64"""
    B, G = q.shape[0], H // Hkv
    ctx, lse = torch.zeros(B, H, D, dtype=torch.float64), torch.full((B, H), -math.inf, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        for h in range(H if n else 0):
            j = h // G
            k, v = cache[b, :n, j * D:(j + 1) * D].double(), cache[b, :n, (Hkv + j) * D:(Hkv + j + 1) * D].double()
            s = k @ q[b, h * D:(h + 1) * D].double() * scale
            lse[b, h] = torch.logsumexp(s, 0)
            ctx[b, h] = torch.softmax(s, 0) @ v
    return ctx.view(B, H * D), lse


@pytest.mark.parametrize('D', [64, 128])
@pytest.mark.parametrize('H,Hkv', [(4, 4), (8, 2), (16, 1)])
def test_decode_twin_matches_fp64(H, Hkv, D):
    gen = torch.Generator().manual_seed(H * D)
    B, Smax, scale = 4, 40, D ** -0.5
    lens = torch.tensor([1, 17, 40, 0], dtype=torch.int32)
    cache = torch.randn(B, Smax, 2 * Hkv * D, generator=gen).to(BF)
    for b in range(B):
        cache[b, int(lens[b]):] = float('nan')                       # the tail is never read
    packed = torch.randn(B, (H + 2 * Hkv) * D, generator=gen).to(BF)
    q = packed[:, :H * D]                                            # a strided view, as in a decode step
    ctx, lse = Tx.attn_decode_gqa(q, cache, lens, H, Hkv, scale, D)
    want_ctx, want_lse = ref64(q, cache, lens, H, Hkv, D, scale)
    assert ctx.dtype == BF and lse.dtype == torch.float32 and ctx.shape == (B, H * D) and lse.shape == (B, H)
    assert not ctx[3].any() and bool((lse[3] == -math.inf).all())
    assert (lse[:3].double() - want_lse[:3]).abs().max() < 1e-5
    assert ((ctx.double() - want_ctx).abs() <= 2.0 ** -8 * want_ctx.abs() + 1e-5).all()   # one bf16 rounding

    # a step: append at the lengths (the full sequence drops its row), then attend over one more key
    before = cache.clone()
    assert Tx.kv_append_(cache, packed, lens, H, Hkv, D) is cache
    for b in range(B):
        n = int(lens[b])
        if n < Smax:
            assert torch.equal(cache[b, n].view(torch.int16), packed[b, H * D:].view(torch.int16))
            before[b, n] = packed[b, H * D:]
    assert torch.equal(cache.view(torch.int16), before.view(torch.int16))
    lens1 = (lens + 1).clamp(max=Smax)
    ctx1, lse1 = Tx.attn_decode_gqa(q, cache, lens1, H, Hkv, scale, D)
    want_ctx, want_lse = ref64(q, cache, lens1, H, Hkv, D, scale)
    assert (lse1.double() - want_lse).abs().max() < 1e-5
    assert ((ctx1.double() - want_ctx).abs() <= 2.0 ** -8 * want_ctx.abs() + 1e-5).all()


def _args(H=8, Hkv=2, D=64, B=2, Smax=8):
    return dict(q=torch.zeros(B, H * D, dtype=BF), kv_cache=torch.zeros(B, Smax, 2 * Hkv * D, dtype=BF),
                seq_lens=torch.ones(B, dtype=torch.int32), H=H, Hkv=Hkv, scale=1.0, head_dim=D)


@pytest.mark.parametrize('change', [
    dict(H=34, q=torch.zeros(2, 34 * 64, dtype=BF)),                           # G = 17
    dict(H=7, q=torch.zeros(2, 7 * 64, dtype=BF)),                             # H % Hkv
    dict(head_dim=32, q=torch.zeros(2, 8 * 32, dtype=BF), kv_cache=torch.zeros(2, 8, 2 * 2 * 32, dtype=BF)),
    dict(kv_cache=torch.zeros(2, 8, 2 * 2 * 64 + 8, dtype=BF)),                # a wrong cache width
    dict(kv_cache=torch.zeros(2, 8, 2 * 2 * 64)),                              # fp32 cache
    dict(seq_lens=torch.ones(2, dtype=torch.int64)),
    dict(q=torch.zeros(2, 8 * 64)),                                            # fp32 q
    dict(q=torch.zeros(2, 8 * 64 * 2, dtype=BF)[:, ::2]),                      # q.stride(1) != 1
], ids=['G17', 'H%Hkv', 'D32', 'width', 'cache-dtype', 'lens-dtype', 'q-dtype', 'q-stride'])
def test_decode_shape_errors(change):
    with pytest.raises(ValueError):
        Tx.attn_decode_gqa(**{**_args(), **change})
    a = {**_args(), **change}
    if 'q' in change and a['q'].dtype == BF and a['q'].stride(1) == 1:        # the cases that are about the heads
        with pytest.raises(ValueError):
            Tx.kv_append_(a['kv_cache'], torch.zeros(2, (a['H'] + 2 * a['Hkv']) * a['head_dim'], dtype=BF),
                          a['seq_lens'], a['H'], a['Hkv'], a['head_dim'])
