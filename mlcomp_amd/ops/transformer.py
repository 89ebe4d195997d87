"""Python entry points of the transformer kernels (``csrc/kernels/transformer.hip`` and the
dense-layer GEMM epilogue of ``igemm.hip``), each with an fp32 PyTorch reference used on
CPU (and by the numerics tests).  Dropout uses the kernels' counter-based hash, which the
CPU path reproduces bit-exactly, so masks agree between the two."""
from __future__ import annotations

import math
import os
import struct
from typing import Optional, Tuple

import torch

from . import _lib
from .functional import NSTAT, _cuda

_M32 = 0xFFFFFFFF


def _hash(seed: int, salt: int, idx: torch.Tensor) -> torch.Tensor:
    x = (idx * 0x9E3779B9) & _M32
    x = x ^ ((seed * 0x85EBCA6B + salt * 0xC2B2AE35) & _M32)
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    x = x ^ (x >> 16)
    return x


def drop_threshold(p: float) -> int:
    """``drop_threshold`` of csrc/kernels/dropout.h: ``(uint32_t)(p * 16777216.0f)`` with p
    already rounded to fp32 (a power-of-two scaling, exact in fp32).  ``int(p * 2**24)`` on
    the double p is one lower for p = 0.3, 0.6 and 0.8, and the element whose hash lands
    there would be kept here and dropped by every kernel."""
    (p32,) = struct.unpack('f', struct.pack('f', p))
    return int(p32 * 16777216.0)


def keep_mask(shape, p: float, seed: int, salt: int, device=None) -> torch.Tensor:
    """Same keep decisions as the kernels for a contiguous tensor of ``shape``."""
    n = 1
    for s in shape:
        n *= s
    idx = torch.arange(n, dtype=torch.int64, device=device)
    return ((_hash(seed, salt, idx) >> 8) >= drop_threshold(p)).reshape(shape)


def _seed_val(seed) -> int:
    return int(seed.item()) if torch.is_tensor(seed) else int(seed or 0)


# ---------------------------------------------------------------------------- LayerNorm
def ln_fwd(x, r, gamma, beta, eps=1e-12, p_in=0.0, p_out=0.0, seed=None, salt_in=0, salt_out=0):
    """y = dropout_out(LN(x + dropout_in(r))).  Returns (y, s, mean, rstd) where s is the
    normalised input (``x`` itself when there is no ``r``)."""
    T, H = x.shape
    if _cuda(x):
        y = torch.empty_like(x)
        s = torch.empty_like(x) if r is not None else x
        mean = torch.empty(T, device=x.device, dtype=torch.float32)
        rstd = torch.empty(T, device=x.device, dtype=torch.float32)
        _lib.call('mlc_ln_fwd', _lib.ptr(x), _lib.ptr(r), _lib.ptr(s if r is not None else None), _lib.ptr(y),
                  _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma), _lib.ptr(beta), T, H, float(eps), float(p_in),
                  float(p_out), _lib.ptr(seed), salt_in, salt_out, _lib.stream())
        return y, s, mean, rstd
    sd = _seed_val(seed)
    v = x.float()
    if r is not None:
        rr = r.float()
        if p_in > 0:
            rr = torch.where(keep_mask((T, H), p_in, sd, salt_in), rr / (1 - p_in), torch.zeros_like(rr))
        v = v + rr
    s = v.to(torch.bfloat16) if r is not None else x
    mean = v.mean(1)
    var = ((v - mean[:, None]) ** 2).mean(1)
    rstd = torch.rsqrt(var + eps)
    y = (v - mean[:, None]) * rstd[:, None] * gamma + beta
    if p_out > 0:
        y = torch.where(keep_mask((T, H), p_out, sd, salt_out), y / (1 - p_out), torch.zeros_like(y))
    return y.to(torch.bfloat16), s, mean, rstd


def ln_bwd(dy, s, mean, rstd, gamma, dgamma, dbeta, sums=None, p_in=0.0, p_out=0.0, seed=None, salt_in=0,
           salt_out=0, want_dr=False, defer_finalize=False):
    """Returns (ds, dr): ds = dLoss/ds, dr = dropout_in'(ds) (None unless ``want_dr``).
    dgamma / dbeta are ACCUMULATED (+=).  ``defer_finalize`` (GPU): leave the per-copy
    partial sums in ``sums`` for a later :class:`LnFinalizer` launch (dgamma/dbeta untouched
    until then)."""
    T, H = dy.shape
    if _cuda(dy):
        ds = torch.empty_like(dy)
        dr = torch.empty_like(dy) if want_dr else None
        if sums is None:
            assert not defer_finalize, 'a deferred finalize needs a persistent sums scratch'
            sums = torch.zeros(NSTAT * 2 * H, device=dy.device, dtype=torch.float32)
        dg, db = (None, None) if defer_finalize else (dgamma, dbeta)
        _lib.call('mlc_ln_bwd', _lib.ptr(dy), _lib.ptr(s), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma),
                  _lib.ptr(ds), _lib.ptr(dr), _lib.ptr(sums), _lib.ptr(dg), _lib.ptr(db), T, H, float(p_in),
                  float(p_out), _lib.ptr(seed), salt_in, salt_out, _lib.stream())
        return ds, dr
    sd = _seed_val(seed)
    d = dy.float()
    if p_out > 0:
        d = torch.where(keep_mask((T, H), p_out, sd, salt_out), d / (1 - p_out), torch.zeros_like(d))
    xh = (s.float() - mean[:, None]) * rstd[:, None]
    dgamma.add_((d * xh).sum(0))
    dbeta.add_(d.sum(0))
    g = d * gamma
    a = g.mean(1, keepdim=True)
    b = (g * xh).mean(1, keepdim=True)
    dsf = rstd[:, None] * (g - a - xh * b)
    ds = dsf.to(torch.bfloat16)
    dr = None
    if want_dr:
        drf = dsf
        if p_in > 0:
            drf = torch.where(keep_mask((T, H), p_in, sd, salt_in), dsf / (1 - p_in), torch.zeros_like(dsf))
        dr = drf.to(torch.bfloat16)
    return ds, dr


_EMB_SCRATCH = {}


def embed_bwd(ds, ids, tt, word_grad, pos_grad, tok_grad):
    """Embedding gradients from ds [B*S, H] (bf16): word_grad[ids] += ds, pos_grad[s] +=
    sum over the batch, tok_grad[tt] += ds (all fp32, accumulated).  ids / tt int64 [B, S]."""
    B, S = ids.shape
    H = ds.shape[-1]
    if _cuda(ds):
        ntypes = tok_grad.shape[0] if tok_grad is not None else 1
        from .functional import workspace_key, workspace_store
        key = (workspace_key(ds.device), S * ntypes * H)
        store = workspace_store(_EMB_SCRATCH)
        pt = store.get(key)
        if pt is None:    # [S][ntypes][H] partial sums, left zeroed by the kernel
            pt = store[key] = torch.zeros(S * ntypes * H, device=ds.device, dtype=torch.float32)
        # contiguous copies bound to names: a temporary freed while the argument list is
        # still being built could hand its block to the next copy before the kernel runs
        dsc, idc = ds.contiguous(), ids.contiguous()
        ttc = tt.contiguous() if tok_grad is not None else None
        _lib.call('mlc_embed_bwd', _lib.ptr(dsc), _lib.ptr(idc), _lib.ptr(ttc), _lib.ptr(word_grad),
                  _lib.ptr(pos_grad), _lib.ptr(tok_grad), _lib.ptr(pt), B, S, H, ntypes, _lib.stream())
        return
    d = ds.float().reshape(B * S, H)
    word_grad.index_add_(0, ids.reshape(-1), d)
    if tok_grad is not None:
        tok_grad.index_add_(0, tt.reshape(-1), d)
    pos_grad[:S].add_(d.view(B, S, H).sum(0))


def embed_ln_fwd(ids, tt, pos_ids, word, pos, tok, gamma, beta, eps=1e-12, p_out=0.0, seed=None, salt_out=0):
    """e = bf16((word[ids] + pos[p]) + tok[tt]) and y = dropout_out(LN(e)) in one kernel
    (``mlc_embed_ln_fwd``); returns (y, e, mean, rstd) as ``ln_fwd`` over the gathered sum does.
    ``ids`` / ``tt`` int64 [B, S] with ``pos_ids`` None (the position of a token is its column),
    or packed [T] with the position of every row in ``pos_ids``; ``tt`` None: type 0.  Tables
    bf16 [rows, H].  The kernel clamps every index into its table; the CPU path indexes as torch
    does."""
    T, H = ids.numel(), word.shape[1]
    if pos_ids is None:
        assert ids.dim() == 2, 'without pos_ids the position of a token is its column: ids [B, S]'
    S = ids.shape[-1]
    if _cuda(word):
        e = torch.empty(T, H, device=word.device, dtype=torch.bfloat16)
        y = torch.empty_like(e)
        mean = torch.empty(T, device=word.device, dtype=torch.float32)
        rstd = torch.empty(T, device=word.device, dtype=torch.float32)
        # contiguous copies bound to names (see embed_bwd)
        idc = ids.contiguous()
        ttc = tt.contiguous() if tt is not None else None
        pc = pos_ids.contiguous() if pos_ids is not None else None
        _lib.call('mlc_embed_ln_fwd', _lib.ptr(idc), _lib.ptr(ttc), _lib.ptr(pc), _lib.ptr(word), _lib.ptr(pos),
                  _lib.ptr(tok), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(e), _lib.ptr(y), _lib.ptr(mean),
                  _lib.ptr(rstd), T, S, H, word.shape[0], pos.shape[0], tok.shape[0], float(eps), float(p_out),
                  _lib.ptr(seed), salt_out, _lib.stream())
        return y, e, mean, rstd
    p = pos[pos_ids] if pos_ids is not None else pos[:S][None]
    t = tok[tt] if tt is not None else tok[0]
    e = (word[ids].float() + p.float() + t.float()).to(torch.bfloat16).view(T, H)
    return ln_fwd(e, None, gamma, beta, eps, p_out=p_out, seed=seed, salt_out=salt_out)


_EMB_PACKED_SCRATCH = {}


def embed_bwd_packed(ds, ids, tt, pos_ids, word_grad, pos_grad, tok_grad):
    """Embedding gradients of packed rows, ds [T, H] bf16: word_grad[ids] += ds,
    pos_grad[pos_ids] += ds, tok_grad[tt] += ds (all fp32, accumulated; ids / tt / pos_ids
    int64 [T]).  One kernel plus a small finish (``mlc_embed_bwd_packed``); at most 4 token types."""
    T, H = ds.shape
    if _cuda(ds):
        ntypes = tok_grad.shape[0]
        from .functional import workspace_key, workspace_store
        key = (workspace_key(ds.device), 32 * ntypes * H)
        store = workspace_store(_EMB_PACKED_SCRATCH)
        scratch = store.get(key)
        if scratch is None:    # [32][ntypes][H] per-type partial sums, left zeroed by the kernel
            scratch = store[key] = torch.zeros(32 * ntypes * H, device=ds.device, dtype=torch.float32)
        dsc, idc, ttc, pc = ds.contiguous(), ids.contiguous(), tt.contiguous(), pos_ids.contiguous()
        _lib.call('mlc_embed_bwd_packed', _lib.ptr(dsc), _lib.ptr(idc), _lib.ptr(ttc), _lib.ptr(pc),
                  _lib.ptr(word_grad), _lib.ptr(pos_grad), _lib.ptr(tok_grad), _lib.ptr(scratch), T, H,
                  word_grad.shape[0], pos_grad.shape[0], ntypes, _lib.stream())
        return
    d = ds.float()
    word_grad.index_add_(0, ids, d)
    tok_grad.index_add_(0, tt, d)
    pos_grad.index_add_(0, pos_ids, d)


def cls_scatter(dcls, cu, T: int):
    """The packed [CLS] gather's gradient: dh [T, H] bf16, row min(cu[b], T-1) takes dcls[b]
    (slots that share a row are summed in fp32 and rounded once), every other row is zero.
    ``dcls`` [n, H] bf16, ``cu`` int32 [n + 1]; one pass that writes all of dh
    (``mlc_cls_scatter``, n <= 1024)."""
    n, H = dcls.shape
    if _cuda(dcls):
        dh = torch.empty(T, H, device=dcls.device, dtype=torch.bfloat16)
        dc, cc = dcls.contiguous(), cu.contiguous()
        _lib.call('mlc_cls_scatter', _lib.ptr(dc), _lib.ptr(cc), _lib.ptr(dh), n, T, H, _lib.stream())
        return dh
    dh = torch.zeros(T, H, device=dcls.device, dtype=torch.float32)
    dh.index_add_(0, cu[:-1].long().clamp(max=T - 1), dcls.float())
    return dh.to(torch.bfloat16)


class LnFinalizer:
    """Finalizes the dgamma / dbeta of many LayerNorms in ONE launch
    (``mlc_ln_finalize_many``): each entry's ``ln_bwd(..., defer_finalize=True)`` left its
    partial sums in a persistent NSTAT-copy scratch; ``run()`` adds every sum into its grad
    slots.  The descriptor table is built once (pointers must stay put), outside capture."""

    def __init__(self):
        self.entries = []        # (sums [NSTAT*2*H], dgamma [H], dbeta [H])
        self.desc = None
        self.max_h = 0

    def add(self, sums, dgamma, dbeta):
        self.entries.append((sums, dgamma, dbeta))

    def build(self):
        if not self.entries or not self.entries[0][0].is_cuda:
            return
        rows = [[s.data_ptr(), g.data_ptr(), b.data_ptr(), g.numel()] for s, g, b in self.entries]
        self.desc = torch.tensor(rows, dtype=torch.int64).to(self.entries[0][0].device)
        self.max_h = max(g.numel() for _, g, _ in self.entries)

    def run(self):
        if not self.entries or not self.entries[0][0].is_cuda:
            return       # the CPU path of ln_bwd accumulates immediately
        if self.desc is None:
            self.build()
        _lib.call('mlc_ln_finalize_many', _lib.ptr(self.desc), len(self.entries), self.max_h, _lib.stream())


# ---------------------------------------------------------------------------- softmax
def softmax_fwd(S, key_bias, rows_per_batch, scale, p=0.0, seed=None, salt=0):
    """S [R, L] bf16 scores; key_bias [B, L] fp32 (0 / -inf) or None.  Returns (P, Pd)."""
    R, L = S.shape
    if _cuda(S):
        P = torch.empty_like(S)
        Pd = torch.empty_like(S) if p > 0 else P
        _lib.call('mlc_softmax_fwd', _lib.ptr(S), _lib.ptr(key_bias), _lib.ptr(P),
                  _lib.ptr(Pd if p > 0 else None), R, L, rows_per_batch, float(scale), float(p), _lib.ptr(seed),
                  salt, _lib.stream())
        return P, Pd
    v = S.float() * scale
    if key_bias is not None:
        v = v + key_bias.repeat_interleave(rows_per_batch, 0)
    Pf = torch.softmax(v, 1).nan_to_num(0.0)
    P = Pf.to(torch.bfloat16)
    if p > 0:
        m = keep_mask((R, L), p, _seed_val(seed), salt)
        Pd = torch.where(m, Pf / (1 - p), torch.zeros_like(Pf)).to(torch.bfloat16)
    else:
        Pd = P
    return P, Pd


def softmax_bwd(P, dPd, scale, p=0.0, seed=None, salt=0):
    R, L = P.shape
    if _cuda(P):
        dS = torch.empty_like(P)
        _lib.call('mlc_softmax_bwd', _lib.ptr(P), _lib.ptr(dPd), _lib.ptr(dS), R, L, float(scale), float(p),
                  _lib.ptr(seed), salt, _lib.stream())
        return dS
    d = dPd.float()
    if p > 0:
        d = torch.where(keep_mask((R, L), p, _seed_val(seed), salt), d / (1 - p), torch.zeros_like(d))
    Pf = P.float()
    dot = (Pf * d).sum(1, keepdim=True)
    return (scale * Pf * (d - dot)).to(torch.bfloat16)


# ---------------------------------------------------------------------------- fused attention
# The streaming kernels measured faster than the whole-tile ones on every shape both take
# (profiles/flash_attn/); MLC_ATTN_KERNEL=tile routes head dim 64, S in {64, 128} back to them.
_FLASH_ONLY = os.environ.get('MLC_ATTN_KERNEL', 'flash') != 'tile'


def _attn_small(S: int, head_dim: int) -> bool:
    """Shapes of the whole-tile kernels ``mlc_attn_fwd`` / ``mlc_attn_bwd`` (transformer.hip)."""
    return head_dim == 64 and S in (64, 128) and not _FLASH_ONLY


def _attn_flash(S: int, head_dim: int) -> bool:
    """Shapes of the streaming kernels ``mlc_flash_fwd`` / ``mlc_flash_bwd`` (flash_attn.hip):
    any S (a partial last 64-key tile is masked in the kernel), head dim 64 or 128."""
    return head_dim in (64, 128) and S >= 1


def _pad_dim(head_dim: int) -> int:
    """The kernel head dim a head dim of ``head_dim`` runs at (zero-padded columns change
    neither the scores nor the kept output columns)."""
    return 64 if head_dim <= 64 else 128


def attn_supported(S: int, head_dim: int) -> bool:
    """Shapes the fused attention path takes: every S >= 1 and head dim <= 128 (head dims
    other than 64 / 128 run zero-padded to the next of the two)."""
    return S >= 1 and 1 <= head_dim <= 128


def _pad_heads(t, rows, groups, H, D, Dp):
    """[rows, groups*H*D] -> [rows, groups*H*Dp] with zero columns after each head."""
    out = torch.zeros(rows, groups, H, Dp, device=t.device, dtype=t.dtype)
    out[..., :D] = t.view(rows, groups, H, D)
    return out.view(rows, groups * H * Dp)


def _unpad_heads(t, rows, groups, H, D, Dp):
    return t.view(rows, groups, H, Dp)[..., :D].reshape(rows, groups * H * D)


def attn_bias_arg(attn_bias, B: int, S: int, H: int):
    """An additive attention mask -> (contiguous fp32 tensor, batch stride, head stride) as
    the kernels read it: element (b, h, q, key) at ``b*stride_b + h*stride_h + q*S + key``.
    Accepted shapes: [S, S]; [B, H, S, S] where size-1 dims broadcast (stride 0); [B*H, S, S]."""
    if attn_bias is None:
        return None, 0, 0
    shape = tuple(attn_bias.shape)
    if attn_bias.dtype == torch.bool:
        raise ValueError('attn_bias is additive (float); turn a bool mask into 0 / -inf first')
    if shape == (S, S):
        b, h = 1, 1
    elif len(shape) == 3 and shape == (B * H, S, S):
        b, h = B, H
    elif len(shape) == 4 and shape[2:] == (S, S) and shape[0] in (1, B) and shape[1] in (1, H):
        b, h = shape[:2]
    else:
        raise ValueError(f'attn_bias shape {shape}: expected [S, S], [B|1, H|1, S, S] or [B*H, S, S] with '
                         f'B={B}, H={H}, S={S}')
    t = attn_bias.reshape(b, h, S, S)
    if t.dtype != torch.float32:
        t = t.float()
    t = t.contiguous()
    return t, (h * S * S if b > 1 else 0), (S * S if h > 1 else 0)


def _attn_ref_scores(qkv, key_bias, B, S, H, scale, D=64, causal=False, attn_bias=None):
    q, k, v = qkv.float().view(B, S, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)   # [B, H, S, D]
    x = torch.matmul(q, k.transpose(-1, -2)) * scale
    if key_bias is not None:
        x = x + key_bias.float()[:, None, None, :]
    if attn_bias is not None:
        x = x + attn_bias_arg(attn_bias, B, S, H)[0]
    if causal:
        x = x.masked_fill(torch.ones(S, S, dtype=torch.bool, device=x.device).triu(1), float('-inf'))
    return q, k, v, x


def _attn_ref_probs(qkv, key_bias, B, S, H, scale, D=64, causal=False, attn_bias=None):
    q, k, v, x = _attn_ref_scores(qkv, key_bias, B, S, H, scale, D, causal, attn_bias)
    P = torch.softmax(x, -1).nan_to_num(0.0)     # a fully masked row: all zeros
    return q, k, v, P, H * D


def attn_fwd(qkv, key_bias, B, S, H, scale, p=0.0, seed=None, salt=0, head_dim: int = 64, *, causal: bool = False,
             attn_bias=None):
    """Fused multi-head attention over the QKV projection output ``qkv`` [B*S, 3*H*D]
    (columns q | k | v, head h at h*D).  Returns (ctx [B*S, H*D] bf16, lse [B*H*S] fp32).
    Attention-probability dropout uses the softmax kernel's mask indexing
    (((b*H + h)*S + q)*S + key), so every path drops the same elements.
    ``causal``: query q attends to keys <= q.  ``attn_bias``: an additive float mask ([S, S],
    [B|1, H|1, S, S] or [B*H, S, S]; finite or -inf) summed with the scaled scores; both
    compose with ``key_bias`` and dropout and always run the streaming kernels.  A fully
    masked row gives zero context and lse = +inf."""
    D = head_dim
    masked = bool(causal) or attn_bias is not None
    if _cuda(qkv) and D not in (64, 128):
        assert attn_supported(S, D), (S, D)
        Dp = _pad_dim(D)
        ctx, lse = attn_fwd(_pad_heads(qkv, B * S, 3, H, D, Dp), key_bias, B, S, H, scale, p, seed, salt, Dp,
                            causal=causal, attn_bias=attn_bias)
        return _unpad_heads(ctx, B * S, 1, H, D, Dp), lse
    if _cuda(qkv):
        assert attn_supported(S, D) and qkv.is_contiguous() and tuple(qkv.shape) == (B * S, 3 * H * D)
        assert key_bias is None or (key_bias.is_contiguous() and tuple(key_bias.shape) == (B, S))
        ctx = torch.empty(B * S, H * D, device=qkv.device, dtype=torch.bfloat16)
        lse = torch.empty(B * H * S, device=qkv.device, dtype=torch.float32)
        if masked:
            ab, sb, sh = attn_bias_arg(attn_bias, B, S, H)
            _lib.call('mlc_flash_fwd_masked', _lib.ptr(qkv), _lib.ptr(key_bias), _lib.ptr(ctx), _lib.ptr(lse), B, S,
                      H, D, float(scale), float(p), _lib.ptr(seed), salt, int(bool(causal)), _lib.ptr(ab), sb, sh,
                      _lib.stream())
        elif _attn_small(S, D):
            _lib.call('mlc_attn_fwd', _lib.ptr(qkv), _lib.ptr(key_bias), _lib.ptr(ctx), _lib.ptr(lse), B, S, H,
                      float(scale), float(p), _lib.ptr(seed), salt, _lib.stream())
        else:
            _lib.call('mlc_flash_fwd', _lib.ptr(qkv), _lib.ptr(key_bias), _lib.ptr(ctx), _lib.ptr(lse), B, S, H, D,
                      float(scale), float(p), _lib.ptr(seed), salt, _lib.stream())
        return ctx, lse
    q, k, v, x = _attn_ref_scores(qkv, key_bias, B, S, H, scale, D, causal, attn_bias)
    P = torch.softmax(x, -1).nan_to_num(0.0)
    Pd = P
    if p > 0:
        m = keep_mask((B, H, S, S), p, _seed_val(seed), salt)
        Pd = torch.where(m, P / (1 - p), torch.zeros_like(P))
    ctx = torch.matmul(Pd, v).permute(0, 2, 1, 3).reshape(B * S, H * D)
    lse = torch.logsumexp(x, -1).reshape(-1)
    if masked:
        lse = torch.where(lse == float('-inf'), torch.full_like(lse, float('inf')), lse)   # the kernels' +inf
    return ctx.to(torch.bfloat16), lse


def attn_bwd(qkv, key_bias, dctx, lse, B, S, H, scale, p=0.0, seed=None, salt=0, head_dim: int = 64, ctx=None, *,
             causal: bool = False, attn_bias=None):
    """Gradient of :func:`attn_fwd` wrt ``qkv``: returns dqkv [B*S, 3*H*D] bf16.  ``ctx``
    (the forward output) is needed by the streaming kernels (rowsum(dO * O)).  ``causal`` /
    ``attn_bias`` as in the forward; masks are constants (no gradient)."""
    D = head_dim
    masked = bool(causal) or attn_bias is not None
    if _cuda(qkv) and D not in (64, 128):
        assert attn_supported(S, D) and ctx is not None, (S, D)
        Dp = _pad_dim(D)
        dq = attn_bwd(_pad_heads(qkv, B * S, 3, H, D, Dp), key_bias, _pad_heads(dctx, B * S, 1, H, D, Dp), lse,
                      B, S, H, scale, p, seed, salt, Dp, ctx=_pad_heads(ctx, B * S, 1, H, D, Dp), causal=causal,
                      attn_bias=attn_bias)
        return _unpad_heads(dq, B * S, 3, H, D, Dp)
    if _cuda(qkv):
        assert attn_supported(S, D) and qkv.is_contiguous() and tuple(qkv.shape) == (B * S, 3 * H * D)
        assert dctx.is_contiguous() and tuple(dctx.shape) == (B * S, H * D) and lse.numel() == B * H * S
        assert key_bias is None or (key_bias.is_contiguous() and tuple(key_bias.shape) == (B, S))
        dqkv = torch.empty_like(qkv)
        if masked:
            assert ctx is not None and ctx.is_contiguous() and ctx.shape == dctx.shape
            ab, sb, sh = attn_bias_arg(attn_bias, B, S, H)
            dot = torch.empty(B * H * S, device=qkv.device, dtype=torch.float32)
            _lib.call('mlc_flash_bwd_masked', _lib.ptr(qkv), _lib.ptr(key_bias), _lib.ptr(ctx), _lib.ptr(dctx),
                      _lib.ptr(lse), _lib.ptr(dot), _lib.ptr(dqkv), B, S, H, D, float(scale), float(p),
                      _lib.ptr(seed), salt, int(bool(causal)), _lib.ptr(ab), sb, sh, _lib.stream())
        elif _attn_small(S, D):
            _lib.call('mlc_attn_bwd', _lib.ptr(qkv), _lib.ptr(key_bias), _lib.ptr(dctx), _lib.ptr(lse),
                      _lib.ptr(dqkv), B, S, H, float(scale), float(p), _lib.ptr(seed), salt, _lib.stream())
        else:
            assert ctx is not None and ctx.is_contiguous() and ctx.shape == dctx.shape
            dot = torch.empty(B * H * S, device=qkv.device, dtype=torch.float32)
            _lib.call('mlc_flash_bwd', _lib.ptr(qkv), _lib.ptr(key_bias), _lib.ptr(ctx), _lib.ptr(dctx),
                      _lib.ptr(lse), _lib.ptr(dot), _lib.ptr(dqkv), B, S, H, D, float(scale), float(p),
                      _lib.ptr(seed), salt, _lib.stream())
        return dqkv
    q, k, v, P, E = _attn_ref_probs(qkv, key_bias, B, S, H, scale, D, causal, attn_bias)
    do = dctx.float().view(B, S, H, D).permute(0, 2, 1, 3)
    m = keep_mask((B, H, S, S), p, _seed_val(seed), salt) if p > 0 else None
    Pd = torch.where(m, P / (1 - p), torch.zeros_like(P)) if m is not None else P
    dv = torch.matmul(Pd.transpose(-1, -2), do)
    dPd = torch.matmul(do, v.transpose(-1, -2))
    dP = torch.where(m, dPd / (1 - p), torch.zeros_like(dPd)) if m is not None else dPd
    dS = scale * P * (dP - (P * dP).sum(-1, keepdim=True))
    dq = torch.matmul(dS, k)
    dk = torch.matmul(dS.transpose(-1, -2), q)
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B * S, 3 * E)
    return dqkv.to(torch.bfloat16)


# ---------------------------------------------------------------------------- grouped-query attention
def _gqa_group(H: int, Hkv: int) -> int:
    if Hkv < 1 or H % Hkv != 0:
        raise ValueError(f'grouped-query attention: {H} query heads are no multiple of {Hkv} key/value heads')
    return H // Hkv


def _gqa_expand(qkv, B, S, H, Hkv, D):
    """fp32 q [B, H, S, D] and k, v expanded to the query heads (head h reads K/V head h / G)."""
    G = H // Hkv
    q, k, v = qkv.float().view(B, S, H + 2 * Hkv, D).permute(0, 2, 1, 3).split([H, Hkv, Hkv], 1)
    return q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)


def attn_fwd_gqa(qkv, key_bias, B, S, H, Hkv, scale, p=0.0, seed=None, salt=0, head_dim: int = 64, *,
                 causal: bool = False, attn_bias=None):
    """Grouped-query attention: ``Hkv`` key/value heads serve ``H`` query heads (``H % Hkv == 0``,
    ``Hkv == 1`` is multi-query), query head h reading K/V head ``h // (H // Hkv)`` - what
    ``F.scaled_dot_product_attention(enable_gqa=True)`` computes.  ``qkv`` [B*S, (H + 2*Hkv)*D]:
    Q head h at column h*D, K head j at (H + j)*D, V head j at (H + Hkv + j)*D.  Returns
    (ctx [B*S, H*D] bf16, lse [B*H*S] fp32).  ``key_bias`` / ``causal`` / ``attn_bias`` / dropout
    as in :func:`attn_fwd`; the bias and the dropout element are indexed by the query head, so a
    call of :func:`attn_fwd` over expanded K/V sees the same bias and drops the same elements.
    Always the streaming kernels (``mlc_flash_fwd_gqa``)."""
    D = head_dim
    _gqa_group(H, Hkv)
    if _cuda(qkv) and D not in (64, 128):
        assert attn_supported(S, D), (S, D)
        Dp = _pad_dim(D)
        ctx, lse = attn_fwd_gqa(_pad_heads(qkv, B * S, 1, H + 2 * Hkv, D, Dp), key_bias, B, S, H, Hkv, scale, p, seed,
                                salt, Dp, causal=causal, attn_bias=attn_bias)
        return _unpad_heads(ctx, B * S, 1, H, D, Dp), lse
    if _cuda(qkv):
        assert attn_supported(S, D) and qkv.is_contiguous() and tuple(qkv.shape) == (B * S, (H + 2 * Hkv) * D)
        assert key_bias is None or (key_bias.is_contiguous() and tuple(key_bias.shape) == (B, S))
        ctx = torch.empty(B * S, H * D, device=qkv.device, dtype=torch.bfloat16)
        lse = torch.empty(B * H * S, device=qkv.device, dtype=torch.float32)
        ab, sb, sh = attn_bias_arg(attn_bias, B, S, H)
        _lib.call('mlc_flash_fwd_gqa', _lib.ptr(qkv), _lib.ptr(key_bias), _lib.ptr(ctx), _lib.ptr(lse), B, S, H, Hkv,
                  D, float(scale), float(p), _lib.ptr(seed), salt, int(bool(causal)), _lib.ptr(ab), sb, sh,
                  _lib.stream())
        return ctx, lse
    q, k, v = _gqa_expand(qkv, B, S, H, Hkv, D)
    x = _gqa_scores(q, k, key_bias, B, S, H, scale, causal, attn_bias)
    P = torch.softmax(x, -1).nan_to_num(0.0)
    if p > 0:
        m = keep_mask((B, H, S, S), p, _seed_val(seed), salt)
        P = torch.where(m, P / (1 - p), torch.zeros_like(P))
    ctx = torch.matmul(P, v).permute(0, 2, 1, 3).reshape(B * S, H * D)
    lse = torch.logsumexp(x, -1).reshape(-1)
    lse = torch.where(lse == float('-inf'), torch.full_like(lse, float('inf')), lse)   # the kernels' +inf
    return ctx.to(torch.bfloat16), lse


def _gqa_scores(q, k, key_bias, B, S, H, scale, causal, attn_bias):
    x = torch.matmul(q, k.transpose(-1, -2)) * scale
    if key_bias is not None:
        x = x + key_bias.float()[:, None, None, :]
    if attn_bias is not None:
        x = x + attn_bias_arg(attn_bias, B, S, H)[0]
    if causal:
        x = x.masked_fill(torch.ones(S, S, dtype=torch.bool, device=x.device).triu(1), float('-inf'))
    return x


def attn_bwd_gqa(qkv, key_bias, dctx, lse, B, S, H, Hkv, scale, p=0.0, seed=None, salt=0, head_dim: int = 64,
                 ctx=None, *, causal: bool = False, attn_bias=None):
    """Gradient of :func:`attn_fwd_gqa` wrt ``qkv``: dqkv [B*S, (H + 2*Hkv)*D] bf16, fully
    written.  dK / dV of a K/V head are the sum over its group's query heads, accumulated in
    fp32 inside one kernel block (``mlc_flash_bwd_gqa``) and rounded once.  ``ctx`` is the
    forward output."""
    D = head_dim
    G = _gqa_group(H, Hkv)
    if _cuda(qkv) and D not in (64, 128):
        assert attn_supported(S, D) and ctx is not None, (S, D)
        Dp = _pad_dim(D)
        dq = attn_bwd_gqa(_pad_heads(qkv, B * S, 1, H + 2 * Hkv, D, Dp), key_bias,
                          _pad_heads(dctx, B * S, 1, H, D, Dp), lse, B, S, H, Hkv, scale, p, seed, salt, Dp,
                          ctx=_pad_heads(ctx, B * S, 1, H, D, Dp), causal=causal, attn_bias=attn_bias)
        return _unpad_heads(dq, B * S, 1, H + 2 * Hkv, D, Dp)
    if _cuda(qkv):
        assert attn_supported(S, D) and qkv.is_contiguous() and tuple(qkv.shape) == (B * S, (H + 2 * Hkv) * D)
        assert dctx.is_contiguous() and tuple(dctx.shape) == (B * S, H * D) and lse.numel() == B * H * S
        assert key_bias is None or (key_bias.is_contiguous() and tuple(key_bias.shape) == (B, S))
        assert ctx is not None and ctx.is_contiguous() and ctx.shape == dctx.shape
        dqkv = torch.empty_like(qkv)
        ab, sb, sh = attn_bias_arg(attn_bias, B, S, H)
        dot = torch.empty(B * H * S, device=qkv.device, dtype=torch.float32)
        _lib.call('mlc_flash_bwd_gqa', _lib.ptr(qkv), _lib.ptr(key_bias), _lib.ptr(ctx), _lib.ptr(dctx),
                  _lib.ptr(lse), _lib.ptr(dot), _lib.ptr(dqkv), B, S, H, Hkv, D, float(scale), float(p),
                  _lib.ptr(seed), salt, int(bool(causal)), _lib.ptr(ab), sb, sh, _lib.stream())
        return dqkv
    q, k, v = _gqa_expand(qkv, B, S, H, Hkv, D)
    P = torch.softmax(_gqa_scores(q, k, key_bias, B, S, H, scale, causal, attn_bias), -1).nan_to_num(0.0)
    do = dctx.float().view(B, S, H, D).permute(0, 2, 1, 3)
    m = keep_mask((B, H, S, S), p, _seed_val(seed), salt) if p > 0 else None
    Pd = torch.where(m, P / (1 - p), torch.zeros_like(P)) if m is not None else P
    dPd = torch.matmul(do, v.transpose(-1, -2))
    dP = torch.where(m, dPd / (1 - p), torch.zeros_like(dPd)) if m is not None else dPd
    dS = scale * P * (dP - (P * dP).sum(-1, keepdim=True))
    dq = torch.matmul(dS, k)
    dk = torch.matmul(dS.transpose(-1, -2), q).view(B, Hkv, G, S, D).sum(2)      # the group's sum
    dv = torch.matmul(Pd.transpose(-1, -2), do).view(B, Hkv, G, S, D).sum(2)
    dqkv = torch.cat([dq, dk, dv], 1).permute(0, 2, 1, 3).reshape(B * S, (H + 2 * Hkv) * D)
    return dqkv.to(torch.bfloat16)


# ---------------------------------------------------------------------------- packed (varlen) attention
def check_cu_seqlens(cu_seqlens, T: int, max_len: int):
    """``cu_seqlens`` (int32 [nseq_max + 1]: sequence b owns rows cu[b] .. cu[b+1]-1 of a
    [T]-row buffer) checked while it is still on the host: starts at 0, non-decreasing, ends
    within ``T``, every length <= ``max_len``.  ValueError otherwise.  The kernels clamp what
    they read from device memory, so a bad vector there costs wrong numbers, never a fault; a
    vector that is already on the device is not read back."""
    if cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 or cu_seqlens.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'cu_seqlens: a 1-D int32 vector of nseq_max + 1 entries, not {tuple(cu_seqlens.shape)} '
                         f'{cu_seqlens.dtype}')
    if cu_seqlens.device.type != 'cpu':
        return
    cu = cu_seqlens.tolist()
    lens = [b - a for a, b in zip(cu, cu[1:])]
    if cu[0] != 0 or min(lens) < 0:
        raise ValueError(f'cu_seqlens must start at 0 and be non-decreasing (got {cu})')
    if cu[-1] > T:
        raise ValueError(f'cu_seqlens ends at row {cu[-1]}, past the {T} rows of the buffer')
    if max(lens) > max_len:
        raise ValueError(f'a sequence of {max(lens)} rows is over max_len {max_len}')


def _no_bias_with_cu(key_bias, attn_bias):
    if key_bias is not None or attn_bias is not None:
        raise ValueError('the packed (cu_seqlens) attention takes no key_bias / attn_bias: sequences are '
                         'delimited by cu_seqlens, and additive masks are not part of the varlen kernels')


def _seq_keep(b, H, L, max_len, p, seed, salt):
    """Keep mask [H, L, L] of packed sequence b: the padded layout's element index at
    S = max_len, ((b*H + h)*max_len + q)*max_len + key."""
    h = torch.arange(H, dtype=torch.int64)[:, None, None]
    q = torch.arange(L, dtype=torch.int64)[None, :, None]
    k = torch.arange(L, dtype=torch.int64)[None, None, :]
    idx = ((b * H + h) * max_len + q) * max_len + k
    return (_hash(_seed_val(seed), salt, idx) >> 8) >= drop_threshold(p)


def _seq_slices(cu_seqlens):
    cu = cu_seqlens.tolist()
    return [(b, c0, c1) for b, (c0, c1) in enumerate(zip(cu, cu[1:])) if c1 > c0]


def _varlen_alloc(max_len, D, causal):
    """How a packed call's outputs are allocated: the whole-sequence kernels (``max_len`` <= 128,
    D = 64, not causal, knob ``MLC_ATTN_VARLEN128`` on) zero the rows of no sequence themselves,
    the streaming kernels write real rows only and want zero-filled buffers."""
    whole = _lib.load().mlc_flash_varlen128_ok(int(max_len), int(D), int(bool(causal))) == 1
    return torch.empty if whole else torch.zeros


def attn_fwd_varlen(qkv, cu_seqlens, max_len, H, scale, p=0.0, seed=None, salt=0, head_dim: int = 64, *,
                    causal: bool = False, key_bias=None, attn_bias=None):
    """Fused attention over packed sequences: ``qkv`` [T, 3*H*D] holds the sequences back to
    back, sequence b in rows cu_seqlens[b] .. cu_seqlens[b+1]-1 (int32 [nseq_max + 1]; equal
    neighbours = an empty slot), every length <= ``max_len``.  Returns (ctx [T, H*D] bf16, lse
    [H*T] fp32, index h*T + row).  Rows that belong to no sequence (cu[-1] .. T-1) come back as
    exact zeros (the whole-sequence kernels' tail blocks write them; the streaming kernels get
    zero-filled outputs and write real rows only).  Dropout drops element
    ((b*H + h)*max_len + q)*max_len + key with q / key relative to the sequence - exactly what
    :func:`attn_fwd` over the same sequences padded to S = max_len drops.  ``causal`` as in
    :func:`attn_fwd`; bias operands are refused (ValueError).  ``cu_seqlens`` is validated
    (:func:`check_cu_seqlens`) when it arrives on the host."""
    _no_bias_with_cu(key_bias, attn_bias)
    D, T = head_dim, qkv.shape[0]
    check_cu_seqlens(cu_seqlens, T, max_len)
    nseq = cu_seqlens.numel() - 1
    if _cuda(qkv) and D not in (64, 128):
        assert attn_supported(max_len, D), (max_len, D)
        Dp = _pad_dim(D)
        ctx, lse = attn_fwd_varlen(_pad_heads(qkv, T, 3, H, D, Dp), cu_seqlens, max_len, H, scale, p, seed, salt, Dp,
                                   causal=causal)
        return _unpad_heads(ctx, T, 1, H, D, Dp), lse
    if _cuda(qkv):
        assert attn_supported(max_len, D) and qkv.is_contiguous() and tuple(qkv.shape) == (T, 3 * H * D)
        cu = cu_seqlens.to(device=qkv.device, dtype=torch.int32).contiguous()
        new = _varlen_alloc(max_len, D, causal)
        ctx = new(T, H * D, device=qkv.device, dtype=torch.bfloat16)
        lse = new(H * T, device=qkv.device, dtype=torch.float32)
        _lib.call('mlc_flash_fwd_varlen', _lib.ptr(qkv), _lib.ptr(cu), _lib.ptr(ctx), _lib.ptr(lse), T, nseq,
                  int(max_len), H, D, float(scale), float(p), _lib.ptr(seed), salt, int(bool(causal)), _lib.stream())
        return ctx, lse
    ctx = torch.zeros(T, H * D)
    lse = torch.zeros(H, T)
    for b, c0, c1 in _seq_slices(cu_seqlens):
        L = c1 - c0
        q, k, v, x = _attn_ref_scores(qkv[c0:c1], None, 1, L, H, scale, D, causal)
        P = torch.softmax(x, -1)
        if p > 0:
            P = torch.where(_seq_keep(b, H, L, max_len, p, seed, salt)[None], P / (1 - p), torch.zeros_like(P))
        ctx[c0:c1] = torch.matmul(P, v).permute(0, 2, 1, 3).reshape(L, H * D)
        lse[:, c0:c1] = torch.logsumexp(x, -1)[0]
    return ctx.to(torch.bfloat16), lse.reshape(-1)


def attn_bwd_varlen(qkv, cu_seqlens, max_len, dctx, lse, H, scale, p=0.0, seed=None, salt=0, head_dim: int = 64,
                    ctx=None, *, causal: bool = False, key_bias=None, attn_bias=None):
    """Gradient of :func:`attn_fwd_varlen` wrt ``qkv``: dqkv [T, 3*H*D] bf16, exact zeros in
    the rows of no sequence.  ``ctx`` is the forward's output (the kernels need it)."""
    _no_bias_with_cu(key_bias, attn_bias)
    D, T = head_dim, qkv.shape[0]
    check_cu_seqlens(cu_seqlens, T, max_len)
    nseq = cu_seqlens.numel() - 1
    if _cuda(qkv) and D not in (64, 128):
        assert attn_supported(max_len, D) and ctx is not None, (max_len, D)
        Dp = _pad_dim(D)
        dq = attn_bwd_varlen(_pad_heads(qkv, T, 3, H, D, Dp), cu_seqlens, max_len, _pad_heads(dctx, T, 1, H, D, Dp),
                             lse, H, scale, p, seed, salt, Dp, ctx=_pad_heads(ctx, T, 1, H, D, Dp), causal=causal)
        return _unpad_heads(dq, T, 3, H, D, Dp)
    if _cuda(qkv):
        assert attn_supported(max_len, D) and qkv.is_contiguous() and tuple(qkv.shape) == (T, 3 * H * D)
        assert dctx.is_contiguous() and tuple(dctx.shape) == (T, H * D) and lse.numel() == H * T
        assert ctx is not None and ctx.is_contiguous() and ctx.shape == dctx.shape
        cu = cu_seqlens.to(device=qkv.device, dtype=torch.int32).contiguous()
        dqkv = _varlen_alloc(max_len, D, causal)(T, 3 * H * D, device=qkv.device, dtype=torch.bfloat16)
        dot = torch.empty(H * T, device=qkv.device, dtype=torch.float32)
        _lib.call('mlc_flash_bwd_varlen', _lib.ptr(qkv), _lib.ptr(cu), _lib.ptr(ctx), _lib.ptr(dctx), _lib.ptr(lse),
                  _lib.ptr(dot), _lib.ptr(dqkv), T, nseq, int(max_len), H, D, float(scale), float(p), _lib.ptr(seed),
                  salt, int(bool(causal)), _lib.stream())
        return dqkv
    E = H * D
    dqkv = torch.zeros(T, 3 * E)
    for b, c0, c1 in _seq_slices(cu_seqlens):
        L = c1 - c0
        q, k, v, P, _ = _attn_ref_probs(qkv[c0:c1], None, 1, L, H, scale, D, causal)
        do = dctx[c0:c1].float().view(1, L, H, D).permute(0, 2, 1, 3)
        m = _seq_keep(b, H, L, max_len, p, seed, salt)[None] if p > 0 else None
        Pd = torch.where(m, P / (1 - p), torch.zeros_like(P)) if m is not None else P
        dv = torch.matmul(Pd.transpose(-1, -2), do)
        dPd = torch.matmul(do, v.transpose(-1, -2))
        dP = torch.where(m, dPd / (1 - p), torch.zeros_like(dPd)) if m is not None else dPd
        dS = scale * P * (dP - (P * dP).sum(-1, keepdim=True))
        dq = torch.matmul(dS, k)
        dk = torch.matmul(dS.transpose(-1, -2), q)
        dqkv[c0:c1] = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(L, 3 * E)
    return dqkv.to(torch.bfloat16)


# ---------------------------------------------------------------------------- packed grouped-query attention
def attn_fwd_gqa_varlen(qkv, cu_seqlens, max_len, H, Hkv, scale, p=0.0, seed=None, salt=0, head_dim: int = 64, *,
                        causal: bool = False, key_bias=None, attn_bias=None):
    """Grouped-query attention over packed sequences: the rows of :func:`attn_fwd_varlen`
    (``cu_seqlens`` int32 [nseq_max + 1], every length <= ``max_len``) with the columns of
    :func:`attn_fwd_gqa`: ``qkv`` [T, (H + 2*Hkv)*D], Q head h at column h*D, K head j at
    (H + j)*D, V head j at (H + Hkv + j)*D.  Returns (ctx [T, H*D] bf16, lse [H*T] fp32, index
    h*T + row with h the query head).  Rows of no sequence come back as exact zeros.  Dropout
    drops element ((b*H + h)*max_len + q)*max_len + key, what the padded grouped call at
    S = max_len drops.  Bias operands are refused (ValueError).  Always the streaming kernels
    (``mlc_flash_fwd_gqa_varlen``), whatever ``max_len``.  Rotary embeddings on a packed batch:
    ``rope_qkv_(pos_ids=)`` on ``qkv`` first."""
    _no_bias_with_cu(key_bias, attn_bias)
    _gqa_group(H, Hkv)
    D, T = head_dim, qkv.shape[0]
    check_cu_seqlens(cu_seqlens, T, max_len)
    nseq = cu_seqlens.numel() - 1
    if _cuda(qkv) and D not in (64, 128):
        assert attn_supported(max_len, D), (max_len, D)
        Dp = _pad_dim(D)
        ctx, lse = attn_fwd_gqa_varlen(_pad_heads(qkv, T, 1, H + 2 * Hkv, D, Dp), cu_seqlens, max_len, H, Hkv, scale,
                                       p, seed, salt, Dp, causal=causal)
        return _unpad_heads(ctx, T, 1, H, D, Dp), lse
    if _cuda(qkv):
        assert attn_supported(max_len, D) and qkv.is_contiguous() and tuple(qkv.shape) == (T, (H + 2 * Hkv) * D)
        cu = cu_seqlens.to(device=qkv.device, dtype=torch.int32).contiguous()
        ctx = torch.zeros(T, H * D, device=qkv.device, dtype=torch.bfloat16)
        lse = torch.zeros(H * T, device=qkv.device, dtype=torch.float32)
        _lib.call('mlc_flash_fwd_gqa_varlen', _lib.ptr(qkv), _lib.ptr(cu), _lib.ptr(ctx), _lib.ptr(lse), T, nseq,
                  int(max_len), H, Hkv, D, float(scale), float(p), _lib.ptr(seed), salt, int(bool(causal)),
                  _lib.stream())
        return ctx, lse
    ctx = torch.zeros(T, H * D)
    lse = torch.zeros(H, T)
    for b, c0, c1 in _seq_slices(cu_seqlens):
        L = c1 - c0
        q, k, v = _gqa_expand(qkv[c0:c1], 1, L, H, Hkv, D)
        x = _gqa_scores(q, k, None, 1, L, H, scale, causal, None)
        P = torch.softmax(x, -1)
        if p > 0:
            P = torch.where(_seq_keep(b, H, L, max_len, p, seed, salt)[None], P / (1 - p), torch.zeros_like(P))
        ctx[c0:c1] = torch.matmul(P, v).permute(0, 2, 1, 3).reshape(L, H * D)
        lse[:, c0:c1] = torch.logsumexp(x, -1)[0]
    return ctx.to(torch.bfloat16), lse.reshape(-1)


def attn_bwd_gqa_varlen(qkv, cu_seqlens, max_len, dctx, lse, H, Hkv, scale, p=0.0, seed=None, salt=0,
                        head_dim: int = 64, ctx=None, *, causal: bool = False, key_bias=None, attn_bias=None):
    """Gradient of :func:`attn_fwd_gqa_varlen` wrt ``qkv``: dqkv [T, (H + 2*Hkv)*D] bf16, exact
    zeros in the rows of no sequence.  dK / dV of a K/V head are the sum over its group's query
    heads, accumulated in fp32 inside one kernel block per (sequence, K/V head, 128 keys) that
    streams only its own sequence's tiles (``mlc_flash_bwd_gqa_varlen``).  ``ctx`` is the
    forward output."""
    _no_bias_with_cu(key_bias, attn_bias)
    G = _gqa_group(H, Hkv)
    D, T = head_dim, qkv.shape[0]
    check_cu_seqlens(cu_seqlens, T, max_len)
    nseq = cu_seqlens.numel() - 1
    if _cuda(qkv) and D not in (64, 128):
        assert attn_supported(max_len, D) and ctx is not None, (max_len, D)
        Dp = _pad_dim(D)
        dq = attn_bwd_gqa_varlen(_pad_heads(qkv, T, 1, H + 2 * Hkv, D, Dp), cu_seqlens, max_len,
                                 _pad_heads(dctx, T, 1, H, D, Dp), lse, H, Hkv, scale, p, seed, salt, Dp,
                                 ctx=_pad_heads(ctx, T, 1, H, D, Dp), causal=causal)
        return _unpad_heads(dq, T, 1, H + 2 * Hkv, D, Dp)
    if _cuda(qkv):
        assert attn_supported(max_len, D) and qkv.is_contiguous() and tuple(qkv.shape) == (T, (H + 2 * Hkv) * D)
        assert dctx.is_contiguous() and tuple(dctx.shape) == (T, H * D) and lse.numel() == H * T
        assert ctx is not None and ctx.is_contiguous() and ctx.shape == dctx.shape
        cu = cu_seqlens.to(device=qkv.device, dtype=torch.int32).contiguous()
        dqkv = torch.zeros_like(qkv)
        dot = torch.empty(H * T, device=qkv.device, dtype=torch.float32)
        _lib.call('mlc_flash_bwd_gqa_varlen', _lib.ptr(qkv), _lib.ptr(cu), _lib.ptr(ctx), _lib.ptr(dctx),
                  _lib.ptr(lse), _lib.ptr(dot), _lib.ptr(dqkv), T, nseq, int(max_len), H, Hkv, D, float(scale),
                  float(p), _lib.ptr(seed), salt, int(bool(causal)), _lib.stream())
        return dqkv
    dqkv = torch.zeros(T, (H + 2 * Hkv) * D)
    for b, c0, c1 in _seq_slices(cu_seqlens):
        L = c1 - c0
        q, k, v = _gqa_expand(qkv[c0:c1], 1, L, H, Hkv, D)
        P = torch.softmax(_gqa_scores(q, k, None, 1, L, H, scale, causal, None), -1)
        do = dctx[c0:c1].float().view(1, L, H, D).permute(0, 2, 1, 3)
        m = _seq_keep(b, H, L, max_len, p, seed, salt)[None] if p > 0 else None
        Pd = torch.where(m, P / (1 - p), torch.zeros_like(P)) if m is not None else P
        dPd = torch.matmul(do, v.transpose(-1, -2))
        dP = torch.where(m, dPd / (1 - p), torch.zeros_like(dPd)) if m is not None else dPd
        dS = scale * P * (dP - (P * dP).sum(-1, keepdim=True))
        dq = torch.matmul(dS, k)
        dk = torch.matmul(dS.transpose(-1, -2), q).view(1, Hkv, G, L, D).sum(2)      # the group's sum
        dv = torch.matmul(Pd.transpose(-1, -2), do).view(1, Hkv, G, L, D).sum(2)
        dqkv[c0:c1] = torch.cat([dq, dk, dv], 1).permute(0, 2, 1, 3).reshape(L, (H + 2 * Hkv) * D)
    return dqkv.to(torch.bfloat16)


# ---------------------------------------------------------------------------- dense layers
_WS = {}
_WS_OLD = []   # superseded buffers stay alive: a captured graph may still point at them


def gemm_workspace(device, n: int) -> torch.Tensor:
    """fp32 split-K slab workspace per device (``splits`` x M x N partial sums, fully
    overwritten by each split-K GEMM), grown on demand - first during eager warm-up, so
    graph capture reuses it."""
    from .functional import workspace_key, workspace_store
    key = workspace_key(device)
    store = workspace_store(_WS)
    buf = store.get(key)
    if buf is None or buf.numel() < n:
        if buf is not None:
            _WS_OLD.append(buf)
        buf = torch.empty(max(n, 1 << 20), device=device, dtype=torch.float32)
        store[key] = buf
    return buf


def _gelu(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def _dgelu(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def dense_fwd(x, w, bias=None, act: int = 0, want_preact: bool = False, addend=None):
    """y = act(x @ w^T + bias) [+ addend]: x [M, K] bf16, w [N, K] bf16, bias fp32 [N],
    addend bf16 [M, N] (a residual summed in the epilogue).  Returns (y, u) with u the bf16
    pre-activation (when ``want_preact``).  ``act`` 1 = exact-erf GELU; 2 = GELU returning
    u = gelu'(pre-activation) instead, for ``dense_dgrad(..., dact_is_deriv=True)`` (the
    backward epilogue then only multiplies)."""
    M, K = x.shape
    N = w.shape[0]
    if _cuda(x):
        y = torch.empty(M, N, device=x.device, dtype=torch.bfloat16)
        u = torch.empty_like(y) if want_preact else None
        if addend is not None:
            assert addend.dtype == torch.bfloat16 and addend.is_contiguous() and tuple(addend.shape) == (M, N)
        _lib.call('mlc_gemm_bf16_ex', _lib.ptr(x), _lib.ptr(w), _lib.ptr(y), M, N, K, K, K, N, 0, 1,
                  _lib.ptr(bias), act, _lib.ptr(u), _lib.ptr(addend), None,
                  _lib.ptr(gemm_workspace(x.device, 4 * M * N)), 4 * M * N, _lib.stream())
        return y, u
    z = x.float() @ w.float().t()
    if bias is not None:
        z = z + bias
    if act == 2:
        u = _dgelu(z).to(torch.bfloat16) if want_preact else None
    else:
        u = z.to(torch.bfloat16) if want_preact else None
    if act in (1, 2):
        z = _gelu(z)
    if addend is not None:
        z = z + addend.float()
    return z.to(torch.bfloat16), u


def dense_dgrad(dy, w, dact_u=None, addend=None, wt=None, dact_is_deriv=False):
    """dx = (dy @ w) [* gelu'(dact_u)] [+ addend]: dy [M, N], w [N, K] -> [M, K] bf16.
    ``dact_is_deriv``: ``dact_u`` already holds gelu'(u) (``dense_fwd(act=2)``), multiply.
    ``wt`` = w^T ([K, N], e.g. a ``Fn.WtTable`` view): the GEMM reads both operands
    K-contiguous (the LDS-DMA main loop) instead of w as an MN-contiguous tile."""
    M, N = dy.shape
    K = w.shape[1]
    if _cuda(dy):
        dx = torch.empty(M, K, device=dy.device, dtype=torch.bfloat16)
        b, ldb, tb = (wt, N, 1) if wt is not None else (w, K, 0)
        if wt is not None:
            assert tuple(wt.shape) == (K, N), (wt.shape, w.shape)
        _lib.call('mlc_gemm_bf16_ex', _lib.ptr(dy), _lib.ptr(b), _lib.ptr(dx), M, K, N, N, ldb, K, 0, tb, None,
                  4 if (dact_u is not None and dact_is_deriv) else 0,
                  None, _lib.ptr(addend), _lib.ptr(dact_u), _lib.ptr(gemm_workspace(dy.device, 4 * M * K)),
                  4 * M * K, _lib.stream())
        return dx
    if wt is not None:
        w = wt.t()
    z = dy.float() @ w.float()
    z = z.to(torch.bfloat16).float()
    if dact_u is not None:
        z = z * (dact_u.float() if dact_is_deriv else _dgelu(dact_u.float()))
    if addend is not None:
        z = z + addend.float()
    return z.to(torch.bfloat16)


def dact_gelu(dy, u):
    """dy * gelu'(u) as a standalone op (used when the GEMM producing dy cannot fuse it)."""
    return (dy.float() * _dgelu(u.float())).to(torch.bfloat16)


_SCRATCH = {}


def colsum_scratch(device, C: int) -> torch.Tensor:
    """A zeroed NSTAT*C fp32 buffer per device, grown on demand; the kernel leaves it
    zeroed, so every call of a step (and a captured graph) can share it."""
    from .functional import workspace_key, workspace_store
    # per stream role and capture scope, like the split-K slabs: the kernel relies on the
    # buffer being zero on entry, so two colsums that overlap must never share one
    key = workspace_key(device)
    store = workspace_store(_SCRATCH)
    buf = store.get(key)
    if buf is None or buf.numel() < NSTAT * C:
        if buf is not None:
            _WS_OLD.append(buf)
        buf = torch.zeros(NSTAT * max(C, 4096), device=device, dtype=torch.float32)
        store[key] = buf
    return buf


def colsum_acc(g, out, scratch=None):
    """out += column sums of g [R, C] bf16."""
    R, C = g.shape
    if _cuda(g):
        sc = scratch if scratch is not None else colsum_scratch(g.device, C)
        _lib.call('mlc_colsum_acc', _lib.ptr(g), _lib.ptr(out), _lib.ptr(sc), R, C, _lib.stream())
        return out
    out.add_(g.float().sum(0))
    return out


def dropout(x, p, seed, salt):
    if p <= 0:
        return x
    if _cuda(x):
        y = torch.empty_like(x)
        _lib.call('mlc_dropout', _lib.ptr(x), _lib.ptr(y), x.numel(), float(p), _lib.ptr(seed), salt, _lib.stream())
        return y
    m = keep_mask(tuple(x.shape), p, _seed_val(seed), salt)
    return torch.where(m, x.float() / (1 - p), torch.zeros_like(x, dtype=torch.float32)).to(x.dtype)


# ---------------------------------------------------------------------------- decoder pointwise kernels
# MLC_DECODER_NATIVE=1 (default): on the GPU rotary embedding, RMSNorm and SwiGLU run their
# kernels (csrc/kernels/decoder.hip).  0: the fp32 torch compositions below run on the GPU
# tensors too.  Measured (scripts/bench_decoder_block.py, profiles/decoder_block/): no kernel
# loses to its torch composition.
_DECODER_NATIVE = os.environ.get('MLC_DECODER_NATIVE', '1') == '1'


def decoder_native() -> bool:
    return _DECODER_NATIVE


def set_decoder_native(on: bool) -> bool:
    """Switch the decoder kernels on or off; returns the previous setting."""
    global _DECODER_NATIVE
    was, _DECODER_NATIVE = _DECODER_NATIVE, bool(on)
    return was


def _decoder_kernel(t) -> bool:
    return _cuda(t) and _DECODER_NATIVE


def rope_table(npos: int, D: int, base: float = 10000.0, device=None) -> torch.Tensor:
    """The rotary table, fp32 [npos, D]: cos(p * base^(-2i/D)) in columns [0, D/2), sin in
    [D/2, D), computed in fp64 and rounded once."""
    inv = torch.pow(torch.tensor(float(base), dtype=torch.float64),
                    -torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.arange(npos, dtype=torch.float64)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.sin()], 1).float().to(device)


def rope_qkv_(qkv, table, S, H, Hkv, D, pos_ids=None, inverse=False):
    """Rotate the Q and K heads of ``qkv`` [T, (H + 2*Hkv)*D] bf16 IN PLACE (rotate-half, as HF
    Llama; ``mlc_rope_qkv``) and return it; the V heads keep their bits.  Row r has position
    ``pos_ids[r]`` (int64 [T]) or ``r % S``, clamped into the table.  ``inverse`` negates sin: the
    inverse rotation, which is also the backward.  Like the kernel's, the torch path's write does
    not bump autograd's version counter: the caller owns the buffer."""
    T = qkv.shape[0]
    assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous() and tuple(qkv.shape) == (T, (H + 2 * Hkv) * D)
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[1] == D
    if _decoder_kernel(qkv):
        pc = pos_ids.contiguous() if pos_ids is not None else None
        _lib.call('mlc_rope_qkv', _lib.ptr(qkv), _lib.ptr(table), _lib.ptr(pc), T, S, H, Hkv, D, table.shape[0],
                  int(bool(inverse)), _lib.stream())
        return qkv
    p = pos_ids.long() if pos_ids is not None else torch.arange(T, device=qkv.device) % S
    p = p.clamp(0, table.shape[0] - 1)
    cs, sn = table[p, None, :D // 2], table[p, None, D // 2:]
    if inverse:
        sn = -sn
    heads = qkv.data.view(T, H + 2 * Hkv, D)[:, :H + Hkv]
    x1, x2 = heads[..., :D // 2].float(), heads[..., D // 2:].float()
    heads.copy_(torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1))
    return qkv


def rms_fwd(x, gamma, eps):
    """RMSNorm over rows: (y, rstd) with rstd = rsqrt(mean(x^2) + eps) fp32 [T] and
    y = bf16(x * rstd * gamma); x [T, H] bf16, gamma fp32 [H] (``mlc_rms_fwd``: H % 8 == 0,
    H <= 4096)."""
    T, H = x.shape
    if _decoder_kernel(x):
        y = torch.empty_like(x)
        rstd = torch.empty(T, device=x.device, dtype=torch.float32)
        _lib.call('mlc_rms_fwd', _lib.ptr(x), _lib.ptr(gamma), _lib.ptr(y), _lib.ptr(rstd), T, H, float(eps),
                  _lib.stream())
        return y, rstd
    xf = x.float()
    rstd = torch.rsqrt((xf * xf).mean(1) + eps)
    return (xf * rstd[:, None] * gamma).to(torch.bfloat16), rstd


_RMS_SCRATCH = {}
RMS_NSTAT = 32     # partial-sum copies of mlc_rms_bwd (fixed: deterministic mode runs one block per copy)


def rms_bwd(dy, x, rstd, gamma, dgamma, sums=None):
    """dx of :func:`rms_fwd`; ``dgamma`` is ACCUMULATED (+=).  ``sums``: fp32 [RMS_NSTAT * H]
    scratch, zero on entry and left zeroed by the kernel (a cached one by default)."""
    T, H = dy.shape
    if _decoder_kernel(dy):
        if sums is None:
            from .functional import workspace_key, workspace_store
            key = (workspace_key(dy.device), RMS_NSTAT * H)
            store = workspace_store(_RMS_SCRATCH)
            sums = store.get(key)
            if sums is None:
                sums = store[key] = torch.zeros(RMS_NSTAT * H, device=dy.device, dtype=torch.float32)
        dx = torch.empty_like(dy)
        _lib.call('mlc_rms_bwd', _lib.ptr(dy), _lib.ptr(x), _lib.ptr(rstd), _lib.ptr(gamma), _lib.ptr(dx),
                  _lib.ptr(sums), _lib.ptr(dgamma), T, H, _lib.stream())
        return dx
    d = dy.float()
    xh = x.float() * rstd[:, None]
    dgamma.add_((d * xh).sum(0))
    g = d * gamma
    b = (g * xh).mean(1, keepdim=True)
    return (rstd[:, None] * (g - xh * b)).to(torch.bfloat16)


def swiglu_fwd(gu):
    """h [T, F] = bf16(silu(g) * u) for gu [T, 2F] bf16 = gate | up (``mlc_swiglu_fwd``, F % 8 == 0)."""
    T, F2 = gu.shape
    F = F2 // 2
    if _decoder_kernel(gu):
        h = torch.empty(T, F, device=gu.device, dtype=torch.bfloat16)
        _lib.call('mlc_swiglu_fwd', _lib.ptr(gu), _lib.ptr(h), T, F, _lib.stream())
        return h
    g, u = gu[:, :F].float(), gu[:, F:].float()
    return (g * torch.sigmoid(g) * u).to(torch.bfloat16)


def swiglu_bwd(gu, dh, out=None):
    """dgu [T, 2F] bf16 of :func:`swiglu_fwd`, written into ``out`` when given (``out`` may be
    ``gu`` itself)."""
    T, F2 = gu.shape
    F = F2 // 2
    if out is None:
        out = torch.empty_like(gu)
    if _decoder_kernel(gu):
        _lib.call('mlc_swiglu_bwd', _lib.ptr(gu), _lib.ptr(dh), _lib.ptr(out), T, F, _lib.stream())
        return out
    g, u, d = gu[:, :F].float(), gu[:, F:].float(), dh.float()
    sg = torch.sigmoid(g)
    out.copy_(torch.cat([d * u * sg * (1 + g * (1 - sg)), d * g * sg], 1))
    return out


# ---------------------------------------------------------------------------- language-model head + loss
# csrc/kernels/lmhead.hip: softmax cross-entropy over z = h w^T with the logits kept in MFMA
# accumulators.  The backward writes one bf16 dlogits chunk at a time into a cached buffer and
# hands it to the existing dgrad / wgrad GEMMs.
_LM_DL = {}
LM_DL_BYTES = 256 << 20     # target size of the dlogits chunk buffer


def _lm_shapes(h, w, labels):
    T, K = h.shape
    V = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K or tuple(labels.shape) != (T,):
        raise ValueError(f'lm head: h {tuple(h.shape)}, w {tuple(w.shape)}, labels {tuple(labels.shape)} '
                         '(expected [T, K], [V, K], [T])')
    if T < 1 or K % 64 or V % 8:
        raise ValueError(f'lm head: T = {T}, K = {K}, V = {V}; the kernels need T >= 1, K % 64 == 0 and V % 8 == 0')
    assert h.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and labels.dtype == torch.int64
    assert h.is_contiguous() and w.is_contiguous() and labels.is_contiguous()
    return T, K, V


def _lm_logits(h, w, labels, ignore_index):
    """fp32 twin: logits, lse, clamped labels and the ignored-row mask"""
    z = h.float() @ w.float().t()
    ign = labels == ignore_index
    lab = torch.where(ign, torch.zeros_like(labels), labels.clamp(0, w.shape[0] - 1))
    return z, torch.logsumexp(z, 1), lab, ign


def lm_loss_fwd(h, w, labels, ignore_index=-100, splits=0):
    """Per-token cross-entropy of the logits h w^T without storing them: (nll, lse), fp32 [T].
    h [T, K] bf16, w [V, K] bf16, labels int64 [T] (``mlc_lmhead_lse``: K % 64 == 0, V % 8 == 0).
    ``nll`` is 0 where the label equals ``ignore_index``.  ``splits``: vocabulary splits per row
    tile, 0 = enough to fill the chip."""
    T, K, V = _lm_shapes(h, w, labels)
    if _cuda(h):
        sp = _lib.load().mlc_lmhead_splits(T, V, int(splits))
        part = torch.empty((2 * sp + 1) * T, device=h.device, dtype=torch.float32)
        nll, lse = (torch.empty(T, device=h.device, dtype=torch.float32) for _ in range(2))
        _lib.call('mlc_lmhead_lse', _lib.ptr(h), _lib.ptr(w), _lib.ptr(labels), _lib.ptr(part), _lib.ptr(lse),
                  _lib.ptr(nll), T, V, K, sp, int(ignore_index), _lib.stream())
        return nll, lse
    z, lse, lab, ign = _lm_logits(h, w, labels, ignore_index)
    nll = lse - z.gather(1, lab[:, None])[:, 0]
    return torch.where(ign, torch.zeros_like(nll), nll), lse


def lm_dlogits_buffer(device, rows: int, V: int) -> torch.Tensor:
    """The bf16 [rows, V] dlogits chunk, cached per device (and stream role / capture scope) like
    :func:`gemm_workspace`; superseded buffers stay alive for captured graphs."""
    from .functional import workspace_key, workspace_store
    key = workspace_key(device)
    store = workspace_store(_LM_DL)
    buf = store.get(key)
    if buf is None or buf.numel() < rows * V:
        if buf is not None:
            _WS_OLD.append(buf)
        buf = store[key] = torch.empty(rows * V, device=device, dtype=torch.bfloat16)
    return buf[:rows * V].view(rows, V)


def lm_loss_bwd(h, w, labels, lse, dnll, dw, ignore_index=-100, chunk_rows=None):
    """Backward of :func:`lm_loss_fwd`: returns dh [T, K] bf16 and ACCUMULATES (+=) the weight
    gradient into ``dw`` [V, K] fp32.  ``dnll`` fp32 [T] is the gradient arriving at each row's
    nll.  Rows go through in chunks of ``chunk_rows`` (default: the multiple of 128 that keeps the
    chunk near 256 MB): ``mlc_lmhead_dlogits`` recomputes the chunk's logits and writes
    (softmax - onehot) * dnll as bf16 into one reused buffer, then ``dense_dgrad`` and
    ``linear_wgrad`` consume it."""
    from . import functional as Fn
    T, K, V = _lm_shapes(h, w, labels)
    if chunk_rows is None:
        chunk_rows = max(128, LM_DL_BYTES // (2 * V) // 128 * 128)
    chunk_rows = min(int(chunk_rows), T)
    dh = torch.empty(T, K, device=h.device, dtype=torch.bfloat16)
    dl = lm_dlogits_buffer(h.device, chunk_rows, V) if _cuda(h) else None
    for r0 in range(0, T, chunk_rows):
        n = min(chunk_rows, T - r0)
        hc, lc = h[r0:r0 + n], labels[r0:r0 + n]
        if _cuda(h):
            g = dl[:n]
            _lib.call('mlc_lmhead_dlogits', _lib.ptr(hc), _lib.ptr(w), _lib.ptr(lc), _lib.ptr(lse[r0:r0 + n]),
                      _lib.ptr(dnll[r0:r0 + n]), _lib.ptr(g), n, V, K, 0, int(ignore_index), _lib.stream())
        else:
            z, _, lab, ign = _lm_logits(hc, w, lc, ignore_index)
            p = torch.exp(z - lse[r0:r0 + n, None])
            p.scatter_add_(1, lab[:, None], -torch.ones(n, 1))
            g = (p * torch.where(ign, torch.zeros(n), dnll[r0:r0 + n])[:, None]).to(torch.bfloat16)
        dh[r0:r0 + n] = dense_dgrad(g, w)
        Fn.linear_wgrad(g, hc, out=dw, accumulate=True)
    return dh


class _LmHeadLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, weight, labels, ignore_index, mean):
        h = hidden.reshape(-1, hidden.shape[-1]).to(torch.bfloat16).contiguous()
        w = weight.to(torch.bfloat16).contiguous()
        lab = labels.reshape(-1).contiguous()
        nll, lse = lm_loss_fwd(h, w, lab, ignore_index)
        # the normaliser stays on the device: no host sync, capturable
        scale = 1.0 / (lab != ignore_index).sum().clamp_min(1).float() if mean else torch.ones((), device=h.device)
        ctx.save_for_backward(h, w, lab, lse, scale)
        ctx.ignore_index, ctx.hshape, ctx.dtypes = ignore_index, hidden.shape, (hidden.dtype, weight.dtype)
        return nll.sum() * scale

    @staticmethod
    def backward(ctx, dloss):
        h, w, lab, lse, scale = ctx.saved_tensors
        dnll = (dloss.float() * scale).expand(h.shape[0]).contiguous()
        dw = torch.zeros(w.shape, device=w.device, dtype=torch.float32)
        dh = lm_loss_bwd(h, w, lab, lse, dnll, dw, ctx.ignore_index)
        return dh.view(ctx.hshape).to(ctx.dtypes[0]), dw.to(ctx.dtypes[1]), None, None, None


def lm_head_loss(hidden, weight, labels, ignore_index=-100, reduction='mean'):
    """Cross-entropy of ``hidden @ weight.T`` against ``labels`` as a 0-dim fp32 loss, differentiable
    in ``hidden`` ([..., K], flattened to rows) and ``weight`` ([V, K]; fp32 master weights are cast to
    bf16), on the fused kernels: :func:`lm_loss_fwd` / :func:`lm_loss_bwd`.  ``reduction``: 'mean'
    over the rows whose label is not ``ignore_index`` (counted on the device), or 'sum'."""
    if reduction not in ('mean', 'sum'):
        raise ValueError(f"lm_head_loss: reduction {reduction!r} (expected 'mean' or 'sum')")
    return _LmHeadLoss.apply(hidden, weight, labels, int(ignore_index), reduction == 'mean')


# ---------------------------------------------------------------------------- single-token attention over a K/V cache
# csrc/kernels/attn_decode.hip: one new query row per sequence against kv_cache [B, Smax, 2*Hkv*D]
# (K head j of a position at column j*D, V head j at (Hkv + j)*D: the tail of a packed qkv row).
# The lengths are device data, so one captured graph serves every step of a generation.
# With ``block_table`` (int32 [B, max_blocks]) the cache is a paged pool [num_blocks, page, 2*Hkv*D]:
# entry [b, p] names the pool block that holds positions [p*page, (p + 1)*page) of sequence b.
_DEC_PART = {}


def _decode_heads(H, Hkv, D, what):
    G = _gqa_group(H, Hkv)
    if G > 16:
        raise ValueError(f'{what}: {G} query heads per key/value head (the kernel serves at most 16)')
    if D not in (64, 128):
        raise ValueError(f'{what}: head_dim {D} (expected 64 or 128)')


def _decode_shapes(kv_cache, seq_lens, H, Hkv, D, what):
    _decode_heads(H, Hkv, D, what)
    if kv_cache.dim() != 3 or kv_cache.shape[1] < 1 or kv_cache.shape[2] != 2 * Hkv * D:
        raise ValueError(f'{what}: kv_cache {tuple(kv_cache.shape)} (expected [B, Smax >= 1, 2*Hkv*D = {2 * Hkv * D}])')
    if kv_cache.dtype != torch.bfloat16 or seq_lens.dtype != torch.int32:
        raise ValueError(f'{what}: kv_cache {kv_cache.dtype}, seq_lens {seq_lens.dtype} (expected bfloat16, int32)')
    if tuple(seq_lens.shape) != (kv_cache.shape[0],) or not kv_cache.is_contiguous() or not seq_lens.is_contiguous():
        raise ValueError(f'{what}: seq_lens {tuple(seq_lens.shape)} for kv_cache {tuple(kv_cache.shape)} '
                         '(expected [B], both contiguous)')
    return kv_cache.shape[0], kv_cache.shape[1]


def _paged_shapes(kv_pool, block_table, seq_lens, H, Hkv, D, what):
    """(B, num_blocks, page, max_blocks) of a paged pool [num_blocks, page, 2*Hkv*D] and its block table"""
    _decode_heads(H, Hkv, D, what)
    if kv_pool.dim() != 3 or kv_pool.shape[0] < 1 or kv_pool.shape[2] != 2 * Hkv * D:
        raise ValueError(f'{what}: kv_cache {tuple(kv_pool.shape)} with a block table '
                         f'(expected [num_blocks >= 1, page, 2*Hkv*D = {2 * Hkv * D}])')
    if kv_pool.shape[1] not in (16, 32, 64, 128):
        raise ValueError(f'{what}: page size {kv_pool.shape[1]} (expected 16, 32, 64 or 128)')
    if kv_pool.dtype != torch.bfloat16 or seq_lens.dtype != torch.int32 or block_table.dtype != torch.int32:
        raise ValueError(f'{what}: kv_cache {kv_pool.dtype}, seq_lens {seq_lens.dtype}, block_table {block_table.dtype} '
                         '(expected bfloat16, int32, int32)')
    if (block_table.dim() != 2 or block_table.shape[1] < 1 or block_table.stride(1) != 1
            or block_table.shape[0] > 1 and block_table.stride(0) < block_table.shape[1]):
        raise ValueError(f'{what}: block_table {tuple(block_table.shape)} strides {tuple(block_table.stride())} '
                         '(expected [B, max_blocks >= 1] with unit inner stride, rows not overlapping)')
    if (tuple(seq_lens.shape) != (block_table.shape[0],) or not kv_pool.is_contiguous() or not seq_lens.is_contiguous()
            or block_table.device != kv_pool.device):
        raise ValueError(f'{what}: seq_lens {tuple(seq_lens.shape)} for block_table {tuple(block_table.shape)} '
                         '(expected [B]; kv_cache and seq_lens contiguous, the table on the cache\'s device)')
    if block_table.shape[1] * kv_pool.shape[1] >= 2 ** 31 - 512:
        raise ValueError(f'{what}: {block_table.shape[1]} blocks of {kv_pool.shape[1]} positions per sequence '
                         '(at most 2^31 - 512 positions)')
    return block_table.shape[0], kv_pool.shape[0], kv_pool.shape[1], block_table.shape[1]


def _gather_pages(kv_pool, block_table):
    """The logical contiguous cache [B, max_blocks*page, W] of a paged pool (CPU twin); blocks that the
    table does not name (ids outside the pool) read as zeros."""
    nblk, page, W = kv_pool.shape
    ok = (block_table >= 0) & (block_table < nblk)
    pages = kv_pool[block_table.long().clamp(0, nblk - 1)]
    return torch.where(ok[:, :, None, None], pages, torch.zeros_like(pages)).reshape(block_table.shape[0], -1, W)


def decode_partials(device, n: int) -> torch.Tensor:
    """The fp32 partials of the split decode kernel, cached per device (and stream role / capture
    scope) like :func:`gemm_workspace`; superseded buffers stay alive for captured graphs."""
    from .functional import workspace_key, workspace_store
    key = workspace_key(device)
    store = workspace_store(_DEC_PART)
    buf = store.get(key)
    if buf is None or buf.numel() < n:
        if buf is not None:
            _WS_OLD.append(buf)
        buf = store[key] = torch.empty(n, device=device, dtype=torch.float32)
    return buf


def attn_decode_gqa(q, kv_cache, seq_lens, H, Hkv, scale, head_dim: int = 64, *, max_len=None, splits: int = 0,
                    out=None, block_table=None):
    """One decode step of grouped-query attention: query row b (``q`` [B, H*D] bf16, unit inner
    stride, any row stride: the Q columns of the step's packed projection output pass as a view)
    against the first ``seq_lens[b]`` positions of ``kv_cache`` [B, Smax, 2*Hkv*D] bf16, query head h
    reading K/V head ``h // (H // Hkv)``.  ``seq_lens`` int32 [B] stays on the device.  Returns
    (ctx [B, H*D] bf16, lse [B, H] fp32 = log sum exp(scale * q.k)); a length of 0 gives ctx = 0 and
    lse = -inf; cache rows at or past the length are never used (they may hold NaN).  ``max_len``: a
    host-side upper bound of the lengths (default Smax) that sizes the key splits; ``splits``: 0 =
    chosen to fill the chip (``mlc_attn_decode_splits``).  ``out``: a contiguous [B, H*D] bf16 ctx.
    ``block_table`` (int32 [B, max_blocks], unit inner stride, any row stride, on the device): ``kv_cache``
    is a paged pool [num_blocks, page, 2*Hkv*D] with page 16 / 32 / 64 / 128, position n of sequence b is row
    ``n % page`` of block ``block_table[b, n // page]``, and Smax is ``max_blocks * page``
    (``mlc_attn_decode_paged``).  Table entries at or past ``ceil(seq_lens[b] / page)`` are not read; a
    block id outside the pool reads as zeros.  With the same split count the result is bit-equal to the
    contiguous call on the same logical data."""
    D = head_dim
    if block_table is not None:
        B, nblk, page, maxb = _paged_shapes(kv_cache, block_table, seq_lens, H, Hkv, D, 'attn_decode_gqa')
        Smax = maxb * page
    else:
        B, Smax = _decode_shapes(kv_cache, seq_lens, H, Hkv, D, 'attn_decode_gqa')
    if q.dim() != 2 or tuple(q.shape) != (B, H * D) or q.dtype != torch.bfloat16 or q.stride(1) != 1:
        raise ValueError(f'attn_decode_gqa: q {tuple(q.shape)} {q.dtype} strides {tuple(q.stride())} '
                         f'(expected [{B}, {H * D}] bfloat16 with unit inner stride)')
    if out is not None and (tuple(out.shape) != (B, H * D) or out.dtype != torch.bfloat16 or not out.is_contiguous()):
        raise ValueError(f'attn_decode_gqa: out {tuple(out.shape)} {out.dtype} (expected contiguous [{B}, {H * D}] bfloat16)')
    max_len = Smax if max_len is None else max(1, min(int(max_len), Smax))
    ctx = out if out is not None else torch.empty(B, H * D, device=q.device, dtype=torch.bfloat16)
    if _cuda(q):
        if B > 1 and q.stride(0) % 8 or q.data_ptr() % 16:
            raise ValueError('attn_decode_gqa: q rows must start on 16-byte boundaries')
        lse = torch.empty(B, H, device=q.device, dtype=torch.float32)
        sp = _lib.load().mlc_attn_decode_splits(B, Hkv, max_len, int(splits))
        part = decode_partials(q.device, B * H * sp * (D + 2)) if sp > 1 else None
        if block_table is not None:
            _lib.call('mlc_attn_decode_paged', _lib.ptr(q), q.stride(0) if B > 1 else H * D, _lib.ptr(kv_cache),
                      _lib.ptr(block_table), block_table.stride(0) if B > 1 else maxb, _lib.ptr(seq_lens), _lib.ptr(part),
                      _lib.ptr(ctx),
                      _lib.ptr(lse), B, nblk, page, maxb, H, Hkv, D, max_len, sp, float(scale), _lib.stream())
            return ctx, lse
        _lib.call('mlc_attn_decode', _lib.ptr(q), q.stride(0) if B > 1 else H * D, _lib.ptr(kv_cache),
                  _lib.ptr(seq_lens), _lib.ptr(part), _lib.ptr(ctx), _lib.ptr(lse), B, Smax, H, Hkv, D, max_len, sp,
                  float(scale), _lib.stream())
        return ctx, lse
    if block_table is not None:
        kv_cache = _gather_pages(kv_cache, block_table)
    G = H // Hkv
    lse = torch.full((B, H), -math.inf)
    ctx.zero_()
    for b in range(B):
        n = min(max(int(seq_lens[b]), 0), Smax)
        if n == 0:
            continue
        k, v = kv_cache[b, :n].float().view(n, 2, Hkv, D).unbind(1)               # [n, Hkv, D] each
        s = torch.einsum('jgd,njd->jgn', q[b].float().view(Hkv, G, D), k) * scale   # [Hkv, G, n]
        lse[b] = torch.logsumexp(s, -1).reshape(H)
        ctx[b] = torch.einsum('jgn,njd->jgd', torch.softmax(s, -1), v).reshape(H * D).to(torch.bfloat16)
    return ctx, lse


def kv_append_(kv_cache, qkv_rows, seq_lens, H, Hkv, head_dim: int = 64, *, block_table=None):
    """Write the K/V columns [H*D, (H + 2*Hkv)*D) of packed row b of ``qkv_rows`` [B, (H + 2*Hkv)*D]
    bf16 to ``kv_cache[b, seq_lens[b]]`` IN PLACE (``mlc_kv_append``) and return the cache; a position
    outside [0, Smax) drops its row.  ``seq_lens`` is not advanced: the caller adds 1 with a torch
    op, which a graph captures.  With ``block_table`` (see :func:`attn_decode_gqa`) the row goes to
    ``kv_cache[block_table[b, pos // page], pos % page]`` of the paged pool (``mlc_kv_append_paged``); a
    position outside [0, max_blocks * page) or a block id outside the pool drops its row."""
    D = head_dim
    if block_table is not None:
        B, nblk, page, maxb = _paged_shapes(kv_cache, block_table, seq_lens, H, Hkv, D, 'kv_append_')
        Smax = maxb * page
    else:
        B, Smax = _decode_shapes(kv_cache, seq_lens, H, Hkv, D, 'kv_append_')
    if (qkv_rows.dim() != 2 or tuple(qkv_rows.shape) != (B, (H + 2 * Hkv) * D) or qkv_rows.dtype != torch.bfloat16
            or qkv_rows.stride(1) != 1):
        raise ValueError(f'kv_append_: qkv_rows {tuple(qkv_rows.shape)} {qkv_rows.dtype} '
                         f'(expected [{B}, {(H + 2 * Hkv) * D}] bfloat16 with unit inner stride)')
    if _cuda(kv_cache):
        if B > 1 and qkv_rows.stride(0) % 8 or qkv_rows.data_ptr() % 16:
            raise ValueError('kv_append_: qkv_rows rows must start on 16-byte boundaries')
        if block_table is not None:
            _lib.call('mlc_kv_append_paged', _lib.ptr(qkv_rows), qkv_rows.stride(0) if B > 1 else (H + 2 * Hkv) * D,
                      _lib.ptr(kv_cache), _lib.ptr(block_table), block_table.stride(0) if B > 1 else maxb,
                      _lib.ptr(seq_lens), B, nblk, page, maxb, H, Hkv, D, _lib.stream())
            return kv_cache
        _lib.call('mlc_kv_append', _lib.ptr(qkv_rows), qkv_rows.stride(0) if B > 1 else (H + 2 * Hkv) * D,
                  _lib.ptr(kv_cache), _lib.ptr(seq_lens), B, Smax, H, Hkv, D, _lib.stream())
        return kv_cache
    for b in range(B):
        pos = int(seq_lens[b])
        if not 0 <= pos < Smax:
            continue
        if block_table is None:
            kv_cache[b, pos] = qkv_rows[b, H * D:]
        elif 0 <= int(block_table[b, pos // page]) < nblk:
            kv_cache[int(block_table[b, pos // page]), pos % page] = qkv_rows[b, H * D:]
    return kv_cache


__all__ = ['attn_decode_gqa', 'kv_append_', 'lm_loss_fwd', 'lm_loss_bwd', 'lm_head_loss', 'ln_fwd', 'ln_bwd', 'LnFinalizer', 'embed_bwd', 'embed_ln_fwd', 'embed_bwd_packed', 'cls_scatter', 'softmax_fwd', 'softmax_bwd', 'dense_fwd', 'dense_dgrad', 'dact_gelu', 'colsum_acc',
           'dropout', 'keep_mask', 'attn_fwd_varlen', 'attn_bwd_varlen', 'check_cu_seqlens',
           'attn_fwd_gqa', 'attn_bwd_gqa', 'attn_fwd_gqa_varlen', 'attn_bwd_gqa_varlen', 'rope_table', 'rope_qkv_', 'rms_fwd', 'rms_bwd', 'swiglu_fwd', 'swiglu_bwd',
           'decoder_native', 'set_decoder_native']
