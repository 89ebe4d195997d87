"""`csrc/kernels/attn_decode.hip` per element: mlc_attn_decode and mlc_kv_append against a reference
written out in torch fp64 from the bf16 inputs widened to fp64, on guarded storage
(tests/test_transformer_pointwise_gpu.py), and a captured decode loop against the CPU twins.

Bounds, with Es[b, h] = scale D 2^-24 max_k sum_d |q_d k_d| (the worst-case error of an fp32 dot
product summed in any order), u = 2^-8 (the unit roundoff of P, rounded to bf16 once before P V; the
sum l keeps the unrounded fp32 values) and e32 = max |fp32 run - fp64 run| of the same reference:

  lse   |got - ref| <= Es + 4 e32
  ctx   |got - ref| <= ulp_bf16(ref) + (2 u + 3 Es) sum_k p_k |v_k| + 4 e32
  an empty sequence: ctx exactly zero, lse = -inf

The key tile is 32 (a divisor of 128), so the lengths 1 / 129 / 333 / 0 sit on its edges."""
import functools
import math

import pytest
import torch

from mlcomp_amd.ops import _lib
from mlcomp_amd.ops import transformer as Tx
from test_transformer_pointwise_gpu import BF, DEV, F32, Guarded, _bf, _bits, ulp_bf16

pytestmark = pytest.mark.gpu
F64 = torch.float64
B, SMAX, LENS = 4, 400, (1, 129, 333, 0)
HEADS = [(4, 4), (8, 2), (16, 1)]


def ref(q, cache, H, Hkv, D, scale, dt):
    """q [B, H*D], cache [B, Smax, 2*Hkv*D] -> ctx [B, H, D], lse [B, H], sum_k p |v| [B, H, D], Es [B, H]"""
    G = H // Hkv
    ctx, pav = torch.zeros(B, H, D, dtype=dt), torch.zeros(B, H, D, dtype=dt)
    lse, es = torch.full((B, H), -math.inf, dtype=dt), torch.zeros(B, H, dtype=dt)
    for b, n in enumerate(LENS):
        if n == 0:
            continue
        k, v = cache[b, :n].to(dt).view(n, 2, Hkv, D).unbind(1)
        k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)          # [n, H, D]
        qb = q[b].to(dt).view(H, D)
        s = torch.einsum('hd,nhd->hn', qb, k) * scale
        p = torch.softmax(s, 1)
        lse[b], ctx[b], pav[b] = torch.logsumexp(s, 1), torch.einsum('hn,nhd->hd', p, v), torch.einsum('hn,nhd->hd', p, v.abs())
        es[b] = scale * D * 2.0 ** -24 * torch.einsum('hd,nhd->hn', qb.abs(), k.abs()).max(1).values
    return ctx, lse, pav, es


@functools.lru_cache(maxsize=None)
def case(D, H, Hkv):
    """inputs and references of one shape, computed once and left unchanged"""
    gen = torch.Generator().manual_seed(D + 7 * H + Hkv)
    G, scale = H // Hkv, D ** -0.5
    packed, cache = _bf(B, (H + 2 * Hkv) * D, gen=gen), _bf(B, SMAX, 2 * Hkv * D, gen=gen)
    q = packed[:, :H * D]
    for b, n in enumerate(LENS):
        for j in range(Hkv if n else 0):          # one key per sequence and K/V head whose score passes 60
            kk = cache[b, n // 2, j * D:(j + 1) * D]
            s = scale * (q[b, j * G * D:(j * G + 1) * D].double() @ kk.double())
            kk.copy_((kk.double() * 70.0 / s.abs()).to(BF))
            assert abs(scale * (q[b, j * G * D:(j * G + 1) * D].double() @ kk.double())) > 60
        cache[b, n:] = float('nan')               # never read: 0 * NaN must not reach the output
    return packed, cache, scale, ref(q, cache, H, Hkv, D, scale, F64), ref(q, cache, H, Hkv, D, scale, F32)


def check(name, got, want, twin, bound, live):
    e32 = (twin.double() - want)[live].abs().max().item()
    err, tol = (got.double() - want)[live].abs(), (bound + 4 * e32)[live]
    print(f'ATTN_DECODE {name}: max err/bound {(err / tol).max().item():.3f}, e32 {e32:.3e}, {err.numel()} elements')
    assert bool((err <= tol).all()), (name, int((~(err <= tol)).sum()), e32)     # a NaN fails too


@pytest.mark.parametrize('splits', [1, 3, 0])
@pytest.mark.parametrize('H,Hkv', HEADS)
@pytest.mark.parametrize('D', [64, 128])
def test_decode_per_element(D, H, Hkv, splits):
    """every element within the bounds of the module docstring for each split count, and two runs of one
    split count bit-equal (the two repetitions)"""
    packed, cache, scale, (ctx64, lse64, pav, es), (ctx32, lse32, _, _) = case(D, H, Hkv)
    W, R = 2 * Hkv * D, 2
    sp = _lib.load().mlc_attn_decode_splits(B, Hkv, SMAX, splits)
    assert sp == (splits or 1)                    # 400 keys: splits = 0 keeps one split (none under 256 keys)
    Q, KV = Guarded(1, packed.numel(), BF, 8, data=packed), Guarded(1, cache.numel(), BF, 8, data=cache)
    LEN = Guarded(1, B, F32, 4, data=torch.tensor(LENS, dtype=torch.int32).view(F32))
    CTX, LSE = Guarded(R, B * H * D, BF, 8), Guarded(R, B * H, F32, 1)
    PART = Guarded(R, B * H * sp * (D + 2), F32, 1) if sp > 1 else None
    for r in range(R):
        _lib.call('mlc_attn_decode', Q.ptr(), packed.shape[1], KV.ptr(), LEN.ptr(), PART.ptr(r) if PART else None,
                  CTX.ptr(r), LSE.ptr(r), B, SMAX, H, Hkv, D, SMAX, splits, scale, _lib.stream())
    torch.cuda.synchronize()
    for name, arr in (('q', Q), ('kv_cache', KV), ('seq_lens', LEN)):
        arr.untouched(name)
    for name, arr in (('ctx', CTX), ('lse', LSE)) + ((('partials', PART),) if PART else ()):
        arr.written(name)
    ctx, lse = CTX.cpu(B, H, D), LSE.cpu(B, H)
    assert torch.equal(_bits(ctx[0]), _bits(ctx[1])) and torch.equal(_bits(lse[0]), _bits(lse[1])), 'two runs differ'
    live = torch.tensor([n > 0 for n in LENS])
    check('lse', lse[0], lse64, lse32, es, live)
    check('ctx', ctx[0], ctx64, ctx32, ulp_bf16(ctx64) + (2 * 2.0 ** -8 + 3 * es)[..., None] * pav, live)
    assert not _bits(ctx[0][~live]).any() and bool((lse[0][~live] == -math.inf).all()), 'the empty sequence'


@pytest.mark.parametrize('Hkv', [1, 4])
@pytest.mark.parametrize('D', [64, 128])
def test_kv_append(D, Hkv):
    H, smax = 2 * Hkv, 7
    W, pos = 2 * Hkv * D, [0, 5, smax - 1, smax]              # the last position is dropped
    gen = torch.Generator().manual_seed(D + Hkv)
    rows, cache = _bf(4, H * D + W, gen=gen), _bf(4, smax, W, gen=gen)
    ROWS, KV = Guarded(1, rows.numel(), BF, 8, data=rows), Guarded(1, cache.numel(), BF, 8, data=cache)
    POS = Guarded(1, 4, F32, 4, data=torch.tensor(pos, dtype=torch.int32).view(F32))
    _lib.call('mlc_kv_append', ROWS.ptr(), rows.shape[1], KV.ptr(), POS.ptr(), 4, smax, H, Hkv, D, _lib.stream())
    torch.cuda.synchronize()
    ROWS.untouched('qkv rows')
    POS.untouched('seq_lens')
    for b in range(3):
        cache[b, pos[b]] = rows[b, H * D:]
    want = KV.before.clone()                                  # guards and every other element as they were
    want[0, KV.lead:KV.lead + KV.n] = cache.reshape(-1).to(DEV)
    assert torch.equal(_bits(KV.store), _bits(want))


@pytest.mark.parametrize('D,H,Hkv,splits', [(64, 8, 2, 2), (128, 16, 1, 0)])
def test_decode_loop_in_a_graph(D, H, Hkv, splits):
    """one step (append, lengths + 1, attend) captured once and replayed three times on new rows;
    every replay against the CPU twins on the same data"""
    from mlcomp_amd.train.graphed import work_stream
    nb, smax, scale = 3, 300, D ** -0.5
    gen = torch.Generator().manual_seed(D)
    cache_c = _bf(nb, smax, 2 * Hkv * D, gen=gen)
    lens_c = torch.tensor([0, 127, 297], dtype=torch.int32)   # the last sequence fills up at the third step
    steps = [_bf(nb, (H + 2 * Hkv) * D, gen=gen) for _ in range(4)]
    cache, lens, rows = cache_c.to(DEV), lens_c.to(DEV), steps[0].to(DEV)
    ctx = torch.empty(nb, H * D, device=DEV, dtype=BF)

    def step(cache, rows, lens, out):
        Tx.kv_append_(cache, rows, lens, H, Hkv, D)
        lens.add_(1)
        return Tx.attn_decode_gqa(rows[:, :H * D], cache, lens, H, Hkv, scale, D, splits=splits, out=out)

    with work_stream(DEV):
        step(cache.clone(), rows, lens.clone(), ctx)           # warm-up: library load, allocator, partials
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _, lse = step(cache, rows, lens, ctx)
        cache.copy_(cache_c)                                   # the capture ran nothing: start from the start
        lens.copy_(lens_c)
        for new in steps[1:]:
            rows.copy_(new)
            graph.replay()
            torch.cuda.synchronize()
            want_ctx, want_lse = step(cache_c, new, lens_c, None)
            assert torch.equal(lens.cpu(), lens_c) and torch.equal(_bits(cache.cpu()), _bits(cache_c))
            rel = ((ctx.float().cpu() - want_ctx.float()).norm() / want_ctx.float().norm()).item()
            assert rel < 1e-2 and (lse.cpu() - want_lse).abs().max().item() < 1e-3, (rel, lens_c.tolist())
