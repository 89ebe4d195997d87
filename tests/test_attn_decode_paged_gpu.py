"""The paged path of `csrc/kernels/attn_decode.hip` (mlc_attn_decode_paged, mlc_kv_append_paged): per
element against the fp64 reference of tests/test_attn_decode_gpu.py, on that module's inputs and with
the bounds derived in its docstring, unchanged (lse: Es + 4 e32; ctx: ulp_bf16 + (2 u + 3 Es) sum p |v|
+ 4 e32; an empty sequence: ctx exactly zero, lse = -inf), and bit for bit against mlc_attn_decode on
the logical contiguous cache with the same split count.  The logical cache (lengths 1 / 129 / 333 / 0,
one key per sequence and K/V head whose score passes 60, NaN from the length on) is cut into pages that
a seeded permutation scatters over the even blocks of the pool, so no two logical neighbours are
physical neighbours; the odd blocks, the rows from a length on inside its last page and the guards
hold NaN, and the table holds -1 and num_blocks from ceil(len / page) on."""
import math

import pytest
import torch

from mlcomp_amd.ops import _lib
from mlcomp_amd.ops import transformer as Tx
from test_attn_decode_gpu import B, LENS, SMAX, case, check
from test_transformer_pointwise_gpu import BF, DEV, F32, Guarded, _bf, _bits, ulp_bf16

pytestmark = pytest.mark.gpu
I32 = torch.int32


def scatter(cache, lens, page, seed):
    """logical cache [B, S, W] -> (pool [2 * used + 1, page, W], table [B, ceil(S / page)]) as the module
    docstring describes"""
    nb, S, W = cache.shape
    maxb, used = -(-S // page), [-(-n // page) for n in lens]
    ids = (2 * torch.randperm(sum(used), generator=torch.Generator().manual_seed(seed))).tolist()
    nblk = 2 * sum(used) + 1
    pool = torch.full((nblk, page, W), float('nan'), dtype=BF)
    table = torch.tensor([-1, nblk], dtype=I32).repeat(nb, maxb)[:, :maxb].contiguous()
    for b in range(nb):
        for p in range(used[b]):
            rows, table[b, p] = cache[b, p * page:(p + 1) * page], ids.pop()
            pool[table[b, p], :len(rows)] = rows
    return pool, table


@pytest.mark.parametrize('splits', [1, 3])
@pytest.mark.parametrize('page', [16, 32, 128])
@pytest.mark.parametrize('H,Hkv', [(8, 2), (16, 1)])
@pytest.mark.parametrize('D', [64, 128])
def test_paged_decode_per_element(D, H, Hkv, page, splits):
    packed, cache, scale, (ctx64, lse64, pav, es), (ctx32, lse32, _, _) = case(D, H, Hkv)
    pool, table = scatter(cache, LENS, page, seed=page + D)
    nblk, maxb, R = pool.shape[0], table.shape[1], 2
    sp = _lib.load().mlc_attn_decode_splits(B, Hkv, SMAX, splits)
    assert sp == splits and maxb * page >= SMAX
    Q, KV = Guarded(1, packed.numel(), BF, 8, data=packed), Guarded(1, cache.numel(), BF, 8, data=cache)
    POOL = Guarded(1, pool.numel(), BF, 8, data=pool)
    TAB = Guarded(1, table.numel(), F32, 4, data=table.view(F32))
    LEN = Guarded(1, B, F32, 4, data=torch.tensor(LENS, dtype=I32).view(F32))
    CTX, LSE = Guarded(R + 1, B * H * D, BF, 8), Guarded(R + 1, B * H, F32, 1)      # the last: the contiguous kernel's
    PART = Guarded(R + 1, B * H * sp * (D + 2), F32, 1) if sp > 1 else None
    for r in range(R):
        _lib.call('mlc_attn_decode_paged', Q.ptr(), packed.shape[1], POOL.ptr(), TAB.ptr(), maxb, LEN.ptr(),
                  PART.ptr(r) if PART else None, CTX.ptr(r), LSE.ptr(r), B, nblk, page, maxb, H, Hkv, D, SMAX, splits,
                  scale, _lib.stream())
    _lib.call('mlc_attn_decode', Q.ptr(), packed.shape[1], KV.ptr(), LEN.ptr(), PART.ptr(R) if PART else None,
              CTX.ptr(R), LSE.ptr(R), B, SMAX, H, Hkv, D, SMAX, splits, scale, _lib.stream())
    torch.cuda.synchronize()
    for name, arr in (('q', Q), ('kv_pool', POOL), ('block_table', TAB), ('seq_lens', LEN)):
        arr.untouched(name)
    for name, arr in (('ctx', CTX), ('lse', LSE)) + ((('partials', PART),) if PART else ()):
        arr.written(name)
    ctx, lse = CTX.cpu(B, H, D), LSE.cpu(B, H)
    for r in (1, R):
        assert torch.equal(_bits(ctx[0]), _bits(ctx[r])) and torch.equal(_bits(lse[0]), _bits(lse[r])), \
            'two runs differ' if r < R else 'paged and contiguous differ'
    live = torch.tensor([n > 0 for n in LENS])
    check('paged lse', lse[0], lse64, lse32, es, live)
    check('paged ctx', ctx[0], ctx64, ctx32, ulp_bf16(ctx64) + (2 * 2.0 ** -8 + 3 * es)[..., None] * pav, live)
    assert not _bits(ctx[0][~live]).any() and bool((lse[0][~live] == -math.inf).all()), 'the empty sequence'


@pytest.mark.parametrize('Hkv', [1, 4])
@pytest.mark.parametrize('D', [64, 128])
def test_paged_kv_append(D, Hkv):
    H, page, maxb, nblk = 2 * Hkv, 16, 2, 11
    W, pos = 2 * Hkv * D, [0, 15, 16, maxb * page, 3]         # the fourth is full; the fifth's block id is num_blocks
    gen = torch.Generator().manual_seed(D + Hkv)
    rows, pool = _bf(5, H * D + W, gen=gen), _bf(nblk, page, W, gen=gen)
    table = torch.tensor([[7, 2], [4, 9], [0, 5], [1, 8], [nblk, 3]], dtype=I32)
    ROWS, POOL = Guarded(1, rows.numel(), BF, 8, data=rows), Guarded(1, pool.numel(), BF, 8, data=pool)
    TAB = Guarded(1, table.numel(), F32, 4, data=table.view(F32))
    POS = Guarded(1, 5, F32, 4, data=torch.tensor(pos, dtype=I32).view(F32))
    _lib.call('mlc_kv_append_paged', ROWS.ptr(), rows.shape[1], POOL.ptr(), TAB.ptr(), maxb, POS.ptr(), 5, nblk, page,
              maxb, H, Hkv, D, _lib.stream())
    torch.cuda.synchronize()
    for name, arr in (('qkv rows', ROWS), ('block_table', TAB), ('seq_lens', POS)):
        arr.untouched(name)
    for b in range(3):
        pool[table[b, pos[b] // page], pos[b] % page] = rows[b, H * D:]
    want = POOL.before.clone()                                # guards and every other element as they were
    want[0, POOL.lead:POOL.lead + POOL.n] = pool.reshape(-1).to(DEV)
    assert torch.equal(_bits(POOL.store), _bits(want))


@pytest.mark.parametrize('D,H,Hkv,splits', [(64, 8, 2, 2), (128, 16, 1, 0)])
def test_paged_decode_loop_in_a_graph(D, H, Hkv, splits):
    """one step (paged append, lengths + 1, paged attend) captured once and replayed three times on new
    rows, the sequences crossing page boundaries; every replay against the CPU twins on the same data"""
    from mlcomp_amd.train.graphed import work_stream
    nb, page, maxb, scale = 3, 16, 9, D ** -0.5
    gen = torch.Generator().manual_seed(D)
    lens_c = torch.tensor([0, 15, 30], dtype=I32)
    pool_c, table_c = scatter(_bf(nb, maxb * page, 2 * Hkv * D, gen=gen), [maxb * page] * nb, page, seed=D)
    steps = [_bf(nb, (H + 2 * Hkv) * D, gen=gen) for _ in range(4)]
    pool, table, lens, rows = pool_c.to(DEV), table_c.to(DEV), lens_c.to(DEV), steps[0].to(DEV)
    ctx = torch.empty(nb, H * D, device=DEV, dtype=BF)

    def step(pool, table, rows, lens, out):
        Tx.kv_append_(pool, rows, lens, H, Hkv, D, block_table=table)
        lens.add_(1)
        return Tx.attn_decode_gqa(rows[:, :H * D], pool, lens, H, Hkv, scale, D, splits=splits, out=out, block_table=table)

    with work_stream(DEV):
        step(pool.clone(), table, rows, lens.clone(), ctx)     # warm-up: library load, allocator, partials
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _, lse = step(pool, table, rows, lens, ctx)
        pool.copy_(pool_c)                                     # the capture ran nothing: start from the start
        lens.copy_(lens_c)
        for new in steps[1:]:
            rows.copy_(new)
            graph.replay()
            torch.cuda.synchronize()
            want_ctx, want_lse = step(pool_c, table_c, new, lens_c, None)
            assert torch.equal(lens.cpu(), lens_c) and torch.equal(_bits(pool.cpu()), _bits(pool_c))
            rel = ((ctx.float().cpu() - want_ctx.float()).norm() / want_ctx.float().norm()).item()
            assert rel < 1e-2 and (lse.cpu() - want_lse).abs().max().item() < 1e-3, (rel, lens_c.tolist())
