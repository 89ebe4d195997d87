"""The fp32 CPU twins of the paged decode path (``block_table=`` of attn_decode_gqa / kv_append_)
against the contiguous twins on the gathered pages, exactly, and the wrappers' shape checks."""
import pytest
import torch

from mlcomp_amd.ops import transformer as Tx

BF = torch.bfloat16
B, H, HKV, D, MAXB = 3, 4, 2, 64, 5
NBLK = 2 * B * MAXB


def paged(page):
    """a pool, a table of scattered blocks (row stride MAXB + 3), and the logical cache they describe"""
    gen = torch.Generator().manual_seed(page)
    pool = torch.randn(NBLK, page, 2 * HKV * D, generator=gen).to(BF)
    table = torch.full((B, MAXB + 3), -1, dtype=torch.int32)[:, :MAXB]
    table.copy_(torch.randperm(NBLK, generator=gen)[:B * MAXB].view(B, MAXB))
    rows = torch.randn(B, (H + 2 * HKV) * D, generator=gen).to(BF)
    return pool, table, pool[table.long()].reshape(B, MAXB * page, -1).clone(), rows


@pytest.mark.parametrize('page', [16, 64])
def test_paged_twins_equal_the_contiguous_twins(page):
    pool, table, cache, rows = paged(page)
    lens = torch.tensor([0, 17, MAXB * page - 1], dtype=torch.int32)
    p2 = Tx.kv_append_(pool.clone(), rows, lens, H, HKV, D, block_table=table)
    c2 = Tx.kv_append_(cache.clone(), rows, lens, H, HKV, D)
    assert torch.equal(p2[table.long()].reshape(c2.shape), c2) and not torch.equal(p2, pool)
    got = Tx.attn_decode_gqa(rows[:, :H * D], p2, lens + 1, H, HKV, D ** -0.5, D, block_table=table)
    want = Tx.attn_decode_gqa(rows[:, :H * D], c2, lens + 1, H, HKV, D ** -0.5, D)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a full sequence and a block id outside the pool drop their rows; the third row is written
    table[1, 0] = NBLK
    p3 = Tx.kv_append_(pool.clone(), rows, torch.tensor([MAXB * page, 0, 0], dtype=torch.int32), H, HKV, D, block_table=table)
    pool[table[2, 0].item(), 0] = rows[2, H * D:]
    assert torch.equal(p3, pool)


BAD = {'page 48': lambda pool, tab: (torch.zeros(4, 48, pool.shape[2], dtype=BF), tab),
       'table dtype': lambda pool, tab: (pool, tab.long()),
       'table shape': lambda pool, tab: (pool, tab[:B - 1]),
       'pool width': lambda pool, tab: (pool[:, :, :-8].contiguous(), tab)}


@pytest.mark.parametrize('what', list(BAD))
def test_paged_wrappers_refuse(what):
    pool, table, _, rows = paged(16)
    pool, table = BAD[what](pool, table)
    lens = torch.zeros(B, dtype=torch.int32)
    with pytest.raises(ValueError):
        Tx.attn_decode_gqa(rows[:, :H * D], pool, lens, H, HKV, 1.0, D, block_table=table)
    with pytest.raises(ValueError):
        Tx.kv_append_(pool, rows, lens, H, HKV, D, block_table=table)
