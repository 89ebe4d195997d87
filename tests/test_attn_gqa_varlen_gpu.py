"""Packed grouped-query attention kernels (``mlc_flash_fwd_gqa_varlen`` / ``mlc_flash_bwd_gqa_varlen``)."""
import pytest
import torch

from mlcomp_amd.ops import _lib, transformer as Tx

from test_attn_gqa_varlen_cpu import MODES, SALT, packed_case, packed_run

pytestmark = pytest.mark.gpu
DEV = 'cuda'

CASES = [((1, 0, 100, 192, 37), 352, 192, (6, 2, 64)),   # length 1, an empty slot, partial tiles, unaligned starts, a
         # two-block sequence with an odd tile count (the buffer parity), 22 trailing rows of no sequence
         ((320, 45), 368, 320, (4, 1, 128)),             # multi-query, three key blocks, D = 128
         ((77, 130), 208, 130, (4, 2, 80))]              # padded head dim


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('lengths,T,max_len,heads', CASES, ids=['g3-d64', 'mqa-d128', 'd80'])
def test_kernels_match_fp64_reference(lengths, T, max_len, heads, mode):
    packed_run(lengths, T, max_len, heads, mode, DEV)


def _raw(kind, qkv, cu, dctx, T, nseq, max_len, heads, p, seed, fill):
    """Return codes and (ctx, lse, dqkv, dot) of ``mlc_flash_{fwd,bwd}_<kind>``, causal, D = 64, on filled buffers."""
    P, lib, H = _lib.ptr, _lib.load(), heads[0]
    ctx = torch.full((T, H * 64), fill, device=DEV, dtype=torch.bfloat16)
    lse, dot = torch.full((H * T,), fill, device=DEV), torch.full((H * T,), fill, device=DEV)
    dq = torch.full_like(qkv, fill)
    a = (T, nseq, max_len, *heads, 64, 0.125, p, P(seed), SALT, 1, _lib.stream())
    rc = (getattr(lib, f'mlc_flash_fwd_{kind}')(P(qkv), P(cu), P(ctx), P(lse), *a),
          getattr(lib, f'mlc_flash_bwd_{kind}')(P(qkv), P(cu), P(ctx), P(dctx), P(lse), P(dot), P(dq), *a))
    torch.cuda.synchronize()
    return rc, (ctx, lse, dq, dot)


@pytest.mark.parametrize('p', [0.0, 0.1])
def test_hkv_equal_h_is_the_multi_head_packed_call_bit_for_bit(p):
    """One layout at Hkv == H; 192 > 128 keeps the whole-sequence route out of both arms."""
    qkv, dctx, cu, seed = (t.to(DEV) for t in packed_case((192, 100), 300, 192, (3, 3, 64), 'causal')[:4])
    rc_g, got = _raw('gqa_varlen', qkv, cu, dctx, 300, 2, 192, (3, 3), p, seed, 0.0)
    rc_m, want = _raw('varlen', qkv, cu, dctx, 300, 2, 192, (3,), p, seed, 0.0)
    assert rc_g == rc_m == (0, 0) and all(torch.equal(a, b) for a, b in zip(got[:3], want[:3]))
    assert got[2][:292].float().abs().sum() > 0 and not got[2][292:].any()


def test_sequences_are_isolated():
    lengths, T, max_len, (H, Hkv, D) = CASES[0]
    qkv, dctx, cu, seed = packed_case(*CASES[0], 'causal+dropout')[:4]
    c0, c1 = int(cu[3]), int(cu[4])   # the 192-row sequence
    a, res = (H, Hkv, 0.125, 0.1, seed.to(DEV), SALT), []
    for bump in (0.0, 1.0):
        q2, d2 = qkv.clone(), dctx.clone()
        q2[c0:c1] += bump
        d2[c0:c1] += bump
        ctx, lse = Tx.attn_fwd_gqa_varlen(q2.to(DEV), cu, max_len, *a, head_dim=D, causal=True)
        dq = Tx.attn_bwd_gqa_varlen(q2.to(DEV), cu, max_len, d2.to(DEV), lse, *a, head_dim=D, ctx=ctx, causal=True)
        res.append((ctx, lse.view(H, T).t(), dq))
    keep = torch.ones(T, dtype=torch.bool)
    keep[c0:c1] = False
    assert all(torch.equal(x[keep], y[keep]) and not torch.equal(x[~keep], y[~keep]) for x, y in zip(*res))


@pytest.mark.parametrize('H,Hkv,null_cu', [(4, 3, False), (4, 0, False), (4, 2, True)])
def test_bad_calls_are_rejected_without_a_launch(H, Hkv, null_cu):
    T = 64
    qkv = torch.zeros(T, (H + 2 * max(Hkv, 1)) * 64, device=DEV, dtype=torch.bfloat16)
    cu = None if null_cu else torch.tensor([0, T], dtype=torch.int32, device=DEV)
    rc, bufs = _raw('gqa_varlen', qkv, cu, qkv[:, :H * 64].contiguous(), T, 1, T, (H, Hkv), 0.0, None, 7.0)
    assert rc == (-1, -1) and all((t == 7.0).all() for t in bufs)


def test_graph_replay_on_another_split():
    lengths, T, max_len, (H, Hkv, D) = CASES[0]
    qkv, dctx, cu, seed = (t.to(DEV) for t in packed_case(*CASES[0], 'causal+dropout')[:4])
    a = (H, Hkv, 0.125, 0.1, seed, SALT)

    def body():
        ctx, lse = Tx.attn_fwd_gqa_varlen(qkv, cu, max_len, *a, head_dim=D, causal=True)
        return ctx, lse, Tx.attn_bwd_gqa_varlen(qkv, cu, max_len, dctx, lse, *a, head_dim=D, ctx=ctx, causal=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                   # warm-up: library load, allocator
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = body()
        cu.copy_(torch.tensor([0, 70, 70, 93, 130, 322], dtype=torch.int32))   # another split of the same T
        got = []
        for _ in range(2):                       # more than one replay against the eager result
            graph.replay()
            torch.cuda.synchronize()
            got.append([t.clone() for t in out])
        ref = body()
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(g, r) for rep in got for g, r in zip(rep, ref))
    assert not got[0][2][322:].any() and got[0][2][:322].float().abs().sum() > 0
