"""Whole-sequence packed attention (``fwd128_varlen_kernel`` / ``bwd128_varlen_kernel``: packed
calls with max_len <= 128, D = 64, not causal) against the fp32 CPU twin of
``attn_fwd_varlen`` / ``attn_bwd_varlen`` under the bounds of ``test_attn_varlen_gpu.py``:
rel ctx < 1e-2, rel lse < 1e-4, rel dQ / dK / dV < 2e-2 over the buffer and per sequence (a
one-token sequence's zero dQ / dK block is held to 2e-2 of its dV block).  The length sets are
the smallest that cross the design's boundaries: one token, the 32-row wave groups, the 64-row
images, empty slots, full tiles, and a max_len that is not the longest length (dropout index)."""
import functools
import math

import pytest
import torch

from mlcomp_amd.ops import _lib, transformer as Tx

pytestmark = pytest.mark.gpu
DEV, H, D, E = 'cuda', 2, 64, 128
SCALE = 1.0 / math.sqrt(D)
# (lengths, max_len, tail rows)
CASES = [([1], 1, 5), ([31, 32, 33, 1], 33, 5), ([31, 32, 33, 1], 128, 5), ([0, 63, 0, 64, 65, 0], 128, 5),
         ([96, 97, 127], 128, 5), ([128, 128], 128, 0)]


def _bf(*s, seed):
    return (torch.randn(*s, generator=torch.Generator().manual_seed(seed)) * 0.7).to(torch.bfloat16)


def _cu(lengths):
    return torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32)


def _seed(dev):
    return torch.tensor([29], dtype=torch.int32, device=dev)


def _run(qkv, dctx, cu, ml, p, dev):
    qkv, dctx = qkv.to(dev), dctx.to(dev)
    ctx, lse = Tx.attn_fwd_varlen(qkv, cu, ml, H, SCALE, p, _seed(dev), 33, head_dim=D)
    return ctx, lse, Tx.attn_bwd_varlen(qkv, cu, ml, dctx, lse, H, SCALE, p, _seed(dev), 33, head_dim=D, ctx=ctx)


@functools.lru_cache(maxsize=None)
def _case(lengths, ml, tail, p, seed=16):
    """Inputs and the CPU twin's results of one case, computed once and left unchanged."""
    T = sum(lengths) + tail
    qkv, dctx, cu = _bf(T, 3 * E, seed=seed), _bf(T, E, seed=seed + 1), _cu(lengths)
    return (qkv, dctx, cu) + tuple(_run(qkv, dctx, cu, ml, p, 'cpu'))


def _rel(a, b, scale_ref):
    a, b = a.float().cpu(), b.float().cpu()
    ref = scale_ref.float().cpu() if float(b.norm()) == 0.0 else b   # the one-token rule
    return ((a - b).norm() / (ref.norm() + 1e-12)).item()


def _check(got, ref, cu):
    (ctx_g, lse_g, dq_g), (ctx_r, lse_r, dq_r) = got, ref
    assert all(torch.isfinite(t.float()).all() for t in got)
    fig = [_rel(ctx_g, ctx_r, ctx_r), _rel(lse_g, lse_r, lse_r)]
    spans = [(0, dq_r.shape[0])] + [(c0, c1) for c0, c1 in zip(cu[:-1].tolist(), cu[1:].tolist()) if c1 > c0]
    for c0, c1 in spans:   # the whole buffer, then every sequence
        fig += [_rel(dq_g[c0:c1, i * E:(i + 1) * E], dq_r[c0:c1, i * E:(i + 1) * E], dq_r[c0:c1, 2 * E:])
                for i in range(3)]
    print('rel ctx, lse, then dQ / dK / dV per span:', ' '.join(f'{v:.2e}' for v in fig))
    assert fig[0] < 1e-2 and fig[1] < 1e-4 and max(fig[2:]) < 2e-2, fig
    end = int(cu[-1])   # the rows of no sequence: exactly zero
    assert ctx_g[end:].abs().sum().item() == 0 and dq_g[end:].abs().sum().item() == 0
    assert lse_g.view(H, -1)[:, end:].abs().sum().item() == 0


def _whole_sequence(ml):
    return _lib.load().mlc_flash_varlen128_ok(ml, D, 0) == 1


@pytest.mark.parametrize('p', [0.0, 0.1], ids=['plain', 'dropout'])
@pytest.mark.parametrize('lengths,ml,tail', CASES, ids=[f'{"-".join(map(str, c[0]))}@{c[1]}' for c in CASES])
def test_whole_sequence_fwd_bwd(lengths, ml, tail, p):
    assert _whole_sequence(ml)
    qkv, dctx, cu, *ref = _case(tuple(lengths), ml, tail, p)
    got = _run(qkv, dctx, cu, ml, p, DEV)
    torch.cuda.synchronize()
    _check(got, ref, cu)


@pytest.mark.parametrize('p', [0.0, 0.1], ids=['plain', 'dropout'])
def test_poisoned_outputs_through_raw_entry_points(p):
    """out, lse and dqkv arrive full of NaN: the launches write every row themselves."""
    assert _whole_sequence(33)
    qkv, dctx, cu, *ref = _case((31, 32, 33, 1), 33, 5, p)
    T, n = qkv.shape[0], cu.numel() - 1
    qkv, dctx, cud, seed = qkv.to(DEV), dctx.to(DEV), cu.to(DEV), _seed(DEV)
    nan = lambda *s, dt: torch.full(s, float('nan'), device=DEV, dtype=dt)  # noqa: E731
    out, lse, dqkv = nan(T, E, dt=torch.bfloat16), nan(H * T, dt=torch.float32), nan(T, 3 * E, dt=torch.bfloat16)
    dot = torch.empty(H * T, device=DEV)
    P = _lib.ptr
    _lib.call('mlc_flash_fwd_varlen', P(qkv), P(cud), P(out), P(lse), T, n, 33, H, D, SCALE, p, P(seed), 33, 0,
              _lib.stream())
    _lib.call('mlc_flash_bwd_varlen', P(qkv), P(cud), P(out), P(dctx), P(lse), P(dot), P(dqkv), T, n, 33, H, D,
              SCALE, p, P(seed), 33, 0, _lib.stream())
    torch.cuda.synchronize()
    _check((out, lse, dqkv), ref, cu)


@pytest.mark.parametrize('fwd_whole', [True, False], ids=['whole-then-streaming', 'streaming-then-whole'])
def test_mixed_forms(fwd_whole):
    """lse has one layout: a forward by one form serves the other form's backward."""
    lengths, ml, p = (0, 63, 0, 64, 65, 0), 128, 0.1
    qkv, dctx, cu, *ref = _case(lengths, ml, 5, p)
    qkv, dctx = qkv.to(DEV), dctx.to(DEV)
    lib = _lib.load()
    old = lib.mlc_flash_varlen128_get_set(0, int(fwd_whole))
    try:
        assert _whole_sequence(ml) == fwd_whole
        ctx, lse = Tx.attn_fwd_varlen(qkv, cu, ml, H, SCALE, p, _seed(DEV), 33, head_dim=D)
        lib.mlc_flash_varlen128_get_set(0, int(not fwd_whole))
        assert _whole_sequence(ml) != fwd_whole
        dq = Tx.attn_bwd_varlen(qkv, cu, ml, dctx, lse, H, SCALE, p, _seed(DEV), 33, head_dim=D, ctx=ctx)
        torch.cuda.synchronize()
    finally:
        lib.mlc_flash_varlen128_get_set(0, old)
    _check((ctx, lse, dq), ref, cu)


def test_graph_replay_on_another_split():
    """Captured once at nseq_max = 5; cu_seqlens and qkv are overwritten in place with a split
    that has a longer tail and other empty slots: the replay equals an eager call."""
    first, new, ml = [100, 0, 128, 40, 17], [0, 128, 33, 0, 64], 128
    assert _whole_sequence(ml)
    T = sum(first) + 5
    qkv, dctx, cu, seed = _bf(T, 3 * E, seed=16).to(DEV), _bf(T, E, seed=17).to(DEV), _cu(first).to(DEV), _seed(DEV)

    def body():
        ctx, lse = Tx.attn_fwd_varlen(qkv, cu, ml, H, SCALE, 0.1, seed, 33, head_dim=D)
        return ctx, lse, Tx.attn_bwd_varlen(qkv, cu, ml, dctx, lse, H, SCALE, 0.1, seed, 33, head_dim=D, ctx=ctx)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                   # warm-up: library load, allocator
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = body()
        cu.copy_(_cu(new).to(DEV))
        qkv.copy_(_bf(T, 3 * E, seed=61).to(DEV))
        for _ in range(2):                       # the second replay runs over the first one's results
            graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out]
        ref = body()
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    end = sum(new)
    for g, r in zip(got, ref):
        assert torch.equal(g, r)
    assert got[0][end:].abs().sum().item() == 0 and got[2][end:].abs().sum().item() == 0
    assert got[1].view(H, -1)[:, end:].abs().sum().item() == 0 and got[0][:end].abs().sum().item() > 0
