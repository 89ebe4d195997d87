"""Packed variable-length attention on the GPU: the varlen flash kernels
(``mlc_flash_fwd_varlen`` / ``mlc_flash_bwd_varlen``) against the fp32 CPU twin under the
bounds of ``test_masked_flash_attention_fwd_bwd``, per sequence as well as over the whole
buffer; exact zeros in the rows of no sequence; packed against the padded kernels at
S = max_len; bit-exact isolation between sequences; and one captured graph replayed on another
split of the same token budget.

A sequence of one token has dQ = dK = 0 exactly (one key: the softmax Jacobian is zero), so a
relative error against that block is undefined.  There the kernels' block is held to 2e-2 of
the sequence's dV block instead - the same figure, measured against the scale of that
sequence's gradient."""
import functools
import math

import pytest
import torch

from mlcomp_amd.ops import transformer as Tx

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NEG = float('-inf')

# (lengths, H, D, tail rows)
CASES = {1: ([1], 2, 64, 5),
         2: ([45, 1, 64, 100], 3, 64, 5),      # partial tile, S = 1, one full tile, partial second tile
         3: ([0, 130, 0, 63, 0], 2, 64, 5),    # leading / inner / trailing empty slots, a second 128-row block
         4: ([192, 77], 2, 128, 5),
         5: ([200, 33], 2, 80, 5),             # zero-padded head dim
         6: ([320, 0, 0, 0], 2, 128, 0)}       # nseq_max = 4: three trailing empty slots, no tail
PARAMS = [(c, ml, 'plain') for c in CASES for ml in ('longest', 384)] \
    + [(c, ml, m) for c in (2, 3, 4) for ml in ('longest', 384) for m in ('causal', 'dropout')]


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def rel_or_scale(a, b, scale_ref):
    """rel(a, b); where the reference block is exactly zero, |a| against ``scale_ref``'s norm."""
    a, b = a.float().cpu(), b.float().cpu()
    if float(b.norm()) == 0.0:
        return (a.norm() / (scale_ref.float().cpu().norm() + 1e-12)).item()
    return rel(a, b)


def _bf(*s, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*s, generator=g) * scale).to(torch.bfloat16)


def _cu(lengths):
    return torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32)


def _run(qkv, dctx, cu, max_len, H, D, dev, p=0.0, causal=False, seed=None):
    scale = 1.0 / math.sqrt(D)
    seed = (seed if seed is not None else torch.tensor([29], dtype=torch.int32)).to(dev)
    qkv, dctx = qkv.to(dev), dctx.to(dev)
    ctx, lse = Tx.attn_fwd_varlen(qkv, cu, max_len, H, scale, p, seed, 33, head_dim=D, causal=causal)
    dq = Tx.attn_bwd_varlen(qkv, cu, max_len, dctx, lse, H, scale, p, seed, 33, head_dim=D, ctx=ctx, causal=causal)
    return ctx, lse, dq


@functools.lru_cache(maxsize=None)
def _case(idx, max_len, mode):
    """Inputs and the CPU twin's results of one case, computed once and left unchanged."""
    lengths, H, D, tail = CASES[idx]
    T = sum(lengths) + tail
    ml = max(lengths) if max_len == 'longest' else max_len
    qkv = _bf(T, 3 * H * D, seed=16, scale=0.7)
    dctx = _bf(T, H * D, seed=17)
    kw = dict(p=0.1 if mode == 'dropout' else 0.0, causal=mode == 'causal')
    cu = _cu(lengths)
    return (qkv, dctx, cu, ml, kw) + tuple(_run(qkv, dctx, cu, ml, H, D, 'cpu', **kw))


@pytest.mark.parametrize('idx,max_len,mode', PARAMS, ids=[f'case{c}-{ml}-{m}' for c, ml, m in PARAMS])
def test_varlen_flash_attention_fwd_bwd(idx, max_len, mode):
    lengths, H, D, tail = CASES[idx]
    E = H * D
    qkv, dctx, cu, ml, kw, ctx_r, lse_r, dq_r = _case(idx, max_len, mode)
    ctx_g, lse_g, dq_g = _run(qkv, dctx, cu, ml, H, D, DEV, **kw)
    torch.cuda.synchronize()
    part = lambda t, i: t[:, i * E:(i + 1) * E]  # noqa: E731
    figures = [rel(ctx_g, ctx_r), rel(lse_g, lse_r)] + [rel_or_scale(part(dq_g, i), part(dq_r, i), part(dq_r, 2))
                                                        for i in range(3)]
    print(idx, max_len, mode, 'rel ctx / lse / dQ / dK / dV:', ' '.join(f'{v:.2e}' for v in figures))
    per_seq = {}
    for b, (c0, c1) in enumerate(zip(cu[:-1].tolist(), cu[1:].tolist())):
        if c1 > c0:
            per_seq[b] = [rel_or_scale(part(dq_g, i)[c0:c1], part(dq_r, i)[c0:c1], part(dq_r, 2)[c0:c1])
                          for i in range(3)]
            print('  sequence', b, 'rows', c0, c1, 'dQ / dK / dV:', ' '.join(f'{v:.2e}' for v in per_seq[b]))
    assert torch.isfinite(ctx_g.float()).all() and torch.isfinite(dq_g.float()).all() and torch.isfinite(lse_g).all()
    assert figures[0] < 1e-2
    assert figures[1] < 1e-4
    for i in range(3):   # dQ, dK, dV separately
        assert figures[2 + i] < 2e-2, i
        for b, f in per_seq.items():
            assert f[i] < 2e-2, (b, i)
    # the rows of no sequence: exactly zero
    end = int(cu[-1])
    assert ctx_g[end:].abs().sum().item() == 0 and dq_g[end:].abs().sum().item() == 0
    assert lse_g.view(H, -1)[:, end:].abs().sum().item() == 0


def _padded(qkv, dctx, cu, S, H, D, p):
    """The same sequences through the padded kernels at [n, S] with a -inf key bias on the padding."""
    lens = (cu[1:] - cu[:-1]).tolist()
    B, E = len(lens), H * D
    pq = torch.zeros(B, S, 3 * E, dtype=torch.bfloat16)
    pd = torch.zeros(B, S, E, dtype=torch.bfloat16)
    kb = torch.zeros(B, S)
    for b, n in enumerate(lens):
        c0 = int(cu[b])
        pq[b, :n], pd[b, :n] = qkv[c0:c0 + n], dctx[c0:c0 + n]
        kb[b, n:] = NEG
    scale = 1.0 / math.sqrt(D)
    seed = torch.tensor([29], dtype=torch.int32, device=DEV)
    pq, pd, kb = pq.view(B * S, -1).to(DEV), pd.view(B * S, -1).to(DEV), kb.to(DEV)
    ctx, lse = Tx.attn_fwd(pq, kb, B, S, H, scale, p, seed, 33, head_dim=D)
    dq = Tx.attn_bwd(pq, kb, pd, lse, B, S, H, scale, p, seed, 33, head_dim=D, ctx=ctx)
    return ctx.view(B, S, -1), dq.view(B, S, -1)


@pytest.mark.parametrize('idx', [2, 4])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_packed_agrees_with_padded_kernels(idx, p, monkeypatch):
    """Same sequences, same dropout elements: every real row of the varlen result against the
    padded streaming kernels at S = max_len."""
    monkeypatch.setattr(Tx, '_FLASH_ONLY', True)
    lengths, H, D, tail = CASES[idx]
    E = H * D
    qkv, dctx, cu, ml, _, _, _, _ = _case(idx, 'longest', 'plain')
    ctx_v, _, dq_v = _run(qkv, dctx, cu, ml, H, D, DEV, p=p)
    ctx_p, dq_p = _padded(qkv, dctx, cu, ml, H, D, p)
    torch.cuda.synchronize()
    worst = 0.0
    for b, n in enumerate(lengths):
        c0 = int(cu[b])
        worst = max(worst, (ctx_v[c0:c0 + n].float() - ctx_p[b, :n].float()).abs().max().item(),
                    (dq_v[c0:c0 + n].float() - dq_p[b, :n].float()).abs().max().item())
        assert rel(ctx_v[c0:c0 + n], ctx_p[b, :n]) < 1e-2, b
        for i in range(3):
            got, ref = dq_v[c0:c0 + n, i * E:(i + 1) * E], dq_p[b, :n, i * E:(i + 1) * E]
            assert rel_or_scale(got, ref, dq_p[b, :n, 2 * E:]) < 2e-2, (b, i)
    print(f'case {idx} p={p}: largest elementwise difference packed vs padded {worst:.3e}')


def test_sequences_are_isolated():
    """Every row of sequence 1 of case 2 perturbed: the ctx, lse and dqkv rows of sequences 0, 2
    and 3 are bit-identical."""
    lengths, H, D, tail = CASES[2]
    qkv, dctx, cu, ml, _, _, _, _ = _case(2, 'longest', 'plain')
    other, dother = qkv.clone(), dctx.clone()
    c0, c1 = int(cu[1]), int(cu[2])
    other[c0:c1] = _bf(c1 - c0, qkv.shape[1], seed=53, scale=2.0)
    dother[c0:c1] = _bf(c1 - c0, dctx.shape[1], seed=54, scale=2.0)
    a = _run(qkv, dctx, cu, ml, H, D, DEV, p=0.1)
    b = _run(other, dother, cu, ml, H, D, DEV, p=0.1)
    torch.cuda.synchronize()
    keep = torch.ones(qkv.shape[0], dtype=torch.bool)
    keep[c0:c1] = False
    assert torch.equal(a[0][keep], b[0][keep]) and torch.equal(a[2][keep], b[2][keep])
    assert torch.equal(a[1].view(H, -1)[:, keep], b[1].view(H, -1)[:, keep])
    assert not torch.equal(a[0][~keep], b[0][~keep])


def test_graph_replay_on_another_split():
    """Forward + backward captured once for case 3's T and nseq_max; cu_seqlens and qkv are
    overwritten in place with another split and the replay equals an eager call."""
    lengths, H, D, tail = CASES[3]
    E, T, ml = H * D, sum(lengths) + tail, 130
    scale = 1.0 / math.sqrt(D)
    qkv, dctx = _bf(T, 3 * E, seed=16, scale=0.7).to(DEV), _bf(T, E, seed=17).to(DEV)
    cu = _cu(lengths).to(DEV)
    seed = torch.tensor([29], dtype=torch.int32, device=DEV)

    def body():
        ctx, lse = Tx.attn_fwd_varlen(qkv, cu, ml, H, scale, 0.1, seed, 33, head_dim=D)
        return ctx, lse, Tx.attn_bwd_varlen(qkv, cu, ml, dctx, lse, H, scale, 0.1, seed, 33, head_dim=D, ctx=ctx)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                   # warm-up: library load, allocator
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = body()
        new = [70, 0, 23, 100, 0]
        assert sum(new) <= T
        cu.copy_(_cu(new).to(DEV))
        qkv.copy_(_bf(T, 3 * E, seed=61, scale=0.7).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out]
        ref = body()
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for g, r in zip(got, ref):
        assert torch.equal(g, r)
    end = sum(new)
    assert got[0][end:].abs().sum().item() == 0 and got[2][end:].abs().sum().item() == 0
    assert got[0][:end].abs().sum().item() > 0
