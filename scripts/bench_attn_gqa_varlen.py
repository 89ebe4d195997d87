"""Packed grouped-query attention against the two ways round it, on one GPU.

Three arms per case, causal forward + backward without dropout, each captured into a graph once
and timed by replaying it, the arms alternating within every round:

* ``packed``   - ``attn_fwd_gqa_varlen`` + ``attn_bwd_gqa_varlen`` on qkv [T, (H + 2*Hkv)*D];
* ``expanded`` - ``repeat_interleave`` K / V to H heads, ``attn_fwd_varlen`` + ``attn_bwd_varlen``
  on [T, 3*H*D], then the group sum of dK / dV back to Hkv heads;
* ``padded``   - ``attn_fwd_gqa`` + ``attn_bwd_gqa`` on the same sequences right-padded to
  [nseq, max_len] (causal: no real query sees a padding key, so no key bias; the copies into and
  out of the padded layout are not timed).

Lengths are seeded, uniform in [max_len/16, max_len], drawn until they fill T = 16384 rows (the
last one cut to fit).  Prints (and appends to ``out.jsonl`` when given) one JSON line per case:
median and spread (max - min) over the rounds, in ms."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlcomp_amd.ops import transformer as Tx  # noqa: E402
from bench_attn_gqa import capture, replay_ms  # noqa: E402

T = 16384
# (H, Hkv, D, max_len)
CASES = [(32, 8, 128, 512), (32, 8, 128, 2048), (16, 4, 64, 512), (16, 4, 64, 2048)]


def lengths_for(max_len, seed=0):
    g, out = torch.Generator().manual_seed(seed), []
    while sum(out) < T:
        out.append(min(int(torch.randint(max_len // 16, max_len + 1, (1,), generator=g)), T - sum(out)))
    return out


def arms(H, Hkv, D, max_len, lens, dev='cuda'):
    G, scale, n, W = H // Hkv, 1 / math.sqrt(D), len(lens), (H + 2 * Hkv) * D
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.randn(T, W, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    dctx = torch.randn(T, H * D, device=dev, generator=g).to(torch.bfloat16)
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    pq = torch.zeros(n, max_len, W, device=dev, dtype=torch.bfloat16)
    pd = torch.zeros(n, max_len, H * D, device=dev, dtype=torch.bfloat16)
    for b, L in enumerate(lens):
        c0 = int(cu[b])
        pq[b, :L], pd[b, :L] = qkv[c0:c0 + L], dctx[c0:c0 + L]
    pq, pd = pq.view(n * max_len, W), pd.view(n * max_len, H * D)

    def packed():
        ctx, lse = Tx.attn_fwd_gqa_varlen(qkv, cu, max_len, H, Hkv, scale, head_dim=D, causal=True)
        return ctx, Tx.attn_bwd_gqa_varlen(qkv, cu, max_len, dctx, lse, H, Hkv, scale, head_dim=D, ctx=ctx, causal=True)

    def expanded():
        q, k, v = qkv.view(T, H + 2 * Hkv, D).split([H, Hkv, Hkv], 1)
        wide = torch.cat([q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)], 1).view(T, 3 * H * D)
        ctx, lse = Tx.attn_fwd_varlen(wide, cu, max_len, H, scale, head_dim=D, causal=True)
        d = Tx.attn_bwd_varlen(wide, cu, max_len, dctx, lse, H, scale, head_dim=D, ctx=ctx, causal=True)
        dq, dk, dv = d.view(T, 3, H, D).unbind(1)
        dk, dv = (t.reshape(T, Hkv, G, D).sum(2) for t in (dk, dv))
        return ctx, torch.cat([dq, dk, dv], 1).view(T, W)

    def padded():
        ctx, lse = Tx.attn_fwd_gqa(pq, None, n, max_len, H, Hkv, scale, head_dim=D, causal=True)
        return ctx, Tx.attn_bwd_gqa(pq, None, pd, lse, n, max_len, H, Hkv, scale, head_dim=D, ctx=ctx, causal=True)

    return {'packed': packed, 'expanded': expanded, 'padded': padded}


def main(out=None, rounds=7):
    assert torch.cuda.is_available(), 'this measures GPU kernels: it needs a GPU'
    for H, Hkv, D, max_len in CASES:
        lens = lengths_for(max_len)
        fns = arms(H, Hkv, D, max_len, lens)   # kept to the end of the case: the closures own qkv, dctx and cu
        graphs = {name: capture(fn) for name, fn in fns.items()}
        for gr, _ in graphs.values():
            gr.replay()
        torch.cuda.synchronize()
        (ctx_a, d_a), (ctx_b, d_b), (ctx_p, _) = (graphs[n][1] for n in ('packed', 'expanded', 'padded'))
        rel = lambda x, y: ((x.float() - y.float()).norm() / y.float().norm()).item()
        r = dict(H=H, Hkv=Hkv, D=D, max_len=max_len, T=T, nseq=len(lens), padded_rows=len(lens) * max_len, rounds=rounds,
                 kv_blocks=len(lens) * Hkv * ((max_len + 127) // 128), ctx_equal_expanded=bool(torch.equal(ctx_a, ctx_b)),
                 dqkv_rel_diff_expanded=round(rel(d_a, d_b), 6),
                 ctx_equal_padded_seq0=bool(torch.equal(ctx_a[:lens[0]], ctx_p[:lens[0]])))
        # a window of about 0.2 s per arm and round, sized from a first replay timing
        iters = {n: max(5, min(400, int(200 / max(replay_ms(gr, 5), 1e-3)))) for n, (gr, _) in graphs.items()}
        times = {n: [] for n in graphs}
        for _ in range(rounds):
            for n, (gr, _) in graphs.items():
                times[n].append(replay_ms(gr, iters[n]))
        for n, t in times.items():
            r[n] = dict(median_ms=round(sorted(t)[len(t) // 2], 4), spread_ms=round(max(t) - min(t), 4), iters=iters[n])
        for n in ('expanded', 'padded'):
            r[f'{n}_over_packed'] = round(r[n]['median_ms'] / r['packed']['median_ms'], 3)
        print(json.dumps(r), flush=True)
        if out:
            with open(out, 'a') as f:
                f.write(json.dumps(r) + '\n')
        del graphs, fns
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
