"""Grouped-query attention against what a user had to do without it, on one GPU.

Two arms per shape, forward + backward, each captured into a graph once and timed by replaying
it (device events around ``iters`` replays), the arms alternating within every round:

* ``gqa``      - ``attn_fwd_gqa`` + ``attn_bwd_gqa`` on qkv [B*S, (H + 2*Hkv)*D];
* ``expanded`` - ``repeat_interleave`` K / V to H heads, ``attn_fwd`` + ``attn_bwd`` on
  [B*S, 3*H*D], then the group sum of dK / dV back to Hkv heads.

Prints (and appends to ``out.jsonl`` when given) one JSON line per shape: median and spread
(max - min) over the rounds, in ms.  The last shape under-fills the dK / dV grid
(B * Hkv * ceil(S/128) = 16 blocks)."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlcomp_amd.ops import transformer as Tx  # noqa: E402

# (B, S, H, Hkv, D, causal)
SHAPES = [(8, 2048, 32, 8, 128, True), (32, 512, 12, 4, 64, False), (2, 512, 16, 2, 64, True)]


def arms(B, S, H, Hkv, D, causal, dev='cuda'):
    G, scale = H // Hkv, 1 / math.sqrt(D)
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.randn(B * S, (H + 2 * Hkv) * D, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    dctx = torch.randn(B * S, H * D, device=dev, generator=g).to(torch.bfloat16)

    def gqa():
        ctx, lse = Tx.attn_fwd_gqa(qkv, None, B, S, H, Hkv, scale, head_dim=D, causal=causal)
        return ctx, Tx.attn_bwd_gqa(qkv, None, dctx, lse, B, S, H, Hkv, scale, head_dim=D, ctx=ctx, causal=causal)

    def expanded():
        q, k, v = qkv.view(B * S, H + 2 * Hkv, D).split([H, Hkv, Hkv], 1)
        wide = torch.cat([q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)], 1).view(B * S, 3 * H * D)
        ctx, lse = Tx.attn_fwd(wide, None, B, S, H, scale, head_dim=D, causal=causal)
        d = Tx.attn_bwd(wide, None, dctx, lse, B, S, H, scale, head_dim=D, ctx=ctx, causal=causal)
        dq, dk, dv = d.view(B * S, 3, H, D).unbind(1)
        dk, dv = (t.reshape(B * S, Hkv, G, D).sum(2) for t in (dk, dv))
        return ctx, torch.cat([dq, dk, dv], 1).view(B * S, (H + 2 * Hkv) * D)

    return {'gqa': gqa, 'expanded': expanded}


def capture(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def replay_ms(graph, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main(out=None, rounds=7):
    assert torch.cuda.is_available(), 'this measures GPU kernels: it needs a GPU'
    for B, S, H, Hkv, D, causal in SHAPES:
        graphs = {name: capture(fn) for name, fn in arms(B, S, H, Hkv, D, causal).items()}
        (ctx_a, d_a), (ctx_b, d_b) = graphs['gqa'][1], graphs['expanded'][1]
        for gr, _ in graphs.values():
            gr.replay()
        torch.cuda.synchronize()
        rel = lambda x, y: ((x.float() - y.float()).norm() / y.float().norm()).item()
        r = dict(B=B, S=S, H=H, Hkv=Hkv, D=D, causal=causal, rounds=rounds, kv_blocks=B * Hkv * ((S + 127) // 128),
                 ctx_equal=bool(torch.equal(ctx_a, ctx_b)), dqkv_rel_diff=round(rel(d_a, d_b), 6))
        # a window of about 0.2 s per arm and round, sized from a first replay timing
        iters = {n: max(5, min(400, int(200 / max(replay_ms(gr, 5), 1e-3)))) for n, (gr, _) in graphs.items()}
        times = {n: [] for n in graphs}
        for _ in range(rounds):
            for n, (gr, _) in graphs.items():
                times[n].append(replay_ms(gr, iters[n]))
        for n, t in times.items():
            r[n] = dict(median_ms=round(sorted(t)[len(t) // 2], 4), spread_ms=round(max(t) - min(t), 4), iters=iters[n])
        r['expanded_over_gqa'] = round(r['expanded']['median_ms'] / r['gqa']['median_ms'], 3)
        print(json.dumps(r), flush=True)
        if out:
            with open(out, 'a') as f:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
