"""Single-token grouped-query attention over a K/V cache against what a user had to do without it,
on one GPU.

The arms of a shape, each captured into a graph once and timed by replaying it (device events around
``iters`` replays), alternating within every round:

* ``decode``   - ``attn_decode_gqa`` on kv_cache [B, L, 2*Hkv*D] (csrc/kernels/attn_decode.hip);
* ``paged16``, ``paged128`` - the same call with ``block_table=`` on the same logical data in pages of
  16 / 128 positions: the contiguous cache itself as the pool under the identity table, and
  ``*_shuffled``: a pool whose blocks a seeded permutation has scattered;
* ``composed`` - ``repeat_interleave`` of K / V to H heads, then bf16 ``bmm``, masked softmax, ``bmm``.

Prints (and appends to ``out.jsonl`` when given) one JSON line per shape: median and spread
(max - min) over the rounds in ms, the decode arm's bandwidth on its byte floor
B * Hkv * L * 2 * D * 2 (every K and V element of the cache read once), each paged arm's median over
the decode arm's, and whether every paged arm's ctx has the decode arm's bits.  All lengths equal L."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlcomp_amd.ops import _lib  # noqa: E402
from mlcomp_amd.ops import transformer as Tx  # noqa: E402
from bench_attn_gqa import capture, replay_ms  # noqa: E402  (scripts/ is the script's own directory)

# (B, L, H, Hkv, D); in the second only the key split fills the chip
SHAPES = [(64, 4096, 32, 8, 128), (1, 32768, 32, 8, 128), (8, 1024, 16, 4, 64)]


def arms(B, L, H, Hkv, D, dev='cuda'):
    G, scale = H // Hkv, 1 / math.sqrt(D)
    g = torch.Generator(device=dev).manual_seed(0)
    cache = (torch.randn(B, L, 2 * Hkv * D, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    packed = torch.randn(B, (H + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16)
    q = packed[:, :H * D]
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    ctx = torch.empty(B, H * D, device=dev, dtype=torch.bfloat16)

    def decode():
        return Tx.attn_decode_gqa(q, cache, lens, H, Hkv, scale, D, out=ctx)[0]

    def paged(page, shuffled):
        nblk = B * L // page
        order = torch.randperm(nblk, device=dev, generator=g) if shuffled else torch.arange(nblk, device=dev)
        pool = cache.view(nblk, page, -1)
        if shuffled:                                   # logical page i lives in block order[i]
            pool = torch.empty_like(pool)
            pool[order] = cache.view(nblk, page, -1)
        table, out = order.to(torch.int32).view(B, L // page), torch.empty_like(ctx)
        return lambda: Tx.attn_decode_gqa(q, pool, lens, H, Hkv, scale, D, out=out, block_table=table)[0]

    def composed():
        k, v = cache.view(B, L, 2, Hkv, D).unbind(2)
        k = k.repeat_interleave(G, 2).permute(0, 2, 1, 3).reshape(B * H, L, D)
        v = v.repeat_interleave(G, 2).permute(0, 2, 1, 3).reshape(B * H, L, D)
        s = torch.bmm(q.reshape(B * H, 1, D), k.transpose(1, 2)) * scale
        live = (torch.arange(L, device=dev)[None, :] < lens[:, None]).repeat_interleave(H, 0)[:, None, :]
        p = torch.softmax(s.float().masked_fill(~live, -math.inf), -1).to(torch.bfloat16)
        return torch.bmm(p, v).view(B, H * D)

    return {'decode': decode, 'paged16': paged(16, False), 'paged16_shuffled': paged(16, True),
            'paged128': paged(128, False), 'paged128_shuffled': paged(128, True), 'composed': composed}


def main(out=None, rounds=7):
    assert torch.cuda.is_available(), 'this measures GPU kernels: it needs a GPU'
    with torch.cuda.stream(torch.cuda.Stream()):
        for B, L, H, Hkv, D in SHAPES:
            graphs = {name: capture(fn) for name, fn in arms(B, L, H, Hkv, D).items()}
            for gr, _ in graphs.values():
                gr.replay()
            torch.cuda.synchronize()
            a, b = graphs['decode'][1].float(), graphs['composed'][1].float()
            r = dict(B=B, L=L, H=H, Hkv=Hkv, D=D, rounds=rounds, splits=_lib.load().mlc_attn_decode_splits(B, Hkv, L, 0),
                     ctx_rel_diff=round(((a - b).norm() / b.norm()).item(), 6),
                     paged_bit_equal=all(torch.equal(graphs['decode'][1].view(torch.int16), o.view(torch.int16))
                                         for n, (_, o) in graphs.items() if n.startswith('paged')))
            # a window of about 0.2 s per arm and round, sized from a first replay timing
            iters = {n: max(5, min(2000, int(200 / max(replay_ms(gr, 5), 1e-3)))) for n, (gr, _) in graphs.items()}
            times = {n: [] for n in graphs}
            for _ in range(rounds):
                for n, (gr, _) in graphs.items():
                    times[n].append(replay_ms(gr, iters[n]))
            for n, t in times.items():
                r[n] = dict(median_ms=round(sorted(t)[len(t) // 2], 4), spread_ms=round(max(t) - min(t), 4), iters=iters[n])
            floor = B * Hkv * L * 2 * D * 2
            r['floor_bytes'] = floor
            r['decode_tb_per_s'] = round(floor / (r['decode']['median_ms'] * 1e-3) / 1e12, 3)
            for n in graphs:
                if n != 'decode':
                    r[n + '_over_decode'] = round(r[n]['median_ms'] / r['decode']['median_ms'], 3)
            print(json.dumps(r), flush=True)
            if out:
                with open(out, 'a') as f:
                    f.write(json.dumps(r) + '\n')
            del graphs
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
