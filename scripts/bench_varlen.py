"""Packed (varlen) against padded, interleaved in one process on one GPU; JSON lines on stdout.

``attn``: BERT-base attention (H = 12, D = 64, max_len = 128), lengths drawn once (seeded,
uniform in [8, 128]) to fill T = 4096: varlen forward + backward against the padded flash
kernels over the same sequences at [n, 128] with a -inf key bias.
``step``: the BERT-base training step, ``pack_tokens=4096`` against the padded step at
32 x 128, on the same seeded variable-length data (each loads its batches the way the runner
would); sequences/s and real tokens/s.

Every pair is timed back to back and the pairs are repeated; medians and spreads (max - min)
are reported.  Usage: ``python scripts/bench_varlen.py attn|step [--pairs N]``."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlcomp_amd.ops import transformer as Tx  # noqa: E402
from mlcomp_amd.train.data import TokenBudgetBatchSampler  # noqa: E402
from mlcomp_amd.train.graphed import work_stream  # noqa: E402

DEV = 'cuda'
H, D, MAX_LEN, T = 12, 64, 128, 4096


def draw_lengths(total, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    while True:
        n = int(torch.randint(8, MAX_LEN + 1, (1,), generator=g))
        if sum(out) + n > total:
            return out
        out.append(n)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters       # us per call


def summary(v):
    return {'median': round(statistics.median(v), 2), 'spread': round(max(v) - min(v), 2), 'n': len(v)}


def bench_attn(pairs, iters=50):
    lengths = draw_lengths(T)
    n, E, scale = len(lengths), H * D, 1.0 / math.sqrt(D)
    cu = torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(1)
    qkv = (torch.randn(T, 3 * E, generator=g) * 0.7).to(torch.bfloat16).to(DEV)
    dctx = torch.randn(T, E, generator=g).to(torch.bfloat16).to(DEV)
    pq = torch.zeros(n, MAX_LEN, 3 * E, dtype=torch.bfloat16, device=DEV)
    pd = torch.zeros(n, MAX_LEN, E, dtype=torch.bfloat16, device=DEV)
    kb = torch.zeros(n, MAX_LEN, device=DEV)
    for b, L in enumerate(lengths):
        c0 = int(cu[b])
        pq[b, :L], pd[b, :L] = qkv[c0:c0 + L], dctx[c0:c0 + L]
        kb[b, L:] = float('-inf')
    pq, pd = pq.view(n * MAX_LEN, -1), pd.view(n * MAX_LEN, -1)
    seed = torch.tensor([3], dtype=torch.int32, device=DEV)

    def varlen():
        ctx, lse = Tx.attn_fwd_varlen(qkv, cu, MAX_LEN, H, scale, 0.1, seed, 16, head_dim=D)
        Tx.attn_bwd_varlen(qkv, cu, MAX_LEN, dctx, lse, H, scale, 0.1, seed, 16, head_dim=D, ctx=ctx)

    def padded():
        ctx, lse = Tx.attn_fwd(pq, kb, n, MAX_LEN, H, scale, 0.1, seed, 16, head_dim=D)
        Tx.attn_bwd(pq, kb, pd, lse, n, MAX_LEN, H, scale, 0.1, seed, 16, head_dim=D, ctx=ctx)

    res = {'varlen': [], 'padded': []}
    with work_stream(torch.device(DEV)):
        for fn in (varlen, padded):
            timed(fn, 10)
        for _ in range(pairs):
            res['varlen'].append(timed(varlen, iters))
            res['padded'].append(timed(padded, iters))
    print(json.dumps({'bench': 'attn_fwd_bwd_us', 'H': H, 'D': D, 'max_len': MAX_LEN, 'T': T, 'nseq': n,
                      'tokens': sum(lengths), 'varlen': summary(res['varlen']), 'padded': summary(res['padded']),
                      'raw': res}))


def bench_step(pairs, steps=20):
    from mlcomp_amd.train.data import SyntheticTextClassification
    from mlcomp_amd.train.native_bert_step import NativeBertStep
    ds = SyntheticTextClassification(num_samples=4096, seq_len=MAX_LEN, lengths={'min': 8, 'max': MAX_LEN}, seed=0)
    lens = ds.lengths()
    nseq_max = 128

    def batches(index_lists):
        out = []
        for idx in index_lists:
            out.append((ds.ids[idx], ds.y[idx], ds.tt[idx], ds.mask[idx]))
        return out

    packed_b = batches(list(TokenBudgetBatchSampler(lens, T, nseq_max)))
    padded_b = batches([list(range(i, i + 32)) for i in range(0, len(lens) - 31, 32)])
    mk = lambda **kw: NativeBertStep('bert-base', device=DEV, use_graph=True, warmup_eager=2, **kw)  # noqa: E731
    packed = mk(batch=nseq_max, seq_len=MAX_LEN, pack_tokens=T)
    padded = mk(batch=32, seq_len=MAX_LEN)

    def run(step, data, k0, n):
        seqs = toks = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            ids, y, tt, mask = data[(k0 + i) % len(data)]
            step.load_batch(ids, y, tt, mask)
            step()
            seqs += ids.shape[0]
            toks += int(mask.sum())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return seqs / dt, toks / dt

    for st, data in ((packed, packed_b), (padded, padded_b)):
        run(st, data, 0, 6)          # eager warm-up, capture, first replays
    res = {'packed_seq_s': [], 'packed_tok_s': [], 'padded_seq_s': [], 'padded_tok_s': []}
    for p in range(pairs):
        for name, st, data in (('packed', packed, packed_b), ('padded', padded, padded_b)):
            s, t = run(st, data, 6 + p * steps, steps)
            res[name + '_seq_s'].append(s)
            res[name + '_tok_s'].append(t)
    assert packed.graph is not None and padded.graph is not None
    print(json.dumps({'bench': 'bert_base_step', 'pack_tokens': T, 'nseq_max': nseq_max, 'padded': '32x128',
                      'lengths': 'uniform[8,128]', 'steps_per_run': steps,
                      'mean_seqs_per_packed_step': round(sum(b[0].shape[0] for b in packed_b) / len(packed_b), 1),
                      **{k: summary(v) for k, v in res.items()}, 'raw': res}))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['attn', 'step'])
    ap.add_argument('--pairs', type=int, default=None)
    a = ap.parse_args()
    if a.what == 'attn':
        bench_attn(a.pairs or 7)
    else:
        bench_step(a.pairs or 3)
