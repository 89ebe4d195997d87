"""The fused language-model head + cross-entropy against the composed path, on one GPU.

Two arms per shape, forward + backward (loss per token, dh bf16, dw fp32 accumulated), eager on a
side stream, alternating within every round after a warm-up call each:

* ``fused``    - ``lm_loss_fwd`` + ``lm_loss_bwd`` (csrc/kernels/lmhead.hip: no [T, V] array; the
  backward goes through one reused dlogits chunk);
* ``composed`` - ``dense_fwd`` (bf16 logits), ``.float()``, ``softmax_ce`` (bf16 dlogits),
  ``dense_dgrad``, ``linear_wgrad``.

Per arm: median and spread (max - min) of the call time over the rounds in ms, the peak of
``torch.cuda.max_memory_allocated`` above the inputs during the warm-up call (workspace caches
emptied first), and the bytes of logits-shaped arrays the arm writes, computed from the shape.  An
arm that cannot be allocated is recorded as such.  Prints (and appends to ``out.jsonl`` when given)
one JSON line per shape."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlcomp_amd.ops import functional as Fn  # noqa: E402
from mlcomp_amd.ops import transformer as Tx  # noqa: E402

# (T, K, V)
CASES = [(8192, 2048, 32000), (8192, 4096, 128256)]


def arms(T, K, V, dev='cuda'):
    g = torch.Generator(device=dev).manual_seed(0)
    h = torch.randn(T, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(V, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
    labels = torch.randint(0, V, (T,), device=dev, generator=g)
    dnll = torch.full((T,), 1.0 / T, device=dev)
    dw, loss = torch.zeros(V, K, device=dev), torch.zeros(1, device=dev)

    def fused():
        nll, lse = Tx.lm_loss_fwd(h, w, labels)
        return nll.sum() / T, Tx.lm_loss_bwd(h, w, labels, lse, dnll, dw)

    def composed():
        z, _ = Tx.dense_fwd(h, w)
        dl = Fn.softmax_ce(z.float(), labels, loss.zero_(), scale=1.0 / T)
        del z
        dh = Tx.dense_dgrad(dl, w)
        Fn.linear_wgrad(dl, h, out=dw, accumulate=True)
        return loss[0] / T, dh

    return {'fused': fused, 'composed': composed}, dw


def timed_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def drop_workspaces():
    for cache in (Tx._WS, Tx._WS_OLD, Tx._LM_DL):
        cache.clear()
    torch.cuda.empty_cache()


def main(out=None, rounds=5):
    assert torch.cuda.is_available(), 'this measures GPU kernels: it needs a GPU'
    with torch.cuda.stream(torch.cuda.Stream()):
        for T, K, V in CASES:
            drop_workspaces()
            fns, dw = arms(T, K, V)
            chunk = min(T, max(128, Tx.LM_DL_BYTES // (2 * V) // 128 * 128))
            r = dict(T=T, K=K, V=V, rounds=rounds, logits_bf16_bytes=T * V * 2, fused_chunk_rows=chunk,
                     logits_shaped_bytes_written=dict(fused=T * V * 2, composed=T * V * (2 + 4 + 2)),
                     logits_shaped_bytes_resident=dict(fused=chunk * V * 2, composed=T * V * (2 + 4 + 2)))
            torch.cuda.synchronize()
            inputs, res, live = torch.cuda.memory_allocated(), {}, {}
            for n, fn in fns.items():
                drop_workspaces()
                torch.cuda.reset_peak_memory_stats()
                try:
                    res[n] = [t.clone() for t in fn()]          # the warm-up call
                    torch.cuda.synchronize()
                    live[n] = fn
                    r[n] = dict(peak_bytes_above_inputs=torch.cuda.max_memory_allocated() - inputs)
                except torch.OutOfMemoryError as e:
                    r[n] = dict(error=f'cannot be allocated: {str(e)[:120]}')
            if len(live) == 2:
                rel = lambda x, y: ((x.float() - y.float()).norm() / y.float().norm()).item()
                r['loss'] = [res['fused'][0].item(), res['composed'][0].item()]
                r['dh_rel_diff'] = round(rel(res['fused'][1], res['composed'][1]), 6)
            iters = {n: max(2, min(50, int(300 / max(timed_ms(fn, 1), 1e-3)))) for n, fn in live.items()}
            times = {n: [] for n in live}
            for _ in range(rounds):
                for n, fn in live.items():
                    times[n].append(timed_ms(fn, iters[n]))
            for n, t in times.items():
                r[n].update(median_ms=round(sorted(t)[len(t) // 2], 3), spread_ms=round(max(t) - min(t), 3), iters=iters[n])
            if len(live) == 2:
                r['composed_over_fused_time'] = round(r['composed']['median_ms'] / r['fused']['median_ms'], 3)
            print(json.dumps(r), flush=True)
            if out:
                with open(out, 'a') as f:
                    f.write(json.dumps(r) + '\n')
            del fns, live, res, dw, fn      # fn: the loops' last closure still owns this case's tensors
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
