"""What feeding the packed BERT-base step costs, in one process on one GPU; JSON lines on
stdout (kept under ``profiles/text_records/``).

Workload: the ``step`` workload of ``scripts/bench_varlen.py`` - BERT-base, ``pack_tokens=4096``,
at most 64 sequences a step, a seeded file of 4096 sequences with lengths uniform in
[8, 128].  Three feeds of the same captured step, interleaved round by round:

  a. ``resident``: the step replayed on the batch it already holds (no feed at all);
  b. ``records``:  ``TextRecordLoader`` (C++ plan and gather, one copy, ``mlc_text_unpack``)
                   and ``load_text_batch``;
  c. ``python``:   ``DataLoader`` + ``TokenBudgetBatchSampler`` over ``TextRecordFile`` and
                   ``load_batch`` (host pad, host un-pad, six copies).

Reported: sequences/s and ms/step of each (median and spread = max - min over the rounds), the
feed cost b - a per step, and whether b beats c by more than three spreads of c.  Then the
loader alone (sequences/s with nothing consuming the GPU side but the unpack), and, stand-alone
on one batch, the unpack kernel's time against the host work and six copies of
``load_packed``.  Usage: ``python scripts/bench_text_records.py [--rounds 3] [--steps 40]``."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlcomp_amd.train.data import TokenBudgetBatchSampler, collate_dict  # noqa: E402
from mlcomp_amd.train.native_bert_step import NativeBertStep  # noqa: E402
from mlcomp_amd.train.records import TextRecordFile, TextRecordLoader, write_text_records  # noqa: E402

DEV = 'cuda'
MAX_LEN, T, NSEQ, N, VOCAB = 128, 4096, 64, 4096, 30522


def summary(v):
    return {'median': round(statistics.median(v), 3), 'spread': round(max(v) - min(v), 3), 'n': len(v)}


def write_file(path, seed=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(8, MAX_LEN + 1, N)
    seqs = [rng.integers(1, VOCAB, int(k)) for k in lens]
    write_text_records(path, seqs, [int(s[0]) % 2 for s in seqs], type0_lengths=[len(s) // 2 for s in seqs],
                       vocab_size=VOCAB)


def cycle(make):
    """Batches for ever: a new epoch's iterator whenever one runs out."""
    while True:
        yield from make()


def main(rounds, steps):
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, 'bench.mlrec')
    write_file(path)
    step = NativeBertStep('bert-base', batch=NSEQ, seq_len=MAX_LEN, pack_tokens=T, device=DEV, use_graph=True,
                          warmup_eager=2)
    loader = TextRecordLoader(path, NSEQ, max_len=MAX_LEN, pack_tokens=T, layout='packed', vocab_size=VOCAB,
                              num_labels=2, threads=4, device=DEV)
    ds = TextRecordFile(path, seq_len=MAX_LEN)
    sampler = TokenBudgetBatchSampler(ds.lengths(), T, NSEQ, shuffle=True)
    dl = torch.utils.data.DataLoader(ds, batch_sampler=sampler, num_workers=4, collate_fn=collate_dict,
                                     persistent_workers=True)
    rec, py = cycle(lambda: iter(loader)), cycle(lambda: iter(dl))

    def resident():
        step()
        return step.nseq

    def records():
        step.load_text_batch(next(rec)['packed'])
        step()
        return step.nseq

    def python():
        b = next(py)
        step.load_batch(b['input_ids'], b['targets'], b['token_type_ids'], b['attention_mask'])
        step()
        return step.nseq
    feeds = (('resident', resident), ('records', records), ('python', python))

    def run(fn, n):
        torch.cuda.synchronize()
        seqs, t0 = 0, time.perf_counter()
        for _ in range(n):
            seqs += fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return seqs / dt, dt / n * 1e3

    for _, fn in feeds[1:]:
        run(fn, 6)                   # eager warm-up, capture, first replays, loader threads up
    assert step.graph is not None, step.capture_error
    res = {f'{k}_{u}': [] for k, _ in feeds for u in ('seq_s', 'ms')}
    for _ in range(rounds):
        for name, fn in feeds:
            s, ms = run(fn, steps)
            res[f'{name}_seq_s'].append(s)
            res[f'{name}_ms'].append(ms)
    out = {k: summary(v) for k, v in res.items()}
    gain = out['python_ms']['median'] - out['records_ms']['median']
    print(json.dumps({'bench': 'text_records_step', 'model': 'bert-base', 'pack_tokens': T, 'nseq_max': NSEQ,
                      'lengths': 'uniform[8,128]', 'steps_per_run': steps, **out,
                      'feed_cost_ms_b_minus_a': round(out['records_ms']['median'] - out['resident_ms']['median'], 3),
                      'python_minus_records_ms': round(gain, 3),
                      'records_beats_python_by_3_spreads': bool(gain > 3 * out['python_ms']['spread']),
                      'raw': res}))

    # the loader alone: plan, gather, copy and unpack, no step
    rates = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0, seqs = time.perf_counter(), 0
        for b in loader:
            b['packed'].unpack_into(step.ids, step.tt, step.net.pos_ids, step.net.cu, step.y, step.net.slot_w)
            seqs += b['packed'].nseq
        torch.cuda.synchronize()
        rates.append(seqs / (time.perf_counter() - t0))
    print(json.dumps({'bench': 'text_loader_alone', 'threads': 4, 'seq_s': summary(rates)}))

    # one batch, stand-alone: the unpack kernel against load_packed's host work + six copies
    b = next(iter(dl))
    pb = next(iter(loader))['packed']
    p_ids, p_tt, pos, cu, lens = step.pack(b['input_ids'], b['token_type_ids'], b['attention_mask'])
    n_tok, n_seq = int(cu[-1]), lens.numel()

    def unpack():
        pb.unpack_into(step.ids, step.tt, step.net.pos_ids, step.net.cu, step.y, step.net.slot_w)

    def host():
        step.load_packed(p_ids[:n_tok], b['targets'], cu[:n_seq + 1], p_tt, pos)
    times = {}
    for name, fn in (('unpack_kernel_us', unpack), ('load_packed_us', host)):
        for _ in range(10):
            fn()
        v = []
        for _ in range(rounds * 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(50):
                fn()
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) / 50 * 1e6)
        times[name] = summary(v)
    print(json.dumps({'bench': 'text_unpack_vs_load_packed', 'what': 'host clock around 50 calls ending in a sync',
                      **times}))
    loader.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=40)
    a = ap.parse_args()
    main(a.rounds, a.steps)
