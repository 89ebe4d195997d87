"""Text record files on the CPU (`mlcomp_amd/train/records.py`, `csrc/runtime/records.cpp`,
`mlcomp_amd/train/tokenizer.py`): the ``MLTXT001`` format next to the three image formats, the
epoch plan of the C++ loader against ``TokenBudgetBatchSampler._fill``, the PyTorch twin of
``mlc_text_unpack`` against ``NativeBertStep.pack`` / ``load_packed``, the WordPiece tokenizer
against hand-derived ids, the packing CLI, the CPU loader in both layouts, ``dataset: records``
stages through the runner and the sanitizer self-tests of the new C entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from mlcomp_amd.train.data import SyntheticTextClassification, TokenBudgetBatchSampler
from mlcomp_amd.train.records import (CLIP_MAGIC, SEG_MAGIC, TEXT_ENTRY, TEXT_HEADER, TEXT_MAGIC, ClipRecordFile,
                                      PackedTextBatch, RecordFile, SegRecordFile, TextRecordFile, TextRecordLoader,
                                      runtime, text_slot_ints, text_unpack_reference, write_clip_records,
                                      write_records, write_seg_records, write_text_records)
from mlcomp_amd.train.tokenizer import WordPieceTokenizer

from test_bert_packed_cpu import LENGTHS, MAX_LEN, NSEQ_MAX, TOKENS, batch_of, make_step


def text_file(tmp_path, n=300, lo=1, hi=32, vocab=97, seed=0, name='t.mlrec', learnable=False):
    """n sequences of seeded lengths in [lo, hi], ids in [1, vocab), type0_length = length // 2;
    label i % 3, or (first token) % 2 for ``learnable``."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n)
    seqs = [rng.integers(1, vocab, int(k)) for k in lens]
    labels = [int(s[0]) % 2 for s in seqs] if learnable else [i % 3 for i in range(n)]
    path = str(tmp_path / name)
    assert write_text_records(path, seqs, labels, type0_lengths=[len(s) // 2 for s in seqs], vocab_size=vocab) == n
    return path, seqs, labels


# ------------------------------------------------------------------------- 1. format
@pytest.mark.parametrize('vocab,tb', [(97, 2), (65536, 2), (70000, 4)])
def test_text_round_trip(tmp_path, vocab, tb):
    path, seqs, labels = text_file(tmp_path, n=9, hi=12, vocab=vocab, seed=3)
    assert not os.path.exists(path + '.tmp')
    f = TextRecordFile(path)
    total = sum(len(s) for s in seqs)
    assert len(f) == 9 and f.max_len == max(len(s) for s in seqs) and f.vocab_size == vocab
    assert f.token_bytes == tb and f.total_tokens == total and f.lengths() == [len(s) for s in seqs]
    assert os.path.getsize(path) == 64 + 24 * 9 + tb * total
    for i in range(9):
        assert np.array_equal(f.tokens(i), seqs[i]) and f.label(i) == labels[i]
        assert f.type0_length(i) == len(seqs[i]) // 2
    g = TextRecordFile(path, seq_len=16)
    item, want = g[4], SyntheticTextClassification(num_samples=2, seq_len=16, vocab_size=97)[0]
    assert set(item) == set(want) and {k: type(v) for k, v in item.items()} == {k: type(v) for k, v in want.items()}
    n = len(seqs[4])
    assert item['input_ids'].shape == (16,) and item['input_ids'].dtype == torch.int64
    assert item['input_ids'][:n].tolist() == seqs[4].tolist() and not item['input_ids'][n:].any()
    assert item['attention_mask'].tolist() == [1] * n + [0] * (16 - n)
    assert item['token_type_ids'].tolist() == [0] * (n // 2) + [1] * (n - n // 2) + [0] * (16 - n)
    assert item['targets'] == labels[4]
    with pytest.raises(ValueError, match='longest record'):
        TextRecordFile(path, seq_len=f.max_len - 1)
    rt = runtime()
    h = rt.mlr_text_open(path.encode())
    assert h
    shp = (C.c_uint64 * 5)()
    rt.mlr_text_shape(h, shp)
    rt.mlr_close(h)
    assert [int(v) for v in shp] == [9, f.max_len, vocab, tb, total]
    # token types given as rows
    p2 = str(tmp_path / 'tt.mlrec')
    write_text_records(p2, [[5, 6, 7], [8]], [0, 1], token_types=[[0, 1, 1], [0]], vocab_size=10)
    f2 = TextRecordFile(p2)
    assert [f2.type0_length(i) for i in range(2)] == [1, 1] and f2[0]['token_type_ids'].tolist() == [0, 1, 1]
    p3 = str(tmp_path / 'nt.mlrec')
    write_text_records(p3, [[5, 6, 7]], [0], vocab_size=10)            # no types: all type 0
    assert TextRecordFile(p3).type0_length(0) == 3


def test_each_of_the_four_readers_refuses_the_other_three_kinds(tmp_path):
    imgs = np.random.default_rng(2).integers(0, 256, (4, 2, 2, 3), dtype=np.uint8)
    cls, seg, vid, txt = (str(tmp_path / n) for n in ('c.mlrec', 's.mlrec', 'v.mlrec', 't.mlrec'))
    write_records(cls, imgs, list(range(4)))
    write_seg_records(seg, imgs, np.ones((4, 2, 2, 1), np.uint8))
    write_clip_records(vid, imgs[:, None], list(range(4)))
    write_text_records(txt, [[1, 2], [3], [4, 5, 6], [7]], list(range(4)), vocab_size=9)
    rt = runtime()
    views = {cls: RecordFile, seg: SegRecordFile, vid: ClipRecordFile, txt: TextRecordFile}
    opens = {cls: rt.mlr_open, seg: rt.mlr_seg_open, vid: rt.mlr_clip_open, txt: rt.mlr_text_open}
    refused = 0
    for path in views:
        for other in views:
            h = opens[other](path.encode())
            if other == path:
                assert h and len(views[other](path)) == 4
                rt.mlr_close(h)
                continue
            assert not h
            with pytest.raises(ValueError):
                views[other](path)
            refused += 1
    assert refused == 12
    assert len({TEXT_MAGIC, SEG_MAGIC, CLIP_MAGIC}) == 3 and TEXT_MAGIC == b'MLTXT001'
    with pytest.raises(ValueError, match='cannot open text record file'):
        TextRecordLoader(cls, 2, device='cpu')


def test_corrupt_text_files_are_refused(tmp_path):
    path, seqs, _ = text_file(tmp_path, n=12, hi=9, seed=1)
    raw = open(path, 'rb').read()
    total = sum(len(s) for s in seqs)
    H = max(len(s) for s in seqs)
    rt = runtime()

    def refused(data, what):
        p = str(tmp_path / 'bad.mlrec')
        with open(p, 'wb') as f:
            f.write(data)
        assert not rt.mlr_text_open(p.encode()), what
        with pytest.raises(ValueError):
            TextRecordFile(p)

    def with_entry(i, **fields):
        index = np.frombuffer(raw, dtype=TEXT_ENTRY, count=12, offset=64).copy()
        for k, v in fields.items():
            index[i][k] = v
        return raw[:64] + index.tobytes() + raw[64 + 24 * 12:]
    h = rt.mlr_text_open(path.encode())
    assert h
    rt.mlr_close(h)
    refused(raw[:-1], 'short file')
    refused(raw[:40], 'short header')
    refused(with_entry(3, length=0), 'length 0')
    refused(with_entry(3, length=H + 1), 'length > H')
    refused(with_entry(3, type0_length=len(seqs[3]) + 1), 'type0_length > length')
    refused(with_entry(11, token_offset=total - len(seqs[11]) + 1), 'offset past total_tokens')
    refused(with_entry(3, token_offset=2 ** 64 - 2), 'offset + length wraps')
    fields = list(TEXT_HEADER.unpack(raw[:64]))
    refused(TEXT_HEADER.pack(*(fields[:5] + [0] + fields[6:])) + raw[64:], 'count 0')
    refused(TEXT_HEADER.pack(*(fields[:7] + [total + 1])) + raw[64:], 'total_tokens past the file')
    refused(TEXT_HEADER.pack(*([fields[0], fields[1], 70000] + fields[3:])) + raw[64:], 'u16 tokens, vocab 70000')


def test_writer_refuses_bad_ids_and_token_types(tmp_path):
    out = str(tmp_path / 'w.mlrec')
    for kw in (dict(sequences=[[1, 2, 97]], labels=[0], vocab_size=97),                     # id == vocab
               dict(sequences=[[1, -1]], labels=[0], vocab_size=97),
               dict(sequences=[[1, 2], []], labels=[0, 1], vocab_size=97),                  # an empty sequence
               dict(sequences=[[1, 2, 3]], labels=[0], token_types=[[0, 1, 0]], vocab_size=97),   # not a prefix
               dict(sequences=[[1, 2, 3]], labels=[0], token_types=[[1, 0, 0]], vocab_size=97),
               dict(sequences=[[1, 2, 3]], labels=[0], token_types=[[0, 2, 2]], vocab_size=97),
               dict(sequences=[[1, 2, 3]], labels=[0], token_types=[[0, 1]], vocab_size=97),
               dict(sequences=[[1, 2, 3]], labels=[0], type0_lengths=[4], vocab_size=97),
               dict(sequences=[[1], [2]], labels=[0], vocab_size=97),                       # fewer labels
               dict(sequences=[], labels=[], vocab_size=97),
               dict(sequences=[[1]], labels=[0])):                                          # no vocab_size
        with pytest.raises(ValueError):
            write_text_records(out, **kw)
        assert not os.path.exists(out) and not os.path.exists(out + '.tmp')
    assert write_text_records(out, [[0, 96]], [5], token_types=[[0, 1]], vocab_size=97) == 1


# ------------------------------------------------------------------------- 2. plan
MAX_TOKENS, MAX_SEQS = 96, 8


def plan(path, epoch=0, threads=4, world=1, rank=0, train=True, seed=3, max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS,
         max_len=32):
    L = TextRecordLoader(path, max_seqs, max_len=max_len, pack_tokens=max_tokens, train=train, seed=seed, rank=rank,
                         world_size=world, threads=threads, device='cpu', chunk=3)
    L.set_epoch(epoch)
    n = len(L)
    batches = [b['indices'].tolist() for b in L]
    assert len(batches) == n
    L.close()
    return batches


def check_plan(batches, lengths, max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS):
    """Budgets, maximality, and the batches TokenBudgetBatchSampler._fill makes of the same order."""
    for k, b in enumerate(batches):
        tokens = sum(lengths[i] for i in b)
        assert 1 <= len(b) <= max_seqs and tokens <= max_tokens
        if k + 1 < len(batches):
            assert len(b) == max_seqs or tokens + lengths[batches[k + 1][0]] > max_tokens
    order = [i for b in batches for i in b]
    assert len(set(order)) == len(order)
    assert TokenBudgetBatchSampler(lengths, max_tokens, max_seqs)._fill(order) == batches


def test_epoch_plan(tmp_path):
    path, seqs, _ = text_file(tmp_path)
    lengths = [len(s) for s in seqs]
    assert min(lengths) == 1 and max(lengths) == 32
    ref = plan(path, threads=1)
    check_plan(ref, lengths)
    assert sorted(i for b in ref for i in b) == list(range(300))          # world 1: every index exactly once
    assert plan(path, threads=3) == ref and plan(path, threads=8) == ref
    assert plan(path, epoch=1) != ref and plan(path, seed=4) != ref
    assert plan(path, epoch=1) == plan(path, epoch=1, threads=1)
    assert any(len(b) == MAX_SEQS for b in ref) and any(len(b) < MAX_SEQS for b in ref[:-1])   # both budgets bind
    for world in (2, 3):
        ranks = [plan(path, world=world, rank=r) for r in range(world)]
        assert len({len(b) for b in ranks}) == 1                          # equal step counts
        seen = [i for b in ranks for step in b for i in step]
        assert len(set(seen)) == len(seen) and len(seen) > 300 - 2 * world * MAX_SEQS
        for r, b in enumerate(ranks):
            check_plan(b, lengths)
            assert b == plan(path, world=world, rank=r, threads=1)


def test_eval_plan_keeps_file_order_and_every_batch(tmp_path):
    path, seqs, _ = text_file(tmp_path)
    lengths = [len(s) for s in seqs]
    ev = plan(path, train=False)
    check_plan(ev, lengths)
    assert [i for b in ev for i in b] == list(range(300))
    assert ev == TokenBudgetBatchSampler(lengths, MAX_TOKENS, MAX_SEQS)._batches()
    assert plan(path, train=False, epoch=5) == ev
    ranks = [plan(path, train=False, world=3, rank=r) for r in range(3)]
    for r, b in enumerate(ranks):
        assert [i for step in b for i in step] == list(range(r, 300, 3))  # all of its own, no padding
        check_plan(b, lengths)


def test_sequence_budget_binds_when_every_length_is_one(tmp_path):
    path, seqs, _ = text_file(tmp_path, n=37, lo=1, hi=1, name='ones.mlrec')
    batches = plan(path)
    assert [len(b) for b in batches] == [8, 8, 8, 8, 5]
    check_plan(batches, [1] * 37)


def test_loader_arguments(tmp_path):
    path, _, _ = text_file(tmp_path, n=20)
    with pytest.raises(ValueError, match='max_len = 31'):
        TextRecordLoader(path, 4, max_len=31, device='cpu')
    with pytest.raises(ValueError, match='pack_tokens'):
        TextRecordLoader(path, 4, max_len=32, pack_tokens=24, device='cpu')
    with pytest.raises(ValueError, match='multiple of 8'):
        TextRecordLoader(path, 4, max_len=32, pack_tokens=100, device='cpu')
    for bs in (0, 1025):
        with pytest.raises(ValueError, match='1 .. 1024'):
            TextRecordLoader(path, bs, max_len=32, device='cpu')
    with pytest.raises(ValueError) as e:
        TextRecordLoader(path, 4, max_len=32, vocab_size=96, device='cpu')
    assert '97' in str(e.value) and '96' in str(e.value)
    with pytest.raises(ValueError, match='layout'):
        TextRecordLoader(path, 4, max_len=32, layout='nchw', device='cpu')
    rt = runtime()
    h = rt.mlr_text_open(path.encode())
    for args in ((96, 8, 31), (31, 8, 32), (96, 0, 32), (96, 1025, 32)):
        assert not rt.mlr_text_loader_create(h, *args, 1, 0, 0, 1, 1, 2, 4)
    ok = rt.mlr_text_loader_create(h, 96, 8, 32, 1, 0, 0, 1, 1, 2, 4)
    assert ok
    rt.mlr_loader_destroy(ok)
    rt.mlr_close(h)


# ------------------------------------------------------------------------- 3. twin
def slot_of(seqs, labels, t0s, max_tokens, nmax, nseq=None, total=None):
    """The int32 slot head the loader would stage for these sequences."""
    head, _ = text_slot_ints(max_tokens, nmax)
    s = torch.zeros(head, dtype=torch.int32)
    s[0] = len(seqs) if nseq is None else nseq
    s[1] = sum(len(q) for q in seqs) if total is None else total
    for i, q in enumerate(seqs):
        s[2 + 3 * i:5 + 3 * i] = torch.tensor([len(q), t0s[i], labels[i]], dtype=torch.int32)
    tokens = torch.tensor([t for q in seqs for t in q], dtype=torch.int32)[:max_tokens]   # what fits the slot
    s[2 + 3 * nmax:2 + 3 * nmax + tokens.numel()] = tokens
    return s


def test_reference_equals_pack_and_load_packed():
    """The six tensors of the twin are what NativeBertStep.pack + load_packed put into the step's
    buffers for the same sequences; slot_w bit for bit."""
    for lengths, seed in ((LENGTHS, 1), ([48, 48, 48, 16], 2), ([7], 3), ([1, 1, 1, 1, 1, 1], 4)):
        ids, y, tt, mask = batch_of(lengths, seed=seed)
        st = make_step('cpu', True)
        st.load_batch(ids, y, tt, mask)
        seqs = [ids[i, :n].tolist() for i, n in enumerate(lengths)]
        slot = slot_of(seqs, y.tolist(), [n // 2 for n in lengths], TOKENS, NSEQ_MAX)
        got, err = text_unpack_reference(slot, TOKENS, NSEQ_MAX, MAX_LEN, 97, 3)
        assert err == 0
        want = {'ids': st.ids, 'tt': st.tt, 'pos_ids': st.net.pos_ids, 'cu': st.net.cu, 'y': st.y,
                'slot_w': st.net.slot_w}
        for k, v in want.items():
            assert got[k].dtype == v.dtype and got[k].shape == v.shape and torch.equal(got[k], v), k
        pad, err = text_unpack_reference(slot, TOKENS, NSEQ_MAX, MAX_LEN, 97, 3, layout='padded')
        n = len(lengths)
        assert err == 0 and torch.equal(pad['input_ids'][:n], ids) and torch.equal(pad['token_type_ids'][:n], tt)
        assert torch.equal(pad['attention_mask'][:n], mask) and torch.equal(pad['y'][:n], y)
        assert not pad['input_ids'][n:].any() and not pad['attention_mask'][n:].any() and not pad['y'][n:].any()


def test_reference_clamps_and_counts():
    T, nmax, L, V, K = 16, 4, 6, 10, 3
    # nseq 6 > nmax (1); lengths 9 > max_len (1), -2 (1), 5 cut to the 4 rows left of T (1), total (1);
    # type0 7 > 6 (1) and 3 > 0 (1); label 3 (1); tokens 10, 15, -1 among the first 16 (3)
    s = slot_of([[1] * 9, [], [2] * 6, [3] * 5], [0, 1, 3, 2], [7, 3, 2, 1], T, nmax, nseq=6, total=20)
    s[2 + 3] = -2
    tok = 2 + 3 * nmax
    s[tok], s[tok + 3], s[tok + 15] = V, V + 5, -1
    got, err = text_unpack_reference(s, T, nmax, L, V, K)
    assert err == 11
    assert got['cu'].tolist() == [0, 6, 6, 12, 16] and got['y'].tolist() == [0, 1, 2, 2]
    assert got['slot_w'].tolist() == [1 / 3, 0.0, 1 / 3, 1 / 3] or torch.equal(
        got['slot_w'], torch.tensor([1, 0, 1, 1]).float() / 3)
    assert got['ids'].tolist() == [9, 1, 1, 9, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 0]
    assert got['pos_ids'].tolist() == [0, 1, 2, 3, 4, 5] * 2 + [0, 1, 2, 3]
    assert got['tt'].tolist() == [0] * 6 + [0, 0, 1, 1, 1, 1] + [0, 1, 1, 1]
    pad, perr = text_unpack_reference(s, T, nmax, L, V, K, layout='padded')
    assert perr == err and pad['attention_mask'].sum(1).tolist() == [6, 0, 6, 4]
    assert pad['input_ids'][3].tolist() == [2, 2, 2, 0, 0, 0]
    empty, err = text_unpack_reference(slot_of([], [], [], T, nmax), T, nmax, L, V, K)
    assert err == 0 and not any(v.any() for v in empty.values())


# ------------------------------------------------------------------------- 4. tokenizer
VOCAB = ['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]', 'the', 'quick', 'brown', 'fox', 'jump', '##s', '##ed', 'over',
         'lazy', 'dog', ',', '.', '!', '?', 'un', '##aff', '##able', 'cafe', 'resume', 'hello', 'world', '中', '国',
         'a', '##b', '##c', 'is', 'it', "'", 's', 'new', 'york', '-', '##ing', 'play']
CASES = [('The quick  brown fox jumps!', [5, 6, 7, 8, 9, 10, 17]),
         ('Café RÉSUMÉ', [22, 23]),                       # lower-cased, accents stripped
         ('unaffable', [19, 20, 21]),
         ('unaffablez', [1]),                             # no piece for the tail: the whole word is [UNK]
         ('hello, world.', [24, 15, 25, 16]),
         ('中国hello', [26, 27, 24]),                      # CJK characters stand alone
         ("it's", [32, 33, 34]),
         ('abc', [28, 29, 30]),
         ('playing new-york', [39, 38, 35, 37, 36]),
         ('\thello world\n', [24, 25]),
         ('hel\x00lo', [24]),                             # control characters vanish
         ('a' * 101, [1]),                                # over 100 characters
         ('xyz quick', [1, 6]),
         ('', [])]


def vocab_file(tmp_path, tokens=VOCAB):
    p = tmp_path / 'vocab.txt'
    p.write_text('\n'.join(tokens) + '\n', encoding='utf-8')
    return str(p)


def test_wordpiece_tokenizer(tmp_path):
    assert len(VOCAB) == 40
    path = vocab_file(tmp_path)
    tok = WordPieceTokenizer(path)
    for text, want in CASES:
        assert tok.ids(text) == want, text
    cased = WordPieceTokenizer(path, lower=False)
    assert cased.ids('The quick') == [1, 6] and cased.ids('Café') == [1] and cased.ids('cafe') == [22]
    # encoding: [CLS] a [SEP] (b [SEP]), type0_length through the first [SEP]
    assert tok.encode('hello world') == ([2, 24, 25, 3], 4)
    assert tok.encode('') == ([2, 3], 2)
    assert tok.encode('the quick brown fox', max_len=4) == ([2, 5, 6, 3], 4)
    a, b = 'the quick brown fox', 'lazy dog'
    assert tok.encode(a, b) == ([2, 5, 6, 7, 8, 3, 13, 14, 3], 6)
    assert tok.encode(a, b, max_len=8) == ([2, 5, 6, 7, 3, 13, 14, 3], 5)       # the longer side first
    assert tok.encode(a, b, max_len=6) == ([2, 5, 6, 3, 13, 3], 4)              # b on a tie
    assert tok.encode(b, a, max_len=6) == ([2, 13, 14, 3, 5, 3], 4)
    assert tok.encode('', 'lazy dog') == ([2, 3, 13, 14, 3], 2)
    with pytest.raises(ValueError):
        tok.encode(a, max_len=1)
    for lacking in ('[CLS]', '[SEP]', '[UNK]'):
        (tmp_path / 'x').mkdir(exist_ok=True)
        with pytest.raises(ValueError, match='lacks'):
            WordPieceTokenizer(vocab_file(tmp_path / 'x', [t for t in VOCAB if t != lacking]))
    try:                                                   # the same strings through BertTokenizer, where it exists
        from transformers import BertTokenizer
    except ImportError:
        return
    import inspect
    key = 'vocab' if 'vocab' in inspect.signature(BertTokenizer.__init__).parameters else 'vocab_file'
    for lower, ours in ((True, tok), (False, cased)):
        theirs = BertTokenizer(**{key: path}, do_lower_case=lower)
        for text, _ in CASES:
            if '\x00' in text:
                continue
            assert theirs.encode(text, add_special_tokens=False) == ours.ids(text), (text, lower)
        for ml in (16, 8, 6):
            got = theirs(a, b, max_length=ml, truncation='longest_first')
            ids, t0 = ours.encode(a, b, max_len=ml)
            assert got['input_ids'] == ids and got['token_type_ids'] == [0] * t0 + [1] * (len(ids) - t0), ml


# ------------------------------------------------------------------------- 5. CLI
def test_contrib_pack_text_records_cli(tmp_path):
    from click.testing import CliRunner
    from mlcomp_amd.contrib.__main__ import main
    vocab = vocab_file(tmp_path)
    csv = tmp_path / 'data.csv'
    csv.write_text('text,other,label,fold\n'
                   '"The quick brown fox",lazy dog,pos,0\n'
                   '"hello, world.",,neg,1\n'
                   'unaffable,it\'s,pos,0\n'
                   '"jumps over the lazy dog",hello,neg,1\n', encoding='utf-8')
    out = str(tmp_path / 'x.mlrec')
    r = CliRunner().invoke(main, ['pack-text-records', '--csv', str(csv), '--vocab', vocab, '--out', out,
                                  '--max-len', '7'])
    assert r.exit_code == 0, r.output
    f = TextRecordFile(out)
    assert len(f) == 4 and f.vocab_size == 40 and f.token_bytes == 2 and f.max_len == 7
    assert open(out + '.classes').read().split() == ['neg', 'pos']
    assert [f.label(i) for i in range(4)] == [1, 0, 1, 0]
    assert f.tokens(0).tolist() == [2, 5, 6, 7, 8, 3] and f.type0_length(0) == 6
    assert f.tokens(1).tolist() == [2, 24, 15, 25, 16, 3]
    assert f.tokens(3).tolist() == [2, 9, 10, 12, 5, 13, 3]                  # truncated to max_len - 2 pieces
    pair = str(tmp_path / 'p.mlrec')
    r = CliRunner().invoke(main, ['pack-text-records', '--csv', str(csv), '--vocab', vocab, '--out', pair,
                                  '--text-col', 'text', '--text-b-col', 'other', '--label-col', 'label',
                                  '--max-len', '16', '--cased'])
    assert r.exit_code == 0, r.output
    f = TextRecordFile(pair)
    assert f.tokens(0).tolist() == [2, 1, 6, 7, 8, 3, 13, 14, 3] and f.type0_length(0) == 6   # cased: "The" unknown
    assert f.tokens(1).tolist() == [2, 24, 15, 25, 16, 3] and f.type0_length(1) == 6           # no second text
    assert f.tokens(2).tolist() == [2, 19, 20, 21, 3, 32, 33, 34, 3] and f.type0_length(2) == 5
    folds = tmp_path / 'fold.csv'
    folds.write_text('fold\n0\n1\n0\n1\n')
    for extra, want in ((['--fold-csv', str(folds)], [1, 1]), (['--fold-csv', str(folds), '--exclude-fold'], [0, 0]),
                        ([], [1, 1])):                                       # the CSV's own fold column
        o = str(tmp_path / f'f{len(extra)}.mlrec')
        r = CliRunner().invoke(main, ['pack-text-records', '--csv', str(csv), '--vocab', vocab, '--out', o,
                                      '--fold', '0'] + extra)
        assert r.exit_code == 0, r.output
        f = TextRecordFile(o)
        assert [f.label(i) for i in range(len(f))] == want
    r = CliRunner().invoke(main, ['pack-text-records', '--csv', str(csv), '--vocab', vocab, '--out', out,
                                  '--text-col', 'nope'])
    assert r.exit_code != 0 and 'nope' in r.output


# ------------------------------------------------------------------------- 6. CPU loader
@pytest.mark.parametrize('vocab', [97, 70000])
def test_cpu_loader_in_both_layouts(tmp_path, vocab):
    path, seqs, labels = text_file(tmp_path, n=50, hi=20, vocab=vocab, seed=5)
    view = TextRecordFile(path, seq_len=24)
    # padded, plain batches of 8 in file order
    L = TextRecordLoader(path, 8, max_len=24, train=False, layout='padded', num_labels=3, device='cpu')
    assert len(L) == 7 and L.T == 192
    seen = []
    for b in L:
        assert set(b) == {'input_ids', 'token_type_ids', 'attention_mask', 'targets', 'indices'}
        idx = b['indices'].tolist()
        seen += idx
        for k in ('input_ids', 'token_type_ids', 'attention_mask'):
            assert b[k].dtype == torch.int64 and torch.equal(b[k], torch.stack([view[i][k] for i in idx])), k
        assert b['targets'].tolist() == [labels[i] for i in idx] and b['targets'].dtype == torch.int64
    assert seen == list(range(50)) and L.bad_tokens() == 0
    # packed: every batch's tensors against the twin of hand-made slots
    P = TextRecordLoader(path, 6, max_len=24, pack_tokens=64, train=True, layout='packed', num_labels=3, seed=1,
                         device='cpu')
    seen = []
    for b in P:
        assert set(b) == {'packed', 'targets', 'indices'} and isinstance(b['packed'], PackedTextBatch)
        pb, idx = b['packed'], b['indices'].tolist()
        seen += idx
        assert pb.nseq == len(idx) and pb.tokens == sum(len(seqs[i]) for i in idx)
        assert (pb.T, pb.nmax, pb.max_len, pb.vocab, pb.num_labels) == (64, 6, 24, vocab, 3)
        assert b['targets'].tolist() == [labels[i] for i in idx]
        slot = slot_of([seqs[i] for i in idx], [labels[i] for i in idx], [len(seqs[i]) // 2 for i in idx], 64, 6)
        want, _ = text_unpack_reference(slot, 64, 6, 24, vocab, 3)
        got = pb.tensors()
        assert list(got) == ['ids', 'tt', 'pos_ids', 'cu', 'y', 'slot_w']
        for k in want:
            assert torch.equal(got[k], want[k]), k
        with pytest.raises(ValueError, match='unpack_into'):
            pb.unpack_into(*[got[k] for k in ('ids', 'tt', 'pos_ids', 'y', 'cu', 'slot_w')])
    assert sorted(seen) == list(range(50)) and seen != list(range(50))
    # labels the model has no class for are clamped, counted, and the epoch ends with an error
    B = TextRecordLoader(path, 8, max_len=24, train=False, layout='padded', num_labels=2, device='cpu')
    with pytest.raises(ValueError, match='out of range'):
        for b in B:
            assert int(b['targets'].max()) <= 1
    # drop_last, for engines of one batch shape
    D = TextRecordLoader(path, 8, max_len=24, layout='padded', num_labels=3, device='cpu', drop_last=True)
    assert len(D) == 6 and [len(b['targets']) for b in D] == [8] * 6


# ------------------------------------------------------------------------- 7. runner
def stage_cfg(tmp_path, train, valid, **args):
    return {'model_params': {'model': 'bert-tiny', 'num_labels': 3},
            'args': dict({'expdir': '.', 'logdir': str(tmp_path / 'log')}, **args),
            'stages': {'data_params': {'dataset': 'records', 'path': train, 'valid_path': valid, 'seq_len': MAX_LEN,
                                       'batch_size': NSEQ_MAX, 'num_workers': 2, 'seed': 1},
                       'state_params': {'num_epochs': 2, 'main_metric': 'loss', 'minimize_metric': True},
                       'criterion_params': {'criterion': 'CrossEntropyLoss'},
                       'optimizer_params': {'optimizer': 'AdamW', 'lr': 1e-3},
                       'callbacks_params': {'loss': {'callback': 'CriterionCallback'},
                                            'optimizer': {'callback': 'OptimizerCallback'}},
                       'stage1': {}}}


def test_runner_trains_a_packed_native_stage_from_text_records(tmp_path, monkeypatch):
    from mlcomp_amd.train.experiment import ConfigExperiment
    from mlcomp_amd.train.runner import Runner
    monkeypatch.setenv('MLC_NATIVE_CPU', '1')
    train, _, _ = text_file(tmp_path, n=40, lo=2, hi=MAX_LEN, vocab=1000, name='tr.mlrec')
    valid, _, _ = text_file(tmp_path, n=10, lo=2, hi=MAX_LEN, vocab=1000, seed=1, name='va.mlrec')
    torch.manual_seed(0)
    r = Runner(ConfigExperiment(stage_cfg(tmp_path, train, valid, engine='native', pack_tokens=TOKENS)), device='cpu')
    sizes = []
    real = Runner._fire
    monkeypatch.setattr(Runner, '_fire', lambda self, ev: (sizes.append(self.state.batch_size)
                                                          if ev == 'on_batch_end' and self.state.is_train else None,
                                                          real(self, ev))[1])
    state = r.run_experiment()
    assert r.engine_log[0]['engine'] == 'native' and r.engine_log[0]['pack_tokens'] == TOKENS
    tr, va = r.loaders['train'], r.loaders['valid']
    assert isinstance(tr, TextRecordLoader) and tr.layout == 'packed' and tr.train
    assert (tr.max_tokens, tr.max_seqs, tr.max_len, tr.vocab_size, tr.num_labels) == (TOKENS, NSEQ_MAX, MAX_LEN, 1024, 3)
    assert va.layout == 'padded' and not va.train
    ns = r.native_step
    assert ns.packed and ns.net.T == TOKENS and ns.batch == NSEQ_MAX and ns.seq_len == MAX_LEN
    m = state.epoch_metrics
    assert m['train_loss'] == m['train_loss'] and 0 < m['train_loss'] < 3 and np.isfinite(m['valid_loss'])
    assert 0 <= m['train_accuracy01'] <= 1
    assert len(set(sizes)) > 1 and all(1 <= s <= NSEQ_MAX for s in sizes)      # the real sequence counts
    # a file packed with a larger vocabulary than the model's is refused when the loaders are built
    big, _, _ = text_file(tmp_path, n=8, vocab=2000, name='big.mlrec')
    r2 = Runner(ConfigExperiment(stage_cfg(tmp_path, big, None, engine='native', pack_tokens=TOKENS)), device='cpu')
    with pytest.raises(ValueError, match='2000.*1024'):
        r2.run_experiment()


@pytest.mark.parametrize('say_kind', [True, False])
def test_runner_trains_a_padded_torch_stage_from_text_records(tmp_path, say_kind):
    from mlcomp_amd.train.experiment import ConfigExperiment
    from mlcomp_amd.train.runner import Runner
    train, _, _ = text_file(tmp_path, n=20, lo=2, hi=MAX_LEN, vocab=1000, name='tr.mlrec')
    valid, _, _ = text_file(tmp_path, n=7, lo=2, hi=MAX_LEN, vocab=1000, seed=1, name='va.mlrec')
    cfg = stage_cfg(tmp_path, train, valid, engine='torch')
    if say_kind:
        cfg['stages']['data_params']['kind'] = 'text'
    r = Runner(ConfigExperiment(cfg), device='cpu')
    state = r.run_experiment()
    assert all(isinstance(v, TextRecordLoader) and v.layout == 'padded' for v in r.loaders.values())
    assert len(r.loaders['train']) == 4 and len(r.loaders['valid']) == 2
    b = next(iter(r.loaders['valid']))
    assert b['input_ids'].shape == (NSEQ_MAX, MAX_LEN) and b['indices'].tolist() == list(range(NSEQ_MAX))
    m = state.epoch_metrics
    assert np.isfinite(m['train_loss']) and np.isfinite(m['valid_loss'])


# ------------------------------------------------------------------------- 8. sanitizers
@pytest.mark.parametrize('san', ['tsan', 'asan'])
def test_text_loader_sanitizer_selftest(san, tmp_path):
    """ThreadSanitizer / AddressSanitizer+UBSan builds of the C++ runtime under a stand-alone
    driver of the text entry points, run as a child process."""
    from mlcomp_amd.build import build_runtime_selftest
    binary = build_runtime_selftest(san, main='records_text_selftest.cpp')
    assert os.path.basename(binary) == f'mlcomp-records-text-selftest-{san}'
    r = subprocess.run([binary, str(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TSAN_OPTIONS='halt_on_error=1', ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'records text selftest ok' in r.stdout
    assert 'WARNING: ThreadSanitizer' not in r.stderr and 'ERROR: AddressSanitizer' not in r.stderr
