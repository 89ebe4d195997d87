"""Text record files on the GPU: ``mlc_text_unpack`` (`csrc/kernels/text.hip`) against its
PyTorch twin in both modes, its writes confined to the outputs, its clamping contract and its
launcher's refusals; the CUDA ``TextRecordLoader`` against the CPU one; ``load_text_batch``
against ``load_packed`` on a packed tiny-BERT step, before and after graph capture; and a
packed ``dataset: records`` stage through the runner."""
import numpy as np
import pytest
import torch

from mlcomp_amd.ops import _lib
from mlcomp_amd.train.records import TextRecordLoader, text_unpack_reference

from test_bert_packed_cpu import MAX_LEN, NSEQ_MAX, TOKENS, batch_of, make_step
from test_text_records_cpu import slot_of, stage_cfg, text_file

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = -77
KEYS = {'packed': ('ids', 'tt', 'pos_ids', 'cu', 'y', 'slot_w'),
        'padded': ('input_ids', 'token_type_ids', 'attention_mask', 'y')}


class Guarded:
    """The outputs of one launch, each a view into a larger allocation whose margins (T
    elements or more on each side) hold a sentinel, plus the guarded ``err`` counter."""

    def __init__(self, layout, T, nmax, max_len):
        rows = (T,) * 3 if layout == 'packed' else (nmax * max_len,) * 3
        shapes = {'packed': list(zip(KEYS['packed'], rows + (nmax + 1, nmax, nmax),
                                     (torch.int64,) * 3 + (torch.int32, torch.int64, torch.float32))),
                  'padded': list(zip(KEYS['padded'], rows + (nmax,), (torch.int64,) * 4))}[layout]
        self.layout, self.margin, self.big, self.out = layout, max(T, 64), {}, {}
        for k, n, dt in shapes + [('err', 1, torch.int32)]:
            self.big[k] = torch.full((n + 2 * self.margin,), SENT, dtype=dt, device=DEV)
            self.out[k] = self.big[k][self.margin:self.margin + n]
        self.out['err'].zero_()

    def launch(self, staged, T, nmax, max_len, vocab, labels, fn=None):
        o = self.out
        p = [_lib.ptr(o[k]) for k in KEYS[self.layout]]
        if self.layout == 'padded':
            p = p[:3] + [None, p[3], None]
        rc = (fn or _lib.load().mlc_text_unpack)(_lib.ptr(staged), int(self.layout == 'padded'), *p,
                                                 _lib.ptr(o['err']), T, nmax, max_len, vocab, labels, _lib.stream())
        torch.cuda.synchronize()
        return rc

    def margins_intact(self):
        m = self.margin
        return all(bool((b[:m] == SENT).all()) and bool((b[-m:] == SENT).all()) for b in self.big.values())

    def untouched(self):
        return all(bool((b == SENT).all()) for k, b in self.big.items() if k != 'err') and int(self.out['err']) == 0

    def check(self, want, err, T, nmax, max_len):
        assert self.margins_intact()
        assert int(self.out['err']) == err
        for k in KEYS[self.layout]:
            got = self.out[k].cpu().view(want[k].shape)
            assert got.dtype == want[k].dtype and torch.equal(got, want[k]), k


def staged_of(slot, extra=0):
    """The slot head on the device, inside an allocation with room to spare after it."""
    big = torch.zeros(slot.numel() + extra + 64, dtype=torch.int32)
    big[:slot.numel()] = slot
    return big.to(DEV)


def rand_batch(lengths, vocab, labels, seed=0):
    g = torch.Generator().manual_seed(seed)
    seqs = [torch.randint(0, vocab, (n,), generator=g).tolist() for n in lengths]
    return seqs, torch.randint(0, labels, (len(lengths),), generator=g).tolist(), [n // 2 for n in lengths]


CASES = [((64, 8, 16), [1]),                       # one sequence of length 1
         ((64, 8, 16), [16] * 4),                  # total = T exactly
         ((64, 8, 16), [3, 9, 1, 16, 2, 7, 5, 4]), # nseq = nmax, total < T
         ((72, 1, 72), [72]),                      # nmax = 1, T no multiple of the block size
         ((72, 1, 72), [5]),
         ((2048, 1024, 4), [2] * 1024),            # the scan crosses every wave of a block
         ((2048, 1024, 4), [1, 4, 2, 3] * 204),    # more than one block of rows, mixed lengths
         ((64, 8, 16), [])]                        # nseq = 0


@pytest.mark.parametrize('layout', ['packed', 'padded'])
@pytest.mark.parametrize('shape,lengths', CASES)
def test_kernel_equals_reference_and_writes_only_the_outputs(layout, shape, lengths):
    T, nmax, max_len = shape
    vocab, labels = 1000, 5
    seqs, y, t0s = rand_batch(lengths, vocab, labels, seed=len(lengths))
    slot = slot_of(seqs, y, t0s, T, nmax)
    want, err = text_unpack_reference(slot, T, nmax, max_len, vocab, labels, layout)
    assert err == 0
    g = Guarded(layout, T, nmax, max_len)
    assert g.launch(staged_of(slot), T, nmax, max_len, vocab, labels) == 0
    g.check(want, 0, T, nmax, max_len)
    if layout == 'packed' and lengths:
        assert g.out['slot_w'][0].item() == (torch.ones(1) / len(lengths)).item()


@pytest.mark.parametrize('layout', ['packed', 'padded'])
def test_clamping_contract(layout):
    """Every field out of range at once.  All values are small enough that a kernel without
    the clamps would still stay inside this test's guarded allocations (the length sum is 82
    rows of a 64 + 2 * 64 row allocation, nmax + 3 entries are read from the staged buffer's
    own token rows): this checks the clamps' arithmetic, nothing here can leave the buffers."""
    T, nmax, max_len, vocab, labels = 64, 8, 8, 50, 3
    lengths = [16, 12, 16, 14, 5, 10, 4, 5]                      # up to 2 * max_len, 82 in all
    seqs, y, t0s = rand_batch(lengths, vocab, labels, seed=9)
    t0s[2] = lengths[2] + 3                                      # type0_length > length
    y[1] = labels                                                # a label the model has no class for
    slot = slot_of(seqs, y, t0s, T, nmax, nseq=nmax + 3)         # total stays the unclamped 82
    slot[2 + 3 * 4] = -3                                         # a negative length
    tok = 2 + 3 * nmax
    slot[tok + 5], slot[tok + 20], slot[tok + 40] = vocab, vocab + 5, -1
    want, err = text_unpack_reference(slot, T, nmax, max_len, vocab, labels, layout)
    assert err == 14       # nseq 1, lengths 6, total 1, type0 2, label 1, tokens 3
    g = Guarded(layout, T, nmax, max_len)
    assert g.launch(staged_of(slot, extra=T), T, nmax, max_len, vocab, labels) == 0
    g.check(want, err, T, nmax, max_len)
    ids = g.out[KEYS[layout][0]]
    assert int(ids.min()) >= 0 and int(ids.max()) < vocab
    assert int(g.out['y'].min()) >= 0 and int(g.out['y'].max()) < labels
    if layout == 'packed':
        cu = g.out['cu'].cpu()
        assert bool((cu[1:] >= cu[:-1]).all()) and int(cu.max()) <= T and int(cu[0]) == 0
        assert int(g.out['pos_ids'].max()) < max_len
    else:
        assert int(g.out['attention_mask'].sum()) <= T


def test_launcher_refuses_bad_scalars_without_launching():
    T, nmax, max_len, vocab, labels = 64, 8, 16, 100, 3
    seqs, y, t0s = rand_batch([5, 7], vocab, labels)
    staged = staged_of(slot_of(seqs, y, t0s, T, nmax))
    fn = _lib.load().mlc_text_unpack
    bad = [dict(T=0), dict(T=-8), dict(T=60), dict(nmax=0), dict(nmax=1025), dict(max_len=0),
           dict(max_len=T + 1), dict(vocab=0), dict(vocab=-1), dict(labels=0)]
    for layout in ('packed', 'padded'):
        g = Guarded(layout, T, nmax, max_len)
        for kw in bad:
            a = dict(T=T, nmax=nmax, max_len=max_len, vocab=vocab, labels=labels)
            a.update(kw)
            assert g.launch(staged, **a) == -1, kw
            assert g.untouched(), kw
        o = g.out
        full = [_lib.ptr(staged), int(layout == 'padded')] + [_lib.ptr(o[k]) for k in KEYS['packed'] if k in o] \
            if layout == 'packed' else None
        if full:                                                   # a null pointer in every position
            full += [_lib.ptr(o['err'])]
            for i in [0] + list(range(2, 9)):
                args = list(full)
                args[i] = None
                assert fn(*args, T, nmax, max_len, vocab, labels, _lib.stream()) == -1, i
            assert fn(full[0], 2, *full[2:], T, nmax, max_len, vocab, labels, _lib.stream()) == -1     # no such mode
            torch.cuda.synchronize()
            assert g.untouched()
    with pytest.raises(RuntimeError, match='mlc_text_unpack'):
        _lib.call('mlc_text_unpack', _lib.ptr(staged), 0, *[None] * 7, T, nmax, max_len, vocab, labels,
                  _lib.stream())


# ------------------------------------------------------------------------- loaders
@pytest.mark.parametrize('vocab', [97, 70000])
@pytest.mark.parametrize('threads', [1, 4])
@pytest.mark.parametrize('layout', ['packed', 'padded'])
def test_cuda_loader_equals_cpu_loader(tmp_path, layout, threads, vocab):
    path, _, _ = text_file(tmp_path, n=60, hi=20, vocab=vocab, seed=7)
    kw = dict(max_len=24, pack_tokens=64, layout=layout, num_labels=3, seed=2)
    gpu = TextRecordLoader(path, 6, threads=threads, device=DEV, **kw)
    cpu = TextRecordLoader(path, 6, threads=2, device='cpu', **kw)
    steps = len(cpu)
    assert len(gpu) == steps > 5
    n = 0
    for a, b in zip(gpu, cpu):
        assert set(a) == set(b)
        assert a['indices'].device.type == 'cpu' and torch.equal(a['indices'], b['indices'])
        assert torch.equal(a['targets'].cpu(), b['targets'])
        if layout == 'packed':
            assert (a['packed'].nseq, a['packed'].tokens) == (b['packed'].nseq, b['packed'].tokens)
            ta, tb = a['packed'].tensors(), b['packed'].tensors()
            for k in KEYS['packed']:
                assert ta[k].device.type == 'cuda' and torch.equal(ta[k].cpu(), tb[k]), k
        else:
            for k in ('input_ids', 'token_type_ids', 'attention_mask'):
                assert a[k].device.type == 'cuda' and a[k].shape == b[k].shape and torch.equal(a[k].cpu(), b[k]), k
        n += 1
    assert n == steps and gpu.bad_tokens() == 0


def test_two_batches_held_at_once_keep_their_own_content(tmp_path):
    path, _, _ = text_file(tmp_path, n=60, hi=20, seed=7)
    kw = dict(max_len=24, pack_tokens=64, layout='packed', num_labels=3, seed=2)
    want = [b['packed'].tensors() for b in TextRecordLoader(path, 6, device='cpu', **kw)]
    it = iter(TextRecordLoader(path, 6, device=DEV, depth=3, **kw))
    for k in range(0, len(want) - 1, 2):
        first, second = next(it), next(it)                      # both staged before either is unpacked
        for j, b in ((k + 1, second), (k, first)):              # and unpacked newest first
            got = b['packed'].tensors()
            for key in KEYS['packed']:
                assert torch.equal(got[key].cpu(), want[j][key]), (j, key)
    it.close()


# ------------------------------------------------------------------------- step
def packed_args(ids, mask):
    """What load_packed takes for a right-padded batch."""
    lens = mask.sum(1)
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    return mask.bool(), cu


def step_batches(tmp_path):
    """Two different batches as a file of their own each: the padded tensors and the loader's
    PackedTextBatch of the same sequences (file order, one batch)."""
    from mlcomp_amd.train.records import write_text_records
    out = []
    for k, lengths in enumerate(([48, 5, 17, 1, 30], [9, 2, 31, 48, 16, 25])):
        ids, y, tt, mask = batch_of(lengths, seed=20 + k)
        path = str(tmp_path / f's{k}.mlrec')
        write_text_records(path, [ids[i, :n].tolist() for i, n in enumerate(lengths)], y.tolist(),
                           type0_lengths=[n // 2 for n in lengths], vocab_size=97)
        L = TextRecordLoader(path, NSEQ_MAX, max_len=MAX_LEN, pack_tokens=TOKENS, train=False, layout='packed',
                             vocab_size=97, num_labels=3, device=DEV)
        batches = list(L)
        assert len(batches) == 1 and batches[0]['indices'].tolist() == list(range(len(lengths)))
        out.append(((ids, y, tt, mask), batches[0]['packed'], L))
    return out


def buffers(st):
    return {'ids': st.ids, 'tt': st.tt, 'pos_ids': st.net.pos_ids, 'cu': st.net.cu, 'y': st.y, 'slot_w': st.net.slot_w}


def test_load_text_batch_equals_load_packed_before_and_after_capture(tmp_path):
    data = step_batches(tmp_path)
    # lr 0: the weights stay put, so the two steps' losses come from the same forward pass
    a = make_step(DEV, True, use_graph=True, warmup_eager=1)
    b = make_step(DEV, True, use_graph=True, warmup_eager=1)
    for k, ((ids, y, tt, mask), pb, _) in enumerate(data):      # step 0 eager, step 1 captured and replayed
        a.load_text_batch(pb)
        keep, cu = packed_args(ids, mask)
        b.load_packed(ids[keep], y, cu, tt[keep])
        torch.cuda.synchronize()
        assert a.nseq == b.nseq == len(y)
        for name, t in buffers(a).items():
            assert torch.equal(t, buffers(b)[name]), (k, name)
        a()
        b()
        torch.cuda.synchronize()
        la, lb = a.last_loss(), b.last_loss()
        print('batch', k, 'loss', la, lb)
        assert la == la and la == lb, (k, la, lb)
    assert a.graph is not None and b.graph is not None, (a.capture_error, b.capture_error)
    # once more after capture, the first batch again: the replayed graph reads the new buffers
    (ids, y, tt, mask), pb, _ = data[0]
    a.load_text_batch(pb)
    keep, cu = packed_args(ids, mask)
    b.load_packed(ids[keep], y, cu, tt[keep])
    a()
    b()
    torch.cuda.synchronize()
    assert a.last_loss() == b.last_loss() and a.nseq == 5


def test_load_text_batch_refusals(tmp_path):
    (_, pb, _), _ = step_batches(tmp_path)
    with pytest.raises(RuntimeError, match='pack_tokens'):
        make_step(DEV, False).load_text_batch(pb)
    path, _, _ = text_file(tmp_path, n=8, hi=MAX_LEN, name='o.mlrec')
    other = next(iter(TextRecordLoader(path, NSEQ_MAX, max_len=MAX_LEN, pack_tokens=TOKENS + 8, layout='packed',
                                       num_labels=3, device=DEV)))['packed']
    st = make_step(DEV, True)
    before = {k: v.clone() for k, v in buffers(st).items()}
    with pytest.raises(ValueError, match=f'{TOKENS + 8} token rows'):
        st.load_text_batch(other)
    big, _, _ = text_file(tmp_path, n=8, hi=MAX_LEN, vocab=200, name='big.mlrec')
    with pytest.raises(ValueError, match='200.*97'):            # told the model's vocabulary: refused at once
        TextRecordLoader(big, NSEQ_MAX, max_len=MAX_LEN, pack_tokens=TOKENS, vocab_size=97, device=DEV)
    loose = next(iter(TextRecordLoader(big, NSEQ_MAX, max_len=MAX_LEN, pack_tokens=TOKENS, layout='packed',
                                       num_labels=3, device=DEV)))['packed']
    with pytest.raises(ValueError, match='vocab_size = 97'):    # not told: the step refuses before any launch
        st.load_text_batch(loose)
    torch.cuda.synchronize()
    for k, v in buffers(st).items():
        assert torch.equal(v, before[k]), k


# ------------------------------------------------------------------------- runner
def test_runner_trains_a_packed_stage_from_text_records_on_the_gpu(tmp_path, monkeypatch):
    from mlcomp_amd.train.experiment import ConfigExperiment
    from mlcomp_amd.train.runner import Runner
    train, _, _ = text_file(tmp_path, n=192, lo=2, hi=MAX_LEN, vocab=1000, name='tr.mlrec', learnable=True)
    valid, _, _ = text_file(tmp_path, n=24, lo=2, hi=MAX_LEN, vocab=1000, seed=1, name='va.mlrec', learnable=True)
    cfg = stage_cfg(tmp_path, train, valid, engine='native', pack_tokens=TOKENS)
    cfg['model_params']['num_labels'] = 2
    torch.manual_seed(0)
    r = Runner(ConfigExperiment(cfg), device=DEV)
    sizes, losses = [], []
    real = Runner._fire

    def spy(self, ev):
        if ev == 'on_batch_end' and self.state.is_train:
            sizes.append(self.state.batch_size)
        if ev == 'on_epoch_end':
            losses.append(self.state.epoch_metrics['train_loss'])
        return real(self, ev)
    monkeypatch.setattr(Runner, '_fire', spy)
    state = r.run_experiment()
    assert r.engine_log[0]['engine'] == 'native' and r.engine_log[0]['pack_tokens'] == TOKENS
    tr = r.loaders['train']
    assert isinstance(tr, TextRecordLoader) and tr.layout == 'packed' and r.loaders['valid'].layout == 'padded'
    assert r.native_step.packed and r.native_step.net.T == TOKENS
    print('train loss per epoch', losses, 'metrics', state.epoch_metrics)
    assert len(losses) == 2 and losses[1] < losses[0]
    m = state.epoch_metrics
    assert 0 <= m['train_accuracy01'] <= 1 and np.isfinite(m['valid_loss'])
    assert len(set(sizes)) > 1 and all(1 <= s <= NSEQ_MAX for s in sizes)
    assert sum(sizes) == 2 * 192 and tr.bad_tokens() == 0
