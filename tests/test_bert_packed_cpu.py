"""Packed mode of the native BERT engine on its CPU twin: the packed step against the padded
``NativeBertStep`` over the same sequences (loss and every parameter gradient, the position
table's explicitly), packed ``predict``, ``load_batch``'s refusals, the token-budget batch
sampler, and a ``train`` stage with ``args.pack_tokens`` through ``Runner``.

Two evaluations of one engine are compared the way ``tests/test_engines_gpu_vs_cpu.py``
does: the reference step is run again with every weight perturbed by about one bf16 ulp, and
the step under test must be no further from the reference than that perturbation moves it."""
import copy
import logging

import pytest
import torch

from mlcomp_amd.models.bert import BertConfig, BertForSequenceClassification
from mlcomp_amd.train.data import SyntheticTextClassification, TokenBudgetBatchSampler
from mlcomp_amd.train.native_bert_step import NativeBertStep

NSEQ_MAX, MAX_LEN, TOKENS = 6, 48, 160
LENGTHS = [48, 5, 17, 1, 30]


def tiny_model():
    torch.manual_seed(0)
    return BertForSequenceClassification(BertConfig(
        vocab_size=97, hidden=128, layers=2, heads=2, intermediate=512, max_position=64, hidden_dropout=0.0,
        attention_dropout=0.0, num_labels=3))


def batch_of(lengths, seed=1, S=MAX_LEN):
    """A right-padded [n, S] batch: ids, labels, token types, attention mask."""
    g = torch.Generator().manual_seed(seed)
    n = len(lengths)
    mask = (torch.arange(S)[None] < torch.tensor(lengths)[:, None]).long()
    ids = torch.randint(1, 97, (n, S), generator=g) * mask
    tt = (torch.arange(S)[None] >= torch.tensor(lengths)[:, None] // 2).long() * mask
    return ids, torch.randint(0, 3, (n,), generator=g), tt, mask


def make_step(device, packed, model=None, n=len(LENGTHS), **kw):
    kw.setdefault('use_graph', False)
    kw.setdefault('lr', 0.0)
    tm = copy.deepcopy(model if model is not None else tiny_model())
    if packed:
        return NativeBertStep(torch_model=tm, batch=NSEQ_MAX, seq_len=MAX_LEN, device=device, num_labels=3,
                              pack_tokens=TOKENS, **kw)
    return NativeBertStep(torch_model=tm, batch=n, seq_len=MAX_LEN, device=device, num_labels=3, **kw)


def perturb(step, seed=1):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for a in step.net.arena.arenas():
            a.master.mul_(1 + 2 ** -9 * torch.randn(a.master.shape, generator=g).to(a.master.device))
        step.net.arena.decay.refresh_mirror()


def grads(step):
    step()
    if step.device.type == 'cuda':
        torch.cuda.synchronize()
    out = {}
    for name, slot in step.net.arena.by_name.items():
        g = slot.grad.detach().float().cpu().flatten()
        if float(g.norm()) > 0:
            out[name] = g.clone()
    return step.last_loss(), out


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-20))


def _cos(a, b):
    return float(a @ b / (a.norm() * b.norm() + 1e-20))


def assert_within_noise(ref, noise, got, what):
    """The bounds of test_native_engine_gpu_step_matches_cpu_within_bf16_noise."""
    (l_c, g_c), (l_p, g_p), (l_g, g_g) = ref, noise, got
    assert set(g_g) == set(g_c) and len(g_c) > 5, (what, sorted(set(g_c) ^ set(g_g))[:5])
    noise_l, err_l = abs(l_p - l_c) / abs(l_c), abs(l_g - l_c) / abs(l_c)
    assert err_l <= max(1e-2, 2 * noise_l), (what, l_g, l_c, l_p)
    cos_n = sum(_cos(g_p[n], g_c[n]) for n in g_c) / len(g_c)
    cos_g = sum(_cos(g_g[n], g_c[n]) for n in g_c) / len(g_c)
    assert cos_g >= cos_n - 0.02, (what, cos_g, cos_n)
    rn = {n: _rel(g_p[n], g_c[n]) for n in g_c}
    rg = {n: _rel(g_g[n], g_c[n]) for n in g_c}
    bad = {n: (round(rg[n], 4), round(rn[n], 4)) for n in g_c if rg[n] > 3 * rn[n] + 5e-2}
    assert not bad, (what, bad)
    print(f'{what}: {len(g_c)} slots, loss err {err_l:.2e} (noise {noise_l:.2e}), grad cos {cos_g:.4f} '
          f'(noise {cos_n:.4f}), worst grad rel {max(rg.values()):.4f}')
    return rg, rn


def test_packed_step_equals_padded_step():
    batch = batch_of(LENGTHS)
    padded, noisy, packed = make_step('cpu', False), make_step('cpu', False), make_step('cpu', True)
    perturb(noisy)
    for st in (padded, noisy, packed):
        st.load_batch(*batch)
    assert packed.nseq == 5 and packed.net.cu.tolist() == [0, 48, 53, 70, 71, 101, 101]
    ref, got = grads(padded), grads(packed)
    rg, rn = assert_within_noise(ref, grads(noisy), got, 'packed vs padded (cpu)')
    # the position table: fed through pos_ids in packed mode, through the column index when padded
    pos_ref, pos_got = ref[1]['pos'].view(64, 128), got[1]['pos'].view(64, 128)
    assert rg['pos'] <= 3 * rn['pos'] + 5e-2, (rg['pos'], rn['pos'])
    assert pos_got[MAX_LEN:].abs().max().item() == 0 and pos_got[:MAX_LEN].abs().sum(1).min().item() > 0
    for row in (0, 4, 16, 29, 47):      # positions 1, 5, 17, 30 and 48 sequences reach
        assert _rel(pos_got[row], pos_ref[row]) <= 3 * rn['pos'] + 5e-2, row
    assert abs(packed.accuracy() - padded.accuracy()) < 1e-6


def test_packed_predict_equals_padded_predict():
    ids, _, tt, mask = batch_of(LENGTHS, seed=2)
    padded, packed = make_step('cpu', False), make_step('cpu', True)
    want = padded.predict(ids, tt, mask)
    got = packed.predict(ids, tt, mask)
    assert got.shape == (5, 3)
    assert torch.allclose(got, want, atol=2e-3, rtol=1e-2), (got - want).abs().max()
    # a batch of more sequences than nseq_max: predict packs at its own size
    ids, _, tt, mask = batch_of([3, 9, 1, 48, 2, 7, 11, 5], seed=3)
    assert torch.allclose(packed.predict(ids, tt, mask), padded.predict(ids, tt, mask), atol=2e-3, rtol=1e-2)


def test_load_batch_refuses_what_does_not_fit():
    st = make_step('cpu', True)
    with pytest.raises(ValueError, match='nseq_max'):
        st.load_batch(*batch_of([3] * 7))
    with pytest.raises(ValueError, match='token budget'):
        st.load_batch(*batch_of([48, 48, 48, 20]))
    with pytest.raises(ValueError, match='max_len'):
        st.load_batch(*batch_of([49, 3], S=64))
    ids, y, tt, mask = batch_of([10, 20])
    mask[1, 3] = 0                                      # a hole: not right-padded
    with pytest.raises(ValueError, match='right-padded'):
        st.load_batch(ids, y, tt, mask)
    mask = torch.flip(batch_of([10, 20])[3], dims=[1])  # left-padded
    with pytest.raises(ValueError, match='right-padded'):
        st.load_batch(ids, y, tt, mask)
    with pytest.raises(ValueError, match='token ids'):
        st.load_batch(torch.full((2, 48), 97), y, tt, batch_of([10, 20])[3])
    st.load_batch(*batch_of([48, 48, 48, 16]))          # exactly the budget
    assert st.nseq == 4 and int(st.net.cu[-1]) == TOKENS
    # a step built without pack_tokens is today's engine
    assert make_step('cpu', False).packed is False


def test_load_packed_takes_a_loader_s_own_packing():
    a, b = make_step('cpu', True), make_step('cpu', True)
    ids, y, tt, mask = batch_of(LENGTHS, seed=4)
    a.load_batch(ids, y, tt, mask)
    keep = mask.bool()
    cu = torch.tensor([0, 48, 53, 70, 71, 101], dtype=torch.int32)
    b.load_packed(ids[keep], y, cu, tt[keep])
    for name in ('ids', 'tt', 'y'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ('cu', 'pos_ids', 'slot_w'):
        assert torch.equal(getattr(a.net, name), getattr(b.net, name)), name
    assert a.net.slot_w.tolist() == pytest.approx([0.2] * 5 + [0.0])


def test_token_budget_sampler():
    g = torch.Generator().manual_seed(0)
    lengths = torch.randint(1, MAX_LEN + 1, (203,), generator=g).tolist()
    for shuffle in (False, True):
        s = TokenBudgetBatchSampler(lengths, TOKENS, NSEQ_MAX, shuffle=shuffle, seed=3)
        for epoch in range(2):
            s.set_epoch(epoch)
            batches = list(s)
            assert len(batches) == len(s)
            assert sorted(i for b in batches for i in b) == list(range(203))
            assert all(1 <= len(b) <= NSEQ_MAX and sum(lengths[i] for i in b) <= TOKENS for b in batches)
        if not shuffle:
            assert [i for b in batches for i in b] == list(range(203))
    first = list(TokenBudgetBatchSampler(lengths, TOKENS, NSEQ_MAX, shuffle=True, seed=3))
    s.set_epoch(0)
    assert list(s) == first and first != batches      # seeded, and reshuffled per epoch
    with pytest.raises(ValueError, match='does not fit'):
        TokenBudgetBatchSampler([200], TOKENS, NSEQ_MAX)
    ds = SyntheticTextClassification(num_samples=40, seq_len=MAX_LEN, vocab_size=97, lengths={'min': 3, 'max': 40})
    lens = ds.lengths()
    assert min(lens) >= 3 and max(lens) <= 40 and len(set(lens)) > 5
    assert all(int(ds[i]['attention_mask'].sum()) == lens[i] for i in range(40))
    assert SyntheticTextClassification(num_samples=4, seq_len=8, vocab_size=97).lengths() == [8] * 4


def _stage_cfg(logdir, **args):
    return {'model_params': {'model': 'bert-tiny', 'num_labels': 3},
            'args': dict({'expdir': '.', 'logdir': str(logdir)}, **args),
            'stages': {'data_params': {'dataset': 'synthetic_text_classification', 'seq_len': MAX_LEN,
                                       'num_samples': 40, 'vocab_size': 1000, 'num_classes': 3, 'batch_size': NSEQ_MAX,
                                       'lengths': {'min': 2, 'max': MAX_LEN}},
                       'state_params': {'num_epochs': 2, 'main_metric': 'loss', 'minimize_metric': True},
                       'optimizer_params': {'optimizer': 'AdamW', 'lr': 1e-3},
                       'callbacks_params': {'loss': {'callback': 'CriterionCallback'},
                                            'optimizer': {'callback': 'OptimizerCallback'}},
                       'stage1': {}}}


def test_train_stage_with_pack_tokens_through_the_runner(tmp_path, monkeypatch, caplog):
    """A train stage with args.pack_tokens on variable-length synthetic text, on the engine's
    CPU twin (MLC_NATIVE_CPU=1 lets the runner select it without a GPU)."""
    from mlcomp_amd.train.experiment import ConfigExperiment
    from mlcomp_amd.train.runner import Runner
    monkeypatch.setenv('MLC_NATIVE_CPU', '1')
    torch.manual_seed(0)
    r = Runner(ConfigExperiment(_stage_cfg(tmp_path, engine='native', pack_tokens=TOKENS)), device='cpu')
    with caplog.at_level(logging.INFO, logger='mlcomp_amd.train.runner'):
        state = r.run_experiment()
    assert r.engine_log[0]['engine'] == 'native' and r.engine_log[0]['kind'] == 'bert'
    assert r.engine_log[0]['pack_tokens'] == TOKENS
    assert any('packed mode' in rec.getMessage() for rec in caplog.records)
    assert r.native_step.packed and r.native_step.net.T == TOKENS and r.native_step.batch == NSEQ_MAX
    loss = state.epoch_metrics['train_loss']
    assert loss == loss and 0 < loss < 3
    sampler = r.loaders['train'].batch_sampler
    assert isinstance(sampler, TokenBudgetBatchSampler) and len(sampler) < 40


def test_pack_tokens_needs_the_bert_engine(tmp_path, monkeypatch, caplog):
    from mlcomp_amd.train.experiment import ConfigExperiment
    from mlcomp_amd.train.runner import Runner
    monkeypatch.setenv('MLC_NATIVE_CPU', '1')
    cfg = _stage_cfg(tmp_path, engine='native', pack_tokens=TOKENS)
    cfg['model_params'] = {'model': 'LeNet', 'num_classes': 10}
    r = Runner(ConfigExperiment(cfg), device='cpu')
    r.model = r.experiment.get_model('stage1')
    with pytest.raises(RuntimeError, match='pack_tokens'):
        r._select_engine('stage1')
    r.engine = 'auto'
    with caplog.at_level(logging.WARNING, logger='mlcomp_amd.train.runner'):
        got = r._select_engine('stage1')
    assert got['engine'] == 'native' and got['kind'] == 'generic' and 'pack_tokens' not in got
    assert any('pack_tokens ignored' in rec.getMessage() for rec in caplog.records)
    # a token budget the GEMMs cannot take
    from mlcomp_amd.train.native_spec import NativeUnsupported
    with pytest.raises(NativeUnsupported, match='multiple of 8'):
        NativeBertStep(torch_model=tiny_model(), batch=4, seq_len=16, device='cpu', num_labels=3, pack_tokens=100)
