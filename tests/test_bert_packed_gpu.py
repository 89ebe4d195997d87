"""Packed mode of the native BERT engine on the GPU: one packed step of the kernels against
its own CPU twin (the bound the BERT row of ``tests/test_engines_gpu_vs_cpu.py`` uses), and
one captured graph replayed over batches with different numbers and mixes of lengths against
an eager twin."""
import pytest
import torch

from mlcomp_amd.train.graphed import GraphedStep

from test_bert_packed_cpu import LENGTHS, assert_within_noise, batch_of, grads, make_step, perturb

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def test_packed_gpu_step_matches_its_cpu_twin():
    batch = batch_of(LENGTHS)
    cpu, noisy, gpu = make_step('cpu', True), make_step('cpu', True), make_step(DEV, True)
    perturb(noisy)
    for st in (cpu, noisy, gpu):
        st.load_batch(*batch)
    ref, noise, got = grads(cpu), grads(noisy), grads(gpu)
    rg, rn = assert_within_noise(ref, noise, got, 'packed gpu vs cpu')
    assert rg['pos'] <= 3 * rn['pos'] + 5e-2
    assert got[1]['pos'].view(64, 128)[48:].abs().max().item() == 0
    assert abs(gpu.accuracy() - cpu.accuracy()) < 1e-6


def test_one_graph_serves_every_length_mix(monkeypatch):
    """use_graph with one eager warm-up step, then 4 steps whose batches hold 5, 3, 6 and 1
    sequences of different lengths: the losses equal an eager twin's and one graph was
    captured.  The loss bound is the fixed part of the engines' GPU-vs-CPU loss bound (1e-2
    relative); both runs are the same kernels, so they land far inside it."""
    captures = []
    real = GraphedStep._capture
    monkeypatch.setattr(GraphedStep, '_capture', lambda self: captures.append(1) or real(self))
    model = None
    graphed = make_step(DEV, True, model, use_graph=True, warmup_eager=1, lr=1e-3)
    eager = make_step(DEV, True, model, use_graph=False, lr=1e-3)
    mixes = [[48, 5, 17, 1, 30], [40, 40, 40], [9, 2, 31, 48, 16, 25], [23]]
    losses = {0: [], 1: []}
    for i, lengths in enumerate(mixes):
        batch = batch_of(lengths, seed=10 + i)
        for k, st in enumerate((graphed, eager)):
            st.load_batch(*batch)
            st()
            torch.cuda.synchronize()
            assert st.nseq == len(lengths)
            losses[k].append(st.last_loss())
    print('graph', losses[0], 'eager', losses[1])
    assert graphed.graph is not None, graphed.capture_error
    assert len(captures) == 1
    for a, b in zip(*losses.values()):
        assert a == a and abs(a - b) / abs(b) <= 1e-2, (losses[0], losses[1])
