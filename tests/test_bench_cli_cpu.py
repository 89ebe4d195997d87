"""``bench.py`` options that need no GPU: ``--full`` / ``--dump-outputs`` parse, and the
output dump writes float32 / float64 ``.npy`` arrays, samples long ones at fixed (seeded)
positions and gives the same files for the same step."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_options_parse(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '3'])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 3 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'somewhere'])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == 'somewhere'


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_native_arenas(tmp_path, monkeypatch):
    from mlcomp_amd.ops.arena import ParamArena
    monkeypatch.setattr(bench, 'DUMP_MAX_ELEMS', 1000)
    arena = ParamArena()
    w = arena.weight('w', (70, 64))       # 4480 elements: sampled
    b = arena.vector('b', (70,))          # padded to 128: written whole
    arena.finalize('cpu')
    g = torch.Generator().manual_seed(0)
    w.master.copy_(torch.randn(70, 64, generator=g))
    b.master.fill_(2.0)
    step = types.SimpleNamespace(net=types.SimpleNamespace(arena=arena), bn_buffers=torch.arange(6.0))
    bench._dump_outputs(step, 1.25, str(tmp_path / 'a'))
    bench._dump_outputs(step, 1.25, str(tmp_path / 'b'))
    a, again = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    assert sorted(a) == ['bn_buffers', 'loss', 'params_decay', 'params_nodecay']
    assert a['loss'].dtype == np.float64 and a['loss'].tolist() == [1.25]
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64), k
        assert np.array_equal(v, again[k]), k
    idx = np.sort(np.random.default_rng(0).choice(arena.decay.numel, 1000, replace=False))
    assert np.array_equal(a['params_decay'], arena.decay.master.numpy()[idx])
    assert np.array_equal(a['params_nodecay'], arena.nodecay.master.numpy())
    assert np.array_equal(a['bn_buffers'], np.arange(6, dtype=np.float32))


def test_dump_torch_model(tmp_path):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3))
    model(torch.randn(5, 4))                     # one training-mode forward moves the running statistics
    step = types.SimpleNamespace(model=model)
    bench._dump_outputs(step, None, str(tmp_path))
    a = _load(tmp_path)
    assert np.isnan(a['loss']).all()
    assert sorted(a) == ['bn_buffers', 'loss', 'params'] and a['params'].shape == (4 * 3 + 3 + 3 + 3,)
    assert np.array_equal(a['params'][:12], model[0].weight.detach().numpy().reshape(-1))
    assert a['bn_buffers'].shape == (6,)         # running mean and variance
