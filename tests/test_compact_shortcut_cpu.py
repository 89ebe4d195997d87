"""MLC_COMPACT_SHORTCUT_GRAD on / off on the CPU path of the native ops: the two blocks of
tests/test_compact_shortcut_gpu.py (same builder), where nothing is reordered, so every
gradient must be equal; and which shortcut convs the knob applies to."""
import importlib.util
import os

import torch.nn as nn

_spec = importlib.util.spec_from_file_location(
    'compact_shortcut_blocks', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_compact_shortcut_gpu.py'))
blocks = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(blocks)


def test_cpu_compact_shortcut_grad_is_exact():
    blocks.compare(blocks.run_blocks('cpu', True), blocks.run_blocks('cpu', False), exact=True)


def test_compact_dx_applies_to_plain_strided_1x1_shortcuts_only(monkeypatch):
    from mlcomp_amd.ops import layers
    ctx = layers.NativeContext()

    def unit(k, s, p):
        return layers.ConvBN(ctx, f'u{k}{s}{p}', nn.Conv2d(16, 16, k, s, p, bias=False), nn.BatchNorm2d(16), act=False)
    monkeypatch.setattr(layers, 'COMPACT_SHORTCUT_GRAD', True)
    assert unit(1, 2, 0).compact_dx() and unit(1, 3, 0).compact_dx()
    assert not unit(1, 1, 0).compact_dx() and not unit(3, 2, 1).compact_dx() and not unit(1, 2, 1).compact_dx()
    monkeypatch.setattr(layers, 'COMPACT_SHORTCUT_GRAD', False)
    assert not unit(1, 2, 0).compact_dx()
