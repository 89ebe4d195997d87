"""MLC_COMPACT_SHORTCUT_GRAD on / off through a whole ``ResidualBlock`` backward: a bottleneck
32 -> (16, 16, 64) with a 1x1 / stride-2 shortcut at 2 x 9 x 9, behind an identity
bottleneck, so the first unit's dgrad also runs the previous block's fused BN-backward
reduction (``prev_spec``: masked by that block's output) in its epilogue.

Knob on: the shortcut's input gradient is one stride-1 GEMM on the 2 x 5 x 5 grid and
reaches the first unit's dgrad as the compact strided addend.  Knob off: four parity-class
GEMMs write the 2 x 9 x 9 tensor that dgrad reads back.  The same bf16 values are added at
the same pixels, so the input gradient must be equal.  The BN dgamma / dbeta and the weight
gradients come from the same operands and may differ by the order of their fp32 atomics
only: they are held to MARGIN_F32 = 1e-4 (max |delta| over the reference's RMS), the bound
tests/test_conv1x1_bwd_fused_gpu.py derives for its own knob-on / knob-off comparison (a
worst-case linear fp32 accumulation over n <= 1024 rows, n * 2^-24 < 1e-4; here n = 162).
In deterministic mode (a child process: the mode is process-wide) everything is equal."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN_F32 = 1e-4
ORDERINGS = ['down_side', 'pend', 'inline']


def _unit(ctx, name, ci, co, k, s, act, g):
    from mlcomp_amd.ops.layers import ConvBN
    conv = nn.Conv2d(ci, co, k, s, k // 2, bias=False)
    bn = nn.BatchNorm2d(co)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
        bn.weight.copy_(0.5 + torch.rand(co, generator=g))
        bn.bias.copy_(torch.randn(co, generator=g) * 0.2)
    return ConvBN(ctx, name, conv, bn, act=act)


def run_blocks(device, compact, ordering='down_side'):
    """Forward + backward of the two blocks; {name: CPU tensor} of every gradient."""
    from mlcomp_amd.ops import layers
    from mlcomp_amd.ops.layers import NativeContext, ResidualBlock
    g = torch.Generator().manual_seed(7)
    ctx = NativeContext()
    b0 = ResidualBlock([_unit(ctx, 'b0.cb1', 32, 8, 1, 1, True, g), _unit(ctx, 'b0.cb2', 8, 8, 3, 1, True, g),
                        _unit(ctx, 'b0.cb3', 8, 32, 1, 1, True, g)], None)
    b1 = ResidualBlock([_unit(ctx, 'b1.cb1', 32, 16, 1, 1, True, g), _unit(ctx, 'b1.cb2', 16, 16, 3, 2, True, g),
                        _unit(ctx, 'b1.cb3', 16, 64, 1, 1, True, g)],
                       _unit(ctx, 'b1.down', 32, 64, 1, 2, False, g))
    b1.prev = b0
    ctx.finalize(device)
    units = b0.units + b1.units + [b1.down]
    for u in units:
        u.load_from_torch()
    ctx.arena.decay.refresh_mirror()
    x = torch.randn(2, 9, 9, 32, generator=g).to(torch.bfloat16).to(device).requires_grad_()
    dout = torch.randn(2, 5, 5, 64, generator=g).to(torch.bfloat16).to(device)
    old = layers.COMPACT_SHORTCUT_GRAD, os.environ.get('MLC_WGRAD_STREAM')
    layers.COMPACT_SHORTCUT_GRAD = compact
    try:
        if ordering == 'pend':
            os.environ['MLC_WGRAD_STREAM'] = '2'    # read by backward: one join per block
        for b in (b0, b1):
            b.down_stream = ordering == 'down_side'
        assert b1.down.compact_dx() == compact
        ctx.ws.zero()
        out = b1(b0(x))
        ctx.refresh_wt()
        out.backward(dout)
        ctx.flush_wgrad()
        if torch.device(device).type == 'cuda':
            torch.cuda.synchronize()
    finally:
        layers.COMPACT_SHORTCUT_GRAD = old[0]
        if old[1] is None:
            os.environ.pop('MLC_WGRAD_STREAM', None)
        else:
            os.environ['MLC_WGRAD_STREAM'] = old[1]
    res = {'dx': x.grad.detach().float().cpu()}
    for u in units:
        res[f'{u.name}.dw'] = u.w.grad.detach().float().cpu().clone()
        res[f'{u.name}.dgamma'] = u.gamma.grad.detach().float().cpu().clone()
        res[f'{u.name}.dbeta'] = u.beta.grad.detach().float().cpu().clone()
    return res


def compare(on, off, exact):
    assert set(on) == set(off)
    assert torch.equal(on['dx'], off['dx'])
    assert on['dx'].abs().sum().item() > 0
    for k in sorted(on):
        if exact:
            assert torch.equal(on[k], off[k]), k
            continue
        rms = off[k].pow(2).mean().sqrt().item()
        err = (on[k] - off[k]).abs().max().item() / max(rms, 1e-30)
        print(f'{k}: max |delta| / rms = {err:.3e}')
        assert rms > 0 and err <= MARGIN_F32, (k, err)


@pytest.mark.gpu
@pytest.mark.parametrize('ordering', ORDERINGS)
def test_compact_shortcut_grad_matches_full_resolution_path(ordering):
    compare(run_blocks('cuda', True, ordering), run_blocks('cuda', False, ordering), exact=False)


@pytest.mark.gpu
def test_compact_shortcut_grad_deterministic_mode_is_exact(tmp_path):
    path = str(tmp_path / 'grads.pt')
    env = dict(os.environ, MLC_DETERMINISTIC='1', PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    on, off = torch.load(path)
    compare(on, off, exact=True)


if __name__ == '__main__':
    from mlcomp_amd.ops import _lib
    assert _lib.DETERMINISTIC
    torch.save((run_blocks('cuda', True), run_blocks('cuda', False)), sys.argv[1])
