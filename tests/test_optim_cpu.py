"""The fused arena optimizers (`mlcomp_amd/train/optim.py`) against fp64 ``torch.optim`` over
several steps, per element.

Each case takes five steps with fresh gradients and compares the arena's fp32 masters after
every step with ``torch.optim`` run in fp64 on clones.  The tolerance is derived, not chosen:
4 x the largest elementwise difference between an fp32 ``torch.optim`` run and the fp64 run of
the same steps (the factor covers a different but equally valid fp32 evaluation order and FMA
contraction).  The same tests run on the CPU path of ``Fn.sgd_step`` / ``Fn.adam_step`` and,
under the ``gpu`` mark, on the HIP kernels.
"""
import pytest
import torch

from mlcomp_amd.ops.arena import ParamArena
from mlcomp_amd.train import graphed
from mlcomp_amd.train.optim import FusedAdam, FusedSGD

DEVICES = ['cpu', pytest.param('cuda', marks=pytest.mark.gpu)]
STEPS = 5


def _arena(device, seed=0):
    """A decay arena with a bf16 mirror (two weights, one padded to 4 floats) and a no-decay
    vector arena, masters drawn on the CPU so both devices start from the same bits."""
    pa = ParamArena()
    pa.weight('w1', (5, 7))
    pa.weight('w2', (3, 4))
    pa.vector('b', (6,))
    pa.vector('g', (4,))
    pa.finalize(device)
    gen = torch.Generator().manual_seed(seed)
    for a in pa.arenas():
        a.master.copy_(torch.randn(a.numel, generator=gen))
        a.refresh_mirror()
    return pa


def _grads(pa, step, seed=100):
    gen = torch.Generator().manual_seed(seed + step)
    return [torch.randn(a.numel, generator=gen) for a in pa.arenas()]


def _torch_run(pa, make_opt, dtype, steps=STEPS):
    """``steps`` steps of ``make_opt(params)`` on clones of the masters in ``dtype``; the
    parameters after every step."""
    params = [a.master.detach().cpu().to(dtype).clone().requires_grad_() for a in pa.arenas()]
    opt = make_opt(params)
    out = []
    for s in range(steps):
        for p, g in zip(params, _grads(pa, s)):
            p.grad = g.to(dtype)
        opt.step()
        out.append([p.detach().clone() for p in params])
    return out


def _fused_step(pa, opt, s):
    for a, g in zip(pa.arenas(), _grads(pa, s)):
        a.grad.copy_(g)
    opt.prepare()
    opt.step()


def _check(pa, ref64, ref32, s, what):
    """masters within 4 x the fp32 reference's own error of the fp64 reference, per element; the
    mirror is the master rounded to bf16, bit for bit"""
    for a, r64, r32 in zip(pa.arenas(), ref64[s], ref32[s]):
        tol = 4 * (r32.double() - r64).abs().max().item()
        err = (a.master.detach().cpu().double() - r64).abs().max().item()
        print(f'{what} step {s + 1} {a.name}: max|fused - ref64| = {err:.3e}, tol = {tol:.3e}')
        assert tol < 1e-5, tol
        assert err <= tol, (what, s + 1, a.name, err, tol)
        if a.mirror is not None:
            assert torch.equal(a.mirror.cpu().view(torch.int16), a.master.cpu().to(torch.bfloat16).view(torch.int16))


SGD_CASES = [(mu, nes, damp) for mu in (0.0, 0.9) for nes in (False, True) for damp in (0.0, 0.5)
             if not (nes and (mu == 0.0 or damp != 0.0))]   # torch: nesterov needs momentum and no dampening


@pytest.mark.parametrize('device', DEVICES)
@pytest.mark.parametrize('momentum,nesterov,dampening', SGD_CASES)
def test_fused_sgd_matches_torch_optim(device, momentum, nesterov, dampening):
    """decay_all=True is torch.optim.SGD's semantics.  The first step of a damped run stores
    momentum = d, not (1-dampening)*d; without that the masters were off by 0.125, 0.237, 0.339
    (max abs) after steps 1-3 at dampening 0.5.  Measured max|fused - ref64| on the CPU path:
    at most 3.8e-7 over all cases and steps, a quarter of the derived tolerance of that step
    (2.5e-7 after one step to 1.5e-6 after five)."""
    kw = dict(lr=0.1, momentum=momentum, weight_decay=0.01, nesterov=nesterov, dampening=dampening)
    pa = _arena(device)
    ref64 = _torch_run(pa, lambda ps: torch.optim.SGD(ps, **kw), torch.float64)
    ref32 = _torch_run(pa, lambda ps: torch.optim.SGD(ps, **kw), torch.float32)
    opt = FusedSGD(pa, decay_all=True, **kw)
    for s in range(STEPS):
        _fused_step(pa, opt, s)
        _check(pa, ref64, ref32, s, f'sgd mu={momentum} nesterov={nesterov} damp={dampening}')


@pytest.mark.parametrize('device', DEVICES)
@pytest.mark.parametrize('decoupled', [False, True], ids=['adam', 'adamw'])
def test_fused_adam_matches_torch_optim(device, decoupled):
    kw = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.1)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    pa = _arena(device)
    ref64 = _torch_run(pa, lambda ps: cls(ps, **kw), torch.float64)
    ref32 = _torch_run(pa, lambda ps: cls(ps, **kw), torch.float32)
    opt = FusedAdam(pa, decoupled=decoupled, decay_all=True, **kw)
    for s in range(STEPS):
        _fused_step(pa, opt, s)
        _check(pa, ref64, ref32, s, 'adamw' if decoupled else 'adam')


def _sgd_formula(pa, dtype, lr, mu, damp, wd, steps=STEPS):
    """torch.optim.SGD's update written out, with weight decay on the decay arena only"""
    ps = [a.master.detach().cpu().to(dtype).clone() for a in pa.arenas()]
    ms = [None, None]
    out = []
    for s in range(steps):
        for k, (g, w) in enumerate(zip(_grads(pa, s), (wd, 0.0))):
            d = g.to(dtype) + w * ps[k]
            ms[k] = d.clone() if ms[k] is None else mu * ms[k] + (1 - damp) * d
            ps[k] = ps[k] - lr * ms[k]
        out.append([p.clone() for p in ps])
    return out


@pytest.mark.parametrize('device', DEVICES)
def test_fused_sgd_decay_arena_only(device):
    """decay_all=False (the hand-lowered engines): the no-decay arena gets wd = 0."""
    lr, mu, damp, wd = 0.1, 0.9, 0.5, 0.1
    pa = _arena(device)
    ref64 = _sgd_formula(pa, torch.float64, lr, mu, damp, wd)
    ref32 = _sgd_formula(pa, torch.float32, lr, mu, damp, wd)
    # decay on the no-decay arena would be visible: lr*wd*|p| against the tolerance
    assert lr * wd * pa.nodecay.master.abs().max().item() > 1e-3
    opt = FusedSGD(pa, lr=lr, momentum=mu, weight_decay=wd, dampening=damp)
    for s in range(STEPS):
        _fused_step(pa, opt, s)
        _check(pa, ref64, ref32, s, 'sgd decay arena only')


@pytest.mark.parametrize('device', DEVICES)
def test_fused_sgd_dampening_resumes_from_state_dict(device):
    """A run resumed with steps > 0 continues the loaded momentum instead of seeding it again."""
    kw = dict(lr=0.1, momentum=0.9, weight_decay=0.01, dampening=0.5)
    pa = _arena(device)
    ref64 = _torch_run(pa, lambda ps: torch.optim.SGD(ps, **kw), torch.float64)
    ref32 = _torch_run(pa, lambda ps: torch.optim.SGD(ps, **kw), torch.float32)
    opt = FusedSGD(pa, decay_all=True, **kw)
    for s in range(2):
        _fused_step(pa, opt, s)
    saved = opt.state_dict()
    pb = _arena(device, seed=7)
    for a, b in zip(pa.arenas(), pb.arenas()):
        b.master.copy_(a.master)
    opt2 = FusedSGD(pb, decay_all=True, **kw)
    opt2.load_state_dict(saved)
    for s in range(2, STEPS):
        _fused_step(pb, opt2, s)
        assert not opt2.seeds_momentum
        _check(pb, ref64, ref32, s, 'sgd resumed')


class _Graph:
    def __init__(self, body):
        self.body = body

    def replay(self):
        self.body()


class _Step(graphed.GraphedStep):
    """GraphedStep over a FusedSGD with the capture replaced by a recorder (CPU)."""

    def __init__(self, pa, opt, warmup_eager):
        self.device = torch.device('cpu')
        self.pa, self.opt = pa, opt
        self.use_graph, self.warmup_eager = True, warmup_eager
        self.captured_at = None
        self.seeded_in_capture = None

    def _body(self):
        for a, g in zip(self.pa.arenas(), _grads(self.pa, self.calls - 1)):
            a.grad.copy_(g)
        self.opt.step()

    def _capture(self):
        self.captured_at = self.calls
        self.seeded_in_capture = self.opt.seeds_momentum
        return _Graph(self._body)


class _NoStream:
    """stand-in for the side stream of the eager warm-up steps (there is no HIP stream on the CPU)"""

    def __init__(self, *a, **k):
        pass

    def wait_stream(self, other):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@pytest.mark.parametrize('warmup_eager', [0, 2])
def test_damped_first_step_is_never_captured(warmup_eager, monkeypatch):
    """The step that seeds momentum has its own kernel argument, so it runs eagerly even with
    warmup_eager == 0, and what is captured afterwards is the steady-state step."""
    monkeypatch.setattr(torch.cuda, 'Stream', _NoStream)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **k: _NoStream())
    monkeypatch.setattr(torch.cuda, 'stream', lambda s: s)
    kw = dict(lr=0.1, momentum=0.9, weight_decay=0.01, dampening=0.5)
    pa = _arena('cpu')
    ref64 = _torch_run(pa, lambda ps: torch.optim.SGD(ps, **kw), torch.float64)
    ref32 = _torch_run(pa, lambda ps: torch.optim.SGD(ps, **kw), torch.float32)
    step = _Step(pa, FusedSGD(pa, decay_all=True, **kw), warmup_eager)
    for s in range(STEPS):
        step()
        _check(pa, ref64, ref32, s, f'graphed warmup={warmup_eager}')
    assert step.captured_at == max(warmup_eager + 1, 2) and step.seeded_in_capture is False
    undamped = _Step(pa, FusedSGD(pa, decay_all=True, lr=0.1, momentum=0.9), 0)
    undamped()
    assert undamped.captured_at == 1    # dampening == 0: nothing changes
