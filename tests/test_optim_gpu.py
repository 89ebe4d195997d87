"""`csrc/kernels/optim.hip` per element: mlc_sgd, mlc_adam, mlc_sqnorm, mlc_zero4.

The reference of every update is written out here in fp64 torch ops from the bit-identical
fp32 inputs (not the CPU branch of ``Fn.sgd_step`` / ``Fn.adam_step``, which is checked against
the same reference).  p, m and v are compared element by element: ``|gpu - ref64| <= tol`` with
``tol = 4 x max|fp32 twin - ref64|`` on the same inputs, the twin being the CPU branch (the same
formula in fp32 on the device for the two grid-wrap cases).  The factor 4 covers FMA contraction
and the device's sqrtf / division rounding.

|p| is drawn from [0.5, 2] and |g| from [0.5, 2] with random signs, lr = wd = 0.1 and
grad scale 0.5, so that decaying or not decaying ONE element, the grad scale, and ``first`` each
move an element by more than 1000 x tol (asserted): a decay or mirror boundary that is off by
one float4 cannot hide in a norm.  Every array is longer than n and sentinel-filled past n; the
bf16 mirror past ``nbf`` and a guard past every output must keep the sentinel bit for bit.  Rows
with tiny n run many independent problems (one launch each) so that the derived tolerance is a
maximum over some hundreds of elements, not over four.

Measured on an MI355X (max over all rows of a mode, |gpu - ref64| against the twin's own
maximum; the tolerance is 4 x the latter): the kernels need about 1.1 x, never 4 x.  The
figures are in the tests' docstrings and in profiles/optim_pool_tests/README.md.
"""
import pytest
import torch

from mlcomp_amd.ops import _lib
from mlcomp_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu

DEV = 'cuda'
PAD = 8                    # sentinel floats past n (two float4: the guard the issue asks for and one more)
SENT = -7.5                # fp32 sentinel
SENT16 = 0x4243            # bf16 sentinel bits (non-zero)
EPS32 = 2.0 ** -23


def f32(x):
    """x rounded to fp32, as a Python float: what a kernel's ``float`` argument holds"""
    return torch.tensor(x, dtype=torch.float32).item()


LR, GS, WD = f32(0.1), 0.5, f32(0.1)
MU, DAMP = f32(0.9), 0.25
B1, B2, EPS = f32(0.9), f32(0.99), f32(1e-8)
BC1, BC2 = f32(0.9), f32(0.99)          # hyper[2], hyper[3] as the existing tests pass them

# (n, ndecay, nbf): every boundary on and off an 8-float chunk and at both ends, ndecay != nbf.
# sgd_kernel / adam_kernel work in float4 (i < ndecay4, i < nbf4); adam8_kernel in pairs of
# float4 (2c+h < ndecay4; mirror: 16-byte store when 2c+1 < nbf4, 8-byte when only 2c < nbf4);
# n % 8 == 4 adds mlc_adam's tail launch on offset pointers (ndr / nbr).
ROWS = [
    (4, 0, 4),           # one float4, one block, lanes clamped to n4-1; n < 8: adam_kernel in every variant
    (4, 4, 0),           # nbf == 0 with a mirror pointer: nothing may be written
    (8, 4, 8),           # n == 8: one adam8 chunk, decay ends inside it (h = 0 only)
    (8, 8, 4),           # mirror ends inside the chunk: the 8-byte store_bf16x4 branch
    (8, 0, 4),           # no decay at all
    (12, 4, 8),          # adam8 chunk + tail launch with ndr = nbr = 0 (pbf passed as null)
    (12, 8, 12),         # tail launch with nbr = 4 (mirror on offset pointer), ndr = 0
    (12, 12, 4),         # tail launch with ndr = 4, nbr = 0
    (12, 12, 8),         # tail decays, mirror ends exactly at the tail's start
    (8196, 0, 8196),     # ndecay = 0, mirror everywhere, tail launch mirrors
    (8196, 8196, 0),     # decay everywhere, no mirror element
    (8196, 4, 8192),     # decay on the first float4 only; mirror ends at the tail's start
    (8196, 8192, 4),     # mirror on the first float4 only; decay ends at the tail's start
    (8196, 4100, 4104),  # decay % 8 == 4 (inside a chunk), mirror % 8 == 0
    (8196, 4104, 4100),  # the reverse: mirror ends inside a chunk
    (8196, 8192, 8196),  # n-4 / n
    (8196, 8196, 8192),  # n / n-4
    (8200, 4100, 8196),  # n % 8 == 0: no tail; mirror ends inside the last chunk
    (8200, 8196, 4100),  # decay ends inside the last chunk
    (8200, 4104, 8200),
    (8200, 8200, 4104),
]
WRAP_SGD_N = 8192 * 256 * 2 * 4 + 4100      # just past blocks_for's 8192 blocks x 2 float4 x 256 lanes
WRAP_ADAM8_N = 16384 * 256 * 8 + 12         # just past adam8's 16384 blocks, n % 8 == 4 (tail launch)


def _reps(n):
    return max(1, 512 // n)


def _signed(shape, gen, device='cpu'):
    """magnitudes in [0.5, 2] with random signs"""
    mag = 0.5 + 1.5 * torch.rand(shape, generator=gen, device=device)
    return mag * (torch.randint(0, 2, shape, generator=gen, device=device).float() * 2 - 1)


def _inputs(n, seed, device='cpu', reps=None):
    shape = (_reps(n) if reps is None else reps, n)
    gen = torch.Generator(device=device).manual_seed(seed)
    p, g = _signed(shape, gen, device), _signed(shape, gen, device)
    m = torch.randn(shape, generator=gen, device=device) * 0.5
    v = torch.rand(shape, generator=gen, device=device) * 0.5 + 0.05
    return p, g, m, v


# ------------------------------------------------------------------ the references, written out
def sgd_ref(p, g, m, lr, gs, nd, mu, damp, wd, nesterov, first):
    d = g * gs
    d[..., :nd] += wd * p[..., :nd]
    if mu:
        m = d.clone() if first else mu * m + (1 - damp) * d
        d = d + mu * m if nesterov else m
    return p - lr * d, m


def adam_ref(p, g, m, v, lr, gs, bc1, bc2, nd, b1, b2, eps, wd, decoupled):
    d = g * gs
    if not decoupled:
        d[..., :nd] += wd * p[..., :nd]
    m = b1 * m + (1 - b1) * d
    v = b2 * v + (1 - b2) * d * d
    p = p.clone()
    if decoupled:
        p[..., :nd] -= lr * wd * p[..., :nd]
    return p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps), m, v


# ------------------------------------------------------------------ device arrays with guards
def _guarded(x):
    """[reps, n] fp32 -> device [reps, n + PAD] with the sentinel past n"""
    out = torch.full((x.shape[0], x.shape[1] + PAD), SENT, dtype=torch.float32, device=DEV)
    out[:, :x.shape[1]] = x.to(DEV)
    return out


def _mirror(reps, n):
    return torch.full((reps, n + PAD), SENT16, dtype=torch.int16, device=DEV)


def _launch_sgd(P, G, M, BF, hyper, n, nd, nb, mu, damp, wd, nesterov, first):
    for r in range(P.shape[0]):
        _lib.call('mlc_sgd', _lib.ptr(P[r]), _lib.ptr(G[r]), _lib.ptr(M[r]) if M is not None else None,
                  _lib.ptr(BF[r]) if BF is not None else None, _lib.ptr(hyper), n, nd, nb, mu, damp, wd,
                  int(nesterov), int(first), _lib.stream())


def _launch_adam(P, G, M, V, BF, hyper, n, nd, nb, wd, decoupled):
    for r in range(P.shape[0]):
        _lib.call('mlc_adam', _lib.ptr(P[r]), _lib.ptr(G[r]), _lib.ptr(M[r]), _lib.ptr(V[r]),
                  _lib.ptr(BF[r]) if BF is not None else None, _lib.ptr(hyper), n, nd, nb, B1, B2, EPS, wd,
                  int(decoupled), _lib.stream())


def _close(name, got, ref64, twin, row, worst):
    """got within 4 x the fp32 twin's own error of ref64, per element; returns that tolerance"""
    twin_err = (twin.double() - ref64).abs().max().item()
    # the twin itself is a handful of fp32 operations on values of the reference's size
    assert twin_err <= 16 * EPS32 * max(1.0, ref64.abs().max().item()), (name, row, twin_err)
    tol = 4 * twin_err
    err = (got.double() - ref64).abs().max().item()
    rel = ((got.double() - ref64).abs() / ref64.abs().clamp_min(1e-30)).max().item()
    w = worst.setdefault(name, [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], err), max(w[1], rel), max(w[2], twin_err)
    assert err <= tol, (name, row, err, tol)
    return tol


def _check_mirror_and_guards(row, P, BF, nb, n, others=()):
    if BF is not None:
        want = P[:, :nb].to(torch.bfloat16).view(torch.int16)
        assert torch.equal(BF[:, :nb], want), ('mirror', row)
        assert bool((BF[:, nb:] == SENT16).all()), ('mirror written past nbf', row)
    for name, t in (('p', P),) + tuple(others):
        if t is not None:
            assert bool((t[:, n:] == SENT).all()), (name, 'written past n', row)


SGD_MODES = [(mu, nes, damp, first, mirror)
             for mu in (0.0, MU) for nes in (False, True) for damp in (0.0, DAMP)
             for first in (False, True) for mirror in (False, True)
             if not (nes and (mu == 0.0 or damp != 0.0))]      # torch rejects these


@pytest.mark.parametrize('mu,nesterov,damp,first,mirror', SGD_MODES)
def test_sgd_per_element(mu, nesterov, damp, first, mirror):
    """Every mode of sgd_kernel over the boundary table.  Measured on an MI355X, worst mode:
    p 1.34e-7 abs (1.0e-7 relative) against the CPU twin's 1.42e-7; m 2.13e-7 against 2.13e-7;
    no mode's GPU maximum exceeded its twin's."""
    hyper_c = torch.tensor([LR, GS, 123.0, -5.0])        # slots 2 and 3 are not SGD's
    hyper = hyper_c.to(DEV)
    worst = {}
    for row in ROWS:
        n, nd, nb = row
        p, g, m, _ = _inputs(n, seed=n * 31 + nd)
        if not mu:
            m = None
        rp, rm = sgd_ref(p.double(), g.double(), m.double() if mu else None, LR, GS, nd, mu, damp, WD, nesterov, first)
        tp, tm = p.clone(), (m.clone() if mu else None)
        for r in range(p.shape[0]):                          # the CPU twin, row by row like the launches
            Fn.sgd_step(tp[r], g[r], tm[r] if mu else None, None, hyper_c, nd, 0, mu, damp, WD, nesterov, first)
        P, G, M = _guarded(p), _guarded(g), (_guarded(m) if mu else None)
        BF = _mirror(p.shape[0], n) if mirror else None
        _launch_sgd(P, G, M, BF, hyper, n, nd, nb, mu, damp, WD, nesterov, first)
        torch.cuda.synchronize()
        tol = _close('p', P[:, :n].cpu(), rp, tp, row, worst)
        if mu:
            _close('m', M[:, :n].cpu(), rm, tm, row, worst)
        _check_mirror_and_guards(row, P, BF, nb, n, (('m', M),))
        assert bool((G == _guarded(g)).all())                # the gradient is read-only
        # what a slip would move, against the tolerance: decay on/off, the grad scale, first
        alt = lambda **k: sgd_ref(p.double(), g.double(), m.double() if mu else None,   # noqa: E731
                                  **{**dict(lr=LR, gs=GS, nd=nd, mu=mu, damp=damp, wd=WD, nesterov=nesterov,
                                            first=first), **k})[0]
        assert (alt(nd=n) - alt(nd=0)).abs().min().item() >= 1000 * tol, row
        assert (alt(gs=1.0) - rp).abs().min().item() >= 1000 * tol, row
        if mu:
            assert (alt(first=not first) - rp).abs().median().item() >= 1000 * tol, row
    print('GPU_MAXIMA_SGD', (mu, nesterov, damp, first, mirror),
          {k: ['%.3e' % x for x in w] for k, w in worst.items()}, '(abs, rel, twin abs)')


@pytest.mark.parametrize('decoupled', [True, False], ids=['adamw', 'adam'])
@pytest.mark.parametrize('variant', [0, 1, 2])
def test_adam_per_element(variant, decoupled):
    """adam_kernel (0), adam8_kernel (1) and its nontemporal form (2) over the boundary table,
    decoupled and coupled decay, always with a mirror.  Measured on an MI355X, worst case:
    p 2.15e-7 abs against the CPU twin's 1.96e-7 (1.10 x, of the 4 x allowed; relative 1.3e-5
    at an element the step moved next to zero); m 1.14e-7 against 1.19e-7; v 5.8e-8 against 5.9e-8."""
    lib = _lib.load()
    old = lib.mlc_opt_config(0, variant)
    try:
        hyper_c = torch.tensor([LR, GS, BC1, BC2])
        hyper = hyper_c.to(DEV)
        worst = {}
        for row in ROWS:
            n, nd, nb = row
            p, g, m, v = _inputs(n, seed=n * 17 + nb)
            ref = lambda **k: adam_ref(p.double(), g.double(), m.double(), v.double(),   # noqa: E731
                                       **{**dict(lr=LR, gs=GS, bc1=BC1, bc2=BC2, nd=nd, b1=B1, b2=B2, eps=EPS,
                                                 wd=WD, decoupled=decoupled), **k})
            rp, rm, rv = ref()
            tp, tm, tv = p.clone(), m.clone(), v.clone()
            for r in range(p.shape[0]):
                Fn.adam_step(tp[r], g[r], tm[r], tv[r], None, hyper_c, nd, 0, B1, B2, EPS, WD, decoupled)
            P, G, M, V = _guarded(p), _guarded(g), _guarded(m), _guarded(v)
            BF = _mirror(p.shape[0], n)
            _launch_adam(P, G, M, V, BF, hyper, n, nd, nb, WD, decoupled)
            torch.cuda.synchronize()
            tol = _close('p', P[:, :n].cpu(), rp, tp, row, worst)
            tol_m = _close('m', M[:, :n].cpu(), rm, tm, row, worst)
            _close('v', V[:, :n].cpu(), rv, tv, row, worst)
            _check_mirror_and_guards(row, P, BF, nb, n, (('m', M), ('v', V)))
            assert bool((G == _guarded(g)).all())
            # decoupled decay moves p by lr*wd*|p|; coupled decay enters through d, where Adam's
            # normalisation can cancel it in p for single elements but m moves by (1-b1)*wd*|p|
            k, t = (0, tol) if decoupled else (1, tol_m)
            assert (ref(nd=n)[k] - ref(nd=0)[k]).abs().min().item() >= 1000 * t, row
            assert (ref(gs=1.0)[0] - rp).abs().median().item() >= 1000 * tol, row
        print('GPU_MAXIMA_ADAM', (variant, decoupled), {k: ['%.3e' % x for x in w] for k, w in worst.items()},
              '(abs, rel, twin abs)')
    finally:
        lib.mlc_opt_config(0, old)


def _wrap_check(name, got, ref64, twin):
    twin_err = (twin.double() - ref64).abs().max().item()
    err = (got.double() - ref64).abs().max().item()
    print(f'GPU_MAXIMA_WRAP {name}: max|gpu - ref64| = {err:.3e}, twin = {twin_err:.3e}, tol = {4 * twin_err:.3e}')
    assert err <= 4 * twin_err, (name, err, 4 * twin_err)


def test_sgd_grid_wrap():
    """n just past the 8192-block cap: the grid-stride loop runs a second pass in which most
    lanes' second float4 is clamped to n4-1 and skipped.  Reference and fp32 twin are torch ops
    on the device; the whole tensor is compared.  Measured on an MI355X: p 1.36e-7 (twin
    1.39e-7), m 2.40e-7 (twin 2.40e-7); 0.15 s."""
    n = WRAP_SGD_N
    nd, nb = n // 2 // 8 * 8 + 4, n - 4100 + 8            # mirror ends inside the second pass
    p, g, m, _ = _inputs(n, seed=5, device=DEV, reps=1)
    hyper = torch.tensor([LR, GS, 0.0, 0.0], device=DEV)
    rp, rm = sgd_ref(p.double(), g.double(), m.double(), LR, GS, nd, MU, DAMP, WD, False, False)
    tp, tm = sgd_ref(p.clone(), g, m, LR, GS, nd, MU, DAMP, WD, False, False)
    P, G, M, BF = _guarded(p), _guarded(g), _guarded(m), _mirror(1, n)
    del p, m
    _launch_sgd(P, G, M, BF, hyper, n, nd, nb, MU, DAMP, WD, False, False)
    torch.cuda.synchronize()
    _wrap_check('sgd p', P[:, :n], rp, tp)
    _wrap_check('sgd m', M[:, :n], rm, tm)
    _check_mirror_and_guards((n, nd, nb), P, BF, nb, n, (('m', M),))


@pytest.mark.parametrize('variant,n', [(0, WRAP_SGD_N), (1, WRAP_ADAM8_N)], ids=['adam_kernel', 'adam8'])
def test_adam_grid_wrap(variant, n):
    """adam_kernel past blocks_for's cap, and adam8_kernel past its 16384 blocks with n % 8 == 4
    (so the tail launch on offset pointers runs, mirrored and decayed).  Measured on an MI355X:
    adam_kernel p 2.90e-7 (twin 3.22e-7), m 2.13e-7 (2.13e-7), v 5.99e-8 (6.01e-8), 0.13 s; adam8
    p 3.05e-7 (3.53e-7), m 1.22e-7 (2.24e-7), v 3.07e-8 (6.02e-8)."""
    lib = _lib.load()
    old = lib.mlc_opt_config(0, variant)
    try:
        nd, nb = n, n - 8 if variant == 0 else n        # adam8: the tail float4 decays and is mirrored
        p, g, m, v = _inputs(n, seed=6, device=DEV, reps=1)
        hyper = torch.tensor([LR, GS, BC1, BC2], device=DEV)
        args = (LR, GS, BC1, BC2, nd, B1, B2, EPS, WD, True)
        rp, rm, rv = adam_ref(p.double(), g.double(), m.double(), v.double(), *args)
        tp, tm, tv = adam_ref(p, g.clone(), m, v, *args)
        P, G, M, V, BF = _guarded(p), _guarded(g), _guarded(m), _guarded(v), _mirror(1, n)
        del p, m, v
        _launch_adam(P, G, M, V, BF, hyper, n, nd, nb, WD, True)
        torch.cuda.synchronize()
        _wrap_check('adam p', P[:, :n], rp, tp)
        _wrap_check('adam m', M[:, :n], rm, tm)
        _wrap_check('adam v', V[:, :n], rv, tv)
        _check_mirror_and_guards((n, nd, nb), P, BF, nb, n, (('m', M), ('v', V)))
    finally:
        lib.mlc_opt_config(0, old)


@pytest.mark.parametrize('n,nd,nb', [(6, 4, 4), (8, 6, 4), (8, 4, 6), (10, 0, 0)])
def test_launchers_refuse_sizes_not_multiple_of_4(n, nd, nb):
    """n, ndecay or nbf % 4 != 0: -1 and nothing is written."""
    lib = _lib.load()
    hyper = torch.tensor([LR, GS, BC1, BC2], device=DEV)
    arrs = [torch.full((16,), SENT, device=DEV) for _ in range(4)]
    bf = torch.full((16,), SENT16, dtype=torch.int16, device=DEV)
    p, g, m, v = [_lib.ptr(a) for a in arrs]
    assert lib.mlc_sgd(p, g, m, _lib.ptr(bf), _lib.ptr(hyper), n, nd, nb, MU, 0.0, WD, 0, 0, _lib.stream()) == -1
    assert lib.mlc_adam(p, g, m, v, _lib.ptr(bf), _lib.ptr(hyper), n, nd, nb, B1, B2, EPS, WD, 1, _lib.stream()) == -1
    torch.cuda.synchronize()
    assert all(bool((a == SENT).all()) for a in arrs) and bool((bf == SENT16).all())


def test_hyper_is_read_on_the_device_at_launch():
    """lr changes with fill_ on the same device tensor between two launches (what set_lr does,
    and what a replayed graph relies on): the second launch uses the new value."""
    n = 4096
    p, g, _, _ = _inputs(n, seed=9, reps=1)
    hyper = torch.tensor([LR, GS, 0.0, 0.0], device=DEV)
    P, G = _guarded(p), _guarded(g)
    _launch_sgd(P, G, None, None, hyper, n, 0, 0, 0.0, 0.0, 0.0, False, False)
    lr2 = f32(0.7)
    hyper[0].fill_(lr2)
    _launch_sgd(P, G, None, None, hyper, n, 0, 0, 0.0, 0.0, 0.0, False, False)
    torch.cuda.synchronize()
    ref = p.double() - LR * (g.double() * GS) - lr2 * (g.double() * GS)
    stale = p.double() - 2 * LR * (g.double() * GS)
    twin = (p - LR * (g * GS)) - lr2 * (g * GS)
    tol = 4 * (twin.double() - ref).abs().max().item()
    assert (P[:, :n].cpu().double() - ref).abs().max().item() <= tol
    assert (stale - ref).abs().min().item() >= 1000 * tol


# ------------------------------------------------------------------ mlc_sqnorm
@pytest.mark.parametrize('scale', [1.0, 0.5])
@pytest.mark.parametrize('n', [1, 63, 64, 255, 256, 257, 2048 * 256 * 8 + 5])
def test_sqnorm(n, scale):
    """out[0] += sum((x*scale)^2): out is pre-loaded because the kernel accumulates; the last n is
    past the 2048-block cap (grid-stride loop).  Only the summation order differs from fp64, so
    the bound is the worst case of an fp32 sum in any order, (n + 4) * eps32 * (out0 + sum), the
    4 for the roundings of x*scale, its square and the final add onto out; where that is looser
    than the 1e-5 relative the BN statistics tests document, 1e-5 relative holds instead.
    Measured on an MI355X: at most 6.5e-8 relative up to n = 257, 2.5e-7 at n = 4194309."""
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    out0 = 3.0
    ref = out0 + ((x.double() * scale) ** 2).sum().item()
    tol = min((n + 4) * EPS32 * ref, 1e-5 * ref)
    out = torch.full((2,), out0, device=DEV)
    xg = torch.cat([x, torch.full((PAD,), 1e6)]).to(DEV)       # a read past n would be loud
    _lib.call('mlc_sqnorm', _lib.ptr(xg), n, _lib.ptr(out), scale, _lib.stream())
    torch.cuda.synchronize()
    got = out.cpu().double()
    print(f'GPU_MAXIMA_SQNORM n={n} scale={scale}: rel err {abs(got[0].item() - ref) / ref:.3e}, tol {tol / ref:.3e}')
    assert abs(got[0].item() - ref) <= tol, (got[0].item(), ref, tol)
    assert got[1].item() == out0
    assert abs(Fn.sqnorm(x, torch.full((1,), out0), scale).item() - ref) <= tol     # the CPU twin


# ------------------------------------------------------------------ mlc_zero4 (Fn.zero_many)
def _inside(numel, lead):
    """a view of ``numel`` floats starting ``lead`` floats into a sentinel-filled storage"""
    store = torch.full((lead + numel + PAD,), SENT, device=DEV)
    return store, store[lead:lead + numel]


@pytest.mark.parametrize('case', ['one', 'four', 'five-with-none'])
def test_zero_many(case):
    """1, 4 and 5 tensors (two launches), sizes 1000x apart (the grid is sized by the largest, the
    largest is past one pass of the 2048-block cap), numel % 4 != 0 (scalar tail), a view that
    starts one float into its storage (the unaligned branch), a None in the list."""
    big = 2048 * 256 * 4 + 2501
    specs = {'one': [(4099, 1)],
             'four': [(5, 4), (big, 4), (2099, 1), (4, 4)],
             'five-with-none': [(2099, 1), None, (big, 1), (7, 4), (1, 4), (4096, 8)]}[case]
    made = [None if s is None else _inside(*s) for s in specs]
    views = [None if m is None else m[1] for m in made]
    assert any(v is not None and v.data_ptr() % 16 != 0 for v in views)         # the unaligned branch runs
    if case != 'one':
        assert any(v is not None and v.data_ptr() % 16 == 0 and v.numel() % 4 for v in views)
    Fn.zero_many(views)
    torch.cuda.synchronize()
    for spec, m in zip(specs, made):
        if m is None:
            continue
        (numel, lead), (store, view) = spec, m
        assert bool((view.view(torch.int32) == 0).all()), spec              # +0.0, every element
        assert bool((store[:lead] == SENT).all()) and bool((store[lead + numel:] == SENT).all()), spec
