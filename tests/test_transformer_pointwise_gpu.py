"""`csrc/kernels/transformer.hip` per element: mlc_ln_fwd, mlc_ln_bwd, mlc_ln_finalize_many,
mlc_softmax_fwd, mlc_softmax_bwd, mlc_colsum_acc, mlc_dropout (and dropout.h through them).

Reference: every operation is written out below in torch fp64 from the bf16 inputs widened to
fp64 (``ln_fwd_ref`` ...); the same function run in fp32 is the "twin" that sizes the tolerance.
Neither calls the fp32 CPU paths of ``mlcomp_amd.ops.transformer``.  Dropout decisions come from
``keep_mask``, an exact integer function that the boundary tests at the end tie to the kernels
(`tests/test_dropout_mask_cpu.py` ties it to dropout.h on the host).

Tolerances, per element, ``e32`` = max |twin - ref64| over the case:
  fp32 outputs (mean, rstd, dgamma, dbeta, sums, colsum out)   |got - ref64| <= 4 e32
  bf16 outputs of LayerNorm, softmax backward, dropout         |got - ref64| <= ulp/2 + 4 e32
  softmax forward (``__expf``: no CPU twin has its error)      |got - ref64| <= ulp
with ulp the bf16 spacing at ref64.  Tiny shapes run many independent problems, one launch
each, so that e32 is a maximum over some hundreds of elements and not over four.

Storage: every array a kernel sees is a view into a larger sentinel-filled buffer (NaN for bf16
and fp32 outputs and for the inputs, so a read past a row is as loud as a write; a finite 12345
around accumulated outputs and scratch).  After a call everything outside the view must hold the
sentinel bit for bit and no NaN may be left inside.  bf16 views start 8 bytes into their buffer
(not 16), gamma / beta and the colsum input 16 bytes, as the kernels' vector accesses require.

Measured figures (MI355X) are in profiles/transformer_tests/README.md."""
import math
import time

import pytest
import torch

from mlcomp_amd.ops import _lib
from mlcomp_amd.ops import transformer as Tx
from test_dropout_mask_cpu import fp32_threshold, placements

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 64                  # sentinel elements past every view
NAN = float('nan')
FIN = 12345.0               # sentinel around accumulated fp32 arrays
BF, F32 = torch.bfloat16, torch.float32


def f32(x):
    """x rounded to fp32, as a Python float: what a kernel's ``float`` argument holds"""
    return torch.tensor(x, dtype=F32).item()


EPS = f32(1e-12)
WORST = {}                  # name -> [max err / bound, max e32, elements]
SOFTMAX_NEAREST = [0, 0]    # [elements that are not the nearest bf16, elements]


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for name, (ratio, e32, n) in sorted(WORST.items()):
        print(f'POINTWISE_WORST {name}: max err/bound {ratio:.3f}, max e32 {e32:.3e}, {n} elements')
    if SOFTMAX_NEAREST[1]:
        print(f'POINTWISE_SOFTMAX_NOT_NEAREST {SOFTMAX_NEAREST[0]} of {SOFTMAX_NEAREST[1]}')


# ------------------------------------------------------------------ guarded storage
def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class Guarded:
    """``reps`` independent arrays of ``n`` elements, each ``lead`` elements into its own
    sentinel-filled row of lead + n + GUARD elements"""

    def __init__(self, reps, n, dtype, lead, fill=NAN, data=None):
        self.store = torch.full((reps, lead + n + GUARD), fill, dtype=dtype, device=DEV)
        self.pat = _bits(torch.full((1,), fill, dtype=dtype, device=DEV))
        self.lead, self.n, self.fill = lead, n, fill
        if data is not None:
            self.inner.copy_(data.reshape(reps, n))
        self.before = self.store.clone() if data is not None else None

    @property
    def inner(self):
        return self.store[:, self.lead:self.lead + self.n]

    def ptr(self, r=0):
        v = self.store[r, self.lead:]
        assert v.data_ptr() % (8 if v.element_size() == 2 else 4) == 0
        return _lib.ptr(v)

    def cpu(self, *shape):
        return self.inner.cpu().reshape(self.store.shape[0], *shape)

    def guards_ok(self, name):
        b = _bits(self.store)
        ok = bool((b[:, :self.lead] == self.pat).all()) and bool((b[:, self.lead + self.n:] == self.pat).all())
        assert ok, f'{name}: written outside its array'

    def written(self, name):
        """an output: guards intact, no sentinel left inside"""
        self.guards_ok(name)
        assert not bool(torch.isnan(self.inner).any()), f'{name}: an element was left unwritten (or is NaN)'

    def untouched(self, name):
        if self.before is not None:
            assert torch.equal(_bits(self.store), _bits(self.before)), f'{name}: a read-only array changed'
        else:
            assert bool((_bits(self.store) == self.pat).all()), f'{name}: written, but nothing should be'


def seed_dev(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ tolerances
def ulp_bf16(v):
    """bf16 spacing at the fp64 value v (2**-133 at 0)"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))        # |v| = m * 2**e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), e - 8)


def close(name, case, got, ref64, twin, kind):
    """kind 'f32': 4 e32; 'bf16': ulp/2 + 4 e32; 'bf16-2': ulp (one of the two bf16 neighbours)"""
    got = got.double().cpu().reshape(ref64.shape)
    e32 = (twin.double() - ref64).abs().max().item() if twin is not None else 0.0
    tol = {'f32': lambda: torch.full_like(ref64, 4 * e32),
           'bf16': lambda: 0.5 * ulp_bf16(ref64) + 4 * e32,
           'bf16-2': lambda: ulp_bf16(ref64)}[kind]()
    err = (got - ref64).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    bad = err > tol
    ratio = torch.where(err > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err)).max().item()
    w = WORST.setdefault(name, [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], ratio), max(w[1], e32), w[2] + err.numel()
    if bool(bad.any()):
        i = int(torch.where(bad.reshape(-1), err.reshape(-1) / tol.reshape(-1).clamp_min(1e-300),
                            torch.zeros_like(err).reshape(-1)).argmax())
        print(f'POINTWISE_FAIL {name} {case}: {int(bad.sum())} of {bad.numel()} elements, worst at flat {i}: '
              f'got {got.reshape(-1)[i].item():.9g} ref {ref64.reshape(-1)[i].item():.9g} '
              f'tol {tol.reshape(-1)[i].item():.3e} e32 {e32:.3e} ratio {ratio:.3f}')
    assert not bool(bad.any()), (name, case, int(bad.sum()), ratio, e32)


def inv_keep(p, dt):
    """1 / (1 - p) as the launchers compute it (fp32) or in fp64 from the fp32 p"""
    if p <= 0:
        return 1.0
    if dt == F32:
        return (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=F32))).item()
    return 1.0 / (1.0 - f32(p))


def masks(shape, p, seed, salt):
    return Tx.keep_mask(shape, p, seed, salt) if p > 0 else None


def drop(v, keep, p, dt):
    return v if keep is None else torch.where(keep, v * inv_keep(p, dt), torch.zeros_like(v))


# ------------------------------------------------------------------ the references, written out
def ln_fwd_ref(x, r, gamma, beta, p_in, p_out, keep_in, keep_out, dt):
    """x, r [reps, T, H]; returns s, y, mean, rstd in dt"""
    H = x.shape[-1]
    v = x.to(dt)
    if r is not None:
        v = v + drop(r.to(dt), keep_in, p_in, dt)
    mean = v.sum(-1) / H
    d = v - mean[..., None]
    rstd = ((d * d).sum(-1) / H + EPS).rsqrt()
    y = d * rstd[..., None] * gamma.to(dt) + beta.to(dt)
    return v, drop(y, keep_out, p_out, dt), mean, rstd


def ln_bwd_ref(dy, s, mean, rstd, gamma, p_in, p_out, keep_in, keep_out, dt):
    """returns ds, dr, sum_T(d * xhat), sum_T(d)"""
    H = dy.shape[-1]
    d = drop(dy.to(dt), keep_out, p_out, dt)
    xh = (s.to(dt) - mean.to(dt)[..., None]) * rstd.to(dt)[..., None]
    g = d * gamma.to(dt)
    a = g.sum(-1, keepdim=True) / H
    b = (g * xh).sum(-1, keepdim=True) / H
    ds = rstd.to(dt)[..., None] * (g - a - xh * b)
    return ds, drop(ds, keep_in, p_in, dt), (d * xh).sum(-2), d.sum(-2)


def softmax_fwd_ref(S, kb, rpb, scale, dt):
    v = S.to(dt) * scale
    if kb is not None:
        v = v + kb.to(dt).repeat_interleave(rpb, 0)[:S.shape[0]]
    m = v.max(-1, keepdim=True).values
    e = torch.where(v == -math.inf, torch.zeros_like(v), (v - torch.where(m == -math.inf, torch.zeros_like(m), m)).exp())
    tot = e.sum(-1, keepdim=True)
    return torch.where(tot > 0, e / tot, torch.zeros_like(e))


def softmax_bwd_ref(P, dPd, scale, p, keep, dt):
    d = drop(dPd.to(dt), keep, p, dt)
    Pf = P.to(dt)
    return scale * Pf * (d - (Pf * d).sum(-1, keepdim=True))


def _bf(*shape, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


def _reps(T, H):
    return max(1, -(-32 // T), -(-256 // (T * H)))


# ------------------------------------------------------------------ LayerNorm forward
LN_H = [4, 252, 256, 260, 516, 1028, 2044, 2048]      # H/4 = 1, 63, 64, 65, 129, 257, 511, 512
# (r given, p_in, p_out)
LN_FWD_VARIANTS = [(False, 0.0, 0.0), (False, 0.0, 0.3), (True, 0.0, 0.0), (True, 0.1, 0.0), (True, 0.0, 0.3),
                   (True, 0.3, 0.1)]


GROUPS = [('', slice(2, None)), (' (offset row)', slice(1, 2)), (' (constant row)', slice(0, 1))]


def _ln_inputs(T, H, reps, seed):
    gen = torch.Generator().manual_seed(seed)
    x, r = _bf(reps, T, H, gen=gen), _bf(reps, T, H, gen=gen)
    if T >= 2:
        x[:, 0], r[:, 0] = 1.5, 0.25                  # a constant row, with and without r: variance 0
        # mean >> spread: 16 + k/8 (bf16 spacing at 16 is 1/8); a one-pass E[x^2] - mean^2 loses it
        x[:, 1] = (16 + torch.randint(-2, 3, (reps, H), generator=gen) / 8).to(BF)
        r[:, 1] = _bf(reps, H, gen=gen, scale=0.05)
    gamma = torch.rand(H, generator=gen) + 0.5
    beta = torch.randn(H, generator=gen) * 0.1
    return x, r, gamma, beta


@pytest.mark.parametrize('T', [1, 7])
@pytest.mark.parametrize('H', LN_H)
def test_ln_fwd_per_element(H, T):
    reps = max(32, _reps(T, H))        # 32 or more samples of each kind of row
    x, r, gamma, beta = _ln_inputs(T, H, reps, seed=H * 10 + T)
    G, B_ = Guarded(1, H, F32, 4, data=gamma), Guarded(1, H, F32, 4, data=beta)
    X, R = Guarded(reps, T * H, BF, 4, data=x), Guarded(reps, T * H, BF, 4, data=r)
    sd, salt_in, salt_out = 7 + H, 3, 4
    seed = seed_dev(sd)
    for has_r, p_in, p_out in LN_FWD_VARIANTS:
        case = (H, T, has_r, p_in, p_out)
        # a salt pair per problem: the masks, and with them the statistics of every row, differ
        k_in = torch.stack([Tx.keep_mask((T, H), p_in, sd, salt_in + 16 * i) for i in range(reps)]) if p_in else None
        k_out = torch.stack([Tx.keep_mask((T, H), p_out, sd, salt_out + 16 * i) for i in range(reps)]) if p_out else None
        ref = ln_fwd_ref(x, r if has_r else None, gamma, beta, p_in, p_out, k_in, k_out, torch.float64)
        twin = ln_fwd_ref(x, r if has_r else None, gamma, beta, p_in, p_out, k_in, k_out, F32)
        S, Y = Guarded(reps, T * H, BF, 4), Guarded(reps, T * H, BF, 4)
        MEAN, RSTD = Guarded(reps, T, F32, 1), Guarded(reps, T, F32, 1)
        for i in range(reps):
            _lib.call('mlc_ln_fwd', X.ptr(i), R.ptr(i) if has_r else None, S.ptr(i) if has_r else None, Y.ptr(i),
                      MEAN.ptr(i), RSTD.ptr(i), G.ptr(), B_.ptr(), T, H, EPS, p_in, p_out, _lib.ptr(seed),
                      salt_in + 16 * i, salt_out + 16 * i, _lib.stream())
        torch.cuda.synchronize()
        for name, arr in (('x', X), ('r', R), ('gamma', G), ('beta', B_)):
            arr.untouched(name)
        Y.written('y'), MEAN.written('mean'), RSTD.written('rstd')
        S.written('s_out') if has_r else S.untouched('s_out')
        y = Y.cpu(T, H)
        # e32 is taken per kind of row: the constant row's rstd is 1e6 and the offset row's mean
        # 16, and their fp32 errors would loosen the bound of the ordinary rows a thousandfold
        for tag, rows in GROUPS if T >= 2 else [('', slice(None))]:
            got = (S.cpu(T, H), y, MEAN.cpu(T), RSTD.cpu(T))
            for k, (name, kind) in enumerate((('s_out', 'bf16'), ('y', 'bf16'), ('mean', 'f32'), ('rstd', 'f32'))):
                if name != 's_out' or has_r:
                    close(f'ln_fwd {name}{tag}', case, got[k][:, rows], ref[k][:, rows], twin[k][:, rows], kind)
        if k_out is not None:
            assert bool((y[~k_out] == 0).all())
        if T >= 2 and p_in == 0 and p_out == 0:       # the constant row: y is beta rounded, exactly
            assert torch.equal(y[:, 0], beta.to(BF).expand(reps, H)), case


@pytest.mark.parametrize('H', [2052, 6])
def test_ln_refuses_widths(H):
    """H % 4 != 0 and H > 2048: -1 from forward and backward, every buffer keeps its sentinel"""
    lib, T = _lib.load(), 2
    arrs = [Guarded(1, T * 2052, BF, 4) for _ in range(6)] + [Guarded(1, 2052, F32, 4) for _ in range(4)] + \
           [Guarded(1, lib.mlc_get_stat_copies() * 2 * 2052, F32, 4, fill=FIN)]
    x, r, s, y, dy, ds, mean, rstd, gamma, beta, sums = arrs
    seed = seed_dev(1)
    assert lib.mlc_ln_fwd(x.ptr(), r.ptr(), s.ptr(), y.ptr(), mean.ptr(), rstd.ptr(), gamma.ptr(), beta.ptr(), T, H,
                          EPS, 0.1, 0.1, _lib.ptr(seed), 1, 2, _lib.stream()) == -1
    assert lib.mlc_ln_bwd(dy.ptr(), s.ptr(), mean.ptr(), rstd.ptr(), gamma.ptr(), ds.ptr(), r.ptr(), sums.ptr(),
                          beta.ptr(), gamma.ptr(), T, H, 0.1, 0.1, _lib.ptr(seed), 1, 2, _lib.stream()) == -1
    torch.cuda.synchronize()
    for a in arrs:
        a.untouched('refused call')


# ------------------------------------------------------------------ LayerNorm backward
def _ln_bwd_inputs(T, H, reps, seed):
    gen = torch.Generator().manual_seed(seed)
    dy, s = _bf(reps, T, H, gen=gen), _bf(reps, T, H, gen=gen, scale=1.5)
    s64 = s.double()
    mean = s64.mean(-1)
    rstd = (s64.var(-1, unbiased=False) + 1e-5).rsqrt()
    gamma = torch.rand(H, generator=gen) + 0.5
    pre = torch.randn(2, reps, H, generator=gen)           # dgamma / dbeta are accumulated into
    return dy, s, mean.float(), rstd.float(), gamma, pre[0], pre[1]


def _run_ln_bwd(T, H, reps, seed, variants, tag):
    ncopy = _lib.load().mlc_get_stat_copies()
    nblk = min(512, -(-T // 4))
    dy, s, mean, rstd, gamma, dg0, db0 = _ln_bwd_inputs(T, H, reps, seed)
    DY, S_ = Guarded(reps, T * H, BF, 4, data=dy), Guarded(reps, T * H, BF, 4, data=s)
    MEAN, RSTD = Guarded(reps, T, F32, 1, data=mean), Guarded(reps, T, F32, 1, data=rstd)
    G = Guarded(1, H, F32, 4, data=gamma)
    sd, salt_in, salt_out = 11 + H, 5, 6
    sdev = seed_dev(sd)
    for want_dr, p_in, p_out in variants:
        case = (tag, T, H, want_dr, p_in, p_out)
        k_in, k_out = masks((T, H), p_in, sd, salt_in), masks((T, H), p_out, sd, salt_out)
        ref = ln_bwd_ref(dy, s, mean, rstd, gamma, p_in, p_out, k_in, k_out, torch.float64)
        twin = ln_bwd_ref(dy, s, mean, rstd, gamma, p_in, p_out, k_in, k_out, F32)
        DS, DR = Guarded(reps, T * H, BF, 4), Guarded(reps, T * H, BF, 4)
        SUMS = Guarded(reps, ncopy * 2 * H, F32, 4, fill=FIN, data=torch.zeros(reps, ncopy * 2 * H))
        DG, DB = Guarded(reps, H, F32, 4, fill=FIN, data=dg0), Guarded(reps, H, F32, 4, fill=FIN, data=db0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(reps):
            _lib.call('mlc_ln_bwd', DY.ptr(i), S_.ptr(i), MEAN.ptr(i), RSTD.ptr(i), G.ptr(), DS.ptr(i),
                      DR.ptr(i) if want_dr else None, SUMS.ptr(i), DG.ptr(i), DB.ptr(i), T, H, p_in, p_out,
                      _lib.ptr(sdev), salt_in, salt_out, _lib.stream())
        torch.cuda.synchronize()
        if reps == 1:
            print(f'POINTWISE_TIME ln_bwd T={T} H={H}: launch to sync {1e3 * (time.perf_counter() - t0):.2f} ms')
        for name, arr in (('dy', DY), ('s', S_), ('mean', MEAN), ('rstd', RSTD), ('gamma', G)):
            arr.untouched(name)
        DS.written('ds')
        close('ln_bwd ds', case, DS.cpu(T, H), ref[0], twin[0], 'bf16')
        if want_dr:
            DR.written('dr')
            dr = DR.cpu(T, H)
            close('ln_bwd dr', case, dr, ref[1], twin[1], 'bf16')
            if k_in is not None:
                assert bool((dr[:, ~k_in] == 0).all())
        else:
            DR.untouched('dr')
        DG.guards_ok('dgamma'), DB.guards_ok('dbeta'), SUMS.guards_ok('sums')
        close('ln_bwd dgamma', case, DG.cpu(H), dg0.double() + ref[2], dg0 + twin[2], 'f32')
        close('ln_bwd dbeta', case, DB.cpu(H), db0.double() + ref[3], db0 + twin[3], 'f32')
        # what the call leaves in the scratch: the partial sums, block b's in copy b % ncopy, NOT
        # zeroed (the next call needs them zeroed again by the caller); unused copies stay zero
        left = SUMS.cpu(ncopy, 2, H).double()
        close('ln_bwd sums', case, left.sum(1), torch.stack([ref[2], ref[3]], 1), torch.stack([twin[2], twin[3]], 1),
              'f32')
        assert bool((left[:, nblk:] == 0).all()), case
        assert bool((left[:, :min(nblk, ncopy)].abs().sum((2, 3)) > 0).all()), case


LN_BWD_VARIANTS = [(False, 0.0, 0.0), (True, 0.0, 0.0), (False, 0.3, 0.1), (True, 0.3, 0.1)]   # want_dr, p_in, p_out


@pytest.mark.parametrize('H', LN_H)
def test_ln_bwd_per_element(H):
    _run_ln_bwd(7, H, _reps(7, H), seed=H + 1, variants=LN_BWD_VARIANTS, tag='small')


@pytest.mark.parametrize('T,H', [(2051, 8), (4099, 260)])
def test_ln_bwd_grid_stride(T, H):
    """512 blocks x 4 waves = 2048 rows per sweep: rows 2048.. take a second (and third) sweep
    that only the first waves run"""
    _run_ln_bwd(T, H, 1, seed=T, variants=[(True, 0.3, 0.1)], tag='stride')


def test_ln_bwd_deferred_finalize_many():
    """two LayerNorms of widths 260 and 8 leave their sums for ONE mlc_ln_finalize_many launch,
    whose grid is sized by the wider: both gradient pairs right, nothing past column 8 of the
    narrow one"""
    T, ncopy = 7, _lib.load().mlc_get_stat_copies()
    fin, checks = Tx.LnFinalizer(), []
    sdev = seed_dev(9)
    for H in (260, 8):
        dy, s, mean, rstd, gamma, dg0, db0 = _ln_bwd_inputs(T, H, 1, seed=100 + H)
        ref = ln_bwd_ref(dy, s, mean, rstd, gamma, 0.0, 0.0, None, None, torch.float64)
        twin = ln_bwd_ref(dy, s, mean, rstd, gamma, 0.0, 0.0, None, None, F32)
        DY, S_ = Guarded(1, T * H, BF, 4, data=dy), Guarded(1, T * H, BF, 4, data=s)
        MEAN, RSTD = Guarded(1, T, F32, 1, data=mean), Guarded(1, T, F32, 1, data=rstd)
        G, DS = Guarded(1, H, F32, 4, data=gamma), Guarded(1, T * H, BF, 4)
        SUMS = Guarded(1, ncopy * 2 * H, F32, 4, fill=FIN, data=torch.zeros(1, ncopy * 2 * H))
        DG, DB = Guarded(1, H, F32, 4, fill=FIN, data=dg0), Guarded(1, H, F32, 4, fill=FIN, data=db0)
        _lib.call('mlc_ln_bwd', DY.ptr(), S_.ptr(), MEAN.ptr(), RSTD.ptr(), G.ptr(), DS.ptr(), None, SUMS.ptr(), None,
                  None, T, H, 0.0, 0.0, _lib.ptr(sdev), 0, 0, _lib.stream())
        fin.add(SUMS.inner[0], DG.inner[0], DB.inner[0])
        checks.append((H, DS, DG, DB, dg0, db0, ref, twin, (DY, S_, MEAN, RSTD, G, SUMS)))
    torch.cuda.synchronize()
    for H, DS, DG, DB, dg0, db0, ref, twin, _ in checks:          # deferred: the gradients are not touched yet
        DG.untouched('dgamma before finalize'), DB.untouched('dbeta before finalize')
        close('ln_bwd ds', ('deferred', H), DS.cpu(T, H), ref[0], twin[0], 'bf16')
    fin.run()
    torch.cuda.synchronize()
    assert fin.max_h == 260
    for H, DS, DG, DB, dg0, db0, ref, twin, _ in checks:
        DG.guards_ok('dgamma'), DB.guards_ok('dbeta')
        close('ln_finalize_many dgamma', ('deferred', H), DG.cpu(H), dg0.double() + ref[2], dg0 + twin[2], 'f32')
        close('ln_finalize_many dbeta', ('deferred', H), DB.cpu(H), db0.double() + ref[3], db0 + twin[3], 'f32')


# ------------------------------------------------------------------ softmax
SM_L = [4, 68, 252, 256, 260, 1028, 2048]
SM_R, SM_RPB, SM_SCALE = 7, 3, 0.5


def _scores(L, gen):
    """rows 0..4: every score equal but one that is 8.0 higher after the scale, at column 0, 3,
    255, 256, L-1 in turn (those inside the row); rows 5, 6 random"""
    S = _bf(SM_R, L, gen=gen, scale=3.0)
    spikes = sorted({c for c in (0, 3, 255, 256, L - 1) if c < L})
    for row in range(5):
        c = torch.randint(-8, 9, (1,), generator=gen).item() / 4
        S[row] = c
        S[row, spikes[row % len(spikes)]] = c + 8.0 / SM_SCALE
    return S


def _key_bias(kind, L, gen):
    if kind == 'none':
        return None
    kb = torch.zeros(3, L)
    if kind in ('suffix', 'full'):
        kb[0, L // 2 + 1:] = -math.inf
        kb[2, L - 1:] = -math.inf
    if kind == 'scattered':
        kb[:, L - 1] = -math.inf                          # the last column
        kb[:, 4 * (L // 8)] = -math.inf                   # an 8-byte chunk's first column
        if L > 256:
            kb[:, 256] = -math.inf                        # the first column of the lanes' second pass
        kb[1][torch.rand(L, generator=gen) < 0.3] = -math.inf
        kb[2, 0] = -math.inf
    if kind == 'full':
        kb[1] = -math.inf                                 # rows 3..5: no key left
    return kb


@pytest.mark.parametrize('bias', ['none', 'suffix', 'scattered', 'full'])
@pytest.mark.parametrize('L', SM_L)
def test_softmax_fwd_bwd_per_element(L, bias):
    gen = torch.Generator().manual_seed(L * 7 + len(bias))
    S, kb = _scores(L, gen), _key_bias(bias, L, gen)
    if kb is not None and bool((kb == -math.inf).all(1).any()) and bias != 'full':
        kb[:, 1] = 0.0                                    # L = 4: keep a key in every batch
    dPd = _bf(SM_R, L, gen=gen)
    P64 = softmax_fwd_ref(S, kb, SM_RPB, SM_SCALE, torch.float64)
    masked = (kb.repeat_interleave(SM_RPB, 0)[:SM_R] == -math.inf) if kb is not None else torch.zeros(SM_R, L).bool()
    SG, DP = Guarded(1, SM_R * L, BF, 4, data=S), Guarded(1, SM_R * L, BF, 4, data=dPd)
    KB = Guarded(1, 3 * L, F32, 1, data=kb) if kb is not None else None
    sd, salt = 13 + L, 9
    sdev = seed_dev(sd)
    # backward input: the fp64 probabilities rounded to bf16, row 6 replaced by a one-hot row
    Pin = P64.float().to(BF)
    Pin[6] = 0
    Pin[6, L - 1] = 1
    PIN = Guarded(1, SM_R * L, BF, 4, data=Pin)
    for p in (0.0, 0.1, 0.3):
        case = (L, bias, p)
        keep = masks((SM_R, L), p, sd, salt)
        P, PD = Guarded(1, SM_R * L, BF, 4), Guarded(1, SM_R * L, BF, 4)
        _lib.call('mlc_softmax_fwd', SG.ptr(), KB.ptr() if KB else None, P.ptr(), PD.ptr() if p > 0 else None, SM_R, L,
                  SM_RPB, SM_SCALE, p, _lib.ptr(sdev), salt, _lib.stream())
        DS = Guarded(1, SM_R * L, BF, 4)
        _lib.call('mlc_softmax_bwd', PIN.ptr(), DP.ptr(), DS.ptr(), SM_R, L, SM_SCALE, p, _lib.ptr(sdev), salt,
                  _lib.stream())
        torch.cuda.synchronize()
        for name, arr in (('S', SG), ('dPd', DP), ('P in', PIN)) + ((('key_bias', KB),) if KB else ()):
            arr.untouched(name)
        P.written('P')
        got = P.cpu(SM_R, L)[0]
        close('softmax_fwd P', case, got, P64, None, 'bf16-2')
        assert bool((got[masked] == 0).all()), case
        SOFTMAX_NEAREST[0] += int((got != P64.float().to(BF)).sum())
        SOFTMAX_NEAREST[1] += got.numel()
        if p > 0:
            PD.written('Pd')
            gd = PD.cpu(SM_R, L)[0]
            close('softmax_fwd Pd', case, gd, drop(P64, keep, p, torch.float64), None, 'bf16-2')
            assert bool((gd[~keep] == 0).all()) and bool((gd[masked] == 0).all()), case
            assert bool((gd[keep & ~masked & (P64 > 1e-30)] != 0).all()), case
        else:
            PD.untouched('Pd')
        DS.written('dS')
        ref = softmax_bwd_ref(Pin, dPd, SM_SCALE, p, keep, torch.float64)
        twin = softmax_bwd_ref(Pin, dPd, SM_SCALE, p, keep, F32)
        gs = DS.cpu(SM_R, L)[0]
        close('softmax_bwd dS', case, gs, ref, twin, 'bf16')
        assert bool((gs[Pin == 0] == 0).all()), case      # masked keys, fully masked rows, off the one-hot


@pytest.mark.parametrize('L', [6, 2052])
def test_softmax_refuses_widths(L):
    lib = _lib.load()
    arrs = [Guarded(1, SM_R * 2052, BF, 4) for _ in range(4)]
    a, b, c, d = arrs
    seed = seed_dev(1)
    assert lib.mlc_softmax_fwd(a.ptr(), None, b.ptr(), c.ptr(), SM_R, L, SM_RPB, SM_SCALE, 0.1, _lib.ptr(seed), 1,
                               _lib.stream()) == -1
    assert lib.mlc_softmax_bwd(a.ptr(), b.ptr(), d.ptr(), SM_R, L, SM_SCALE, 0.1, _lib.ptr(seed), 1,
                               _lib.stream()) == -1
    torch.cuda.synchronize()
    for t in arrs:
        t.untouched('refused call')


# ------------------------------------------------------------------ dropout
DROP_BIG = 4 * (4096 * 256) + 4 * 5       # the first size at which the 4096-block cap makes threads loop


@pytest.mark.parametrize('n', [4, DROP_BIG])
def test_dropout_per_element(n):
    p, sd = 0.3, 21
    reps = 64 if n == 4 else 1
    gen = torch.Generator().manual_seed(n)
    x = _bf(reps, n, gen=gen)
    X, Y = Guarded(reps, n, BF, 4, data=x), Guarded(reps, n, BF, 4)
    sdev = seed_dev(sd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        _lib.call('mlc_dropout', X.ptr(i), Y.ptr(i), n, p, _lib.ptr(sdev), 100 + i, _lib.stream())
    torch.cuda.synchronize()
    if reps == 1:
        print(f'POINTWISE_TIME dropout n={n}: launch to sync {1e3 * (time.perf_counter() - t0):.2f} ms')
    keep = torch.stack([Tx.keep_mask((n,), p, sd, 100 + i) for i in range(reps)])
    X.untouched('x'), Y.written('y')
    y = Y.cpu(n)
    close('dropout y', (n,), y, drop(x.double(), keep, p, torch.float64), drop(x.float(), keep, p, F32), 'bf16')
    assert bool((y[~keep] == 0).all()) and bool((y[keep & (x != 0)] != 0).all())
    assert 0.25 < 1 - keep.float().mean().item() < 0.35 or n == 4


# ------------------------------------------------------------------ the threshold, on the GPU
@pytest.mark.parametrize('p', [0.1, 0.3, 0.8])
def test_threshold_boundary_on_the_gpu(p):
    """hash >> 8 of one element placed at thr - 1, thr, thr + 1 (the salt solved for, see
    tests/test_dropout_mask_cpu.py): every kernel drops, keeps, keeps.  This makes the kernels'
    ``(uint32_t)(p * 16777216.0f)`` the definition; the CPU paths must give the same masks."""
    sd, T, H, i = 11, 3, 8, 13
    assert fp32_threshold(p) == Tx.drop_threshold(p)
    sdev, scpu = seed_dev(sd), torch.tensor([sd], dtype=torch.int32)
    gen = torch.Generator().manual_seed(2)
    ones, zeros, x = torch.ones(T, H, dtype=BF), torch.zeros(T, H, dtype=BF), _bf(T, H, gen=gen)
    gamma, beta = torch.ones(H), torch.full((H,), 10.0)           # |LN| <= sqrt(H) < 10: y != 0 unless dropped
    G, B_ = Guarded(1, H, F32, 4, data=gamma), Guarded(1, H, F32, 4, data=beta)
    ONES, ZEROS, X = (Guarded(1, T * H, BF, 4, data=t) for t in (ones, zeros, x))
    for salt, kept in placements(p, sd, i):
        other = salt ^ 0x55
        Y, S, Y2, P, PD = (Guarded(1, T * H, BF, 4) for _ in range(5))
        M = [Guarded(1, T, F32, 1) for _ in range(4)]
        _lib.call('mlc_dropout', ONES.ptr(), Y.ptr(), T * H, p, _lib.ptr(sdev), salt, _lib.stream())
        _lib.call('mlc_ln_fwd', ZEROS.ptr(), ONES.ptr(), S.ptr(), Y2.ptr(), M[0].ptr(), M[1].ptr(), G.ptr(), B_.ptr(),
                  T, H, EPS, p, 0.0, _lib.ptr(sdev), salt, other, _lib.stream())
        Y3 = Guarded(1, T * H, BF, 4)
        _lib.call('mlc_ln_fwd', X.ptr(), None, None, Y3.ptr(), M[2].ptr(), M[3].ptr(), G.ptr(), B_.ptr(), T, H, EPS,
                  0.0, p, _lib.ptr(sdev), other, salt, _lib.stream())
        _lib.call('mlc_softmax_fwd', X.ptr(), None, P.ptr(), PD.ptr(), T, H, T, 1.0, p, _lib.ptr(sdev), salt,
                  _lib.stream())
        torch.cuda.synchronize()
        cpu = {'dropout': Tx.dropout(ones, p, scpu, salt),
               'ln_fwd in': Tx.ln_fwd(zeros, ones, gamma, beta, EPS, p_in=p, seed=scpu, salt_in=salt, salt_out=other)[1],
               'ln_fwd out': Tx.ln_fwd(x, None, gamma, beta, EPS, p_out=p, seed=scpu, salt_in=other, salt_out=salt)[0],
               'softmax_fwd': Tx.softmax_fwd(x, None, T, 1.0, p, scpu, salt)[1]}
        for name, arr in (('dropout', Y), ('ln_fwd in', S), ('ln_fwd out', Y3), ('softmax_fwd', PD)):
            arr.written(name)
            got = arr.cpu(T * H)[0]
            assert (got[i].item() != 0) is kept, (name, p, salt, kept)
            assert torch.equal(got != 0, cpu[name].reshape(-1) != 0), (name, p, salt, 'CPU twin mask')


# ------------------------------------------------------------------ bias sums
@pytest.mark.parametrize('R,C', [(1, 8), (17, 8), (530, 24), (37, 2056)])
def test_colsum_acc_per_element(R, C):
    """(17, 8): R % RB != 0 at the RB floor of 16; (530, 24): 34 row blocks on 32 copies;
    (37, 2056): two column blocks, the second with one live lane"""
    ncopy = _lib.load().mlc_get_stat_copies()
    reps = max(1, 2048 // (R * C))
    gen = torch.Generator().manual_seed(R * C)
    g, out0 = _bf(reps, R, C, gen=gen), torch.randn(reps, C, generator=gen)
    GR = Guarded(reps, R * C, BF, 8, data=g)
    OUT = Guarded(reps, C, F32, 4, fill=FIN, data=out0)
    SCR = Guarded(reps, ncopy * C, F32, 4, fill=FIN, data=torch.zeros(reps, ncopy * C))
    for i in range(reps):
        assert GR.store[i, GR.lead:].data_ptr() % 16 == 0
        _lib.call('mlc_colsum_acc', GR.ptr(i), OUT.ptr(i), SCR.ptr(i), R, C, _lib.stream())
    torch.cuda.synchronize()
    GR.untouched('g'), OUT.guards_ok('out'), SCR.untouched('scratch (must be left zeroed)')
    close('colsum_acc out', (R, C), OUT.cpu(C), out0.double() + g.double().sum(1), out0 + g.float().sum(1), 'f32')


def test_colsum_refuses_c12():
    lib = _lib.load()
    g, out, scr = Guarded(1, 64, BF, 8), Guarded(1, 16, F32, 4, fill=FIN), Guarded(1, 32 * 16, F32, 4, fill=FIN)
    assert lib.mlc_colsum_acc(g.ptr(), out.ptr(), scr.ptr(), 2, 12, _lib.stream()) == -1
    torch.cuda.synchronize()
    g.untouched('g'), out.untouched('out'), scr.untouched('scratch')
