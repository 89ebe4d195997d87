"""Weight-stationary streaming forward of the channel-expanding 1x1 convs
(csrc/kernels/conv1x1_fwd.hip, ``Fn.conv1x1_fwd``) against the igemm path it replaces
(``Fn.conv2d_fwd``): y bit for bit, the BN partial sums within twice the igemm path's own
deviation from float64 sums of the stored y, and nothing written outside y / beside the sums.

Shapes (rows = N * H * W; the kernel walks 64-row tiles, one 256-channel chunk per block):
126 rows (no multiple of the tile), 1 row, 507 rows, 6272 rows (98 whole tiles) and ``full``:
6272 rows give a full grid of one block per CU less than one tile per block, so ``full`` is the
smallest row count at which every block of that grid gets two tiles and the last tile is partial,
(2 * groups - 1) * 64 + 1 rows with groups = CUs / (Co / 256)."""
import pytest
import torch
import torch.nn.functional as F

from mlcomp_amd.ops import _lib
from mlcomp_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu

DEV = 'cuda'
PAIRS = [(128, 512), (256, 1024)]
SHAPES = {'126': (2, 7, 9), '1': (1, 1, 1), '507': (3, 13, 13), '6272': (8, 28, 28), 'full': None}
BM, CHUNK = 64, 256
_cache = {}


def _shape(name, Co):
    if SHAPES[name] is not None:
        return SHAPES[name]
    groups = torch.cuda.get_device_properties(0).multi_processor_count // (Co // CHUNK)
    return (1, 1, (2 * groups - 1) * BM + 1)


def _case(Ci, Co, name):
    """Inputs and the igemm results, computed once per (pair, shape) and left unchanged."""
    key = (Ci, Co, name)
    if key not in _cache:
        N, H, W = _shape(name, Co)
        g = torch.Generator().manual_seed(Ci + 7 * N * H * W)
        x = torch.randn(N, H, W, Ci, generator=g).to(torch.bfloat16).to(DEV)
        w = (torch.randn(Co, 1, 1, Ci, generator=g) * Ci ** -0.5).to(torch.bfloat16).to(DEV)
        s1, s2 = Fn.stat_buffers(Co, DEV)
        y = Fn.conv2d_fwd(x, w, 1, 0, stats=(s1, s2))
        torch.cuda.synchronize()
        _cache[key] = dict(x=x, w=w, y=y, s1=s1, s2=s2)
    return _cache[key]


def _fold(s, Co):
    return s.reshape(Fn.NSTAT, Co).double().sum(0)


def _dev(s1, s2, y, Co):
    """Largest deviation of the folded partial sums from float64 sums of the stored bf16 y."""
    yd = y.reshape(-1, Co).double()
    return ((_fold(s1, Co) - yd.sum(0)).abs().max().item(),
            (_fold(s2, Co) - (yd * yd).sum(0)).abs().max().item())


def _run(c, Co, prefill=0.0):
    rows = c['y'].numel() // Co
    s1, s2 = Fn.stat_buffers(Co, DEV)
    s1.fill_(prefill)
    s2.fill_(prefill)
    buf = torch.full(((rows + BM) * Co,), -7.0, device=DEV, dtype=torch.bfloat16)   # one tile of slack
    y = Fn.conv1x1_fwd(c['x'], c['w'], (s1, s2), out=buf[:rows * Co].view(c['y'].shape))
    torch.cuda.synchronize()
    return y, s1, s2, buf[rows * Co:]


def _check(Ci, Co, name):
    c = _case(Ci, Co, name)
    y, s1, s2, tail = _run(c, Co)
    # y: bit for bit the igemm result, and within the igemm test's tolerance of the fp32 conv
    assert torch.equal(y.view(torch.int16), c['y'].view(torch.int16))
    assert torch.all(tail == -7.0)
    ref = F.conv2d(c['x'].permute(0, 3, 1, 2).float(), c['w'].permute(0, 3, 1, 2).float()).permute(0, 2, 3, 1)
    assert ((y.float() - ref).norm() / (ref.norm() + 1e-12)).item() < 1e-2
    # statistics: at most twice the igemm path's own deviation from the float64 sums
    new, old = _dev(s1, s2, y, Co), _dev(c['s1'], c['s2'], c['y'], Co)
    print(f'conv1x1_fwd {Ci}>{Co} rows {y.numel() // Co}: sum dev new {new[0]:.3e} igemm {old[0]:.3e}; '
          f'sumsq dev new {new[1]:.3e} igemm {old[1]:.3e}')
    assert new[0] <= 2 * old[0] and new[1] <= 2 * old[1], (new, old)
    return c, s1, s2


@pytest.mark.parametrize('name', list(SHAPES))
@pytest.mark.parametrize('Ci,Co', PAIRS)
def test_matches_igemm(Ci, Co, name):
    _check(Ci, Co, name)


@pytest.mark.parametrize('Ci,Co', PAIRS)
def test_few_blocks_walk_many_tiles(Ci, Co):
    """Grid capped to 3 blocks (whole row groups: one block per 256-channel chunk at the least),
    so one block walks all 98 tiles of the 6272 rows with its sums carried across them."""
    lib = _lib.load()
    old = lib.mlc_conv1x1_fwd_get_set(0, 3)
    try:
        _check(Ci, Co, '6272')
    finally:
        lib.mlc_conv1x1_fwd_get_set(0, old)


@pytest.mark.parametrize('Ci,Co', PAIRS)
def test_sums_are_added_to(Ci, Co):
    c, s1, s2 = _check(Ci, Co, '507')
    _, p1, p2, _ = _run(c, Co, prefill=0.5)
    # the same per-block partials land on 0.5 instead of 0: fp32 rounding of one more add each
    assert torch.allclose(p1, s1 + 0.5, rtol=1e-5, atol=1e-5)
    assert torch.allclose(p2, s2 + 0.5, rtol=1e-5, atol=1e-5)
    assert torch.all(p1 != 0) and torch.all(p2 != 0)


def test_ok_reports_instantiations():
    for Ci, Co in PAIRS:
        assert Fn.conv1x1_fwd_available(Ci, Co)
    for Ci, Co in [(64, 64), (512, 2048), (128, 500)]:
        assert not Fn.conv1x1_fwd_available(Ci, Co)
