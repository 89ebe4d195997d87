"""`csrc/kernels/embed.hip` on the GPU: the fused embedding + LayerNorm forward against the
gather + `ln_fwd` path it replaces (bit for bit), the packed embedding backward against
`index_add_`, and the packed head's two kernels against the torch code they replace."""
import pytest
import torch

from mlcomp_amd.ops import functional as Fn
from mlcomp_amd.ops import transformer as Tx

pytestmark = pytest.mark.gpu
DEV = 'cuda'
VOCAB, NPOS = 50, 12


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _tables(H, ntypes, seed):
    g = torch.Generator().manual_seed(seed)
    tbl = [torch.randn(n, H, generator=g).to(torch.bfloat16) for n in (VOCAB, NPOS, ntypes)]
    return tbl + [torch.rand(H, generator=g) + 0.5, torch.randn(H, generator=g) * 0.1]


# H: the smallest and largest width of every MAXC instantiation (1: <= 256, 2: <= 512, 4: <= 1024,
# 8: <= 2048); at H = 64 lanes 16..63 own no chunk.  T = 5 leaves a partial block.
@pytest.mark.parametrize('H,padded,use_tt,p,bad', [
    (64, False, True, 0.0, False), (256, False, True, 0.1, False), (260, True, False, 0.0, False),
    (512, False, True, 0.1, False), (516, True, True, 0.1, False), (768, False, True, 0.1, False),
    (768, True, True, 0.0, False), (1024, False, False, 0.1, False), (1028, False, True, 0.0, False),
    (2048, False, True, 0.1, False), (768, False, True, 0.1, True)])
def test_embed_ln_fwd_equals_gather_then_ln(H, padded, use_tt, p, bad):
    word, pos, tok, gamma, beta = _tables(H, 2, H)
    g = torch.Generator().manual_seed(H + 1)
    if padded:   # ids [2, 5]: the position of a token is its column
        ids, pos_ids, pidx = torch.randint(0, VOCAB, (2, 5), generator=g), None, torch.arange(5).repeat(2)
    else:        # packed rows with positions that are not monotone
        ids, pos_ids = torch.randint(0, VOCAB, (5,), generator=g), torch.tensor([3, 0, 11, 1, 0])
        pidx = pos_ids
    tt = torch.randint(0, 2, ids.shape, generator=g) if use_tt else None
    if bad:      # one past each table: clamped, never read
        ids[1], pos_ids[2] = VOCAB, NPOS
        pidx = pos_ids.clamp(max=NPOS - 1)
    ic = ids.clamp(max=VOCAB - 1)
    seed = torch.tensor([7], dtype=torch.int32)
    got = Tx.embed_ln_fwd(*(t if t is None else t.to(DEV) for t in (ids, tt, pos_ids, word, pos, tok, gamma, beta)),
                          1e-12, p_out=p, seed=seed.to(DEV), salt_out=1)
    # the path it replaces, on the GPU: torch gathers, then mlc_ln_fwd
    wd, pd, td = word.to(DEV), pos.to(DEV), tok.to(DEV)
    ty = tt.reshape(-1).to(DEV) if use_tt else torch.zeros(ids.numel(), dtype=torch.long, device=DEV)
    e = (wd[ic.reshape(-1).to(DEV)].float() + pd[pidx.to(DEV)].float() + td[ty].float()).to(torch.bfloat16)
    ref = Tx.ln_fwd(e, None, gamma.to(DEV), beta.to(DEV), 1e-12, p_out=p, seed=seed.to(DEV), salt_out=1)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):   # y, e, mean, rstd
        assert torch.equal(a, b)
    twin = Tx.embed_ln_fwd(ic, tt, pidx if pos_ids is not None else None, word, pos, tok, gamma, beta, 1e-12,
                           p_out=p, seed=seed, salt_out=1)
    assert rel(got[0], twin[0]) < 1e-2 and rel(got[1], twin[1]) < 1e-2
    assert rel(got[2], twin[2]) < 1e-4 and rel(got[3], twin[3]) < 1e-4


@pytest.mark.parametrize('T,H,ntypes', [(37, 64, 1), (37, 768, 2), (256, 128, 4)])
def test_embed_bwd_packed_matches_index_add(T, H, ntypes):
    """Half the ids are 0, many short sequences (position 0 repeats), tail rows with a nonzero
    gradient; the second call into the same gradients shows the scratch was left zeroed."""
    g = torch.Generator().manual_seed(T + H)
    ds = torch.randn(T, H, generator=g).to(torch.bfloat16)
    ids = torch.randint(0, VOCAB, (T,), generator=g) * torch.randint(0, 2, (T,), generator=g)
    tt = torch.randint(0, ntypes, (T,), generator=g)
    pos_ids, r = torch.zeros(T, dtype=torch.long), 0
    while r < T - 4:     # lengths 1..9; the last rows stay a tail at position 0
        n = min(int(torch.randint(1, 10, (1,), generator=g)), T - 4 - r)
        pos_ids[r:r + n] = torch.arange(n)
        r += n
    ref = [torch.zeros(n, H) for n in (VOCAB, NPOS, ntypes)]
    for t, ix in zip(ref, (ids, pos_ids, tt)):
        t.index_add_(0, ix, ds.float())
    out = [torch.zeros(n, H, device=DEV) for n in (VOCAB, NPOS, ntypes)]
    for _ in range(2):
        Tx.embed_bwd_packed(ds.to(DEV), ids.to(DEV), tt.to(DEV), pos_ids.to(DEV), *out)
    torch.cuda.synchronize()
    for o, t in zip(out, ref):
        assert rel(o, 2 * t) < 1e-5


@pytest.mark.parametrize('V,ld', [(2, 8), (3, 8)])
@pytest.mark.parametrize('n', [1, 5, 64])
def test_softmax_ce_slots(n, V, ld):
    g = torch.Generator().manual_seed(10 * n + V)
    logits = torch.randn(n, ld, generator=g) * 3
    labels = torch.randint(0, V, (n,), generator=g)
    real = torch.ones(n)
    real[1::3] = 0                      # empty slots (none when n = 1)
    w = real / real.sum()
    acc_r, acc_g = torch.tensor([[2.5], [3.0]]), torch.tensor([[2.5], [3.0]], device=DEV)   # the kernel accumulates
    dl_r, wl_r = Fn.softmax_ce_slots(logits, labels, w, acc_r[0], acc_r[1], num_classes=V)
    dl, wl = Fn.softmax_ce_slots(logits.to(DEV), labels.to(DEV), w.to(DEV), acc_g[0], acc_g[1], num_classes=V)
    torch.cuda.synchronize()
    assert abs(acc_g[0].item() - acc_r[0].item()) / acc_r[0].item() < 1e-4
    assert abs(wl.item() - wl_r.item()) / wl_r.item() < 1e-4
    assert acc_g[1].item() == acc_r[1].item()
    assert rel(dl, dl_r) < 1e-2
    assert bool((dl[:, V:] == 0).all()) and bool((dl[real.to(DEV) == 0] == 0).all())


@pytest.mark.parametrize('H', [64, 768])
@pytest.mark.parametrize('cu', [[0, 7, 15, 22, 33], [0, 7, 7, 7, 15, 33], [0, 10, 39, 40, 40, 40]],
                         ids=['plain', 'empty-middle', 'empty-tail-at-T'])
def test_cls_scatter_equals_index_add(cu, H):
    T, n = 40, len(cu) - 1
    dcls = torch.randn(n, H, generator=torch.Generator().manual_seed(H + n)).to(torch.bfloat16)
    cu = torch.tensor(cu, dtype=torch.int32)
    ref = torch.zeros(T, H).index_add_(0, cu[:-1].long().clamp(max=T - 1), dcls.float()).to(torch.bfloat16)
    got = Tx.cls_scatter(dcls.to(DEV), cu.to(DEV), T)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), ref)
