"""The CPU twins of the `embed.hip` wrappers equal, exactly, the plain torch expressions the
native BERT used before them (what its CPU runs still compute)."""
import pytest
import torch

from mlcomp_amd.ops import functional as Fn
from mlcomp_amd.ops import transformer as Tx

T, H, V, LD = 24, 32, 3, 8


def _inputs():
    g = torch.Generator().manual_seed(5)
    word, pos, tok = (torch.randn(n, H, generator=g).to(torch.bfloat16) for n in (40, 9, 2))
    ids, tt = torch.randint(0, 40, (T,), generator=g), torch.randint(0, 2, (T,), generator=g)
    pos_ids = torch.arange(T) % 8
    ds = torch.randn(T, H, generator=g).to(torch.bfloat16)
    cu = torch.tensor([0, 8, 8, 16, 24, 24], dtype=torch.int32)
    n = cu.numel() - 1
    logits = torch.randn(n, LD, generator=g)
    labels, w = torch.randint(0, V, (n,), generator=g), torch.tensor([1 / 3, 0.0, 1 / 3, 1 / 3, 0.0])
    return word, pos, tok, ids, tt, pos_ids, ds, cu, logits, labels, w


@pytest.mark.parametrize('op', ['embed_ln_fwd', 'embed_ln_fwd_padded', 'embed_bwd_packed', 'softmax_ce_slots',
                                'cls_scatter'])
def test_cpu_twin_is_the_torch_code_it_replaces(op):
    word, pos, tok, ids, tt, pos_ids, ds, cu, logits, labels, w = _inputs()
    gamma, beta, seed = torch.rand(H) + 0.5, torch.randn(H), torch.tensor([3], dtype=torch.int32)
    if op.startswith('embed_ln_fwd'):
        if op.endswith('padded'):
            ids, tt, pos_ids, p = ids.view(3, 8), tt.view(3, 8), None, pos[:8][None]
        else:
            p = pos[pos_ids]
        e = (word[ids].float() + p.float() + tok[tt].float()).to(torch.bfloat16).view(T, -1)
        want = Tx.ln_fwd(e, None, gamma, beta, 1e-12, p_out=0.1, seed=seed, salt_out=1)
        got = Tx.embed_ln_fwd(ids, tt, pos_ids, word, pos, tok, gamma, beta, 1e-12, p_out=0.1, seed=seed, salt_out=1)
    elif op == 'embed_bwd_packed':
        want = [torch.ones(n, H) for n in (40, 9, 2)]
        got = [torch.ones(n, H) for n in (40, 9, 2)]
        for t, ix in zip(want, (ids, pos_ids, tt)):
            t.index_add_(0, ix, ds.float())
        Tx.embed_bwd_packed(ds, ids, tt, pos_ids, *got)
    elif op == 'softmax_ce_slots':
        lf, real = logits[:, :V].float(), (w > 0).float()
        logp = torch.log_softmax(lf, 1)
        nll = -logp.gather(1, labels[:, None])[:, 0]
        g = torch.exp(logp)
        g.scatter_add_(1, labels[:, None], torch.full_like(nll, -1.0)[:, None])
        dl = torch.zeros_like(logits, dtype=torch.bfloat16)
        dl[:, :V] = (g * w[:, None]).to(torch.bfloat16)
        want = [dl, (nll * w).sum(), 1.5 + (nll * real).sum(), 2.0 + ((lf.argmax(1) == labels).float() * real).sum()]
        acc = torch.tensor([[1.5], [2.0]])
        got = [*Fn.softmax_ce_slots(logits, labels, w, acc[0], acc[1], num_classes=V), acc[0, 0], acc[1, 0]]
    else:
        dh = torch.zeros(T, H)
        dh.index_add_(0, cu[:-1].long().clamp(max=T - 1), ds[:5].float())
        want, got = [dh.to(torch.bfloat16)], [Tx.cls_scatter(ds[:5], cu, T)]
    for a, b in zip(got, want):
        assert torch.equal(a, b)
