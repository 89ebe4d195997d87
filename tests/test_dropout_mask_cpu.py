"""The host twin of the dropout mask (``keep_mask`` and the CPU paths built on it) at the
threshold, where it has to agree with ``csrc/kernels/dropout.h`` element for element.

``drop_threshold(p)`` of the kernels is ``(uint32_t)(p * 16777216.0f)`` on the fp32 p; the twin
used ``int(p * 16777216.0)`` on the double p, one lower for p = 0.3, 0.6 and 0.8
(5033164 / 10066329 / 13421772 against the kernels' 5033165 / 10066330 / 13421773).  A random
tensor meets the one hash value in 2**24 that tells them apart about never, so the tests here
put it there: ``hash_u32`` is a bijection of u32 for fixed (seed, element index) as a function
of the salt, and ``solve_salt`` inverts it, which places ``hash >> 8`` at thr - 1, thr and
thr + 1 on a chosen element.  The mask must drop the first and keep the other two.
``tests/test_transformer_pointwise_gpu.py`` runs the same placements through the kernels."""
import struct

import pytest
import torch

from mlcomp_amd.ops import transformer as Tx

M32 = 0xFFFFFFFF
PS = [0.05, 0.1, 0.2, 0.3, 0.5, 0.6, 0.8, 0.9]
# thresholds of dropout.h, computed by hand in fp32: p32 = RN32(p) has a 24-bit significand, so
# p32 * 2**24 is exact and the cast truncates it
KERNEL_THR = {0.05: 838860, 0.1: 1677721, 0.2: 3355443, 0.3: 5033165, 0.5: 8388608, 0.6: 10066330,
              0.8: 13421773, 0.9: 15099494}


def fp32_threshold(p):
    """(uint32_t)(p * 16777216.0f) from the bits of the fp32 p, in integers only"""
    (bits,) = struct.unpack('<I', struct.pack('<f', p))
    exp, man = (bits >> 23) & 0xFF, (bits & 0x7FFFFF) | 0x800000      # normal numbers: 0 < p < 1
    shift = exp - 127 - 23 + 24                                       # value = man * 2**(exp-150); times 2**24
    return man << shift if shift >= 0 else man >> -shift


def hash_u32(seed, salt, i):
    """dropout.h hash_u32 in Python integers"""
    x = ((i * 0x9E3779B9) ^ (seed * 0x85EBCA6B + salt * 0xC2B2AE35)) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def solve_salt(seed, i, target):
    """the salt with hash_u32(seed, salt, i) == target: every step of the hash undone in turn
    (x ^= x >> 16 is its own inverse, x ^= x >> 15 needs the 30-bit term too, the odd
    multipliers have inverses mod 2**32)"""
    x = target
    x ^= x >> 16
    x = (x * pow(0x846CA68B, -1, 1 << 32)) & M32
    x = x ^ (x >> 15) ^ (x >> 30)
    x = (x * pow(0x7FEB352D, -1, 1 << 32)) & M32
    x ^= x >> 16
    k = (x ^ (i * 0x9E3779B9)) & M32                    # = seed * A + salt * B
    salt = ((k - seed * 0x85EBCA6B) * pow(0xC2B2AE35, -1, 1 << 32)) & M32
    assert hash_u32(seed, salt, i) == target
    return salt


def placements(p, seed, i):
    """[(salt, keep)] putting hash >> 8 of element i at thr - 1, thr, thr + 1 (low bytes vary)"""
    thr = fp32_threshold(p)
    return [(solve_salt(seed, i, ((thr + d) << 8) | low), d >= 0) for d, low in ((-1, 0xFF), (0, 0x00), (1, 0x5A))]


@pytest.mark.parametrize('p', PS)
def test_threshold_is_the_fp32_one(p):
    """Fails on the parent for p = 0.3, 0.6, 0.8 (twin 5033164, 10066329, 13421772)."""
    assert fp32_threshold(p) == KERNEL_THR[p]
    assert Tx.drop_threshold(p) == KERNEL_THR[p]
    # the same through numpy-free torch fp32 arithmetic
    assert int((torch.tensor(p, dtype=torch.float32) * torch.tensor(16777216.0)).item()) == KERNEL_THR[p]


def test_solver_known_vector_and_twin_hash():
    assert solve_salt(7, 37, (5033164 << 8) | 0x5A) == 408643380
    g = torch.Generator().manual_seed(0)
    for _ in range(50):
        seed, i, t = torch.randint(0, 1 << 32, (3,), generator=g, dtype=torch.int64).tolist()
        salt = solve_salt(seed, i, t)
        assert int(Tx._hash(seed, salt, torch.tensor([i], dtype=torch.int64))[0]) == t


@pytest.mark.parametrize('p', PS)
def test_keep_mask_at_the_boundary(p):
    seed, shape = 7, (5, 12)
    for i in (0, 37, 59):
        for salt, kept in placements(p, seed, i):
            m = Tx.keep_mask(shape, p, seed, salt).reshape(-1)
            assert bool(m[i]) is kept, (p, i, salt)


@pytest.mark.parametrize('p', PS)
def test_cpu_paths_at_the_boundary(p):
    """Tx.dropout, both dropout sites of Tx.ln_fwd and Tx.softmax_fwd on the CPU: element i is
    zero exactly when its hash is below the fp32 threshold."""
    T, H, i = 3, 8, 13
    seed = torch.tensor([11], dtype=torch.int32)
    ones = torch.ones(T, H, dtype=torch.bfloat16)
    zeros = torch.zeros(T, H, dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, H, generator=g).to(torch.bfloat16)
    gamma, beta = torch.ones(H), torch.full((H,), 10.0)       # |LN| <= sqrt(H) < 10: y != 0 unless dropped
    for salt, kept in placements(p, 11, i):
        y = Tx.dropout(ones, p, seed, salt).reshape(-1)
        assert (y[i].item() != 0) is kept, ('dropout', p, salt)
        # residual site: s = 0 + dropout_in(1)
        _, s, _, _ = Tx.ln_fwd(zeros, ones, gamma, beta, 1e-12, p_in=p, seed=seed, salt_in=salt, salt_out=salt ^ 1)
        assert (s.reshape(-1)[i].item() != 0) is kept, ('ln_fwd in', p, salt)
        # output site
        y, _, _, _ = Tx.ln_fwd(x, None, gamma, beta, 1e-12, p_out=p, seed=seed, salt_in=salt ^ 1, salt_out=salt)
        assert (y.reshape(-1)[i].item() != 0) is kept, ('ln_fwd out', p, salt)
        P, Pd = Tx.softmax_fwd(x, None, T, 1.0, p, seed, salt)
        assert bool((P > 0).all())
        assert (Pd.reshape(-1)[i].item() != 0) is kept, ('softmax_fwd', p, salt)


def test_seq_keep_uses_the_same_threshold():
    """the packed-attention twin: element (h, q, k) of sequence b at its padded-layout index"""
    b, H, L, max_len, p, seed = 1, 2, 5, 8, 0.3, 3
    h, q, k = 1, 4, 2
    idx = ((b * H + h) * max_len + q) * max_len + k
    for salt, kept in placements(p, seed, idx):
        assert bool(Tx._seq_keep(b, H, L, max_len, p, seed, salt)[h, q, k]) is kept
