"""Bit-exact attention cases (a helper, not a test module): inputs for which every correct evaluation order of
softmax(q k^T / sqrt(dh) + mask) v gives the same bits, with the expected output stated in closed form.

  uniform   q = 0, so every unmasked key has score 0 and weight exactly 1 / n; n, the number of unmasked keys, is a power of
            two; v holds multiples of 1/8 with |v| <= 8, so the sum of up to 256 rows is exact in fp32 and the division by n
            is a shift.  Expected: the mean of the unmasked v rows.
  one-hot   keys are +-64 sign vectors: position p of key j carries bit (p mod 8) of j, so the unmasked keys are distinct and,
            from dh 16 on, differ in two positions at least.  q_i equals its target key: the target's scaled score exceeds every
            other unmasked key's by 2 * 2 * 4096 / sqrt(dh) >= 2,000 (dh 8: one position, 2,896), whose weight exp(-2000) is exactly
            0 in fp32 while the target's is exp(0) = 1.  Every masked position holds a copy of a target's key with another v.
            v holds integers of at most 8 significant bits.  Expected: v[target].  Targets: the first and the last unmasked
            key and one key of every 32-block that has one.

All values are exact in float16 and bfloat16 as well, so the same arrays serve the three dtypes; the expected output of a
16-bit call is the expected value rounded once (it is representable: nothing is lost).  Mask rows are the four patterns with a
token of tests/contextualize_reference.py ("none" has no softmax to speak of)."""
import numpy as np

from tests import contextualize_reference as CR

PATTERNS = ("full", "prefix", "front", "holes")


def _pow2_tokens(m):
    """the mask row with only its first 2^k tokens kept, 2^k the largest power of two within the row's token count"""
    idx = np.flatnonzero(m)
    n = 1 << (len(idx).bit_length() - 1)
    out = np.zeros_like(m)
    out[idx[:n]] = 1
    return out, n


def uniform(L, H, dh, seed=0):
    """(qkv [4, L, 3E] float32, mask [4, L] float32, expected [4, L, E] float64)"""
    rng = np.random.default_rng([seed, L, H, dh, 1])
    E, B = H * dh, len(PATTERNS)
    qkv = np.zeros((B, L, 3 * E), dtype=np.float32)
    qkv[:, :, E:2 * E] = rng.integers(-16, 17, (B, L, E)) / 4.0                 # any finite k: 0 . k = 0
    qkv[:, :, 2 * E:] = rng.integers(-64, 65, (B, L, E)) / 8.0
    mask = np.zeros((B, L), dtype=np.float32)
    want = np.zeros((B, L, E), dtype=np.float64)
    for b, name in enumerate(PATTERNS):
        mask[b], n = _pow2_tokens(CR.mask_pattern(name, L))
        want[b] = qkv[b, mask[b] != 0, 2 * E:].astype(np.float64).sum(0) / n
    return qkv, mask, want


def sign_key(j, dh):
    """the +-64 sign vector of key j: position p carries bit (p mod 8) of j"""
    p = np.arange(dh)
    return np.where((j >> (p % 8)) & 1, 64.0, -64.0).astype(np.float32)


def targets(m):
    """the target keys of a mask row: first and last unmasked key, and the first unmasked key of every 32-block"""
    idx = np.flatnonzero(m)
    t = [int(idx[0]), int(idx[-1])]
    for blk in range(0, len(m), 32):
        inside = idx[(idx >= blk) & (idx < blk + 32)]
        if len(inside):
            t.append(int(inside[len(inside) // 2]))
    return t


def one_hot(L, H, dh, seed=0):
    """(qkv [4, L, 3E] float32, mask [4, L] float32, expected [4, L, E] float64, target [4, L] int); dh >= 8, L <= 256"""
    assert dh >= 8 and L <= 256
    rng = np.random.default_rng([seed, L, H, dh, 2])
    E, B = H * dh, len(PATTERNS)
    qkv = np.zeros((B, L, 3 * E), dtype=np.float32)
    qkv[:, :, 2 * E:] = rng.integers(-255, 256, (B, L, E))
    mask = np.stack([CR.mask_pattern(name, L) for name in PATTERNS])
    tgt = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        T = targets(mask[b])
        live = np.flatnonzero(mask[b])
        key = np.stack([sign_key(j, dh) for j in range(L)])                      # [L, dh], distinct over j < 256
        for n, j in enumerate(np.flatnonzero(mask[b] == 0)):                     # masked positions: copies of target keys
            key[j] = key[T[n % len(T)]]
        gap = min((2 * 4096 * np.count_nonzero(key[a] != key[c]) / np.sqrt(dh) for a in T for c in live if c != a), default=np.inf)
        assert gap >= 2000, (L, dh, gap)
        for h in range(H):
            qkv[b, :, E + h * dh:E + (h + 1) * dh] = key
        for i in range(L):
            tgt[b, i] = T[(i + b) % len(T)]
            for h in range(H):
                qkv[b, i, h * dh:(h + 1) * dh] = key[tgt[b, i]]
    want = np.stack([qkv[b, tgt[b], 2 * E:] for b in range(B)]).astype(np.float64)
    return qkv, mask, want, tgt
