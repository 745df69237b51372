"""Restatement of the fp8 ColBERT token store (include/mm_native.h): row quantiser, dequantiser, ragged MaxSim.

Format: codes [T, E] uint8 = OCP e4m3fn bytes, scales [T] float32 = one power of two per row.  For a row x (float32 values)
with a = max_k |x_k|:
    s      = 2^clamp(floor(log2 a) - 7, -126, 120), or 1.0 when a == 0
    code_k = RNE_e4m3fn(x_k * (1 / s))
and the row's value is deq(code_k) * s.  The torch form is the one-line cast; the numpy form encodes e4m3fn by hand (numpy has
no such type), so the two check each other.  The MaxSim is computed in float64:
    out[p] = sum_{i, q_mask} max_{t in [begin_p, end_p)} ( scales[t] * sum_k q[i,k] * deq(codes[t,k]) )
with -1000 per live query token for an empty range, and the MM_SIM_ROUND / MM_SUM_ROUND roundings to the query's 16-bit type.
"""
import numpy as np
import torch

SIM_ROUND, SUM_ROUND = 1, 2
U_OUT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


# ------------------------------------------------------------------------------------------ quantiser
def scale_exponent_torch(x: torch.Tensor) -> torch.Tensor:
    """k [T] int32 with s = 2^k, from the float32 values of x [T, E]."""
    a = x.float().abs().amax(dim=1)
    _, e = torch.frexp(a)                              # a = m 2^e with m in [0.5, 1): floor(log2 a) = e - 1
    k = (e - 1 - 7).clamp(-126, 120)
    return torch.where(a == 0, torch.zeros_like(k), k)


def quantize_torch(x: torch.Tensor):
    """(codes [T, E] uint8, scales [T] float32) of x [T, E] (any float dtype, CPU)."""
    k = scale_exponent_torch(x)
    one = torch.ones(x.shape[0], dtype=torch.float32)
    s, inv = torch.ldexp(one, k), torch.ldexp(one, -k)
    codes = (x.float() * inv[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, s


def encode_e4m3fn_numpy(v: np.ndarray) -> np.ndarray:
    """RNE to OCP e4m3fn, by hand, for |v| < 256 (the quantiser's range): uint8 codes."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)
    assert (a < 256).all()
    sign = np.where(np.signbit(v), 0x80, 0).astype(np.int64)
    code = np.zeros(v.shape, dtype=np.int64)
    sub = a < 2.0 ** -6                                 # below the smallest normal: steps of 2^-9 (8 steps reach 2^-6 = code 0x08)
    code[sub] = np.rint(a[sub] * 2.0 ** 9).astype(np.int64)
    n = ~sub
    e = np.floor(np.log2(a[n])).astype(np.int64)
    m = np.rint((a[n] / 2.0 ** e - 1.0) * 8).astype(np.int64)          # np.rint rounds half to even
    e, m = np.where(m == 8, e + 1, e), np.where(m == 8, 0, m)
    code[n] = ((e + 7) << 3) | m
    return (code | sign).astype(np.uint8)


def quantize_numpy(x: np.ndarray):
    """The same quantiser on a float32 array, in numpy."""
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(x).max(axis=1)
    _, e = np.frexp(a)
    k = np.clip(e.astype(np.int64) - 1 - 7, -126, 120)
    k = np.where(a == 0, 0, k)
    s = np.ldexp(np.float32(1), k).astype(np.float32)
    inv = np.ldexp(np.float32(1), -k).astype(np.float32)
    return encode_e4m3fn_numpy(x * inv[:, None]), s


def fold_zero(codes):
    """Both zeros are one value: 0x80 -> 0x00."""
    if isinstance(codes, torch.Tensor):
        return torch.where(codes == 0x80, torch.zeros_like(codes), codes)
    return np.where(codes == 0x80, 0, codes).astype(np.uint8)


# ------------------------------------------------------------------------------------------ dequantiser
def _table():
    t = np.zeros(256, dtype=np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        v = m * 2.0 ** -9 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
        if e == 15 and m == 7:
            v = np.nan
        t[c] = -v if c & 0x80 else v
    return t


E4M3 = _table()


def deq_numpy(codes: np.ndarray) -> np.ndarray:
    """float64 values of the codes (no scale)."""
    return E4M3[np.asarray(codes, dtype=np.uint8)]


def dequantize_numpy(codes: np.ndarray, scales: np.ndarray) -> np.ndarray:
    return deq_numpy(codes) * np.asarray(scales, dtype=np.float64)[:, None]


def dequantize_torch(codes: torch.Tensor, scales: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    return (codes.view(torch.float8_e4m3fn).float() * scales.float()[:, None]).to(dtype)


# ------------------------------------------------------------------------------------------ MaxSim
def _round_to(v: np.ndarray, dtype) -> np.ndarray:
    """float64 -> float32 -> the 16-bit type -> float64, as the kernel rounds its fp32 values."""
    return torch.from_numpy(np.asarray(v, dtype=np.float64)).float().to(dtype).double().numpy()


def _token_maxima(q, codes, scales, doc_begin, doc_end, pairs_per_query):
    """Yields (pair, maxima [Q] float64 or None for an empty range, magnitudes [Q] = max_t s_t sum_k |q_ik| |deq_tk|)."""
    q64 = np.asarray(q, dtype=np.float64)
    for p, (b, e) in enumerate(zip(doc_begin, doc_end)):
        qi = q64[p // pairs_per_query]
        if e <= b:
            yield p, None, np.zeros(qi.shape[0])
            continue
        d = deq_numpy(codes[b:e])
        s = np.asarray(scales[b:e], dtype=np.float64)[:, None]
        sims = (d @ qi.T) * s                                             # [n, Q]
        mags = (np.abs(d) @ np.abs(qi).T) * s
        yield p, sims.max(axis=0), mags.max(axis=0)


def maxsim_ragged_fp8_ref(q, codes, scales, doc_begin, doc_end, q_mask=None, pairs_per_query=1, flags=0, q_dtype=torch.bfloat16):
    """float64 [n_pairs].  q [nq, Q, E] float array holding the 16-bit values; q_mask [nq, Q] bool or None."""
    out = np.zeros(len(doc_begin), dtype=np.float64)
    for p, mx, _ in _token_maxima(q, codes, scales, doc_begin, doc_end, pairs_per_query):
        if mx is None:
            mx = np.full(np.asarray(q).shape[1], -1000.0)
        if flags & SIM_ROUND:
            mx = _round_to(mx, q_dtype)
        live = np.ones(mx.shape[0], dtype=bool) if q_mask is None else np.asarray(q_mask[p // pairs_per_query], dtype=bool)
        total = mx[live].sum()
        out[p] = _round_to(total, q_dtype) if flags & SUM_ROUND else total
    return out


def bound(q, codes, scales, doc_begin, doc_end, ref, q_mask=None, pairs_per_query=1, flags=0, q_dtype=torch.bfloat16):
    """Per pair (E + Q + 2) 2^-24 sum_i max_t s_t sum_k |q_ik| |deq_tk|  (+ u_out |ref| when a flag rounds): the project's
    (n + 2) 2^-24 sum |terms| form — E fp32 additions per similarity (the products and the scale are exact), Q per sum."""
    Q, E = np.asarray(q).shape[1], np.asarray(q).shape[2]
    out = np.zeros(len(doc_begin), dtype=np.float64)
    for p, _, mags in _token_maxima(q, codes, scales, doc_begin, doc_end, pairs_per_query):
        live = np.ones(Q, dtype=bool) if q_mask is None else np.asarray(q_mask[p // pairs_per_query], dtype=bool)
        out[p] = (E + Q + 2) * 2.0 ** -24 * mags[live].sum()
    if flags:
        out = out + U_OUT[q_dtype] * np.abs(ref)
    return out


# ------------------------------------------------------------------------------------------ shared inputs
def special_rows(T, E, dtype, seed):
    """x [T, E] of `dtype` (CPU): seeded rows of mixed magnitude, and — where T allows — a zero row, a row with -0.0
    elements, a row scaled by 1e-30 (it underflows to zeros in fp16), a row whose maximum is an exact power of two and one
    just below it."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, E, generator=g) * torch.exp2(torch.randint(-12, 8, (T, 1), generator=g).float())
    if T > 1:
        x[1] = 0
    if T > 2:
        x[2, ::2] = -0.0
    if T > 3:
        x[3] *= 1e-30
    if T > 4:
        x[4] = x[4].clamp(-1, 1)
        x[4, 0] = 1.0
    if T > 5:
        x[5] = x[5].clamp(-0.9, 0.9)
        x[5, E - 1] = -0.998046875                       # 1 - 2^-9: bf16 rounds it to -1.0, fp16 / fp32 keep it
    return x.to(dtype)


EXACT_LENS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]


def exact_case(Q, E, pairs_per_query, seed):
    """Exactly representable arithmetic: codes = integers in -8..8, scales 2^k with k in -3..3, q integers in -2..2 — every
    similarity is an integer multiple of 1/8 below 2^18 and every sum of Q of them stays below 2^24 / 8: exact in fp32 in any
    order.  12 documents of the lengths EXACT_LENS tile the store (the last one ends at row T) and are scored in a shuffled
    order; with pairs_per_query = 7 the second query is short (5 pairs)."""
    rng = np.random.default_rng(seed)
    lens = np.array(EXACT_LENS)[rng.permutation(len(EXACT_LENS))]
    if lens[-1] == 0:                                    # the document that ends at row T holds rows
        lens[[0, -1]] = lens[[-1, 0]]
    end = np.cumsum(lens).astype(np.int64)
    begin = end - lens
    T = int(end[-1])
    vals = rng.integers(-8, 9, (T, E)).astype(np.float32)
    codes = torch.from_numpy(vals).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(deq_numpy(codes), vals)
    scales = np.ldexp(np.float32(1), rng.integers(-3, 4, T)).astype(np.float32)
    order = rng.permutation(len(lens))                   # (the document that ends at row T is scored wherever this puts it)
    n_pairs = len(lens)
    nq = (n_pairs + pairs_per_query - 1) // pairs_per_query
    q = rng.integers(-2, 3, (nq, Q, E)).astype(np.float32)
    mask = np.ones((nq, Q), dtype=bool)
    mask[:, Q // 2] = False                              # a hole (Q = 1: every token masked, the score is 0)
    if Q > 2:
        mask[0, Q - 1] = False
    return {"q": q, "codes": codes, "scales": scales, "begin": begin[order].copy(), "end": end[order].copy(), "T": T,
            "mask": mask, "n_pairs": n_pairs, "nq": nq}
