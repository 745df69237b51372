"""GPU tests of the device-side ColBERT store writer (mm_store_append / ops.store_append / TokenStoreWriter): bit equality with
the numpy restatement of the reference's encode loop (tests/store_writer_reference.py) over shapes around the 64-row word,
the fp8 output against the restated quantiser and against ops.fp8_quantize_rows, chaining through the device-side fill,
the capacity rule, the refusals, graph capture, and retrieval over a store the writer built."""
import numpy as np
import pytest
import torch

from tests import fp8_store_reference as R8
from tests import store_writer_reference as W
from tests import util

pytestmark = pytest.mark.gpu

DS = [1, 63, 64, 65, 200]
NDOCS = [1, 2, 65, 513]
OUTS = {torch.float16: [torch.float16, torch.float32], torch.bfloat16: [torch.bfloat16, torch.float32],
        torch.float32: [torch.float32, torch.float16, torch.bfloat16]}
PATTERN = 0x5A


class _Dev:
    """The five buffers of a store on the device: rows / codes / scales with `slack` rows beyond the capacity passed to the
    call, every byte set to PATTERN; fill and status zero; a document table of -7."""

    def __init__(self, dev, capacity, E, out_dtype=None, fp8=False, n_docs=0, slack=64):
        self.dev, self.capacity, self.E = dev, capacity, E
        n = capacity + slack
        self.rows = torch.full((n, E), PATTERN, dtype=torch.uint8, device=dev).repeat(1, out_dtype.itemsize).view(out_dtype) \
            if out_dtype is not None else None
        self.codes = torch.full((n, E), PATTERN, dtype=torch.uint8, device=dev) if fp8 else None
        self.scales = torch.full((n * 4,), PATTERN, dtype=torch.uint8, device=dev).view(torch.float32) if fp8 else None
        self.fill = torch.zeros(1, dtype=torch.int64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.begin = torch.full((n_docs,), -7, dtype=torch.int64, device=dev)
        self.end = torch.full((n_docs,), -7, dtype=torch.int64, device=dev)

    def append(self, x, at=0, keep_zero_rows=False, capacity=None):
        from matchmaker_amd import ops
        n = x.shape[0]
        ops.store_append(x, self.rows, self.codes, self.scales, self.capacity if capacity is None else capacity, self.fill,
                         self.begin[at: at + n], self.end[at: at + n], self.status, keep_zero_rows=keep_zero_rows)

    def snapshot(self):
        return [None if t is None else t.clone() for t in (self.rows, self.codes, self.scales, self.fill, self.status, self.begin, self.end)]

    def unchanged_since(self, snap):
        now = (self.rows, self.codes, self.scales, self.fill, self.status, self.begin, self.end)
        return all(a is None or torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(now, snap))

    def tail_is_pattern(self, fill):
        return all(t is None or bool((t[fill:].contiguous().view(torch.uint8) == PATTERN).all()) for t in (self.rows, self.codes, self.scales))


def _want_rows(rows, out_dtype):
    """The kept rows as the store holds them: the bits, or torch's cast (= numpy's, the reference's `token_base[a:b] = reps`)."""
    return rows if rows.dtype == out_dtype else rows.to(out_dtype)


# ------------------------------------------------------------------------------------------ bit equality with the restatement
@pytest.mark.parametrize("dtype, E", [(dt, E) for dt in OUTS for E in ([4] if dt == torch.float32 else []) + [8, 48, 128, 768]])
def test_rows_ranges_and_fill_equal_the_restatement(dtype, E):
    """Every D in {1, 63, 64, 65, 200} x n_docs in {1, 2, 65, 513} for this (dtype, E), every allowed out_dtype, the row
    patterns of pattern_batch (fully live, all zero, only the last row live, a zero row between live rows, one subnormal,
    a row of -0.0) rotated through the documents; and two runs give the same bits."""
    dev = util.require_gpu()
    for si, (D, n_docs) in enumerate((D, n) for D in DS for n in NDOCS):
        x = W.pattern_batch(n_docs, D, E, dtype, seed=100 + si, shift=si)
        rows, begin, end = W.append_batches([(x, False)], fill0=0)
        T = int(end[-1])
        xd = x.to(dev)
        for out_dtype in OUTS[dtype]:
            st = _Dev(dev, T, E, out_dtype, n_docs=n_docs)                 # an exact fit
            st.append(xd)
            what = f"D={D} n_docs={n_docs} {dtype}->{out_dtype}"
            assert int(st.fill) == T and int(st.status) == 0, what
            assert np.array_equal(st.begin.cpu().numpy(), begin) and np.array_equal(st.end.cpu().numpy(), end), what
            want = _want_rows(rows, out_dtype).to(dev)
            assert torch.equal(W.bits(st.rows[:T]), W.bits(want)), what
            assert st.tail_is_pattern(T), what
            if out_dtype == dtype:                                         # a second run, into a second store: the same bits
                st2 = _Dev(dev, T, E, out_dtype, n_docs=n_docs)
                st2.append(xd)
                assert torch.equal(W.bits(st2.rows), W.bits(st.rows)) and torch.equal(st2.begin, st.begin) and torch.equal(st2.end, st.end)


@pytest.mark.parametrize("dtype", list(OUTS))
def test_a_whole_batch_of_zeros_and_keep_zero_rows(dtype):
    dev = util.require_gpu()
    E = 48 if dtype != torch.float32 else 4
    z = torch.zeros(65, 63, E, dtype=dtype)
    z[3, 5] = torch.tensor(-0.0, dtype=dtype)
    st = _Dev(dev, 100, E, dtype, n_docs=65)
    st.fill.fill_(17)
    st.append(z.to(dev))
    assert int(st.fill) == 17 and int(st.status) == 0 and st.tail_is_pattern(0)
    assert bool((st.begin == 17).all()) and bool((st.end == 17).all())     # 65 empty ranges at the fill
    # [B, E] input of the writer = D = 1 with every row kept, the zero ones too
    v = W.pattern_batch(130, 1, E, dtype, seed=3)
    rows, begin, end = W.append_batches([(v, True)], fill0=17)
    assert rows.shape[0] == 130 and bool((v.abs().sum((1, 2)) == 0).any())
    st = _Dev(dev, 147, E, dtype, n_docs=130)
    st.fill.fill_(17)
    st.append(v.to(dev), keep_zero_rows=True)
    assert int(st.fill) == 147 and torch.equal(W.bits(st.rows[17:147]), W.bits(rows.to(dev)))
    assert np.array_equal(st.begin.cpu().numpy(), begin) and np.array_equal(st.end.cpu().numpy(), end)
    assert bool((st.rows[:17].contiguous().view(torch.uint8) == PATTERN).all()) and st.tail_is_pattern(147)


# ------------------------------------------------------------------------------------------ fp8 output
@pytest.mark.parametrize("dtype", list(OUTS))
@pytest.mark.parametrize("E", [16, 128, 768])
def test_fp8_output_equals_the_restated_quantiser_and_the_native_one(dtype, E):
    """special_rows (mixed magnitudes, a zero row, -0.0 elements, a row that underflows fp16, exact powers of two) as 37
    documents of 29 rows with every fifth row zeroed: codes (zeros folded) and scales equal quantize_torch of the
    restatement's kept rows; with both outputs requested they equal ops.fp8_quantize_rows of the rows written, bit for bit;
    and the fp8-only call writes the same codes."""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    n_docs, D = 37, 29
    x = R8.special_rows(n_docs * D, E, dtype, seed=E + 1).view(n_docs, D, E).clone()
    x[:, ::5] = 0
    x[7] = 0
    rows, begin, end = W.append_batches([(x, False)])
    T = int(end[-1])
    both = _Dev(dev, T, E, dtype, fp8=True, n_docs=n_docs)
    both.append(x.to(dev))
    only = _Dev(dev, T, E, None, fp8=True, n_docs=n_docs)
    only.append(x.to(dev))
    for st in (both, only):
        assert int(st.fill) == T and int(st.status) == 0 and st.tail_is_pattern(T)
        assert np.array_equal(st.begin.cpu().numpy(), begin) and np.array_equal(st.end.cpu().numpy(), end)
    c, s = R8.quantize_torch(rows)
    assert torch.equal(R8.fold_zero(both.codes[:T].cpu()), R8.fold_zero(c)) and torch.equal(both.scales[:T].cpu(), s)
    assert torch.equal(W.bits(both.rows[:T]), W.bits(rows.to(dev)))
    cn, sn = ops.fp8_quantize_rows(both.rows[:T].contiguous())
    assert torch.equal(both.codes[:T], cn) and torch.equal(W.bits(both.scales[:T]), W.bits(sn))
    assert torch.equal(only.codes, both.codes) and torch.equal(W.bits(only.scales), W.bits(both.scales))


# ------------------------------------------------------------------------------------------ chaining
@pytest.mark.parametrize("dtype, out_dtype", [(torch.float16, torch.float16), (torch.float32, torch.bfloat16)])
def test_three_appends_chain_through_the_device_side_fill(dtype, out_dtype):
    dev = util.require_gpu()
    E = 128
    xs = [W.pattern_batch(65, 63, E, dtype, seed=1, shift=2), W.pattern_batch(2, 200, E, dtype, seed=2, shift=6),
          W.pattern_batch(130, 1, E, dtype, seed=3)]
    rows, begin, end = W.append_batches([(x, False) for x in xs])
    T = int(end[-1])
    st = _Dev(dev, T, E, out_dtype, fp8=True, n_docs=197)
    xd = [x.to(dev) for x in xs]
    torch.cuda.synchronize()
    at = 0
    for x in xd:                                                           # nothing reads back between the three
        st.append(x, at=at)
        at += x.shape[0]
    assert int(st.fill) == T and int(st.status) == 0
    assert np.array_equal(st.begin.cpu().numpy(), begin) and np.array_equal(st.end.cpu().numpy(), end)
    assert torch.equal(W.bits(st.rows[:T]), W.bits(_want_rows(rows, out_dtype).to(dev))) and st.tail_is_pattern(T)
    c, s = R8.quantize_torch(rows)
    assert torch.equal(R8.fold_zero(st.codes[:T].cpu()), R8.fold_zero(c)) and torch.equal(st.scales[:T].cpu(), s)


# ------------------------------------------------------------------------------------------ capacity
def test_capacity_is_all_or_nothing_and_the_status_is_sticky():
    dev = util.require_gpu()
    E, dtype = 128, torch.float16
    a = W.pattern_batch(65, 64, E, dtype, seed=4, shift=1)
    b = W.pattern_batch(5, 65, E, dtype, seed=5)
    small = W.pattern_batch(1, 1, E, dtype, seed=6)
    ka, kb = int(W.keep_mask(a).sum()), int(W.keep_mask(b).sum())
    rows, begin, end = W.append_batches([(a, False), (b, False)])
    ad, bd, sd = a.to(dev), b.to(dev), small.to(dev)
    # an exact fit: fill == capacity, the 64 rows beyond it untouched
    st = _Dev(dev, ka + kb, E, dtype, fp8=True, n_docs=71)
    st.append(ad)
    assert int(st.fill) == ka and st.tail_is_pattern(ka)
    st.append(bd, at=65)
    assert int(st.fill) == ka + kb == st.capacity and int(st.status) == 0 and st.tail_is_pattern(ka + kb)
    assert torch.equal(W.bits(st.rows[: ka + kb]), W.bits(rows.to(dev)))
    assert np.array_equal(st.begin[:70].cpu().numpy(), begin) and np.array_equal(st.end[:70].cpu().numpy(), end)
    # one row too many: nothing changes but the status
    st = _Dev(dev, ka + kb - 1, E, dtype, fp8=True, n_docs=71)
    st.append(ad)
    snap = st.snapshot()
    st.append(bd, at=65)
    assert int(st.status) == 1
    snap[4] = st.status.clone()
    assert st.unchanged_since(snap) and int(st.fill) == ka and st.tail_is_pattern(ka)
    # sticky: an append that would fit is a no-op now
    st.append(sd, at=70)
    assert st.unchanged_since(snap) and int(st.begin[70]) == -7


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_carry_their_codes_and_write_nothing():
    from matchmaker_amd import NativeError, _lib, ops
    dev = util.require_gpu()
    z = lambda *s, dtype=torch.float16: torch.zeros(*s, dtype=dtype, device=dev)      # noqa: E731

    def refused(code, x, st, rows="rows", fp8=False, **kw):
        snap = st.snapshot()
        with pytest.raises(NativeError) as ei:
            ops.store_append(x, st.rows if rows == "rows" else rows, st.codes if fp8 else None, st.scales if fp8 else None,
                             st.capacity, st.fill, st.begin, st.end, st.status, **kw)
        torch.cuda.synchronize()
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert st.unchanged_since(snap)

    st = _Dev(dev, 50, 12, torch.float16, n_docs=3)
    refused(_lib.MM_EUNSUPPORTED, z(3, 4, 12) + 1, st)                     # 24-byte rows
    st = _Dev(dev, 50, 24, torch.float16, fp8=True, n_docs=3)
    refused(_lib.MM_EUNSUPPORTED, z(3, 4, 24) + 1, st, fp8=True)           # fp8 wants E % 16 == 0 (48-byte rows are fine for 16-bit)
    st = _Dev(dev, 50, 16, torch.bfloat16, n_docs=3)
    refused(_lib.MM_EUNSUPPORTED, z(3, 4, 16) + 1, st)                     # fp16 -> bf16
    st = _Dev(dev, 50, 16, torch.float16, n_docs=3)
    refused(_lib.MM_EINVAL, z(3, 4, 16) + 1, st, rows=None)                # neither output
    # the C entry point itself: the same codes before any launch, and a workspace one byte short
    L = _lib.lib()
    x = z(3, 4, 16) + 1
    need = L.mm_store_append_workspace_bytes(3, 4)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    snap = st.snapshot()

    def raw(rows=st.rows.data_ptr(), out=_lib.MM_F16, E=16, dtype=_lib.MM_F16, codes=None, scales=None, wsb=need):
        return L.mm_store_append(x.data_ptr(), 3, 4, E, dtype, 0, rows, out, codes, scales, st.capacity, st.fill.data_ptr(),
                                 st.begin.data_ptr(), st.end.data_ptr(), st.status.data_ptr(), ws.data_ptr(), wsb, None)

    assert raw(wsb=need - 1) == _lib.MM_EWORKSPACE
    assert raw(E=12) == _lib.MM_EUNSUPPORTED and raw(out=_lib.MM_BF16) == _lib.MM_EUNSUPPORTED
    assert raw(E=24, codes=ws.data_ptr(), scales=ws.data_ptr()) == _lib.MM_EUNSUPPORTED
    assert raw(rows=None) == _lib.MM_EINVAL
    torch.cuda.synchronize()
    assert st.unchanged_since(snap) and not bool(ws.any())
    assert raw() == _lib.MM_OK                                             # (the same arguments with nothing wrong do append)
    torch.cuda.synchronize()
    assert int(st.fill) == 12 and st.end.tolist() == [4, 8, 12]


# ------------------------------------------------------------------------------------------ graph
def test_two_appends_replay_from_one_captured_graph():
    dev = util.require_gpu()
    E, dtype = 128, torch.bfloat16
    xs = [W.pattern_batch(65, 65, E, dtype, seed=7, shift=4), W.pattern_batch(9, 200, E, dtype, seed=8, shift=2)]
    rows, begin, end = W.append_batches([(x, False) for x in xs] * 2)
    T = int(end[-1])
    xd = [x.to(dev) for x in xs]
    warm = _Dev(dev, T, E, dtype, fp8=True, n_docs=74)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                                          # warm-up on a side stream (lazy code-object loading)
        warm.append(xd[0])
        warm.append(xd[1], at=65)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    st = _Dev(dev, T, E, dtype, fp8=True, n_docs=74)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.append(xd[0])
        st.append(xd[1], at=65)
    torch.cuda.synchronize()
    assert int(st.fill) == 0 and st.tail_is_pattern(0)                     # captured, not run
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert int(st.fill) == T and int(st.status) == 0 and st.tail_is_pattern(T)
    assert torch.equal(W.bits(st.rows[:T]), W.bits(rows.to(dev)))          # the two batches, twice
    c, s = R8.quantize_torch(rows)
    assert torch.equal(R8.fold_zero(st.codes[:T].cpu()), R8.fold_zero(c)) and torch.equal(st.scales[:T].cpu(), s)
    # the captured calls write one slice of the document table: it holds the second replay's ranges
    assert np.array_equal(st.begin.cpu().numpy(), begin[74:]) and np.array_equal(st.end.cpu().numpy(), end[74:])


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("fp8", [False, True])
def test_search_over_a_written_store_equals_the_reference_parts_store(fp8):
    from matchmaker_amd.encode import encode_collection
    from matchmaker_amd.token_store import TokenStore, TokenStoreWriter
    dev = util.require_gpu()
    E, D = 128, 48
    rng = np.random.default_rng(21)
    lens = rng.integers(0, D + 1, 40)
    lens[3] = 0
    vecs = rng.standard_normal((40, D, E)).astype(np.float32)
    vecs /= np.linalg.norm(vecs, axis=2, keepdims=True)
    vecs[np.arange(D)[None, :] >= lens[:, None]] = 0                       # the model's mask
    x = torch.from_numpy(vecs).half()
    ids = [f"doc{i}" for i in range(40)]

    class _Model:
        def forward_representation(self, seq, sequence_type=None):
            assert sequence_type == "doc_encode"
            return seq["vecs"]

    batches = [{"seq_tokens": {"vecs": x[a: a + 16].to(dev)}, "seq_id": ids[a: a + 16]} for a in (0, 16, 32)]
    w = TokenStoreWriter(40 * D, E, dtype=torch.float16, device=dev, fp8=fp8)
    assert encode_collection(_Model(), batches, w) == 40
    store = w.finish()
    rows, begin, end = W.append_batches([(x, False)])
    assert np.array_equal(end - begin, lens)
    want = TokenStore.from_reference_parts([rows.numpy()], {s: (0, int(a), int(b)) for s, a, b in zip(ids, begin, end)}, ids, dev, fp8=fp8)
    assert store.seq_ids == want.seq_ids and np.array_equal(store._begin, want._begin) and np.array_equal(store._end, want._end)
    if fp8:
        assert torch.equal(store.codes, want.codes) and torch.equal(W.bits(store.scales), W.bits(want.scales))
    else:
        assert torch.equal(W.bits(store.tokens), W.bits(want.tokens))
    q = rng.standard_normal((5, 32, E)).astype(np.float32)
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    q = torch.from_numpy(q).to(dev)
    kw = {"token_search": "fp8"} if fp8 else {}
    got, ref = store.search(q, 10, 8, **kw), want.search(q, 10, 8, **kw)
    assert got == ref and all(len(r) == 10 for r in got)
