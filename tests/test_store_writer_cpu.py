"""CPU tests of the device-side ColBERT store writer: the C ABI declarations and the binding, the workspace size, and the host
logic of TokenStoreWriter / TokenStore.save_reference / encode_collection driven through a torch-CPU stand-in for the native
call (tests/store_writer_reference.py)."""
import os
import zipfile

import numpy as np
import pytest
import torch

from tests import fp8_store_reference as R8
from tests import store_writer_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ C ABI and binding
def test_header_binding_and_library_agree_on_the_two_entry_points():
    from matchmaker_amd import _lib, build
    from tests import abi
    L = abi.assert_bound(("mm_store_append_workspace_bytes", "mm_store_append"))
    hdr = open(os.path.join(ROOT, "include", "mm_native.h")).read()
    assert "dense_retrieval.py:232-265" in hdr and "#define MM_STORE_KEEP_ZERO_ROWS 1" in hdr and _lib.STORE_KEEP_ZERO_ROWS == 1
    assert "store_writer.hip" in build.SOURCES
    assert L.mm_abi_version() == 4 == _lib.ABI_VERSION


def test_one_copy_of_the_quantisers_row_code():
    csrc = os.path.join(ROOT, "matchmaker_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("fp8_device.h", "maxsim_fp8.hip", "store_writer.hip")}
    assert "void fp8_quantize_row(" in text["fp8_device.h"] and "__builtin_amdgcn_cvt_pk_fp8_f32" in text["fp8_device.h"]
    for f in ("maxsim_fp8.hip", "store_writer.hip"):
        assert "fp8_quantize_row<DT>(" in text[f] and "__builtin_amdgcn_cvt_pk_fp8_f32" not in text[f], f


def test_workspace_size_is_callable_without_a_gpu_and_monotone():
    from matchmaker_amd import _lib, build
    build.build()
    ws = _lib.lib().mm_store_append_workspace_bytes
    assert ws(0, 200) == 0 and ws(512, 200) > 0
    docs = [1, 2, 65, 513, 2048, 100000]
    Ds = [1, 63, 64, 65, 200, 512]
    for D in Ds:
        sizes = [ws(n, D) for n in docs]
        assert sizes == sorted(sizes) and sizes[0] > 0, (D, sizes)
    for n in docs:
        sizes = [ws(n, D) for D in Ds]
        assert sizes == sorted(sizes), (n, sizes)
    assert ws(2048, 200) < 2048 * 200                                      # 12 bytes per 64 rows and three 256-byte roundings


def test_host_refusals_of_the_entry_point_come_before_any_launch():
    from matchmaker_amd import _lib, build
    build.build()
    L = _lib.lib()
    p = 4096                                                               # any non-null aligned value: refused before it is used
    F16, BF16, F32 = _lib.MM_F16, _lib.MM_BF16, _lib.MM_F32

    def call(E=128, dtype=F16, flags=0, rows=p, out=F16, codes=None, scales=None, n_docs=4, ws=p, wsb=1 << 20):
        return L.mm_store_append(p, n_docs, 8, E, dtype, flags, rows, out, codes, scales, 100, p, p, p, p, ws, wsb, None)

    assert call(E=12) == _lib.MM_EUNSUPPORTED and b"16 bytes" in L.mm_last_error()
    assert call(E=24, codes=p, scales=p) == _lib.MM_EUNSUPPORTED and b"fp8" in L.mm_last_error()
    assert call(out=BF16) == _lib.MM_EUNSUPPORTED and call(dtype=BF16, out=F16) == _lib.MM_EUNSUPPORTED
    assert call(rows=None) == _lib.MM_EINVAL and b"neither" in L.mm_last_error()
    assert call(codes=p) == _lib.MM_EINVAL and call(flags=2) == _lib.MM_EINVAL and call(dtype=7) == _lib.MM_EINVAL
    need = L.mm_store_append_workspace_bytes(4, 8)
    assert call(wsb=need - 1) == _lib.MM_EWORKSPACE and call(ws=None, wsb=0) == _lib.MM_EWORKSPACE
    assert call(n_docs=0) == _lib.MM_OK                                    # succeeds and changes nothing
    assert L.mm_store_append(p, 1 << 16, 1 << 15, 8, F16, 0, p, F16, None, None, 100, p, p, p, p, p, 1 << 30, None) == _lib.MM_EUNSUPPORTED


def test_ops_store_append_restates_the_refusals():
    import matchmaker_amd
    from matchmaker_amd import ops, NativeError, _lib
    from matchmaker_amd.token_store import TokenStoreWriter
    assert matchmaker_amd.TokenStoreWriter is TokenStoreWriter
    from matchmaker_amd import torch_ops  # noqa: F401
    assert not hasattr(torch.ops.mm_native, "store_append")               # not a torch op: it mutates five caller buffers
    z64, z32 = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    b = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(NativeError, match="CPU"):
        ops.store_append(torch.zeros(2, 3, 8, dtype=torch.float16), torch.zeros(9, 8, dtype=torch.float16), None, None, 9, z64, b, b.clone(), z32)


# ------------------------------------------------------------------------------------------ TokenStoreWriter through the stand-in
class _CountedFill:
    """The writer's device-side fill with its read-backs counted."""

    def __init__(self, t):
        self.t, self.reads = t, 0

    def item(self):
        self.reads += 1
        return self.t.item()


class _StandIn:
    def __init__(self, refuse_from_call=None):
        self.calls, self.refuse_from_call = [], refuse_from_call

    def __call__(self, x, rows_out, codes_out, scales_out, capacity, fill, doc_begin, doc_end, status, keep_zero_rows=False):
        self.calls.append((tuple(x.shape), x.dtype, keep_zero_rows))
        if self.refuse_from_call is not None and len(self.calls) > self.refuse_from_call:
            capacity = int(fill.t[0])                                      # a device whose store is full from this call on
        W.append_standin(x, rows_out, codes_out, scales_out, capacity, fill.t, doc_begin, doc_end, status, keep_zero_rows)


def _writer(capacity, E, fn, **kw):
    from matchmaker_amd.token_store import TokenStoreWriter
    w = TokenStoreWriter(capacity, E, device="cpu", append_fn=fn, **kw)
    w._fill = _CountedFill(w._fill)
    return w


def _batches(E, dtype):
    """Three batches of different D (patterns of tests/store_writer_reference.pattern_batch: all-zero documents, holes,
    subnormals, -0.0 rows) and one [B, E] batch with a zero vector."""
    out = [(W.pattern_batch(9, 5, E, dtype, seed=1), False), (W.pattern_batch(4, 17, E, dtype, seed=2, shift=3), False),
           (W.pattern_batch(8, 1, E, dtype, seed=3, shift=1), False)]
    v = W.pattern_batch(1, 6, E, dtype, seed=4)[0]
    v[2] = 0
    return out, v


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fp8", [False, True])
def test_finish_equals_from_reference_parts_of_the_same_documents(dtype, fp8):
    from matchmaker_amd.token_store import TokenStore
    E = 16
    batches, vecs = _batches(E, dtype)
    fn = _StandIn()
    fns = {"quantize_fn": R8.quantize_torch}
    w = _writer(9 * 5 + 4 * 17 + 8 + 6, E, fn, dtype=dtype, fp8=fp8, **fns)
    ids, n = [], 0
    for x, _ in batches:
        sid = [f"d{n + i}" for i in range(x.shape[0])]
        w.append(sid, x)
        ids += sid
        n += x.shape[0]
    sid = [f"v{i}" for i in range(6)]
    w.append(sid, vecs)
    ids += sid
    assert fn.calls[-1] == ((6, 1, E), dtype, True) and [c[2] for c in fn.calls[:3]] == [False] * 3
    assert w._fill.reads == 0                                              # the bound fitted: nothing was read back
    store = w.finish()
    rows, begin, end = W.append_batches(batches + [(vecs.unsqueeze(1), True)])
    # the same documents as the reference's writer would have left them: one file, doc_infos = the ranges
    if dtype == torch.bfloat16:
        storage = [rows.float().numpy()]                                   # (numpy has no bf16: the values, exactly)
        want = TokenStore(rows, ids, begin, end) if not fp8 else None
    else:
        storage = [rows.numpy()]
        want = TokenStore.from_reference_parts(storage, {s: (0, int(a), int(b)) for s, a, b in zip(ids, begin, end)}, ids, "cpu",
                                               fp8=fp8, **fns)
    assert store.seq_ids == ids and np.array_equal(store._begin, begin) and np.array_equal(store._end, end)
    lens = end - begin
    assert lens[1] == 0 and lens[8] == 0 and lens[3] == 4 and lens[4] == 1 and lens[5] == 4      # empty documents, a hole, one subnormal row, a -0.0 row
    assert lens[-4] == 1 and bool((vecs[2] == 0).all())                    # [B, E]: the zero vector is kept
    if fp8:
        c, s = R8.quantize_torch(rows)
        assert store.is_fp8 and torch.equal(store.codes, c) and torch.equal(store.scales, s) and store._source_dtype == dtype
        if want is not None:
            assert torch.equal(want.codes, store.codes) and torch.equal(want.scales, store.scales)
            assert want._source_dtype == store._source_dtype
        with pytest.raises(Exception, match="keep_tokens=True"):
            store.tokens
    else:
        assert not store.is_fp8 and store.tokens.dtype == dtype and torch.equal(W.bits(store.tokens), W.bits(want.tokens))
    if want is not None:
        assert np.array_equal(want._begin, store._begin) and np.array_equal(want._end, store._end) and want.seq_ids == store.seq_ids
        assert torch.equal(want._begin_sorted, store._begin_sorted) and torch.equal(want._doc_of_sorted, store._doc_of_sorted)


def test_keep_tokens_compact_and_dtype_conversion():
    E = 16
    x = W.pattern_batch(9, 5, E, torch.float32, seed=5)
    rows, begin, end = W.append_batches([(x, False)])
    rows16, _, end16 = W.append_batches([(x.half(), False)])
    assert int(end16[-1]) == int(end[-1]) - 1                              # the fp32 subnormal's row is a zero row in fp16
    fn = _StandIn()
    w = _writer(60, E, fn, dtype=torch.float16, fp8=True, keep_tokens=True, quantize_fn=R8.quantize_torch)
    w.append(list(range(9)), x)
    assert fn.calls[0][1] == torch.float16                                 # an fp8 store is quantised from the store dtype's values
    store = w.finish(compact=True)
    T = int(end16[-1])
    assert store.tokens.shape == (T, E) and store.tokens.dtype == torch.float16 and store.codes.shape == (T, E)
    assert store.tokens.untyped_storage().nbytes() == T * E * 2            # cloned to the exact size
    assert torch.equal(W.bits(store.tokens), W.bits(rows16))
    c, s = R8.quantize_torch(rows16)
    assert torch.equal(store.codes, c) and torch.equal(store.scales, s)
    # a 16-bit store from fp32 output: the native call converts (the stand-in: torch's cast), the writer does not
    fn2 = _StandIn()
    w2 = _writer(60, E, fn2, dtype=torch.float16)
    w2.append(list(range(9)), x)
    assert fn2.calls[0][1] == torch.float32
    assert torch.equal(W.bits(w2.finish().tokens), W.bits(rows.half()))
    # fp16 output into a bf16 store is converted by the writer: the native call refuses that pair
    fn3 = _StandIn()
    w3 = _writer(60, E, fn3, dtype=torch.bfloat16)
    w3.append(list(range(9)), x.half())
    assert fn3.calls[0][1] == torch.bfloat16


def test_duplicate_ids_wrong_shapes_and_a_finished_writer_are_refused():
    from matchmaker_amd import NativeError
    E = 16
    w = _writer(100, E, _StandIn())
    x = W.pattern_batch(3, 4, E, torch.float16, seed=6)
    w.append(["a", "b", "c"], x)
    with pytest.raises(NativeError, match="'b' was appended before"):
        w.append(["d", "b", "e"], x)
    with pytest.raises(NativeError, match="'d' was appended before"):
        w.append(["d", "d", "e"], x)
    with pytest.raises(NativeError, match="seq_ids and vectors"):
        w.append(["d", "e"], x)
    with pytest.raises(NativeError, match="seq_ids and vectors"):
        w.append(["d", "e", "f"], x[:, :, :8])
    assert w.seq_ids == ["a", "b", "c"]                                    # a refused append adds nothing
    w.append(["d", "e", "f"], x)
    store = w.finish()
    assert store.seq_ids == ["a", "b", "c", "d", "e", "f"]
    with pytest.raises(NativeError, match="finish\\(\\) was called"):
        w.append(["g", "h", "i"], x)


def test_the_document_table_grows_past_its_first_size():
    E = 16
    w = _writer(3000, E, _StandIn())
    x = W.pattern_batch(700, 1, E, torch.float16, seed=7)
    for r in range(3):
        w.append([(r, i) for i in range(700)], x)
    store = w.finish()
    rows, begin, end = W.append_batches([(x, False)] * 3)
    assert len(store.seq_ids) == 2100 and np.array_equal(store._begin, begin) and np.array_equal(store._end, end)
    assert torch.equal(W.bits(store.tokens), W.bits(rows))


def test_the_upper_bound_reads_fill_back_once_and_only_when_it_must():
    from matchmaker_amd import NativeError, _lib
    E = 16
    x = W.pattern_batch(6, 10, E, torch.float16, seed=8, shift=6)          # 60 padded rows, fewer kept
    kept = int(W.keep_mask(x).sum())
    assert 21 <= kept < 40
    cap = 3 * kept + 59                                                    # three batches fit, a fourth padded one cannot
    w = _writer(cap, E, _StandIn())
    w.append(list("abcdef"), x)
    w.append(list("ghijkl"), x)
    assert w._fill.reads == 0 and w.rows_upper_bound == 120
    w.append(list("mnopqr"), x)                                            # 180 > cap: one read-back, 2 kept + 60 <= cap
    assert w._fill.reads == 1 and w.rows_upper_bound == 2 * kept + 60
    with pytest.raises(NativeError, match="cannot take") as ei:            # 3 kept + 60 > cap: refused before any launch
        w.append(list("stuvwx"), x)
    assert ei.value.code == _lib.MM_EUNSUPPORTED and w._fill.reads == 2 and len(w._append.calls) == 3
    assert "'s'" in str(ei.value)
    store = w.finish()                                                     # the refused batch left nothing behind
    assert len(store.seq_ids) == 18 and store.tokens.shape[0] == 3 * kept and int(w._status[0]) == 0


def test_finish_reports_a_sticky_device_refusal():
    """The device-side capacity check is the backstop of append()'s host-side bound: a stand-in whose store is full from its
    second call on refuses that batch; the status stays, the later batches are no-ops and finish() names the document."""
    from matchmaker_amd import NativeError
    E = 16
    x = W.pattern_batch(5, 4, E, torch.float16, seed=9)
    fn = _StandIn(refuse_from_call=1)
    w = _writer(1000, E, fn)
    w.append(["a0", "a1", "a2", "a3", "a4"], x)
    w.append(["b0", "b1", "b2", "b3", "b4"], x)
    w.append(["c0", "c1", "c2", "c3", "c4"], x)
    assert len(fn.calls) == 3 and int(w._status[0]) == 1
    kept = int(W.keep_mask(x).sum())
    assert int(w._fill.t[0]) == kept                                       # the later documents are absent
    assert bool((w._table[:, 5:15] == -1).all()) and bool((w._table[:, :5] >= 0).all())
    with pytest.raises(NativeError, match="'b0' \\(number 5\\) did not fit"):
        w.finish()


# ------------------------------------------------------------------------------------------ save_reference
def _npz_members(path):
    with zipfile.ZipFile(path) as z:
        return {n: z.read(n) for n in z.namelist()}


@pytest.mark.parametrize("token_dtype, block", [("float16", 20), ("float32", 20), ("float16", 1000)])
def test_save_reference_is_byte_equal_to_write_reference_store(tmp_path, token_dtype, block):
    """Documents of 5, 9, 6, 0, 7, 13, 20, 1 rows in files of 20: the 6-row document would straddle (5 + 9 + 6 = 20 fits
    exactly, the next 7 roll over), 13 + 20 rolls again and the 20-row document fills a file alone."""
    from matchmaker_amd import NativeError
    from matchmaker_amd.token_store import TokenStore, write_reference_store
    rng = np.random.default_rng(12)
    lens = [5, 9, 6, 0, 7, 13, 20, 1]
    E = 16
    docs = [(rng.standard_normal((n, E)) + 3).astype(token_dtype) for n in lens]
    ids = [f"s{i}" for i in range(len(lens))]
    a, b = str(tmp_path / "ref"), str(tmp_path / "ours")
    write_reference_store(a, docs, ids, token_block_size=block, token_dtype=token_dtype)
    fn = _StandIn()
    w = _writer(len(lens) * 22, E, fn, dtype=getattr(torch, token_dtype))       # (the padded rows are the host-side bound)
    pad = np.zeros((len(lens), 22, E), dtype=token_dtype)                  # the documents as padded encoder output
    for i, d in enumerate(docs):
        pad[i, : d.shape[0]] = d
    w.append(ids[:3], torch.from_numpy(pad[:3]))
    w.append(ids[3:], torch.from_numpy(pad[3:]))
    store = w.finish()
    store.save_reference(b, token_block_size=block)
    infos, filled = W.file_layout(lens, block)
    assert filled == ([20, 20, 20, 1] if block == 20 else [61])
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) == sorted(["doc_infos.npz"] + [f"token_reps_{n}.npy" for n in range(len(filled))])
    for f in names:
        if f.startswith("token_reps_"):
            assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    ma, mb = _npz_members(os.path.join(a, "doc_infos.npz")), _npz_members(os.path.join(b, "doc_infos.npz"))
    assert list(ma) == list(mb) and all(ma[k] == mb[k] for k in ma)        # (the zip container carries the time of writing)
    dfs = np.load(os.path.join(b, "doc_infos.npz"), allow_pickle=True)
    assert dfs["doc_infos"][()] == dict(zip(ids, infos)) and dfs["storage_filled_to_index"].tolist() == filled
    # TokenStore.load reads it back to the same store
    back = TokenStore.load(b, E, token_dtype, block, "cpu")
    assert torch.equal(W.bits(back.tokens), W.bits(store.tokens)) and back.seq_ids == ids
    assert np.array_equal(back._end - back._begin, np.asarray(lens))
    with pytest.raises(NativeError, match="does not fit a file"):
        store.save_reference(str(tmp_path / "small"), token_block_size=19)


def test_save_reference_refuses_an_fp8_only_store_and_casts_on_request(tmp_path):
    from matchmaker_amd import NativeError
    from matchmaker_amd.token_store import TokenStore
    E = 16
    x = W.pattern_batch(4, 6, E, torch.bfloat16, seed=13)
    w = _writer(30, E, _StandIn(), dtype=torch.bfloat16, fp8=True, quantize_fn=R8.quantize_torch)
    w.append(list("abcd"), x)
    with pytest.raises(NativeError, match="save_fp8"):
        w.finish().save_reference(str(tmp_path / "x"), 100)
    w = _writer(30, E, _StandIn(), dtype=torch.bfloat16)
    w.append(list("abcd"), x)
    store = w.finish()
    with pytest.raises(NativeError, match="float16 or float32"):
        store.save_reference(str(tmp_path / "y"), 100)
    store.save_reference(str(tmp_path / "z"), 100, token_dtype="float32")
    back = TokenStore.load(str(tmp_path / "z"), E, "float32", 100, "cpu")
    assert torch.equal(back.tokens, store.tokens.float())


# ------------------------------------------------------------------------------------------ encode_collection
def test_encode_collection_calls_the_model_as_the_indexer_head_does():
    from matchmaker_amd.encode import encode_collection
    E = 16
    calls = []

    class _Model:
        def forward_representation(self, seq, sequence_type=None):
            calls.append((sequence_type, torch.is_grad_enabled()))
            return seq["vecs"]

    xs = [W.pattern_batch(3, 4, E, torch.float16, seed=20), W.pattern_batch(2, 7, E, torch.float16, seed=21)]
    batches = [{"seq_tokens": {"vecs": xs[0]}, "seq_id": ["a", "b", "c"]}, {"seq_tokens": {"vecs": xs[1]}, "seq_id": ["d", "e"]}]
    w = _writer(100, E, _StandIn())
    assert encode_collection(_Model(), batches, w, use_fp16=False) == 5
    assert calls == [("doc_encode", False)] * 2
    store = w.finish()
    rows, begin, end = W.append_batches([(x, False) for x in xs])
    assert store.seq_ids == list("abcde") and np.array_equal(store._begin, begin) and torch.equal(W.bits(store.tokens), W.bits(rows))
