"""CPU test of the argument checks the retrieval operators share (matchmaker_amd.ops: the flat, IVF, quantized and graph
searches with their fp8 forms, k-means, the top-k merge, the ColBERT candidate step, the fp8 row quantiser): every operator
raises every shared check with the text and the NativeError code it had when each wrapper spelled the check out itself; the
expected strings are written out here, not built by the helpers under test.  Fake tensors "on" the device pass the CPU-tensor
refusal, which comes first, and every check below runs before anything touches a device."""
import pytest
import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
U8, I8, I32, I64 = torch.uint8, torch.int8, torch.int32, torch.int64
EUNSUPPORTED = -2          # MM_EUNSUPPORTED (include/mm_native.h)


def _t(*shape, dtype=F16, device="cuda"):
    return torch.empty(*shape, dtype=dtype, device=device)


# operator -> a call whose arguments are all valid (3 queries, 40 store rows in 4 lists, nprobe 2, E 128, k 2) except for the
# ones named in `o`
def _call(ops, op, dev="cuda", **o):
    E = o.get("E", 128)
    dt = o.get("dtype", F16)

    def t(*shape, dtype=dt):
        return _t(*shape, dtype=dtype, device=dev)
    q = o.get("q", t(3, E))
    x = o.get("x", t(40, E))                                 # 16-bit store rows / centroids / vectors
    codes = o.get("codes", t(40, E, dtype=U8))
    scales = o.get("scales", t(40, dtype=F32))
    lb = o.get("list_begin", t(5, dtype=I64))
    probes = o.get("probes", t(3, 2, dtype=I32))
    k = o.get("k", 2)
    return {
        "dot_topk": lambda: ops.dot_topk(q, x, k),
        "dot_topk_fp8": lambda: ops.dot_topk_fp8(q, codes, scales, k),
        "ivf_scan": lambda: ops.ivf_scan(q, x, lb, probes, k),
        "ivf_scan_fp8": lambda: ops.ivf_scan_fp8(q, codes, scales, lb, probes, k),
        "ah_encode": lambda: ops.ah_encode(q, t(3, dtype=I32), x, t(E // 2, 16, 2), 4.0),
        "ah_scan": lambda: ops.ah_scan(q, o.get("codes", t(40, E // 4, dtype=U8)), t(E // 2, 16, 2), lb, probes,
                                       t(*probes.shape, dtype=F32), k),
        "gather_dot": lambda: ops.gather_dot(q, x, t(3, 6, dtype=I64)),
        "graph_search": lambda: ops.graph_search(q, x, t(40, 4, dtype=I32), t(3, 2, dtype=I32), 8, k, width=2),
        "kmeans_assign": lambda: ops.kmeans_assign(q, x),
        "kmeans_segment_sum": lambda: ops.kmeans_segment_sum(x, t(40, dtype=I64), lb),
        "topk_merge": lambda: ops.topk_merge(t(3, 6, dtype=F32), t(3, 6, dtype=I64), k),
        "colbert_candidates": lambda: ops.colbert_candidates(t(3, 8, dtype=I64), t(5, dtype=I64), t(5, dtype=I64),
                                                             t(5, dtype=I32), 40),
        "fp8_quantize_rows": lambda: ops.fp8_quantize_rows(x),
        "hbm_stream_probe": lambda: ops.hbm_stream_probe(x),
        "maxsim_ragged_fp8": lambda: ops.maxsim_ragged_fp8(o.get("q", t(2, 5, E)), codes, scales, t(2, dtype=I64), t(2, dtype=I64)),
    }[op]()


ALL = ("dot_topk", "dot_topk_fp8", "ivf_scan", "ivf_scan_fp8", "ah_encode", "ah_scan", "gather_dot", "graph_search",
       "kmeans_assign", "kmeans_segment_sum", "topk_merge", "colbert_candidates", "fp8_quantize_rows", "hbm_stream_probe",
       "maxsim_ragged_fp8")
# two 16-bit matrices of one dtype and one width, and how each operator's message names their shapes
PAIR16 = {"dot_topk": "[nq, E] and [N, E]", "ivf_scan": "[nq, E] and [n, E]", "ah_encode": "[n, E] and [nlist, E]",
          "gather_dot": "[nq, E] and [n, E]", "graph_search": "[nq, E] and [n, E]", "kmeans_assign": "[n, E] and [nlist, E]"}
FP8 = {"maxsim_ragged_fp8": "T", "dot_topk_fp8": "N", "ivf_scan_fp8": "n"}              # ... and the letter of the store's rows
NATIVE_WIDTH = ("ivf_scan_fp8", "ah_encode", "ah_scan", "gather_dot", "kmeans_assign", "kmeans_segment_sum")
LIST_BEGIN = ("ivf_scan", "ivf_scan_fp8", "ah_scan", "kmeans_segment_sum")
PROBES = ("ivf_scan", "ivf_scan_fp8", "ah_scan")


def _raises(fn, text, code=None):
    from matchmaker_amd import NativeError
    with pytest.raises(NativeError) as err:
        fn()
    assert str(err.value) == text, (str(err.value), text)
    assert err.value.code == code, text


@pytest.fixture
def ops():
    from matchmaker_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        yield ops


@pytest.mark.parametrize("op", ALL)
def test_cpu_tensors_are_refused(op):
    from matchmaker_amd import ops
    _raises(lambda: _call(ops, op, dev="cpu"),
            "matchmaker_amd operators need HIP device tensors (got a CPU tensor); there is no CPU fallback")


@pytest.mark.parametrize("op", sorted(PAIR16))
def test_mixed_dtypes_and_widths_of_a_16_bit_pair(ops, op):
    _raises(lambda: _call(ops, op, x=_t(40, 128, dtype=BF16)),
            f"{op}: float16 / bfloat16 vectors of one dtype needed, got torch.float16 / torch.bfloat16")
    _raises(lambda: _call(ops, op, dtype=F32), f"{op}: float16 / bfloat16 vectors of one dtype needed, got torch.float32 / torch.float32")
    _raises(lambda: _call(ops, op, x=_t(40, 64)), f"{op}: expected {PAIR16[op]}, got (3, 128) (40, 64)")
    _raises(lambda: _call(ops, op, q=_t(3, 5, 128)), f"{op}: expected {PAIR16[op]}, got (3, 5, 128) (40, 128)")


@pytest.mark.parametrize("op", sorted(FP8))
def test_the_fp8_store_and_its_query(ops, op):
    row = FP8[op]
    q32 = _t(2, 5, 128, dtype=F32) if op == "maxsim_ragged_fp8" else _t(3, 128, dtype=F32)
    _raises(lambda: _call(ops, op, q=q32),
            f"{op}: the query is fp16 or bf16 (convert it; an fp32 query has no exact 16-bit MFMA operand)", EUNSUPPORTED)
    _raises(lambda: _call(ops, op, codes=_t(40, 128, dtype=I8)), f"{op}: codes: expected [{row}, E] uint8, got (40, 128) torch.int8")
    _raises(lambda: _call(ops, op, codes=_t(40, dtype=U8)), f"{op}: codes: expected [{row}, E] uint8, got (40,) torch.uint8")
    _raises(lambda: _call(ops, op, scales=_t(39, dtype=F32)),
            f"{op}: scales: expected [40] float32 (one per row of codes), got (39,) torch.float32")
    _raises(lambda: _call(ops, op, scales=_t(40, dtype=F16)),
            f"{op}: scales: expected [40] float32 (one per row of codes), got (40,) torch.float16")
    _raises(lambda: _call(ops, op, scales=_t(40, 1, dtype=F32)),
            f"{op}: scales: expected [40] float32 (one per row of codes), got (40, 1) torch.float32")
    _raises(lambda: _call(ops, op, codes=_t(40, 64, dtype=U8)), "embedding dims differ: 128 vs 64")
    if op != "maxsim_ragged_fp8":
        _raises(lambda: _call(ops, op, q=_t(3, 5, 128)),
                f"{op}: queries: expected [nq, E] float16 / bfloat16, got (3, 5, 128) torch.float16")
        _raises(lambda: _call(ops, op, q=_t(3, 128, dtype=I8)),
                f"{op}: queries: expected [nq, E] float16 / bfloat16, got (3, 128) torch.int8")


@pytest.mark.parametrize("op", NATIVE_WIDTH)
def test_widths_without_a_kernel(ops, op):
    for E in (64, 640, 1024):
        _raises(lambda: _call(ops, op, E=E), f"{op}: E={E} is not one of 128, 256, 384, 512, 768 (pad the vectors)", EUNSUPPORTED)


@pytest.mark.parametrize("op", LIST_BEGIN)
def test_malformed_list_begin(ops, op):
    _raises(lambda: _call(ops, op, list_begin=_t(5, dtype=I32)), f"{op}: list_begin must be int64 [nlist + 1], got torch.int32 (5,)")
    _raises(lambda: _call(ops, op, list_begin=_t(1, dtype=I64)), f"{op}: list_begin must be int64 [nlist + 1], got torch.int64 (1,)")
    _raises(lambda: _call(ops, op, list_begin=_t(5, 1, dtype=I64)), f"{op}: list_begin must be int64 [nlist + 1], got torch.int64 (5, 1)")


@pytest.mark.parametrize("op", PROBES)
def test_malformed_probes_and_k_or_nprobe_out_of_range(ops, op):
    _raises(lambda: _call(ops, op, probes=_t(3, 2, dtype=I64)), f"{op}: probes must be int32 [nq, nprobe], got torch.int64 (3, 2)")
    _raises(lambda: _call(ops, op, probes=_t(2, 2, dtype=I32)), f"{op}: probes must be int32 [nq, nprobe], got torch.int32 (2, 2)")
    _raises(lambda: _call(ops, op, probes=_t(3, 0, dtype=I32)), f"{op}: probes must be int32 [nq, nprobe], got torch.int32 (3, 0)")
    _raises(lambda: _call(ops, op, probes=_t(6, dtype=I32)), f"{op}: probes must be int32 [nq, nprobe], got torch.int32 (6,)")
    _raises(lambda: _call(ops, op, k=0), f"{op}: k=0 / nprobe=2 outside 1 .. 4096")
    _raises(lambda: _call(ops, op, k=4097), f"{op}: k=4097 / nprobe=2 outside 1 .. 4096")
    _raises(lambda: _call(ops, op, probes=_t(3, 4097, dtype=I32)), f"{op}: k=2 / nprobe=4097 outside 1 .. 4096")


def test_what_only_one_operator_checks_keeps_its_text_and_code(ops):
    """The refusals next to the shared ones in the wrappers this change rewrote."""
    _raises(lambda: _call(ops, "ah_scan", codes=_t(40, 31, dtype=U8)),
            "ah_scan: expected [nq, E] queries and uint8 [n, E / 4] codes, got (3, 128) torch.uint8 (40, 31)")
    _raises(lambda: _call(ops, "ah_scan", dtype=F32), "ah_scan: float16 / bfloat16 queries needed, got torch.float32")
    _raises(lambda: _call(ops, "kmeans_segment_sum", dtype=F32),
            "kmeans_segment_sum: expected float16 / bfloat16 [n, E], got torch.float32 (40, 128)")
    _raises(lambda: _call(ops, "kmeans_segment_sum", list_begin=_t(65538, dtype=I64)),
            "kmeans_segment_sum: nlist=65537 outside 1 .. 65536, or n=40 >= 2^31", EUNSUPPORTED)
    _raises(lambda: _call(ops, "kmeans_assign", x=_t(65537, 128)), "kmeans_assign: nlist=65537 outside 1 .. 65536, or n=3 >= 2^31",
            EUNSUPPORTED)
    _raises(lambda: _call(ops, "fp8_quantize_rows", x=_t(40, 72)), "fp8_quantize_rows: E=72 is not a multiple of 16", EUNSUPPORTED)
    _raises(lambda: _call(ops, "fp8_quantize_rows", x=_t(40, 128, dtype=I8)),
            "fp8_quantize_rows: expected [T, E] float tensor, got (40, 128) torch.int8")
