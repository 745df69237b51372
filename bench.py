#!/usr/bin/env python
"""bench.py — query-doc pairs scored / second, ColBERT MaxSim (Q32 / D180 / dim128, bf16,
1000 candidates per query; BASELINE.json configs[1]), on N MI355X GPUs of one node.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]

`--gpus N` with N > 1 starts itself: when no torch.distributed environment is present the script re-executes
under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...` (one process
per GPU over RCCL), the way the reference starts all GPUs from one `python train.py`
(matchmaker/train.py:194-202); launched under torchrun by someone else it just joins the group.

A "step" = one pass of the hot path (mm_maxsim_fwd) over one resident batch of `--queries` x 1000 synthetic
(query, candidate) pairs per GPU.  Inputs are generated on the device before the timed region (resident in
HBM).  Every rank scores its own shard of queries (weak scaling, no data-path collective); with N > 1 one
RCCL all-gather of the fp32 scores per step is part of the timed region (the ranking merge of SURVEY.md §8e).

Prints ONE JSON line (rank 0).  `ms_per_step`: host time of one timed step; `roofline`: algorithmic bytes per launch
 / average kernel time measured with HIP events on the launch stream of the timed steps.

A plain run sets up, runs W warm-up and K timed steps and prints the line, nothing else.  `--full` adds everything
else the benchmark measures and checks: the HBM calibration before the warm-up, the `self_check` of the timed scores
against the numpy oracle, the gather checks and the final sort with a process group, and at N = 1 `cpu_baseline`
(the torch CPU port of the reference's ops, oracle/torch_port.py, timed on this host's cores on a bounded sample of
the same workload; `--no-cpu-baseline` skips it) and `extra` (`--no-extras` skips it): the reference's own batch
layout through the same operator (`dropin_forward`: query
replicated per pair, HF int64 masks — what eval.py:108 hands to ColBERT.forward), and the other BASELINE.json
configs on this GPU (`tk` configs[0] shapes at scale, `tkl` configs[2], `dot_topk` one rank's shard of
configs[4]), each with its own roofline fraction, CPU leg and the rocprof summary it can be checked against.

`--only <leg>` runs ONE leg (headline | dropin_forward | published_checkpoint | all_pairs | tk | tkl | dot_topk |
maxsim_fp32 | eval_batch) and prints it alone: the command tools/profile_round.sh puts under `rocprofv3 --kernel-trace`, so
that every fraction in the line can be re-derived from a profile of the very code that produced it.

`--dump-outputs DIR` writes the scores of the last timed step as DIR/scores.npy (float32; with a process group also
DIR/gathered_scores.npy, the all-gathered scores).  The inputs are seeded, so two builds can be compared output for output.

`--dry` (with `--backend gloo --device cpu`) exercises ONLY the launch + collective plumbing on a machine
without GPUs (tests/test_bench_launch_cpu.py): scores are fabricated, `value` is null — never a measurement.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time
T_PROCESS = time.time()   # (wall_s.process_start_to_headline_done: interpreter start -> the headline measured and checked)

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

Q, D, E, CANDS = 32, 180, 128, 1000
HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
MFMA_PEAK_16BIT = 2.5e15     # dense bf16 / fp16 MFMA peak, FLOP/s (MI355X_MICROARCH.md; no sparsity)
MU = [1.0, 0.9, 0.7, 0.5, 0.3, 0.1, -0.1, -0.3, -0.5, -0.7, -0.9]
LEAN = False                 # --lean: a leg runs its main measurement only (profiling runs: one workload per kernel name)


def algorithmic_bytes(n_queries: int, cands: int) -> int:
    """B*D*E*s + Nq*Q*E*s + 4*(B + Nq) + 4*B  (shared-Q layout, int32 lengths)."""
    B = n_queries * cands
    return B * D * E * 2 + n_queries * Q * E * 2 + 4 * (B + n_queries) + 4 * B


def dropin_bytes(B: int) -> int:
    """The reference's pair-per-row layout (54,280 B/pair) + its int64 HF masks as they are read."""
    return B * ((D + Q) * E * 2 + 8 * (D + Q) + 4)


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(args) -> int:
    """One command starts all ranks (train.py:194-202 starts its GPUs from one process too)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL / cross-process device memory)
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def timed_cpu(fn, budget_s, unit_per_call):
    """2 warm-ups, then whole calls until ~budget_s seconds -> (units/s, calls, seconds)."""
    fn(); fn()
    t_total, n = 0.0, 0
    while t_total < budget_s or n < 5:
        t0 = time.perf_counter()
        fn()
        t_total += time.perf_counter() - t0
        n += 1
        if n >= 5 and t_total >= budget_s:
            break
    return unit_per_call * n / t_total, n, t_total


def both_thread_settings(make_fn, budget_s, unit_per_call):
    """(all-threads rate, single-thread rate, threads): BASELINE.md §2 asks for torch.set_num_threads(1) — what
    the reference's scripts run with (train.py:12 exports OMP_NUM_THREADS=1) — and the host's best case."""
    import torch
    threads = torch.get_num_threads()
    r_all = timed_cpu(make_fn(), budget_s, unit_per_call)
    torch.set_num_threads(1)
    try:
        r_one = timed_cpu(make_fn(), budget_s / 2, unit_per_call)
    finally:
        torch.set_num_threads(threads)
    return r_all, r_one, threads


def cpu_baseline(q_cpu, d_cpu, q_len, d_len, cands, budget_s=12.0):
    """The reference's CPU path for this block = the torch ops of colbert.py:68-75, repeated op by op
    in oracle/torch_port.py (pinned on the real reference's golden outputs); /root/reference itself
    does not exist on the GPU box, hence kind "port".  Reference layout: fp32, query replicated per
    pair, int64 HF masks, one candidate list (1000 pairs) per forward call.  Bounded sample: whole
    queries until ~budget_s seconds; a short single-thread leg is reported too because the
    reference's scripts export OMP_NUM_THREADS=1 (train.py:12)."""
    import torch
    from oracle import torch_port as TP
    from oracle import ref_harness as RH
    from matchmaker_amd import synth
    qn = q_cpu.float()
    nq = qn.shape[0]
    # where the reference tree exists (the build container) the REAL ColBERT.forward (colbert.py:54-86, identity encoder) is
    # what gets timed: kind "reference"; on the GPU box /root/reference is absent and the port of its statements is timed
    use_ref = RH.available()
    if use_ref:
        try:
            RH.colbert_forward(qn[:1, :2], d_cpu[:1, :2].float(), torch.ones(1, 2, dtype=torch.int64), torch.ones(1, 2, dtype=torch.int64))
        except Exception:
            use_ref = False

    # The reference hands the scoring block tensors its encoder has just produced: the fp32 tensors are written per call (untimed)
    # into ONE preallocated pair of buffers.  (A fresh 92 MB tensor per call cost 30 ms of page faults around a 7-12 ms call: 55 of
    # the leg's 75 s of wall clock; same box, same day: 79.6 k pairs/s that way, 80.9 k with tensors prepared once per query and
    # read back from DRAM, 90.1 k this way.  The 128-thread rate moves 80-150 k box to box with the host's other tenants.)
    dn = torch.empty((cands,) + tuple(d_cpu.shape[1:]), dtype=torch.float32)
    qr = torch.empty((cands,) + tuple(qn.shape[1:]), dtype=torch.float32)
    masks = {}

    def run(i):
        dn.copy_(d_cpu[i * cands:(i + 1) * cands])
        qr.copy_(qn[i:i + 1].expand(cands, -1, -1))
        if i not in masks:
            masks[i] = (synth.len_to_mask(q_len[i:i + 1], Q).expand(cands, -1).contiguous(),
                        synth.len_to_mask(d_len[i * cands:(i + 1) * cands], D))
        qm, dm = masks[i]
        t0 = time.perf_counter()
        if use_ref:
            RH.colbert_forward(qr, dn, qm, dm)
        else:
            with torch.no_grad():
                TP.maxsim_forward(qr, dn, qm, dm)
        return time.perf_counter() - t0

    def leg(budget):
        run(0)
        t_total, pairs, i = 0.0, 0, 0
        while t_total < budget:
            t_total += run(i % nq)
            pairs += cands
            i += 1
        return pairs / t_total, i, pairs, t_total

    threads = torch.get_num_threads()
    rate, n, pairs, t_total = leg(budget_s)
    torch.set_num_threads(1)
    rate1, n1, pairs1, t1 = leg(min(4.0, budget_s / 3))
    torch.set_num_threads(threads)
    return {"value": rate, "unit": "pairs/s", "cores": threads, "kind": "reference" if use_ref else "port", "cpu_model": cpu_model(),
            "single_thread_value": rate1,
            "sample": f"{n} forward calls over whole queries ({nq} distinct) x {cands} candidates = {pairs} pairs of the "
                      f"bench workload in {t_total:.1f} s with {threads} torch threads (host has "
                      f"{os.cpu_count()} logical CPUs); " + ("the reference's own ColBERT.forward "
                      "(colbert.py:54-86 imported from the reference tree by oracle/ref_harness.py, identity encoder, fp32)" if use_ref else
                      "fp32 torch CPU port of colbert.py:68-75 (oracle/torch_port.py: bmm, masked assign, max, sum; the reference "
                      "tree is absent on this box)") + f"; single-thread leg "
                      f"(OMP_NUM_THREADS=1 as in train.py:12): {pairs1} pairs in {t1:.1f} s"}


def profile_summary(pattern, kernel_substr, key):
    """A figure from the committed rocprofv3 summaries (profiles/*.json, tools/summarize_rocprof.py):
    returns (value, file) of the newest matching profile, or None."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", pattern))):
        try:
            j = json.load(open(f))
        except Exception:
            continue
        for k, c in j.get("pmc", {}).items():
            if kernel_substr in k and key in c:
                v = c[key]
                best = (v["total"] if isinstance(v, dict) and "total" in v else v, os.path.basename(f), j.get("workload", {}))
    return best


def gpu_time_ms(fn, steps, warmup=2, warm_ms=40.0, timed_ms=25.0, max_calls=400):
    """Median of per-call HIP-event times on the current stream (the stream the operators launch on), in steady state:
    after `warmup` calls the call is repeated until ~warm_ms of device time have passed, and at least `steps` calls — as
    many as ~timed_ms of device time hold — are timed.  A leg whose call takes 0.15-1.5 ms is otherwise measured while the
    GPU still climbs out of its idle clocks: the first ten launches of the 1.4 ms all-pairs kernel ran 12 % slower than
    the next ten in the same process (1.54 vs 1.37 ms); an evaluation loop keeps the device busy."""
    import torch
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    t = max(a.elapsed_time(b), 1e-3)
    for _ in range(min(max_calls, int(warm_ms / t))):
        fn()
    n = min(max_calls, max(steps, int(timed_ms / t)))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[len(ev) // 2]


def smi_sample():
    """Shader / memory clock (MHz) and socket power (W) of this rank's GPU as rocm-smi reports them (~0.5 s per call)."""
    import re
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=30)
    except Exception as e:
        return {"error": repr(e)}
    gpu = os.environ.get("LOCAL_RANK", "0")
    out = {}
    for line in r.stdout.splitlines():
        if not line.startswith(f"GPU[{gpu}]"):
            continue
        m = re.search(r"(sclk|mclk) clock level: \d+: \((\d+)Mhz\)", line)
        if m:
            out[m.group(1) + "_mhz"] = int(m.group(2))
        m = re.search(r"Power \(W\): ([0-9.]+)", line)
        if m:
            out["socket_power_w"] = float(m.group(1))
    return out or {"error": (r.stdout + r.stderr)[-200:]}


def extra_hbm_calibration(d, steps, headline_gbs):
    """What THIS box's memory system gives the headline's access pattern, measured in the same process over the same
    11.8 GB document tensor: (i) mm_hbm_stream_probe = maxsim_stream_kernel's LDS-DMA read stream with the arithmetic
    removed (same geometry, ring, counted waits; no MFMA, no maximum), (ii) a device-to-device copy of half of it
    (hipMemcpyDtoD through torch: bytes read + written).  The headline kernel's rate over (i) separates a slow box from a
    slow kernel: the kernel is at the stream's own limit when the ratio is ~1."""
    import torch
    from matchmaker_amd import ops
    nbytes = d.numel() * d.element_size() // 8192 * 8192
    out = {}
    for name, nt in (("lds_dma_read_stream_nt", True), ("lds_dma_read_stream", False)):
        ms = gpu_time_ms(lambda: ops.hbm_stream_probe(d, nt=nt), steps)
        out[name] = {"ms": ms, "GBps": nbytes / (ms * 1e-3) / 1e9, "bytes": nbytes}
    half = d[: d.shape[0] // 2]
    dst = torch.empty_like(half)
    ms = gpu_time_ms(lambda: dst.copy_(half), steps)
    hb = half.numel() * half.element_size()
    out["memcpy_dtod"] = {"ms": ms, "GBps_read_plus_write": 2 * hb / (ms * 1e-3) / 1e9, "bytes_copied": hb}
    del dst
    torch.cuda.empty_cache()
    if headline_gbs is not None:
        out["headline_kernel_GBps"] = headline_gbs
        out["headline_over_read_stream"] = headline_gbs / out["lds_dma_read_stream_nt"]["GBps"]
    out["kernel"] = "hbm_stream_probe_kernel (csrc/maxsim.hip): the headline kernel's stream, no arithmetic"
    return out


def vendor_gemm_tflops(shapes):
    """torch.mm (hipBLASLt / rocBLAS) at the given {name: (M, N, K, dtype)} shapes, 16-bit output written: a calibration of
    what matrix rate this board sustains, not part of any product path."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {}
    for name, (M, N, K, dt) in shapes.items():
        a = torch.randn(M, K, device=dev, dtype=dt)
        b = torch.randn(N, K, device=dev, dtype=dt)
        c = torch.empty(M, N, device=dev, dtype=dt)
        ms = gpu_time_ms(lambda: torch.mm(a, b.t(), out=c), 5, warm_ms=100.0, timed_ms=60.0)
        res[name] = {"shape_mnk": [M, N, K], "ms": ms, "tflops": 2.0 * M * N * K / (ms * 1e-3) / 1e12}
        del a, b, c
    torch.cuda.empty_cache()
    return res


# ------------------------------------------------------------------------------------------ extras (N = 1)
def extra_dropin_forward(q, d, q_len, d_len, steps):
    """eval.py:108 -> ColBERT.forward -> colbert.py:68-75 exactly as the reference batches it: the query
    replicated per pair, HF int64 attention masks, pairs_per_query = 1 — on the SAME pairs as the headline."""
    import torch
    from matchmaker_amd import ops, synth
    from matchmaker_amd.colbert import ColBERT
    nq, B = q.shape[0], d.shape[0]
    qp = q.repeat_interleave(CANDS, 0).contiguous()
    qm = synth.len_to_mask(q_len, Q, torch.int64).repeat_interleave(CANDS, 0).contiguous()
    dm = synth.len_to_mask(d_len, D, torch.int64)
    # eval.py:83 / colbert.py:60 run the block under autocast: 16-bit similarities and maxima, fp32 sums (MM_SIM_ROUND)
    ref = ops.maxsim(q, d, q_len, d_len, pairs_per_query=CANDS, sim_round=True)
    with torch.autocast("cuda", dtype=torch.float16):
        got = ColBERT._score(qp, d, qm, dm)               # the drop-in's scoring entry (no_grad: native forward)
        same = bool(torch.equal(ref, got))
        ms = gpu_time_ms(lambda: ColBERT._score(qp, d, qm, dm), steps)
    by = dropin_bytes(B)
    gbs = by / (ms * 1e-3) / 1e9
    return {"workload": f"the headline's {nq} x {CANDS} pairs in the reference's batch layout: Q replicated per pair "
                        f"[{B},{Q},{E}] bf16, int64 HF masks [{B},{Q}] / [{B},{D}], pairs_per_query = 1 (ColBERT._score)",
            "dtype": "bf16", "ms": ms, "pairs_per_s": B / (ms * 1e-3), "algorithmic_bytes": by,
            "bytes_per_pair": by // B, "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                                    "frac": gbs / HBM_PEAK_GBS},
            "bit_identical_to_shared_q_scores": same, "profile": "profiles/r04_dropin_forward_trace.json"}


def extra_sustained(score_shard, B, seconds=4.0):
    """The same launch back to back for a few seconds of wall clock: long enough for an external sampler (rocm-smi at a
    multi-second cadence) to see the GPU busy, and a cross-check of the 20-step figure on the host clock."""
    import threading
    import torch
    idle = smi_sample()
    score_shard()
    torch.cuda.synchronize()
    busy = {}
    th = threading.Timer(1.5, lambda: busy.update(smi_sample()))      # one sample while the loop below keeps the GPU busy
    th.start()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(100):
            score_shard()
        torch.cuda.synchronize()
        n += 100
        dt = time.perf_counter() - t0
        if dt >= seconds and not th.is_alive():
            break
    return {"workload": "the headline launch repeated back to back", "steps": n, "seconds": dt, "ms_per_step": 1e3 * dt / n,
            "pairs_per_s": n * B / dt, "rocm_smi_idle_before": idle, "rocm_smi_during": busy}


def tk_exact_f32_subprocess():
    """TK pooling on the exact-f32 MFMA kernel (MM_KP_F32MFMA=1, read once per process -> a child process), timed
    beside the split-bf16 default: VERDICT r01 asked for the A/B in the driver-timed line."""
    env = dict(os.environ, MM_KP_F32MFMA="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_kernel_pool.py"), "--full", "--queries", "64", "--steps", "5"],
                       capture_output=True, text=True, env=env, timeout=300)
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            j = json.loads(line)
            return {"kernel": "kernel_pool_stream_kernel (v_mfma_f32_32x32x2_f32, exact fp32 operands)", "ms": j["ms"],
                    "pairs_per_s": j["pairs_per_s"], "GBps": j["GBps_padded_bytes"]}
    return {"error": (r.stderr or r.stdout)[-300:]}


def extra_tk(steps, cpu_budget):
    """BASELINE.json configs[0] shapes (TK kernel pooling, Q=20 / D=200 / dim=300, fp32) at GPU scale:
    64 queries x 1000 candidates, every position real (the padded figure of DESIGN.md §3.3)."""
    import torch
    from matchmaker_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    nq, C, Qt, Dt, Et = 64, 1000, 20, 200, 300
    B = nq * C
    g = torch.Generator(device=dev).manual_seed(1001)
    q = torch.randn(nq, Qt, Et, generator=g, device=dev)
    d = torch.randn(B, Dt, Et, generator=g, device=dev)
    q_len = torch.full((nq,), Qt, dtype=torch.int32, device=dev)
    d_len = torch.full((B,), Dt, dtype=torch.int32, device=dev)
    prm = [torch.tensor(MU, device=dev), torch.full((11,), 0.1, device=dev), torch.ones(11, device=dev),
           torch.linspace(-0.014, 0.014, 11, device=dev)]
    fn = lambda: ops.kernel_pool(q, d, q_len, d_len, *prm, pairs_per_query=C)
    ms = gpu_time_ms(fn, steps)
    by = B * Dt * Et * 4 + nq * Qt * Et * 4 + 4 * (B + nq) + 4 * B
    gbs = by / (ms * 1e-3) / 1e9
    out = {"workload": f"TK kernel pooling (ecai20_tk.py:105-124), {nq} queries x {C} candidates, Q={Qt}/D={Dt}/dim={Et}, "
                       f"all positions real, shared query tile, int32 lengths",
           "dtype": "fp32 (split-bf16 operands: x = hi + lo, 3 bf16 MFMAs hi.hi + lo.hi + hi.lo, fp32 accumulation)", "ms": ms,
           "pairs_per_s": B / (ms * 1e-3), "algorithmic_bytes": by, "flop": B * (2 * Qt * Dt * Et + 2 * (Qt + Dt) * Et),
           "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS},
           "kernel": "kernel_pool_split_kernel", "profile": "profiles/r06_tk_trace.json, profiles/r06_tk_pmc.json"}
    del q, d
    torch.cuda.empty_cache()
    try:
        if not LEAN:
            out["exact_f32_mfma"] = tk_exact_f32_subprocess()
    except Exception as e:
        out["exact_f32_mfma"] = {"error": repr(e)}
    g = torch.Generator(device=dev).manual_seed(1001)
    q = torch.randn(nq, Qt, Et, generator=g, device=dev)
    d = torch.randn(200, Dt, Et, generator=g, device=dev)
    # --- CPU legs: scoring only (torch port of :105-124) and full forward (+ the 2-layer Transformer contextualiser)
    if cpu_budget > 0:
        from oracle import torch_port as TP
        from matchmaker_amd.tk import ECAI20_TK
        n = 200
        qc, dc = q[:1].cpu().expand(n, -1, -1).contiguous(), d[:n].cpu()
        qm, dm = torch.ones(n, Qt), torch.ones(n, Dt)
        mu, sg = prm[0].cpu().view(1, 1, 1, -1), prm[1].cpu().view(1, 1, 1, -1)
        al, w = prm[2].cpu().view(1, 1, -1), prm[3].cpu().view(1, -1)
        model = ECAI20_TK(Et, MU, [0.1] * 11, att_heads=10, att_layer=2, att_ff_dim=300, max_length=Dt,
                          use_diff_posencoding=True, mix_hybrid_context=True).eval()      # tk.yaml

        def scoring():
            with torch.no_grad():
                TP.tk_kernel_pool(qc, dc, qm, dm, mu, sg, al, w)

        def full():
            with torch.no_grad():
                qx = model.forward_representation(qc, qm, model.positional_features_q[:, :Qt])
                dx = model.forward_representation(dc, dm, model.positional_features_d[:, :Dt])
                TP.tk_kernel_pool(qx, dx, qm, dm, mu, sg, al, w)
        (ra, na, ta), (r1, n1, t1), threads = both_thread_settings(lambda: scoring, cpu_budget, n)
        (fa, _, _), (f1, _, _), _ = both_thread_settings(lambda: full, cpu_budget, n)
        out["cpu_baseline"] = {"value": ra, "unit": "pairs/s", "cores": threads, "kind": "port", "single_thread_value": r1,
                               "full_forward_value": fa, "full_forward_single_thread_value": f1,
                               "sample": f"{n}-pair forward calls, {na} timed calls in {ta:.1f} s ({threads} threads) / {n1} in "
                                         f"{t1:.1f} s (1 thread); scoring only = oracle/torch_port.tk_kernel_pool; full forward = "
                                         f"the drop-in's own PyTorch contextualiser (2 layers, 10 heads, tk.yaml) + that block"}
    return out


def extra_tkl(steps, cpu_budget):
    """BASELINE.json configs[2]: TKL, D = 2048, dim = 300, Q = 20, fp32; 256 documents of U{50..2048} tokens and
    queries of U{3..20} tokens, pre-contextualised packed chunks resident in HBM -> scores."""
    import torch
    from matchmaker_amd import ops
    from matchmaker_amd.tkl import TKL_sigir20, chunk_documents
    dev = torch.device("cuda", torch.cuda.current_device())
    B, Qt, Dt, Et = 256, 20, 2048, 300
    g = torch.Generator(device=dev).manual_seed(3003)
    m = TKL_sigir20(Et, MU, [0.1] * 11, 10, 2, 300, 2000, True, True, "embedding").to(dev).eval()     # tkl.yaml
    q = torch.randn(B, Qt, Et, generator=g, device=dev)
    d = torch.randn(B, Dt, Et, generator=g, device=dev)
    d_len = torch.randint(50, Dt + 1, (B,), generator=g, device=dev)
    q_len = torch.randint(3, Qt + 1, (B,), generator=g, device=dev)
    qm = (torch.arange(Qt, device=dev)[None] < q_len[:, None]).float()
    dm = (torch.arange(Dt, device=dev)[None] < d_len[:, None]).float()
    q_ctx = q * qm.unsqueeze(-1)
    chunks, cmask, slot, C = chunk_documents(d * dm.unsqueeze(-1), dm)       # stands in for the contextualised chunks
    params = m.pack_params()
    P = chunks.shape[0]
    fn = lambda: ops.tkl_score(q_ctx, chunks, cmask, slot, qm, params, B, C, 11, "embedding", check_order=False)   # (chunk_documents packs ascending)
    ms = gpu_time_ms(fn, steps)
    by = P * 50 * Et * 4 + B * Qt * Et * 4 + P * 50 * 4 + 4 * B
    # SURVEY.md §8(d) prices all 50 rows of a packed chunk; the scoring reads the 40 centre rows (sigir20_tkl.py:174) — the
    # bytes the call actually needs, and the tighter fraction
    by_needed = P * 40 * Et * 4 + B * Qt * Et * 4 + P * 40 * 4 + 4 * B
    gbs = by / (ms * 1e-3) / 1e9
    out = {"workload": f"TKL scoring (sigir20_tkl.py:180-286), {B} documents x D={Dt} (lengths U{{50..{Dt}}}: {P} packed chunks "
                       f"of 50 tokens), dim={Et}, Q={Qt} (lengths U{{3..{Qt}}}), embedding saturation",
           "dtype": "fp32 (split-bf16 operands: x = hi + lo, 3 bf16 MFMAs hi.hi + lo.hi + hi.lo, fp32 accumulation)", "ms": ms, "docs_per_s": B / (ms * 1e-3), "algorithmic_bytes": by,
           "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                        "needed_bytes": by_needed, "frac_needed_bytes": by_needed / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
           "kernel": "tkl_prep_kernel + tkl_stage1_rows_kernel + tkl_window_kernel<cos> + tkl_region_kernel: the whole mm_tkl_fwd call",
           "profile": "profiles/r06_tkl_pmc.json, profiles/r06_tkl_trace.json (full documents: profiles/r06_tklfull_pmc.json)"}
    try:
        if not LEAN:
            out["exact_f32_mfma"] = tkl_exact_f32_subprocess()
    except Exception as e:
        out["exact_f32_mfma"] = {"error": repr(e)}
    try:      # the same length distributions at four times the batch: how much of the 256-document figure is fixed cost
        if LEAN:
            raise RuntimeError("skipped (--lean)")
        B4 = 4 * B
        g4 = torch.Generator(device=dev).manual_seed(3004)
        d4 = torch.randn(B4, Dt, Et, generator=g4, device=dev)
        q4 = torch.randn(B4, Qt, Et, generator=g4, device=dev)
        dl4 = torch.randint(50, Dt + 1, (B4,), generator=g4, device=dev)
        ql4 = torch.randint(3, Qt + 1, (B4,), generator=g4, device=dev)
        qm4 = (torch.arange(Qt, device=dev)[None] < ql4[:, None]).float()
        dm4 = (torch.arange(Dt, device=dev)[None] < dl4[:, None]).float()
        ch4, cm4, sl4, C4 = chunk_documents(d4 * dm4.unsqueeze(-1), dm4)
        del d4
        qc4 = q4 * qm4.unsqueeze(-1)
        ms4 = gpu_time_ms(lambda: ops.tkl_score(qc4, ch4, cm4, sl4, qm4, params, B4, C4, 11, "embedding", check_order=False), steps)
        by4 = ch4.shape[0] * 50 * Et * 4 + B4 * Qt * Et * 4 + ch4.shape[0] * 50 * 4 + 4 * B4
        out["batch_1024_documents"] = {"ms": ms4, "docs_per_s": B4 / (ms4 * 1e-3), "algorithmic_bytes": by4,
                                       "frac": by4 / (ms4 * 1e-3) / 1e9 / HBM_PEAK_GBS}
        del ch4, cm4, sl4, qc4, q4
        torch.cuda.empty_cache()
    except Exception as e:
        out["batch_1024_documents"] = {"error": repr(e)}
    if cpu_budget > 0:
        from oracle import torch_port as TP
        n = 4
        keep = (slot.long() // C) < n
        packed = torch.zeros(n * C, dtype=torch.bool)
        packed[slot[keep].long().cpu()] = True
        centre, cm = chunks[keep][:, 5:-5].cpu().contiguous(), cmask[keep][:, 5:-5].cpu().float().contiguous()
        prm = {"mu": m.mu, "sigma": m.sigma, "dense_w": m.dense.weight, "sat_w1": m.saturation_linear.weight,
               "sat_b1": m.saturation_linear.bias, "sat_w2": m.saturation_linear2.weight, "sat_b2": m.saturation_linear2.bias,
               "sat_w3": m.saturation_linear3.weight, "sat_b3": m.saturation_linear3.bias, "ln_w": m.sat_normer.weight,
               "ln_b": m.sat_normer.bias, "emb_reduce_w": m.sat_emb_reduce1.weight, "kernel_mult0": m.kernel_mult[0],
               "chunk_scoring": m.chunk_scoring}
        prm = {k: v.detach().float().cpu().reshape(-1) for k, v in prm.items()}
        qc, qmc = q_ctx[:n].cpu(), qm[:n].cpu()
        mc = TKL_sigir20(Et, MU, [0.1] * 11, 10, 2, 300, 2000, True, True, "embedding").eval()
        dc, dmc = d[:n].cpu() * dm[:n].cpu().unsqueeze(-1), dm[:n].cpu()

        def scoring():
            with torch.no_grad():
                TP.tkl_scoring(qc, centre, cm, packed, n, qmc, prm, "embedding")

        def full():
            with torch.no_grad():
                qx, _ = mc.forward_representation(qc, qmc, mc.positional_features_q[:, :Qt])
                ch, chm, sl, Cc = chunk_documents(dc, dmc)
                cx, _ = mc.forward_representation(ch, chm, mc.positional_features_d[:, :50])
                pk = torch.zeros(n * Cc, dtype=torch.bool)
                pk[sl.long()] = True
                TP.tkl_scoring(qx, cx[:, 5:-5].contiguous(), chm[:, 5:-5].float().contiguous(), pk, n, qmc, prm, "embedding")
        (ra, na, ta), (r1, n1, t1), threads = both_thread_settings(lambda: scoring, cpu_budget, n)
        (fa, _, _), (f1, _, _), _ = both_thread_settings(lambda: full, cpu_budget, n)
        out["cpu_baseline"] = {"value": ra, "unit": "docs/s", "cores": threads, "kind": "port", "single_thread_value": r1,
                               "full_forward_value": fa, "full_forward_single_thread_value": f1,
                               "sample": f"the first {n} documents of the workload per call, {na} timed calls in {ta:.1f} s "
                                         f"({threads} threads) / {n1} in {t1:.1f} s (1 thread); scoring only = "
                                         f"oracle/torch_port.tkl_scoring (sigir20_tkl.py:180-286); full forward adds chunking + the "
                                         f"drop-in's PyTorch chunk Transformer (tkl.yaml)"}
    return out


def tkl_exact_f32_subprocess():
    """TKL with stage 1 on the exact-f32 MFMA kernel (MM_KP_F32MFMA=1 is read once per process -> a child process):
    the reference's own operand precision (tkl.yaml use_fp16: False) beside the split-bf16 default."""
    env = dict(os.environ, MM_KP_F32MFMA="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_tkl.py"), "--steps", "5"],
                       capture_output=True, text=True, env=env, timeout=300)
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            j = json.loads(line)
            return {"kernel": "stage 1 = kernel_pool_stream_kernel<TKL> (v_mfma_f32_32x32x2_f32, exact fp32 operands), stages 2-3 unchanged",
                    "ms": j["ms"], "docs_per_s": j["docs_per_s"], "GBps": j["GBps_algorithmic"],
                    "frac": j["GBps_algorithmic"] / HBM_PEAK_GBS}
    return {"error": (r.stderr or r.stdout)[-300:]}


def extra_maxsim_fp32(steps, cpu_budget):
    """The "fp32 variant" of BASELINE.json configs[1]: ColBERT with use_fp16: False (colbert.py:60 without autocast) —
    fp32 token vectors, Q=32 / D=180 / dim=128, 1000 candidates per query, on the three-term split-bf16 kernel."""
    import torch
    from matchmaker_amd import ops, synth
    dev = torch.device("cuda", torch.cuda.current_device())
    nq = 64
    q, d, q_len, d_len = synth.colbert_batch(nq, CANDS, Q, D, E, torch.float32, dev, seed=3232, lengths="full")
    B = nq * CANDS
    fn = lambda: ops.maxsim(q, d, q_len, d_len, pairs_per_query=CANDS)
    ms = gpu_time_ms(fn, steps)
    by = B * D * E * 4 + nq * Q * E * 4 + 4 * (B + nq) + 4 * B
    gbs = by / (ms * 1e-3) / 1e9
    out = {"workload": f"ColBERT MaxSim, fp32 vectors (use_fp16: False), {nq} queries x {CANDS} candidates, Q={Q}/D={D}/dim={E}, "
                       f"shared query tile, int32 lengths, all positions real",
           "dtype": "fp32 (three-term split-bf16 operands x = hi + lo + c, 6 bf16 MFMAs per K step, fp32 accumulation)",
           "ms": ms, "pairs_per_s": B / (ms * 1e-3), "algorithmic_bytes": by,
           "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS},
           "kernel": "kernel_pool_split128_kernel<MX, two wavefronts per SIMD> (csrc/kernel_pool128.hip)", "profile": "profiles/r06_maxsim_fp32_trace.json, profiles/r06_maxsim_fp32_pmc.json"}
    if cpu_budget > 0:
        from oracle import torch_port as TP
        n = 1000
        qc = q[:1].cpu().expand(n, -1, -1).contiguous()
        dc = d[:n].cpu()
        qm, dm = torch.ones(n, Q, dtype=torch.long), torch.ones(n, D, dtype=torch.long)

        def run():
            with torch.no_grad():
                TP.maxsim_forward(qc, dc, qm, dm)
        (ra, na, ta), (r1, n1, t1), threads = both_thread_settings(lambda: run, cpu_budget, n)
        out["cpu_baseline"] = {"value": ra, "unit": "pairs/s", "cores": threads, "kind": "port", "single_thread_value": r1,
                               "sample": f"{n}-pair forward calls (oracle/torch_port.maxsim_forward, fp32), {na} calls in {ta:.1f} s"}
    return out


def extra_eval_batch(steps, cpu_budget):
    """eval.py-sized calls: `batch_size_eval: 512` pairs per model.forward (config/train/defaults.yaml:115, eval.py:108),
    pair-per-row, in the layouts the reference hands over.  Per shape: device time per call (HIP events), wall time per
    call completed (back-to-back calls, one sync at the end), host time per call ISSUED (the Python + ctypes + launch
    path, GPU running behind), and the HBM fraction of the completed rate.  The calls rotate through enough distinct
    batches to exceed the 256 MB Infinity Cache, so every call streams from HBM as in a real evaluation run."""
    import torch
    from matchmaker_amd import ops
    from matchmaker_amd.colbert import ColBERT
    dev = torch.device("cuda", torch.cuda.current_device())
    Bc = 512
    g = torch.Generator(device=dev).manual_seed(512)
    res = {}

    ac = torch.autocast("cuda", dtype=torch.float16)      # eval.py:83 wraps every batch in autocast (use_fp16); the pooling ops stay fp32
    ac.__enter__()

    def run(name, n_batches, make, call, bytes_per_call, n_calls=400):
        batches = [make() for _ in range(n_batches)]
        for b in batches:
            call(b)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(60)]
        for i, (a, b) in enumerate(ev):
            a.record(); call(batches[i % n_batches]); b.record()
        torch.cuda.synchronize()
        dev_us = 1e3 * sorted(a.elapsed_time(b) for a, b in ev)[len(ev) // 2]
        t0 = time.perf_counter()
        for i in range(n_calls):
            call(batches[i % n_batches])
        t_issue = time.perf_counter() - t0
        torch.cuda.synchronize()
        t_done = time.perf_counter() - t0
        us_done, us_host = 1e6 * t_done / n_calls, 1e6 * t_issue / n_calls
        gbs = bytes_per_call / (us_done * 1e-6) / 1e9
        gbs_dev = bytes_per_call / (dev_us * 1e-6) / 1e9
        res[name] = {"pairs_per_call": Bc, "distinct_batches": n_batches, "bytes_per_call": bytes_per_call,
                     "us_per_call_device": dev_us, "us_per_call_completed": us_done, "us_per_call_host_issue": us_host,
                     "pairs_per_s": Bc / (us_done * 1e-6),
                     "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                                  "frac_device_time_only": gbs_dev / HBM_PEAK_GBS}}
        del batches
        torch.cuda.empty_cache()

    def colbert_batch_maker(Qc, Dc, Ec, dt):
        def make():
            q = (torch.randn(Bc, Qc, Ec, generator=g, device=dev) / Ec ** 0.5).to(dt)
            d = (torch.randn(Bc, Dc, Ec, generator=g, device=dev) / Ec ** 0.5).to(dt)
            return q, d, torch.ones(Bc, Qc, dtype=torch.long, device=dev), torch.ones(Bc, Dc, dtype=torch.long, device=dev)
        return make

    run("colbert_dim128_bf16", 16, colbert_batch_maker(Q, D, E, torch.bfloat16), lambda b: ColBERT._score(*b),
        Bc * ((D + Q) * E * 2 + 8 * (D + Q) + 4))
    # the same calls replayed from HIP graphs (one captured call per resident batch): what rerank.evaluate_batches(graph=True)
    # does per batch shape — the Python + launch path of a call becomes one graph launch
    try:
        make = colbert_batch_maker(Q, D, E, torch.bfloat16)
        batches = [make() for _ in range(16)]
        graphs = []
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for b in batches:
                ColBERT._score(*b)
        torch.cuda.current_stream().wait_stream(side)
        for b in batches:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                o = ColBERT._score(*b)
            graphs.append((gr, o))
        want = ColBERT._score(*batches[3])
        graphs[3][0].replay()
        same = bool(torch.equal(want, graphs[3][1]))
        torch.cuda.synchronize()
        n_calls = 400
        t0 = time.perf_counter()
        for i in range(n_calls):
            graphs[i % 16][0].replay()
        t_issue = time.perf_counter() - t0
        torch.cuda.synchronize()
        t_done = time.perf_counter() - t0
        byc = Bc * ((D + Q) * E * 2 + 8 * (D + Q) + 4)
        res["colbert_dim128_bf16"]["graph_replay"] = {
            "us_per_call_completed": 1e6 * t_done / n_calls, "us_per_call_host_issue": 1e6 * t_issue / n_calls,
            "frac": byc / (t_done / n_calls) / 1e9 / HBM_PEAK_GBS, "replayed_scores_equal_eager": same,
            "what": "torch.cuda.CUDAGraph of one ColBERT._score call per resident batch, replayed back to back"}
        del batches, graphs
        torch.cuda.empty_cache()
    except Exception as e:
        res["colbert_dim128_bf16"]["graph_replay"] = {"error": repr(e)[:300]}
    # the batched entry (mm_maxsim_fwd_batched: ColBERT.score_batches / rerank.evaluate_batches(score_group=16)): sixteen resident
    # batches per launch — for a caller that holds the token vectors of several batches; bit-equal scores (checked here)
    try:
        make = colbert_batch_maker(Q, D, E, torch.bfloat16)
        batches = [make() for _ in range(32)]
        groups = [batches[i:i + 16] for i in range(0, 32, 16)]
        got = ColBERT.score_batches(groups[0])
        same = all(bool(torch.equal(x, ColBERT._score(*b))) for x, b in zip(got, groups[0]))
        for _ in range(5):
            for gr in groups:
                ColBERT.score_batches(gr)
        torch.cuda.synchronize()
        n_calls = 200
        t0 = time.perf_counter()
        for i in range(n_calls):
            ColBERT.score_batches(groups[i % 2])
        t_issue = time.perf_counter() - t0
        torch.cuda.synchronize()
        t_done = time.perf_counter() - t0
        byc = Bc * ((D + Q) * E * 2 + 8 * (D + Q) + 4)
        res["colbert_dim128_bf16"]["batched_entry"] = {
            "batches_per_launch": 16, "us_per_call_completed": 1e6 * t_done / n_calls / 16, "us_per_call_host_issue": 1e6 * t_issue / n_calls / 16,
            "frac": 16 * byc / (t_done / n_calls) / 1e9 / HBM_PEAK_GBS, "scores_bit_equal_to_per_batch_calls": same,
            "what": "ColBERT.score_batches: sixteen 512-pair batches per mm_maxsim_fwd_batched launch; us per 512-pair batch"}
        del batches, groups, got
        torch.cuda.empty_cache()
    except Exception as e:
        res["colbert_dim128_bf16"]["batched_entry"] = {"error": repr(e)[:300]}
    run("colbert_published_dim768_fp16", 3, colbert_batch_maker(38, 200, 768, torch.float16), lambda b: ColBERT._score(*b),
        Bc * ((200 + 38) * 768 * 2 + 8 * (200 + 38) + 4))
    prm = [torch.tensor(MU, device=dev), torch.full((11,), 0.1, device=dev), torch.ones(11, device=dev),
           torch.linspace(-0.014, 0.014, 11, device=dev)]

    def tk_make():
        return (torch.randn(Bc, 20, 300, generator=g, device=dev), torch.randn(Bc, 200, 300, generator=g, device=dev),
                torch.ones(Bc, 20, device=dev), torch.ones(Bc, 200, device=dev))
    run("tk_dim300_fp32", 4, tk_make, lambda b: ops.kernel_pool(b[0], b[1], b[2], b[3], *prm, pairs_per_query=1),
        Bc * ((200 + 20) * 300 * 4 + 4 * (200 + 20) + 4))
    ac.__exit__(None, None, None)
    return {"workload": "512 pairs per call (defaults.yaml:115 batch_size_eval), under autocast as eval.py:83 runs them, pair-per-row, int64 HF masks (ColBERT) / float masks (TK); "
                        "config-2 shapes, the published checkpoint's shapes (Q=38 / D=200 / dim=768 fp16), TK Q=20 / D=200 / dim=300",
            "shapes": res}


def extra_published_checkpoint(steps, cpu_budget):
    """The configuration of the reference's PUBLISHED ColBERT checkpoint (config/huggingface_modelhub/sebastian-hofstaetter/
    colbert-distilbert-margin_mse-T2-msmarco.yaml: colbert_compression_dim 768, max_query_length 30 +
    query_augment_mask_number 8 -> Q = 38, max_doc_length 200, use_fp16) in eval.py's batch layout (ColBERT._score)."""
    import torch
    from matchmaker_amd.colbert import ColBERT
    dev = torch.device("cuda", torch.cuda.current_device())
    n, Qp, Dp, Ep = 16000, 38, 200, 768
    g = torch.Generator(device=dev).manual_seed(768)
    qp = (torch.randn(n, Qp, Ep, generator=g, device=dev) / Ep ** 0.5).half()
    dp = (torch.randn(n, Dp, Ep, generator=g, device=dev) / Ep ** 0.5).half()
    qm = torch.ones(n, Qp, dtype=torch.long, device=dev)
    dm = torch.ones(n, Dp, dtype=torch.long, device=dev)
    with torch.autocast("cuda", dtype=torch.float16):      # use_fp16 (colbert.py:60): fp16 maxima, fp32 sums
        ms = gpu_time_ms(lambda: ColBERT._score(qp, dp, qm, dm), steps)
    by = n * ((Dp + Qp) * Ep * 2 + 8 * (Dp + Qp) + 4)
    gbs = by / (ms * 1e-3) / 1e9
    out = {"workload": f"{n} pairs in the reference's batch layout, Q={Qp} (30 + 8 [MASK]) / D={Dp} / dim={Ep}, fp16, int64 HF masks",
           "dtype": "f16", "ms": ms, "pairs_per_s": n / (ms * 1e-3), "algorithmic_bytes": by,
           "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS},
           "kernel": "pack_mask_kernel + maxsim_stream_kernel with two query tiles (NSL = 6, NQT = 2)",
           "profile": "profiles/r04_published_checkpoint_trace.json"}
    if cpu_budget > 0:
        from oracle import torch_port as TP
        m = 256
        qc, dc, qmc, dmc = qp[:m].float().cpu(), dp[:m].float().cpu(), qm[:m].cpu(), dm[:m].cpu()

        def run():
            with torch.no_grad():
                TP.maxsim_forward(qc, dc, qmc, dmc)
        (ra, na, ta), (r1, n1, t1), threads = both_thread_settings(lambda: run, cpu_budget, m)
        out["cpu_baseline"] = {"value": ra, "unit": "pairs/s", "cores": threads, "kind": "port",
                               "sample": f"{m}-pair batches (oracle/torch_port.maxsim_forward, fp32), {na} calls in {ta:.1f} s",
                               "one_thread": {"value": r1, "cores": 1}}
    return out


def extra_all_pairs(steps, cpu_budget):
    """forward_inbatch_aggregation (colbert.py:154-162) at a teacher batch far beyond the reference's 32 x 32:
    1024 queries x 1024 documents, Q=32 / D=180 / dim=128, bf16, the documents' own masks.  MFMA-shaped: every
    (query, document) pair is a 32 x 180 x 128 product and the documents (47 MB) stay in the Infinity Cache."""
    import torch
    from matchmaker_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    Bq = Bd = 1024
    g = torch.Generator(device=dev).manual_seed(1414)
    q = (torch.randn(Bq, Q, E, generator=g, device=dev) / E ** 0.5).bfloat16()
    d = (torch.randn(Bd, D, E, generator=g, device=dev) / E ** 0.5).bfloat16()
    qm = torch.ones(Bq, Q, dtype=torch.long, device=dev)
    dm = torch.ones(Bd, D, dtype=torch.long, device=dev)     # every position real: the flop count below is what runs
    fn = lambda: ops.maxsim_inbatch(q, qm, d, dm, bug_compatible=False)
    ms = gpu_time_ms(fn, steps)
    flop = 2.0 * Bq * Bd * Q * D * E
    t = ms * 1e-3
    out = {"workload": f"all-pairs MaxSim (colbert.py:154-162), {Bq} queries x {Bd} documents, Q={Q}/D={D}/dim={E}, bf16, "
                       f"all positions real, int64 masks",
           "dtype": "bf16", "ms": ms, "pairs_per_s": Bq * Bd / t, "flop": flop,
           "roofline": {"bound": "mfma", "achieved": flop / t / 1e12, "peak": MFMA_PEAK_16BIT / 1e12, "unit": "TFLOP/s",
                        "frac": flop / t / MFMA_PEAK_16BIT},
           "kernel": "maxsim_allpairs_wg_kernel: 4 wavefronts x 4 queries share one document ring", "profile": "profiles/r03_all_pairs_pmc.json"}
    if not LEAN:
        t0 = gpu_time_ms(lambda: ops.maxsim_inbatch(q[:32], qm[:32], d[:32], dm[:32], bug_compatible=True), steps)
        out["reference_batch_32x32"] = {"ms": t0, "note": "dynamic_teacher.py:245-276 calls it with batch_size_train = 32, bug-compatible masks"}
        # the vendor GEMM on this box: the same product with the [Bq Q, Bd D] score matrix WRITTEN (what colbert.py:154 does
        # before its max / sum passes) and a square 8192^3 (the matrix rate the board's power budget allows)
        out["vendor_gemm"] = vendor_gemm_tflops({"same_product_score_matrix_written_bf16": (Bq * Q, Bd * D, E, torch.bfloat16),
                                                 "square_8192_bf16": (8192, 8192, 8192, torch.bfloat16)})
        out["vendor_gemm"]["this_kernel_over_same_product"] = (flop / t / 1e12) / out["vendor_gemm"]["same_product_score_matrix_written_bf16"]["tflops"]
        out["vendor_gemm"]["this_kernel_over_square_8192"] = (flop / t / 1e12) / out["vendor_gemm"]["square_8192_bf16"]["tflops"]
    if cpu_budget > 0:
        from oracle import torch_port as TP
        n = 64
        qc, dc, qmc, dmc = q[:n].float().cpu(), d[:n].float().cpu(), qm[:n].cpu(), dm[:n].cpu()

        def run():
            with torch.no_grad():
                TP.maxsim_inbatch(qc, qmc, dc, dmc, bug_compatible=False)
        (ra, na, ta), (r1, n1, t1), threads = both_thread_settings(lambda: run, cpu_budget, n * n)
        out["cpu_baseline"] = {"value": ra, "unit": "pairs/s", "cores": threads, "kind": "port",
                               "sample": f"{n} x {n} all-pairs blocks (oracle/torch_port.py, fp32), {na} calls in {ta:.1f} s",
                               "one_thread": {"value": r1, "cores": 1}}
    return out


def extra_dot_topk(steps, cpu_budget):
    """BASELINE.json configs[4], ONE rank's shard: 8,841,823 / 8 passages x dim 768 fp16 against all 6,980 queries,
    exact top-1000 (faiss IndexFlatIP semantics)."""
    import torch
    from matchmaker_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    N, Ed, nq, k = 1105228, 768, 6980, 1000
    g = torch.Generator(device=dev).manual_seed(5005)
    c = torch.empty((N, Ed), dtype=torch.float16, device=dev)
    for s in range(0, N, 1 << 18):
        n = min(1 << 18, N - s)
        c[s:s + n] = torch.randn(n, Ed, generator=g, device=dev).half()
    q = torch.randn(nq, Ed, generator=g, device=dev).half()
    ops.dot_topk(q, c, k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ops.dot_topk(q, c, k)
    torch.cuda.synchronize()
    t = (time.perf_counter() - t0) / steps
    flop = 2.0 * nq * N * Ed
    out = {"workload": f"brute-force inner-product top-{k} (faiss_indices.py:49-74, dense_retrieval.py:391): one rank's shard "
                       f"of configs[4] = {N} passages x dim {Ed} fp16, {nq} queries",
           "dtype": "fp16 (fp32 accumulation)", "ms": t * 1e3, "queries_per_s": nq / t, "flop": flop,
           "roofline": {"bound": "mfma", "achieved": flop / t / 1e12, "peak": MFMA_PEAK_16BIT / 1e12, "unit": "TFLOP/s",
                        "frac": flop / t / MFMA_PEAK_16BIT},
           "kernel": "dot_stream_kernel (sample + filter) + sample_tau_kernel + topk_rows_kernel (whole mm_dot_topk_fwd call, wall clock)",
           "profile": "profiles/r06_dot_topk_trace.json (counters: profiles/r06_dot_topk_pmc.json — the filter launch keeps the matrix pipe busy for 0.64 of its cycles at a 1.70 GHz delivered clock; by-removal and phase history: profiles/r06_experiments/dot_topk_filing_history.txt)"}
    if not LEAN:
        # what the vendor GEMM reaches on THIS box: the same product (one 262,144-passage slice, fp16 scores written, no
        # top-k) and a square 8192^3 — the matrix rate the board's power budget allows, next to the 2.5 PFLOP/s nominal peak
        out["vendor_gemm"] = vendor_gemm_tflops({"same_product_262144_passages_fp16": (nq, 1 << 18, Ed, torch.float16),
                                                 "square_8192_bf16": (8192, 8192, 8192, torch.bfloat16)})
        out["vendor_gemm"]["this_call_over_same_product"] = (flop / t / 1e12) / out["vendor_gemm"]["same_product_262144_passages_fp16"]["tflops"]
        out["vendor_gemm"]["this_call_over_square_8192"] = (flop / t / 1e12) / out["vendor_gemm"]["square_8192_bf16"]["tflops"]
    if cpu_budget > 0:
        nqc, nc = 64, 1 << 16
        qc, cc = q[:nqc].float().cpu(), c[:nc].float().cpu()

        def search():
            with torch.no_grad():
                torch.topk(qc @ cc.T, k, dim=1)
        (ra, na, ta), (r1, n1, t1), threads = both_thread_settings(lambda: search, cpu_budget, nqc * nc)
        out["cpu_baseline"] = {"value": ra, "unit": "query-passage inner products/s", "cores": threads, "kind": "port",
                               "single_thread_value": r1, "gpu_value_same_unit": nq * N / t,
                               "sample": f"{nqc} queries x {nc} passages per call (fp32 torch matmul + topk = IndexFlatIP.search's "
                                         f"definition; faiss is absent here), {na} calls in {ta:.1f} s ({threads} threads) / {n1} in "
                                         f"{t1:.1f} s (1 thread)"}
    return out


def extra_train_step(steps, cpu_budget):
    """The training path (train.py:347-348 forward, :503-524 loss.backward()) through the native operators: forward +
    backward of ColBERT._score (fp16 autocast, defaults.yaml:21), ECAI20_TK's pooling block and TKL's scoring, at
    `batch_size_train: 32` x 2 (positive + negative documents, defaults.yaml:114) and at 2,048 pairs.  Beside each: the same
    step through the reference's own torch statements (oracle/torch_port.py) with autograd ON THIS GPU — the stated eager
    baseline, not a product path.  Bytes: the forward's reads, the backward's re-read of the same operands (nothing is
    saved: the match matrix is recomputed) and the fp32 gradients written."""
    import torch
    from oracle import torch_port as TP
    from matchmaker_amd import ops, synth
    from matchmaker_amd.colbert import ColBERT
    from matchmaker_amd.tk import kernel_pool_train
    from matchmaker_amd.tkl import TKL_sigir20, chunk_documents, tkl_score_train
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {}

    def leg(name, B, fwd, step_native, step_eager, fwd_bytes, grad_bytes, n_timed, bwd_op=None, fwd_bytes_padded=None):
        with torch.no_grad():
            f_ms = gpu_time_ms(fwd, n_timed)
            b_ms = gpu_time_ms(bwd_op, n_timed) if bwd_op is not None else None
        s_ms = gpu_time_ms(step_native, n_timed)
        by = 2 * fwd_bytes + grad_bytes
        row = {"pairs": B, "forward_us": 1e3 * f_ms, "step_us": 1e3 * s_ms, "backward_over_forward": (s_ms - f_ms) / f_ms,
               # the backward operator called directly (no autograd engine around it): what the device spends once the
               # call is large enough to hide the host (the `step` of a 64- or 2,048-pair ColBERT batch is host-bound)
               "backward_op_us": None if b_ms is None else 1e3 * b_ms,
               "backward_op_over_forward": None if b_ms is None else b_ms / f_ms,
               # device time of the step's kernels (forward + backward operator, each timed back to back) and what is left of
               # the step: Python + autograd engine + launch gaps.  (ColBERT's node is C++ since round 5, csrc_host/mm_autograd.cpp:
               # with the Python autograd.Function the 64-pair step was ~150 us around ~45 us of kernels.)
               "kernel_us": None if b_ms is None else 1e3 * (f_ms + b_ms),
               "host_us": None if b_ms is None else max(0.0, 1e3 * (s_ms - f_ms - b_ms)),
               "algorithmic_bytes": by,
               "roofline": {"bound": "hbm", "achieved": by / (s_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": by / (s_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}}
        if fwd_bytes_padded is not None:     # the kernels skip the 32-row blocks past a document's length: `frac` prices the rows they need
            row["roofline"]["frac_padded_bytes"] = (2 * fwd_bytes_padded + grad_bytes) / (s_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
        if B <= 2048 and bwd_op is not None:
            # The step's two operator calls (forward, backward — no autograd engine: capturing loss.backward() is not something
            # train.py does either) captured once into a hipGraph and replayed: what the DEVICE needs for them back to back.  In
            # train.py these launches queue behind the encoder's, so this — not the host-bound eager interval above — is what a
            # small batch adds to an iteration.  (Not `step_us`: the reference's loop is eager, and so is this leg's headline.)
            try:
                def both():
                    fwd()
                    bwd_op()
                with torch.no_grad():
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        for _ in range(3):
                            both()
                    torch.cuda.current_stream().wait_stream(side)
                    torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        both()
                    g_ms = gpu_time_ms(graph.replay, n_timed)
                row["graphed_kernels_us"] = 1e3 * g_ms
                row["graphed_kernels_over_forward"] = g_ms / f_ms
                del graph
            except Exception as e:
                row["graphed_kernels_us"] = None
                row["graphed_kernels_error"] = repr(e)[:200]
                torch.cuda.synchronize()
        try:
            if LEAN:
                raise RuntimeError("skipped (--lean: the profiled run holds the native kernels only)")
            e_ms = gpu_time_ms(step_eager, max(3, n_timed // 2), warm_ms=20.0, timed_ms=15.0, max_calls=50)
            row["eager_gpu_baseline"] = {"step_us": 1e3 * e_ms, "kind": "port",
                                         "what": "oracle/torch_port.py statements + torch autograd on this GPU",
                                         "native_speedup": e_ms / s_ms}
        except Exception as e:      # (an out-of-memory eager step at 2,048 TKL documents is a result, not a failure)
            row["eager_gpu_baseline"] = {"error": repr(e)[:200]}
            torch.cuda.empty_cache()
        res.setdefault(name, {})[f"pairs_{B}"] = row

    # (64 and 2,048 pairs are HOST-bound for ColBERT: ~190 us of Python + autograd engine per step whatever the batch — the
    # event interval around a step includes the idle gaps; 32,768 pairs shows the device-side ratio of the same kernels)
    for B in (64, 2048, 32768):
        # ---- ColBERT: fp16 token vectors as the compressor emits them under autocast, int64 HF masks
        g = torch.Generator(device=dev).manual_seed(64 + B)
        q = torch.nn.functional.normalize(torch.randn(B, Q, E, generator=g, device=dev), dim=-1).half().requires_grad_(True)
        d = torch.nn.functional.normalize(torch.randn(B, D, E, generator=g, device=dev), dim=-1).half().requires_grad_(True)
        qm = synth.len_to_mask(torch.randint(4, Q + 1, (B,), generator=g, device=dev), Q)
        dm = synth.len_to_mask(synth.msmarco_doc_lengths(B, D, g, dev), D)
        go = torch.randn(B, generator=g, device=dev)

        def c_fwd():
            with torch.autocast("cuda", dtype=torch.float16):
                return ColBERT._score(q, d, qm, dm)

        def c_native():
            q.grad = d.grad = None
            with torch.autocast("cuda", dtype=torch.float16):
                ColBERT._score(q, d, qm, dm).backward(go)

        def c_eager():
            q.grad = d.grad = None
            with torch.autocast("cuda", dtype=torch.float16):
                TP.maxsim_forward(q, d, qm, dm).backward(go)
        # bytes: forward and backward each read the 32-row document blocks below the (MSMARCO-shaped) lengths — the kernels skip the
        # rest — + the query tiles and int64 masks; the backward writes EVERY gradient row (zeros past the length)
        rows_c = int((((dm.sum(1) + 31) // 32) * 32).clamp(max=D).sum())
        small_c = B * (Q * E * 2 + 8 * (D + Q) + 4)
        leg("colbert_fp16_autocast_q32_d180_e128", B, c_fwd, c_native, c_eager, rows_c * E * 2 + small_c,
            B * (D + Q) * E * 2, steps, bwd_op=lambda: ops.maxsim_bwd(q, d, qm, dm, go, grad_dtype=q.dtype),
            fwd_bytes_padded=B * D * E * 2 + small_c)
        del q, d

        # ---- TK pooling (tk.yaml: fp32, Q = 20 / D = 200 / dim = 300)
        Qt, Dt, Et = 20, 200, 300
        tq = torch.randn(B, Qt, Et, generator=g, device=dev).requires_grad_(True)
        td = torch.randn(B, Dt, Et, generator=g, device=dev).requires_grad_(True)
        tqm = synth.len_to_mask(torch.randint(3, Qt + 1, (B,), generator=g, device=dev), Qt, torch.float32)
        tdm = synth.len_to_mask(torch.randint(10, Dt + 1, (B,), generator=g, device=dev), Dt, torch.float32)
        mu, sg = torch.tensor(MU, device=dev), torch.full((11,), 0.1, device=dev)
        al = torch.ones(11, device=dev, requires_grad=True)
        w = torch.linspace(-0.014, 0.014, 11, device=dev).requires_grad_(True)
        leaves = (tq, td, al, w)

        def zero():
            for t in leaves:
                t.grad = None

        def t_fwd():
            return ops.kernel_pool(tq, td, tqm, tdm, mu, sg, al, w)

        def t_native():
            zero()
            kernel_pool_train(tq, td, tqm, tdm, mu, sg, al, w).backward(go)      # (the C++ node when the host extension is built)

        def t_eager():
            zero()
            TP.tk_kernel_pool(tq, td, tqm, tdm, mu.view(1, 1, 1, -1), sg.view(1, 1, 1, -1), al.view(1, 1, -1), w.view(1, -1)).backward(go)
        # The backward operator as the step runs it: with the forward's pooled kernel sums (mm_kernel_pool_ex_fwd2 -> _ex_bwd2).
        # Bytes: forward and backward each read the 32-row blocks below a document's length (the kernels skip the rest), the
        # backward writes EVERY gradient row (zeros past the length).
        with torch.no_grad():
            pooled = ops.kernel_pool(tq, td, tqm, tdm, mu, sg, al, w, return_pooled=True)[1]
        rows = int((((tdm.sum(1).long() + 31) // 32) * 32).clamp(max=Dt).sum())
        small = B * (Qt * Et * 4 + 4 * (Dt + Qt) + 4)
        leg("tk_pooling_q20_d200_e300", B, t_fwd, t_native, t_eager, rows * Et * 4 + small,
            B * (Dt + Qt) * Et * 4 + 2 * B * 11 * 4, steps,
            bwd_op=lambda: ops.kernel_pool_bwd(tq, td, tqm, tdm, mu, sg, al, w, go, pooled=pooled),
            fwd_bytes_padded=B * Dt * Et * 4 + small)
        del pooled
        del tq, td
        torch.cuda.empty_cache()

    # ---- TKL scoring (tkl.yaml: fp32, D = 2048, dim = 300, Q = 20): documents are the unit
    Qt, Dt, Et = 20, 2048, 300
    m = TKL_sigir20(Et, MU, [0.1] * 11, 10, 2, 300, 2000, True, True, "embedding").to(dev)
    for B in (64, 2048):
        g = torch.Generator(device=dev).manual_seed(640 + B)
        d_len = torch.randint(50, Dt + 1, (B,), generator=g, device=dev)
        q_len = torch.randint(3, Qt + 1, (B,), generator=g, device=dev)
        qm = synth.len_to_mask(q_len, Qt, torch.float32)
        dm = synth.len_to_mask(d_len, Dt, torch.float32)
        dd = torch.randn(B, Dt, Et, generator=g, device=dev) * dm.unsqueeze(-1)
        chunks, cmask, slot, C = chunk_documents(dd, dm)
        del dd
        chunks = chunks.requires_grad_(True)
        q_ctx = (torch.randn(B, Qt, Et, generator=g, device=dev) * qm.unsqueeze(-1)).requires_grad_(True)
        go = torch.randn(B, generator=g, device=dev)
        scoring, sizes = m._pack_layout()
        packed = m.pack_params()
        P = chunks.shape[0]

        def zero():
            q_ctx.grad = chunks.grad = None
            for t in scoring:
                t.grad = None

        from matchmaker_amd.tkl import _layout_tensor
        layout = _layout_tensor(sizes)          # (cached by the model between steps: TKL_sigir20.forward)

        def l_fwd():
            return ops.tkl_score(q_ctx, chunks, cmask, slot, qm, packed, B, C, 11, "embedding", check_order=False)

        def l_native():
            zero()
            tkl_score_train(q_ctx, chunks, cmask, slot, qm, packed, B, C, 11, "embedding", scoring, sizes, layout)[0].backward(go)      # (the C++ node when the host extension is built)

        prm = {"mu": m.mu, "sigma": m.sigma, "dense_w": m.dense.weight, "sat_w1": m.saturation_linear.weight,
               "sat_b1": m.saturation_linear.bias, "sat_w2": m.saturation_linear2.weight, "sat_b2": m.saturation_linear2.bias,
               "sat_w3": m.saturation_linear3.weight, "sat_b3": m.saturation_linear3.bias, "ln_w": m.sat_normer.weight,
               "ln_b": m.sat_normer.bias, "emb_reduce_w": m.sat_emb_reduce1.weight, "kernel_mult0": m.kernel_mult[0],
               "chunk_scoring": m.chunk_scoring}
        prm = {k: v.reshape(-1) for k, v in prm.items()}
        packed_idx = torch.zeros(B * C, dtype=torch.bool, device=dev)
        packed_idx[slot.long()] = True
        cm40 = cmask[:, 5:-5].float().contiguous()

        def l_eager():
            zero()
            TP.tkl_scoring(q_ctx, chunks[:, 5:-5], cm40, packed_idx, B, qm, prm, "embedding")[0].backward(go)
        fwd_bytes = P * 50 * Et * 4 + B * Qt * Et * 4 + P * 50 * 4 + 4 * B
        # the exact gradient touches at most 15 windows x 30 positions per document; grad_chunks is a full zero-filled tensor
        with torch.no_grad():
            win0 = ops.tkl_score(q_ctx, chunks, cmask, slot, qm, packed, B, C, 11, "embedding", return_windows=True, check_order=False)[1]
        leg("tkl_scoring_d2048_e300", B, l_fwd, l_native, l_eager, fwd_bytes, P * 50 * Et * 4 + B * Qt * Et * 4, max(3, steps // 2),
            bwd_op=lambda: ops.tkl_bwd(q_ctx, chunks, cmask, slot, qm, packed, win0, go, B, C, 11, "embedding"))
        del chunks, q_ctx
        torch.cuda.empty_cache()
    res["note"] = ("step = forward + backward of the scoring block alone (encoders / contextualisers are PyTorch on both sides and "
                   "not part of it); TKL's backward recomputes only the <= 15 windows per document that carry gradient")
    res["profile"] = "profiles/r06_train_step_trace.json (the pooling backward alone: profiles/r06_tk_bwd_trace.json, r06_tk_bwd_pmc.json, r06_tk_bwd_phases.txt)"
    return res


def extra_ragged_aggregate(steps, cpu_budget):
    """SURVEY.md §8 f-3, the ColBERT retrieval aggregate (dense_retrieval.py:398-412): candidates gathered from the resident
    token store (token_reps_N.npy rows, MSMARCO-length passages, fp16, dim 128) and scored by ONE mm_maxsim_ragged_fwd
    launch under the searcher head's autocast (sim_round) — against the reference's structure, one
    forward_aggregation call per candidate (here through the drop-in's own method, i.e. already on the native kernel)."""
    import torch
    from matchmaker_amd import ops, synth
    from matchmaker_amd.colbert import ColBERT
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(3131)
    n_docs, nq, C = 2_000_000, 64, CANDS
    lens = synth.msmarco_doc_lengths(n_docs, D, g, dev).long()
    end = torch.cumsum(lens, 0)
    begin = end - lens
    T = int(end[-1])
    tokens = torch.empty((T, E), dtype=torch.float16, device=dev)
    for s0 in range(0, T, 1 << 24):
        n = min(1 << 24, T - s0)
        tokens[s0:s0 + n] = torch.nn.functional.normalize(torch.randn(n, E, generator=g, device=dev), dim=-1).half()
    q = torch.nn.functional.normalize(torch.randn(nq, Q, E, generator=g, device=dev), dim=-1).half()
    cand = torch.randint(0, n_docs, (nq, C), generator=g, device=dev)
    bb, ee = begin[cand].reshape(-1).contiguous(), end[cand].reshape(-1).contiguous()
    fn = lambda: ops.maxsim_ragged(q, tokens, bb, ee, None, pairs_per_query=C, check_ranges=False, sim_round=True)
    ms = gpu_time_ms(fn, steps)
    by = int((ee - bb).sum()) * E * 2 + nq * Q * E * 2 + 16 * nq * C + 4 * nq * C
    one = lambda: ops.maxsim_ragged(q[:1], tokens, bb[:C], ee[:C], None, pairs_per_query=C, check_ranges=False, sim_round=True)
    ms1 = gpu_time_ms(one, steps)
    out = {"workload": f"{nq} queries x {C} candidates per launch gathered from a resident store of {n_docs} passages "
                       f"({T} token rows, {T * E * 2 / 1e9:.1f} GB fp16, lengths N(70, 25) clipped to [8, {D}]), Q={Q}/dim={E}",
           "dtype": "f16 (fp16 maxima, fp32 sums: the searcher head's autocast)", "ms": ms, "pairs_per_s": nq * C / (ms * 1e-3),
           "algorithmic_bytes": by,
           "roofline": {"bound": "hbm", "achieved": by / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
           "one_query_1000_candidates_us": 1e3 * ms1,
           "kernel": "maxsim_stream_kernel<RAG> (CSR ranges into the store, no gather, no padding)",
           "profile": "profiles/r06_ragged_aggregate_trace.json"}
    if not LEAN:
        # the reference's loop: one forward_aggregation per candidate (dense_retrieval.py:400-410), 1000 calls for one query
        m = ColBERT.__new__(ColBERT)
        torch.nn.Module.__init__(m)
        b0, e0 = bb[:C].tolist(), ee[:C].tolist()

        def loop():
            with torch.autocast("cuda", dtype=torch.float16):
                for a, b in zip(b0, e0):
                    m.forward_aggregation(q[:1], tokens[a:b].unsqueeze(0))
        with torch.no_grad():
            loop()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop()
            torch.cuda.synchronize()
            t_loop = time.perf_counter() - t0
        out["per_candidate_loop"] = {"us_per_query_of_1000_candidates": 1e6 * t_loop,
                                     "what": "1000 forward_aggregation calls (colbert.py:100-112 via the drop-in), wall clock",
                                     "one_launch_speedup": 1e6 * t_loop / (1e3 * ms1)}
    if cpu_budget > 0:
        from oracle import torch_port as TP
        n = 200
        qc = q[:1].float().cpu()
        docs = [tokens[int(bb[i]):int(ee[i])].float().cpu().unsqueeze(0) for i in range(n)]

        def run():
            with torch.no_grad():
                for dv in docs:
                    TP.maxsim_aggregation(qc, dv)
        (ra, na, ta), (r1, n1, t1), threads = both_thread_settings(lambda: run, cpu_budget, n)
        out["cpu_baseline"] = {"value": ra, "unit": "pairs/s", "cores": threads, "kind": "port", "single_thread_value": r1,
                               "sample": f"{n} candidates of one query per call, one oracle/torch_port.maxsim_aggregation call per "
                                         f"candidate as dense_retrieval.py:400-410 loops, {na} calls in {ta:.1f} s"}
    del tokens
    torch.cuda.empty_cache()
    return out


def extra_variants(steps, cpu_budget):
    """the kernel-pooling variants at the shapes their configs give them (max_query_length 30 /
    max_doc_length 200, defaults.yaml:126-127; 11 kernels), 64 queries x 1000 candidates each, on the pooling kernels:
    KNRM (300-d embeddings), Conv-KNRM (3 n-gram widths -> 9 match matrices of 128-d vectors in ONE launch), TK-Sparse
    (TK + the stop-word gate) and IDCM's passage sampler (64-token passages, floor 1e-4 + bias; "ck" 768-d, "ck-small" 128-d)."""
    import torch
    from matchmaker_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    nq, C = 64, 1000
    B = nq * C
    g = torch.Generator(device=dev).manual_seed(9090)
    prm = [torch.tensor(MU, device=dev), torch.full((11,), 0.1, device=dev), torch.ones(11, device=dev),
           torch.linspace(-0.014, 0.014, 11, device=dev)]
    res = {}

    def one(name, Qv, Dv, Ev, n_d=1, gate=False, clamp=1e-10, n_q=1, ref="", kern=None, pats=("r06*variants*pmc*.json",)):
        q = [torch.randn(nq if n_q == 1 and n_d == 1 else B, Qv, Ev, generator=g, device=dev) for _ in range(n_q)]
        d = [torch.randn(B, Dv, Ev, generator=g, device=dev) for _ in range(n_d)]
        q_len = torch.randint(3, Qv + 1, (q[0].shape[0],), generator=g, device=dev).to(torch.int32)
        d_len = torch.randint(max(8, Dv // 4), Dv + 1, (B,), generator=g, device=dev).to(torch.int32)
        if n_d > 1:
            w9 = torch.linspace(-0.014, 0.014, 11 * n_q * n_d, device=dev)
            fn = lambda: ops.kernel_pool_multi(q, d, q_len, d_len, prm[0], prm[1], prm[2], w9)
        else:
            gt = torch.relu(torch.randn(B, Dv, generator=g, device=dev)) if gate else None
            fn = lambda: ops.kernel_pool(q[0], d[0], q_len, d_len, *prm, pairs_per_query=C, d_gate=gt, clamp_min=clamp)
        ms = gpu_time_ms(fn, steps)
        # The kernels skip the 32-row blocks past a document's length, so the bytes the call NEEDS are the rows of the blocks
        # below the lengths (+ queries, lengths, gate rows, scores).  `frac` prices those: a fraction the memory system could
        # deliver.  Rounds 1-5 printed the padded bytes over the same time (0.92-0.96 for kernels that read 0.70 of them:
        # VERDICT r5 weak item 1); that figure stays as `frac_padded_bytes`.
        rows = int(((d_len + 31) // 32 * 32).clamp(max=Dv).sum())
        small = sum(t.numel() for t in q) * 4 + 4 * (B + q[0].shape[0]) + 4 * B
        by = n_d * B * Dv * Ev * 4 + small + (B * Dv * 4 if gate else 0)
        need = n_d * rows * Ev * 4 + small + (rows * 4 if gate else 0)
        roof = {"bound": "hbm", "achieved": need / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": need / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "needed_bytes": need,
                "frac_padded_bytes": by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None}
        tr = None
        for pat in pats:
            tr = tr or (profile_summary(pat, kern, "_hbm_traffic_bytes_per_dispatch") if kern else None)
        if tr is not None:
            roof["traffic"] = tr[0]
            roof["traffic_over_needed"] = tr[0] / need
            roof["traffic_source"] = f"profiles/{tr[1]} ({kern})"
        res[name] = {"shape_QDE": [Qv, Dv, Ev], "pairs": B, "match_matrices_per_pair": n_q * n_d, "ms": ms,
                     "pairs_per_s": B / (ms * 1e-3), "algorithmic_bytes_padded": by,
                     "bytes_of_rows_below_the_document_lengths": n_d * rows * Ev * 4, "roofline": roof, "reference": ref}
        del q, d
        torch.cuda.empty_cache()

    # MM_BENCH_VARIANTS=a,b: a subset (profiling runs: Conv-KNRM's multi launch and IDCM's ck-small sampler are the SAME kernel
    # instantiation, so their counters can only be told apart in separate processes)
    subset = [x for x in os.environ.get("MM_BENCH_VARIANTS", "").split(",") if x]
    _one = one

    def one(name, *a, **kw):
        if not subset or name in subset:
            _one(name, *a, **kw)
    one("knrm", 30, 200, 300, kern="kernel_pool_split_kernel<3, 11, 3, false, false, false, 1>", ref="models/knrm.py:52-84 (alpha = 1, x 0.01 folded into the weights)")
    one("conv_knrm_3x3", 30, 200, 128, n_d=3, n_q=3, kern="kernel_pool_multi128_kernel<2, 11, 3>", pats=("r06*conv_knrm*pmc*.json",), ref="models/conv_knrm.py:144-170: n_grams^2 = 9 poolings + dense, one launch (pair-per-row)")
    one("tk_sparse", 30, 200, 300, gate=True, kern="kernel_pool_split_kernel<3, 11, 3, false, false, true, 1>", ref="published/cikm20_tk_sparse.py:106-146 (stop-word gate)")
    one("idcm_sampler_ck", 30, 64, 768, clamp=1e-4, kern="kernel_pool_split128_kernel<6,", ref="published/sigir21_idcm.py:182-186, sample_context ck (768-d)")
    one("idcm_sampler_ck_small", 30, 64, 128, clamp=1e-4, kern="kernel_pool_split128_kernel<2,", ref="published/sigir21_idcm.py:182-186, sample_context ck-small (128-d)")
    if cpu_budget > 0:
        from oracle import torch_port as TP
        n = 200
        qc, dc = torch.randn(n, 30, 300), torch.randn(n, 200, 300)
        qm, dm = torch.ones(n, 30), torch.ones(n, 200)
        mu, sg = prm[0].cpu().view(1, 1, 1, -1), prm[1].cpu().view(1, 1, 1, -1)

        def run():
            with torch.no_grad():
                TP.tk_kernel_pool(qc, dc, qm, dm, mu, sg, prm[2].cpu().view(1, 1, -1), prm[3].cpu().view(1, -1))
        (ra, na, ta), (r1, n1, t1), threads = both_thread_settings(lambda: run, cpu_budget, n)
        res["cpu_baseline"] = {"value": ra, "unit": "pairs/s", "cores": threads, "kind": "port", "single_thread_value": r1,
                               "sample": f"KNRM / TK-Sparse shape (Q30 / D200 / 300-d): {n}-pair calls of oracle/torch_port.tk_kernel_pool "
                                         f"(the variants differ from it in constants only), {na} calls in {ta:.1f} s"}
    res["profile"] = "profiles/r06_variants_trace.json, profiles/r06_variants_pmc.json"
    return res


LEGS = (("eval_batch", extra_eval_batch), ("maxsim_fp32", extra_maxsim_fp32), ("published_checkpoint", extra_published_checkpoint),
        ("all_pairs", extra_all_pairs), ("tk", extra_tk), ("tkl", extra_tkl), ("train_step", extra_train_step),
        ("ragged_aggregate", extra_ragged_aggregate), ("variants", extra_variants), ("dot_topk", extra_dot_topk))


# ---- the record the driver reads -------------------------------------------------------------------------------------
# The driver keeps the last ~9 KB of stdout and parses the LAST line.  Round 4's single line had grown to 21.7 KB, so the
# head of it (value, ms_per_step, roofline) was cut off and BENCH_r04.parsed came back null.  The last stdout line is
# therefore a compact record (< 4 KB; tests/test_bench_launch_cpu.py bounds it); the full record with every leg's prose
# goes to gpurun_out/bench_full.json and to an EARLIER stdout line ("FULL_RECORD {...}").
_SLIM_NUM = ("ms", "frac", "us_per_call_completed", "us_per_call_device", "step_us", "forward_us", "kernel_us", "host_us",
             "backward_op_over_forward", "frac_needed_bytes")


def _r4(x):
    if isinstance(x, bool) or x is None:
        return x
    if isinstance(x, float):
        return float(f"{x:.4g}")
    return x


def _slim_leg(leg, depth=0):
    """one `extra` leg -> {ms, frac} (+ the same for the sub-measurements it nests), numbers to 4 significant digits"""
    if not isinstance(leg, dict):
        return None
    if "error" in leg:
        return {"error": str(leg["error"])[:80]}
    out = {}
    for k in _SLIM_NUM:
        if isinstance(leg.get(k), (int, float)):
            out[k] = _r4(leg[k])
    roof = leg.get("roofline")
    if isinstance(roof, dict) and isinstance(roof.get("frac"), (int, float)):
        out["frac"] = _r4(roof["frac"])
        if roof.get("bound") == "mfma":
            out["bound"] = "mfma"
    if depth < 3:
        for k, v in leg.items():
            if k in ("roofline", "cpu_baseline", "vendor_gemm", "hbm_calibration", "eager_gpu_baseline", "graph_replay") \
                    or not isinstance(v, dict):
                continue
            sub = _slim_leg(v, depth + 1)
            if sub:
                out[k] = sub
    return out


def compact_record(out, limit=4000):
    """the LAST stdout line: every key of the bench contract + roofline + cpu_baseline, `extra` reduced to {leg: {ms, frac}}"""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "world_size", "dry", "all_gather_verified")
    c = {k: out[k] for k in keep if k in out}
    cfg = dict(out.get("config") or {})
    if isinstance(cfg.get("workload"), str) and len(cfg["workload"]) > 260:
        cfg["workload"] = cfg["workload"][:257] + "..."
    c["config"] = cfg
    coll = out.get("collective")
    if coll:
        c["collective"] = {k: (v[:100] if isinstance(v, str) else v) for k, v in coll.items() if k != "final_sort"}
        if isinstance(coll.get("final_sort"), dict):
            c["collective"]["final_sort"] = {k: v for k, v in coll["final_sort"].items() if k != "what"}
    else:
        c["collective"] = None
    sc = out.get("self_check")
    if sc:
        c["self_check"] = {k: (_r4(v) if not isinstance(v, str) else v[:120]) for k, v in sc.items()}
    roof = out.get("roofline")
    if roof:
        r = {k: roof[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms", "algorithmic_bytes",
                                  "frac_of_calibrated", "calibrated_stream_GBps") if k in roof}
        mu = roof.get("mfma_util") or {}
        r["mfma_util"] = {k: _r4(mu[k]) for k in ("tflops", "frac_of_dense_bf16_peak", "pmc_busy_frac") if k in mu}
        if "traffic_source" in roof:
            r["traffic_source"] = roof["traffic_source"].split(" ")[0]
        c["roofline"] = r
    cb = out.get("cpu_baseline")
    if cb:
        c["cpu_baseline"] = {k: (v[:120] if isinstance(v, str) else v) for k, v in cb.items()
                             if k in ("value", "unit", "cores", "kind", "cpu_model", "single_thread_value", "sample", "error")}
    extra = out.get("extra")
    if isinstance(extra, dict):
        slim = {}
        for name, leg in extra.items():
            if name in ("wall_s", "hbm_calibration"):
                continue
            sl = _slim_leg(leg)
            if sl:
                slim[name] = sl
        c["extra"] = slim
        c["full_record"] = "gpurun_out/bench_full.json (and the FULL_RECORD stdout line before this one)"
        # hard bound: drop the least important numbers first, then the deepest sub-measurements, then whole legs from the end
        def strip(o, key):
            if isinstance(o, dict):
                o.pop(key, None)
                for v in o.values():
                    strip(v, key)
        for key in ("us_per_call_device", "frac_needed_bytes", "forward_us", "backward_op_over_forward", "kernel_us"):
            if len(json.dumps(c)) <= limit:
                break
            strip(slim, key)
        while len(json.dumps(c)) > limit and any(isinstance(v, dict) and any(isinstance(x, dict) for x in v.values())
                                                  for v in slim.values()):
            name = max(slim, key=lambda n: len(json.dumps(slim[n])))
            slim[name] = {k: v for k, v in slim[name].items() if not isinstance(v, dict)} or {"see": "full_record"}
        while len(json.dumps(c)) > limit and slim:
            slim.pop(next(reversed(slim)))
    return c


def emit(out):
    """full record -> gpurun_out/bench_full.json + an earlier stdout line; compact record = the last stdout line"""
    full = json.dumps(out)
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "bench_full.json"), "w") as f:
            f.write(full + "\n")
    except OSError:
        pass
    print("FULL_RECORD " + full, flush=True)
    print(json.dumps(compact_record(out)), flush=True)


def init_dist(args, dev, world, rank, backend):
    import torch.distributed as dist
    # the GPU boxes export NCCL_DEBUG=VERSION and RCCL prints to STDOUT (its banner would follow the JSON line, once
    # per rank; WARN is noisier still): no RCCL logging unless MM_NCCL_DEBUG asks for it — the version is reported
    # in the line itself
    os.environ.pop("NCCL_DEBUG", None)
    if os.environ.get("MM_NCCL_DEBUG"):
        os.environ["NCCL_DEBUG"] = os.environ["MM_NCCL_DEBUG"]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(free_port()))
    kw = {"device_id": dev} if dev.type == "cuda" else {}
    dist.init_process_group(backend, rank=rank, world_size=world, **kw)


def nccl_version(backend):
    import torch
    if backend != "nccl":
        return None
    try:
        return ".".join(str(x) for x in torch.cuda.nccl.version())
    except Exception:
        return "unknown"


def sharded_dot_topk(args, dev, world, rank, backend):
    """BASELINE.json configs[4] as the 8-GPU job runs it: the collection row-sharded over the ranks (sharding.shard_range),
    every rank searches ITS shard for all queries (mm_dot_topk_fwd), two RCCL all-gathers of the [nq, 1000] (score, id) lists and
    the native merge (retrieval.FlatIPIndexer.search_device = faiss_indices.py:62-66 `co.shard` + :29-36).  With one rank and
    --force-dist the collectives and the merge still run (rehearsal on a single-GPU box)."""
    import torch
    import torch.distributed as dist
    from matchmaker_amd.retrieval import FlatIPIndexer
    from matchmaker_amd.sharding import shard_range
    init_dist(args, dev, world, rank, backend)
    Ed, nq, k = 768, 6980, 1000
    lo, hi = shard_range(args.dot_passages, max(world, 8) if world == 1 else world, rank)     # one rank alone: an eighth
    n_local = hi - lo
    g = torch.Generator(device=dev).manual_seed(5005 + rank)
    c = torch.empty((n_local, Ed), dtype=torch.float16, device=dev)
    for s0 in range(0, n_local, 1 << 18):
        n = min(1 << 18, n_local - s0)
        c[s0:s0 + n] = torch.randn(n, Ed, generator=g, device=dev).half()
    gq = torch.Generator(device=dev).manual_seed(5005)                # the same queries on every rank
    q = torch.randn(nq, Ed, generator=gq, device=dev).half()
    ix = FlatIPIndexer({"token_dim": Ed, "token_dtype": "float16"}, device=dev, merge_single_rank=True)
    ix.index_resident(torch.arange(lo, hi, device=dev), c)
    s, ids = ix.search_device(q, k)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    steps = max(2, min(args.steps, 5))
    t0 = time.perf_counter()
    for _ in range(steps):
        s, ids = ix.search_device(q, k)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t = (time.perf_counter() - t0) / steps
    tt = torch.tensor([t], dtype=torch.float64, device=dev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    t = float(tt.item())
    # every rank ends with the same merged lists; the local shard's own top-1 must appear in them with its global id
    from matchmaker_amd import ops
    ls, li = ops.dot_topk(q[:64], c, 1)
    ok = bool((ids[:64] == (li[:, :1] + lo)).any(dim=1).logical_or(s[:64, -1] > ls[:, 0]).all()) and \
        bool((s[:, :-1] >= s[:, 1:]).all())
    n_tot = torch.tensor([n_local], dtype=torch.int64, device=dev)
    dist.all_reduce(n_tot)
    if rank == 0:
        flop = 2.0 * nq * float(n_tot.item()) * Ed
        print(json.dumps({"only": "dot_topk", "sharded": True, "result": {
            "workload": f"configs[4]: {int(n_tot.item())} passages x dim {Ed} fp16 row-sharded over {world} rank(s) "
                        f"({n_local} on rank 0), {nq} queries, exact top-{k}; FlatIPIndexer.search_device = local mm_dot_topk_fwd + "
                        f"2 all-gathers of [nq, {k}] (score, id) + mm_topk_merge",
            "world_size": world, "backend": backend + (" (RCCL)" if backend == "nccl" else ""), "version": nccl_version(backend),
            "ms": 1e3 * t, "queries_per_s": nq / t, "flop": flop,
            "roofline": {"bound": "mfma", "achieved": flop / t / 1e12 / world, "peak": MFMA_PEAK_16BIT / 1e12,
                         "unit": "TFLOP/s per GPU", "frac": flop / t / MFMA_PEAK_16BIT / world},
            "merged_lists_sorted_and_contain_the_local_top1": ok}}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------- main
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--queries", type=int, default=256,
                    help="queries per GPU per step (x1000 candidates; 256 -> 11.8 GB of bf16 token embeddings resident)")
    ap.add_argument("--lengths", default="full", choices=["full", "msmarco"])
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline: HBM calibration, oracle self-check, CPU baseline and the "
                         "extra legs (without it a run only sets up, warms up, times the K steps and prints the result line)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the scores of the last timed step as DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline legs")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the drop-in-layout / TK / TKL / dot-top-k legs "
                                                             "(N = 1 only)")
    ap.add_argument("--backend", default=None, choices=["nccl", "gloo"])
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise the process group and run the per-step all-gather even with one rank (exercises the "
                         "RCCL path on a single-GPU box)")
    ap.add_argument("--only", default=None,
                    choices=["headline", "dropin_forward", "published_checkpoint", "all_pairs", "tk", "tkl", "dot_topk",
                             "maxsim_fp32", "eval_batch", "train_step", "ragged_aggregate", "variants"],
                    help="run ONE leg and print it alone (the command that is put under rocprofv3 --kernel-trace)")
    ap.add_argument("--lean", action="store_true",
                    help="with --only: the leg's main measurement alone (no sub-legs, no child processes): what gets profiled")
    ap.add_argument("--one-device", action="store_true",
                    help="every rank uses device 0 (RCCL test of the N > 1 path on a single-GPU box; RCCL may refuse it)")
    ap.add_argument("--config4", action="store_true",
                    help="BASELINE.json configs[3]: 6,980 queries x 1000 candidates split over 8 ranks with sharding.shard_range "
                         "(873 / 872 queries per rank), scored + gathered by the PADDED all-gather of sharding.all_gather_scores, "
                         "final stable sort timed separately.  Default when --gpus 8; with fewer ranks every rank still holds an "
                         "eighth of the 6,980 (the total shrinks: weak scaling)")
    ap.add_argument("--total-queries", type=int, default=6980, help="--config4: queries of the whole 8-rank job (tests shrink it)")
    ap.add_argument("--dot-passages", type=int, default=8841823, help="--only dot_topk with a process group: passages of the WHOLE "
                                                                       "collection (each rank indexes its shard_range slice)")
    ap.add_argument("--dry", action="store_true",
                    help="launch + collective plumbing only (fabricated scores, value = null); for GPU-less machines")
    args = ap.parse_args()

    global LEAN
    LEAN = bool(args.lean)
    if args.only == "headline":
        args.no_extras = True
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but the torch.distributed environment has WORLD_SIZE={world}")
    if args.device == "cpu" and not args.dry:
        raise SystemExit("--device cpu is only valid with --dry: there is no CPU scoring path")
    backend = args.backend or ("gloo" if args.device == "cpu" else "nccl")
    if args.device == "cuda":
        assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback exists)"
        dev = torch.device("cuda", 0 if args.one_device else local_rank)
        torch.cuda.set_device(dev)
    else:
        dev = torch.device("cpu")
    if args.only == "dot_topk" and (world > 1 or args.force_dist):
        sharded_dot_topk(args, dev, world, rank, backend)
        return
    if args.only and args.only != "headline":
        assert world == 1 and dev.type == "cuda", "--only legs are single-GPU measurements"
        from matchmaker_amd import _lib
        _lib.lib()
        cpu_b = 0.0 if args.no_cpu_baseline else 3.0
        legs = dict(LEGS)
        if args.only == "dropin_forward":
            from matchmaker_amd import synth
            q, d, q_len, d_len = synth.colbert_batch(args.queries, CANDS, Q, D, E, torch.bfloat16, dev, seed=4004, lengths=args.lengths)
            res = extra_dropin_forward(q, d, q_len, d_len, max(5, args.steps // 2))
        else:
            res = legs[args.only](3 if args.only == "dot_topk" else max(args.steps // 2, 5), cpu_b)
        print(json.dumps({"only": args.only, "result": res}), flush=True)
        return
    use_dist = world > 1 or args.force_dist
    if use_dist:
        init_dist(args, dev, world, rank, backend)
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)

    # configs[3] (6,980 queries over 8 ranks) is what an 8-GPU launch runs unless --queries says otherwise
    config4 = (args.config4 or (world == 8 and "--queries" not in sys.argv)) and not args.dry
    nq = args.queries if not args.dry else min(args.queries, 2)
    n_total_q = None
    if config4:
        from matchmaker_amd.sharding import shard_range
        lo, hi = shard_range(args.total_queries, 8, rank % 8)
        nq = hi - lo
        n_total_q = sum(shard_range(args.total_queries, 8, r)[1] - shard_range(args.total_queries, 8, r)[0] for r in range(world))
    B = nq * CANDS
    if args.dry:
        score_shard = lambda: torch.arange(B, dtype=torch.float32, device=dev) + rank * B     # rank-tagged, checkable
    else:
        from matchmaker_amd import ops, synth, _lib
        _lib.lib()   # fail loudly here if the HIP library is missing
        q, d, q_len, d_len = synth.colbert_batch(nq, CANDS, Q, D, E, torch.bfloat16, dev, seed=4004 + rank,
                                                 lengths=args.lengths)
        score_shard = lambda: ops.maxsim(q, d, q_len, d_len, pairs_per_query=CANDS)
    gathered = torch.empty(world * B, dtype=torch.float32, device=dev) if use_dist and not config4 else None
    if config4:
        from matchmaker_amd.sharding import all_gather_scores, rank_candidates

    def merge(s):
        """the ranking merge: RCCL over xGMI.  config 4: unequal shards (873 / 872 queries) -> the padded all-gather of
        sharding.all_gather_scores, [n_total, 1000] on every rank; otherwise equal shards, one raw all_gather_into_tensor"""
        if config4:
            return all_gather_scores(s.view(nq, CANDS), n_total_q, force=use_dist)
        if use_dist:
            dist.all_gather_into_tensor(gathered, s)
        return gathered

    def step():
        s = score_shard()
        if use_dist or config4:
            merge(s)
        return s

    # --full: the box's own stream rate over the SAME document tensor is measured first (N = 1): the calibration legs keep the
    # device at its working clocks, then exactly W warm-up steps and the K timed steps follow — no further untimed steps
    # (rounds 3-5 ran ~40 ms of priming launches between warm-up and timing).
    cal = None
    if args.full and world == 1 and dev.type == "cuda" and not args.dry:
        try:
            cal = extra_hbm_calibration(d, 10, None)
        except Exception as e:
            cal = {"error": repr(e)}
    for _ in range(args.warmup):
        step()

    def barrier():
        sync()
        if use_dist:
            dist.barrier()
            sync()

    # kernel-only timing with HIP events on the launch stream (roofline numerator)
    use_ev = dev.type == "cuda"
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)] if use_ev else []
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        if use_ev:
            ev[i][0].record()
        s = score_shard()
        if use_ev:
            ev[i][1].record()
        if use_dist or config4:
            all_scores = merge(s)
    barrier()
    t = time.perf_counter() - t0
    kern_ms = sum(a.elapsed_time(b) for a, b in ev) / len(ev) if use_ev else None

    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step: this rank's scores [nq * 1000] and, with a process
        # group, the gathered scores of all ranks (float32; the inputs are seeded, so two builds can be compared 1:1)
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "scores.npy"), s.float().cpu().numpy())
        if use_dist or config4:
            np.save(os.path.join(args.dump_outputs, "gathered_scores.npy"), all_scores.float().cpu().numpy())

    gather_matches = None
    sort_info = None
    if config4 and args.full:
        # this rank's rows of the gathered matrix must BE its local scores; the final ranking (core_metrics.py:502-511:
        # stable descending sort per query) is timed on its own, and a sampled query's ranking must equal the ranking of
        # its local scores alone (what a single rank would have produced)
        row0 = sum(shard_range(args.total_queries, 8, r)[1] - shard_range(args.total_queries, 8, r)[0] for r in range(rank))
        gather_matches = bool(torch.equal(all_scores[row0:row0 + nq].reshape(-1), s))
        sort_ms = gpu_time_ms(lambda: rank_candidates(all_scores), 3, warm_ms=10.0, timed_ms=10.0)
        order = rank_candidates(all_scores)
        qs = nq // 2
        same = bool(torch.equal(order[row0 + qs], rank_candidates(s.view(nq, CANDS)[qs:qs + 1])[0]))
        sort_info = {"ms": sort_ms, "rows": int(all_scores.shape[0]), "what": "torch.sort(stable, descending) of the gathered "
                     "[n_total, 1000] scores, outside the timed steps", "ranking_equals_single_rank": same}
    elif use_dist and not args.dry and args.full:      # the gathered tensor's slice of this rank must BE its local scores
        gather_matches = bool(torch.equal(gathered[rank * B:(rank + 1) * B], s))
    tt = torch.tensor([t], dtype=torch.float64, device=dev)
    if use_dist:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    t = float(tt.item())
    gather_ok = None
    if use_dist and args.dry:
        want = torch.arange(world * B, dtype=torch.float32, device=dev)
        gather_ok = bool(torch.equal(gathered, want))

    if rank == 0:
        total_pairs = (n_total_q * CANDS if config4 else world * B) * args.steps
        coll = None
        if use_dist:
            coll = {"backend": backend + (" (RCCL)" if backend == "nccl" else ""), "version": nccl_version(backend), "world_size": world,
                    "op": ("sharding.all_gather_scores: shards padded to ceil(n_total / world) rows, ONE all_gather_into_tensor, rows "
                           "re-assembled; once per step, inside the timed region" if config4 else
                           "all_gather_into_tensor of fp32 scores, once per step, inside the timed region"),
                    "bytes_per_rank": 4 * B, "bytes_total": 4 * (n_total_q * CANDS if config4 else B * world),
                    "gathered_slice_equals_local_scores": gather_matches,
                    "devices": "all ranks on device 0 (--one-device)" if args.one_device else "one device per rank"}
            if sort_info:
                coll["final_sort"] = sort_info
        out = {
            "metric": "query-doc pairs scored/sec (ColBERT MaxSim, Q32/D180/dim128)",
            "value": None if args.dry else total_pairs / t, "unit": "pairs/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * t / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "world_size": world, "collective": coll,
            "config": {"workload": (f"BASELINE.json configs[3]: ColBERT MaxSim, {args.total_queries}-query batch x 1000 candidates "
                                    f"sharded over 8 ranks ({n_total_q} queries on the {world} rank(s) of this job, {nq} on rank 0), "
                                    f"dim=128, Q=32/D=180, bf16, RCCL score all-gather; doc lengths = {args.lengths}" if config4 else
                                    f"BASELINE.json configs[1]: ColBERT MaxSim re-rank, dim=128, Q=32/D=180, "
                                    f"1000 candidates/query, bf16; {nq} queries x 1000 candidates resident per GPU "
                                    f"per step; doc lengths = {args.lengths}"),
                       "queries_per_gpu": nq, "cands_per_query": CANDS, "Q": Q, "D": D, "E": E,
                       "parallelism": f"query-sharded x{world}" + (f", {backend} all-gather of scores" if world > 1 else "")},
        }
        if args.dry:
            out["dry"] = True
            out["note"] = "launch/collective plumbing check only: scores fabricated, nothing measured"
            out["all_gather_verified"] = gather_ok
        else:
            # --full: the timed scores themselves, checked in-process against the oracle on one sampled query (checker only)
            if args.full:
                try:
                    import numpy as np
                    from oracle import np_oracle as O
                    from matchmaker_amd import synth as _synth
                    qi = nq // 2
                    got = s[qi * CANDS:(qi + 1) * CANDS].float().cpu().numpy()
                    ref = O.maxsim_paired(np.repeat(q[qi:qi + 1].float().cpu().numpy(), CANDS, axis=0),
                                          d[qi * CANDS:(qi + 1) * CANDS].float().cpu().numpy(),
                                          _synth.len_to_mask(q_len[qi:qi + 1].cpu(), Q).numpy().repeat(CANDS, axis=0),
                                          _synth.len_to_mask(d_len[qi * CANDS:(qi + 1) * CANDS].cpu(), D).numpy())
                    err = float(np.abs(got - ref).max())
                    out["self_check"] = {"query": qi, "pairs": CANDS, "max_abs_err_vs_oracle": err, "tolerance": 1e-2,
                                         "ok": bool(err <= 1e-2),
                                         "same_order_as_oracle": bool((np.argsort(-got, kind="stable") == np.argsort(-ref, kind="stable")).mean() > 0.99)}
                    if err > 1e-2:
                        out["value"] = None      # a fast kernel whose results differ from the reference's is not a measurement
                except Exception as e:
                    out["self_check"] = {"error": repr(e)}
            ab = algorithmic_bytes(nq, CANDS)
            achieved = ab / (kern_ms * 1e-3) / 1e9
            flop = 2.0 * B * Q * D * E
            out["roofline"] = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                               "kernel": "maxsim_stream_kernel", "kernel_ms": kern_ms, "algorithmic_bytes": ab,
                               "mfma_util": {"flop_per_launch": flop, "tflops": flop / (kern_ms * 1e-3) / 1e12,
                                             "frac_of_dense_bf16_peak": flop / (kern_ms * 1e-3) / MFMA_PEAK_16BIT,
                                             "peak_tflops": MFMA_PEAK_16BIT / 1e12}}
            tr = profile_summary("*maxsim*pmc*.json", "maxsim_stream_kernel", "_hbm_traffic_bytes_per_dispatch")
            if tr is not None and tr[2].get("queries") == nq and tr[2].get("cands") == CANDS and tr[2].get("lengths") == args.lengths:
                out["roofline"]["traffic"] = tr[0]
                out["roofline"]["traffic_source"] = f"profiles/{tr[1]} (rocprofv3 PMC passes of this workload)"
            busy = profile_summary("*maxsim*pmc*.json", "maxsim_stream_kernel", "_mfma_busy_frac")
            if busy is not None:
                out["roofline"]["mfma_util"]["pmc_busy_frac"] = busy[0]
                out["roofline"]["mfma_util"]["pmc_source"] = f"profiles/{busy[1]} (SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8 XCDs), tools/summarize_rocprof.py)"
            out["timing"] = (("(N = 1: the hbm_calibration legs over the same tensor first,) " if args.full else "") +
                             "exactly W warm-up steps, then the K timed steps between barrier + synchronize pairs, nothing in "
                             "between; kernel_ms = mean HIP-event time of the K scoring launches")
            if world == 1 and args.full:      # CPU leg and extras are N = 1 figures; ranks > 0 would idle through them
                if cal is not None and "error" not in cal:   # what this box's memory system gives the same access pattern, same process
                    cal["headline_kernel_GBps"] = achieved
                    cal["headline_over_read_stream"] = achieved / cal["lds_dma_read_stream_nt"]["GBps"]
                    out["roofline"]["frac_of_calibrated"] = cal["headline_over_read_stream"]
                    out["roofline"]["calibrated_stream_GBps"] = cal["lds_dma_read_stream_nt"]["GBps"]
                out.setdefault("extra", {})["hbm_calibration"] = cal
                wall = {"process_start_to_headline_done": round(time.time() - T_PROCESS, 1)}   # host seconds per part of the default run
                if not args.no_cpu_baseline:
                    nsamp = min(nq, 24)
                    t_leg = time.time()
                    out["cpu_baseline"] = cpu_baseline(q[:nsamp].cpu(), d[:nsamp * CANDS].cpu(), q_len[:nsamp].cpu(),
                                                       d_len[:nsamp * CANDS].cpu(), CANDS)
                    wall["cpu_baseline"] = round(time.time() - t_leg, 1)
                if not args.no_extras:
                    extra = out.setdefault("extra", {})
                    cpu_b = 0.0 if args.no_cpu_baseline else 3.0
                    t_leg = time.time()
                    try:
                        extra["sustained"] = extra_sustained(score_shard, B)
                    except Exception as e:
                        extra["sustained"] = {"error": repr(e)}
                    wall["sustained"] = round(time.time() - t_leg, 1)
                    t_leg = time.time()
                    try:
                        extra["dropin_forward"] = extra_dropin_forward(q, d, q_len, d_len, max(5, args.steps // 2))
                    except Exception as e:      # an extra must never take the headline line down with it
                        extra["dropin_forward"] = {"error": repr(e)}
                    wall["dropin_forward"] = round(time.time() - t_leg, 1)
                    del q, d
                    torch.cuda.empty_cache()
                    for name, fn in LEGS:      # host seconds per leg (what the default run's few minutes are spent on)
                        t_leg = time.time()
                        try:
                            extra[name] = fn(3 if name == "dot_topk" else 10, cpu_b)
                        except Exception as e:
                            extra[name] = {"error": repr(e)}
                        torch.cuda.empty_cache()
                        wall[name] = round(time.time() - t_leg, 1)
                    extra["wall_s"] = wall
                    out["extra"] = extra
        emit(out)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
