#!/usr/bin/env python
"""Benchmark of the fused MatchPyramid kernel (mm_matchpyramid_fwd) at the reference shape (Q 30, D 200, E 300, the default
pyramid of config/train/non-bert-defaults.yaml:47-49) on one GPU.  Prints ONE JSON line with the legs

  shared_64x1000       64 queries x 1000 candidates, one query row per 1000 pairs
  replicated_64x1000   the same pairs with one query copy per pair (the reference's layout)
  call_512             an eval.py-sized call: 512 pairs
  generic_64x1000      shared_64x1000 on the generic kernel (MM_MP_GENERIC=1)
  train_64             a training step (forward + backward of the WHOLE module, head included) on 64 pairs
  train_2048           the same on 2,048 pairs

the forward legs each with ms, pairs/s, the fraction of the fp32-matrix bound (27 MFLOP per pair at 157 TFLOP/s: 11 ms for 64,000 pairs) and the
ratio to the SAME module's eager torch path (MatchPyramid.torch_features) timed in the same process on the same GPU in steady
state; the eager path of the 64,000-pair legs is timed on --eager-pairs pairs and scaled per pair (its activations are 0.4 MB
per pair).  Every leg runs in its own child process under its own time limit; the first leg that fails ends the run.
A training leg times, on the same tensors in the same process, the step through the native path (native_backward = True:
mm_matchpyramid_fwd_save + mm_matchpyramid_bwd) and through the module's eager torch layers (native_backward = False), and
beside them the operators alone (the inference forward, the saving forward, the backward) and the eager forward + backward of
torch_features alone; it also reports the bytes of saved state and the largest difference between the two paths' gradients.
Timing: bench.gpu_time_ms (median of per-call HIP events in steady state)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q, D, E = 30, 200, 300
CHANNELS, KERNELS = [16] * 5, [[3, 3]] * 5
POOLS = [[36, 90], [18, 60], [9, 30], [6, 20], [3, 10]]
MFLOP_PER_PAIR = 27.0
MATRIX_TFLOPS = 157.0
LEGS = {"shared_64x1000": {}, "replicated_64x1000": {}, "call_512": {}, "generic_64x1000": {"MM_MP_GENERIC": "1"},
        "train_64": {}, "train_2048": {}}


def run_train_leg(name, a):
    import torch
    import bench
    from matchmaker_amd import ops
    from matchmaker_amd.matchpyramid import MatchPyramid
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = MatchPyramid(CHANNELS, KERNELS, POOLS).to(dev).train()
    g = torch.Generator(device=dev).manual_seed(1)
    B = int(name.split("_")[1])
    q = torch.randn(B, Q, E, generator=g, device=dev).requires_grad_(True)     # the embedding layer's outputs
    d = torch.randn(B, D, E, generator=g, device=dev).requires_grad_(True)
    convs = m._convs()
    w, b = [c.weight for c in convs], [c.bias for c in convs]

    def step(native):
        m.native_backward = native
        m.zero_grad(set_to_none=True)
        q.grad = d.grad = None
        m(q, d, None, None).sum().backward()

    def grads():
        return [q.grad.clone(), d.grad.clone()] + [p.grad.clone() for p in m.parameters()]

    step(True)
    gn = grads()
    step(False)
    ge = grads()
    diff = max(float((x - y).abs().max()) for x, y in zip(gn, ge))
    scale = max(float(y.abs().max()) for y in ge)
    steps = max(3, a.steps)
    t_native = bench.gpu_time_ms(lambda: step(True), steps)
    t_eager = bench.gpu_time_ms(lambda: step(False), steps)
    qd, dd = q.detach(), d.detach()
    with torch.no_grad():
        packed = ops.matchpyramid_pack(w, b)          # as the forward legs: the operators alone, without the packing
        feats, saved = ops.matchpyramid_features_save(qd, dd, w, b, POOLS, packed=packed)
        go = torch.randn(feats.shape, generator=g, device=dev)
        t_fwd = bench.gpu_time_ms(lambda: ops.matchpyramid_features(qd, dd, w, b, POOLS, packed=packed), steps)
        t_save = bench.gpu_time_ms(lambda: ops.matchpyramid_features_save(qd, dd, w, b, POOLS, packed=packed), steps)
        t_bwd = bench.gpu_time_ms(lambda: ops.matchpyramid_bwd(qd, dd, w, b, POOLS, saved, go, packed=packed), steps)

    def eager_features_step():
        m.zero_grad(set_to_none=True)
        q.grad = d.grad = None
        (m.torch_features(q, d) * go).sum().backward()

    t_eager_feat = bench.gpu_time_ms(eager_features_step, steps)
    return {"pairs": B, "native_step_ms": t_native, "eager_step_ms": t_eager, "step_speedup_vs_eager": t_eager / t_native,
            "forward_ms": t_fwd, "forward_save_ms": t_save, "backward_ms": t_bwd,
            "eager_features_fwd_bwd_ms": t_eager_feat, "features_fwd_bwd_speedup_vs_eager": t_eager_feat / (t_save + t_bwd),
            "saved_state_bytes": sum(t.numel() * t.element_size() for t in saved),
            "max_abs_grad_diff_vs_eager": diff, "max_abs_grad_eager": scale}


def run_leg(name, a):
    if name.startswith("train_"):
        return run_train_leg(name, a)
    import torch
    import bench
    from matchmaker_amd.matchpyramid import MatchPyramid
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = MatchPyramid(CHANNELS, KERNELS, POOLS).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(1)
    nq, cands = (1, 512) if name == "call_512" else (a.queries, a.cands)
    B = nq * cands
    q = torch.randn(nq, Q, E, generator=g, device=dev)
    d = torch.randn(B, D, E, generator=g, device=dev)
    convs = m._convs()
    w, b = [c.weight for c in convs], [c.bias for c in convs]
    from matchmaker_amd import ops
    packed = ops.matchpyramid_pack(w, b)
    shared = name != "replicated_64x1000" and name != "call_512"
    qq = q if shared else q.repeat_interleave(cands, dim=0)
    ppq = cands if shared else 1
    ne = min(B, a.eager_pairs)
    q_e = q.repeat_interleave(cands, dim=0)[:ne]
    with torch.no_grad():
        t = bench.gpu_time_ms(lambda: ops.matchpyramid_features(qq, d, w, b, POOLS, ppq, packed=packed), a.steps)
        te = bench.gpu_time_ms(lambda: m.torch_features(q_e, d[:ne]), max(2, a.steps // 3)) * B / ne
        same = float((ops.matchpyramid_features(q_e, d[:ne], w, b, POOLS, 1, packed=packed)
                      - m.torch_features(q_e, d[:ne])).abs().max())
    bound_ms = B * MFLOP_PER_PAIR / MATRIX_TFLOPS / 1e3
    return {"pairs": B, "ms": t, "pairs_per_s": B / t * 1e3, "fraction_of_fp32_matrix_bound": bound_ms / t, "eager_ms": te,
            "eager_timed_on_pairs": ne, "speedup_vs_eager": te / t, "max_abs_diff_vs_eager": same,
            "kernel": "generic (MM_MP_GENERIC=1)" if os.environ.get("MM_MP_GENERIC") == "1" else "reference-config"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--cands", type=int, default=1000)
    ap.add_argument("--eager-pairs", type=int, default=2000)
    ap.add_argument("--leg-timeout", type=int, default=150, help="seconds per leg")
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process")
    a = ap.parse_args()
    if a.leg:
        print("LEG " + json.dumps(run_leg(a.leg, a)))
        return 0
    out = {"shape": {"Q": Q, "D": D, "E": E, "channels": CHANNELS, "kernels": KERNELS, "pools": POOLS, "queries": a.queries,
                     "cands": a.cands}, "legs": {}}
    for name, env in LEGS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--steps", str(a.steps), "--queries", str(a.queries),
               "--cands", str(a.cands), "--eager-pairs", str(a.eager_pairs)]
        try:
            r = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=a.leg_timeout)
        except subprocess.TimeoutExpired:
            out["legs"][name] = {"error": f"time limit of {a.leg_timeout} s"}
            break
        lines = [x for x in r.stdout.splitlines() if x.startswith("LEG ")]
        if r.returncode != 0 or not lines:
            out["legs"][name] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-1500:]}
            break                                   # nothing more is started on the GPU after a failed leg
        out["legs"][name] = json.loads(lines[-1][4:])
    print(json.dumps(out))
    return 0 if all("error" not in v for v in out["legs"].values()) and len(out["legs"]) == len(LEGS) else 1


if __name__ == "__main__":
    sys.exit(main())
