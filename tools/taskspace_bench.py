"""Developer tool: time the task-space calls next to the route to J that existed before them, in one process on the same states.
    python tools/taskspace_bench.py [--reps 30] [--out FILE.json] [--model atlas20] [--batch 4096]
The mapping: a spatial entry on each foot and a linear entry on the pelvis (15 rows).  Timed:
  task_jacobian         one launch of k_task_jacobian (one pass down every entry's ancestor chain);
  old_jacobian          the route behind IKMapping.getRealVelToMappedVelJac batched by hand over B: k_kinematics_vjp on R x B worlds with unit
                        cotangents (the state repeated R times), then the permutation into [B, R, n];
  map_to_acc_fwd        one launch of k_task_accel;
  map_to_acc_fwd_bwd    the same with a scalar loss and its gradients to state and accel (k_task_accel, then k_task_accel_vjp).
HIP events around each path through the public Python layer (transposes included on both sides), 5 warm-up calls, the median and the 10th /
90th percentile of --reps; one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import nimblephysics_amd as na


def times_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default="atlas20")
    ap.add_argument("--batch", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    md = na.atlas(args.model)
    n, B = md.num_dofs, args.batch
    w = na.World(md, device=dev)
    m = na.IKMapping(w)
    m.addSpatialBodyNode("l_foot"); m.addSpatialBodyNode("r_foot"); m.addLinearBodyNode("pelvis")
    R = m.getVelDim()
    rng = np.random.default_rng(0)
    S = torch.tensor(np.concatenate([rng.uniform(-1, 1, (B, n)), rng.uniform(-2, 2, (B, n))], 1), device=dev)
    A = torch.tensor(rng.uniform(-5, 5, (B, n)), device=dev)
    last = {}

    def new_jacobian():
        last["new"] = na.task_jacobian(w, m, S)

    def old_jacobian():
        s_soa = w.to_soa(S)
        rep = s_soa.repeat(1, R)                                      # world p * B + b = (row p, world b)
        eye = torch.eye(R, dtype=torch.float64, device=dev).repeat_interleave(B, dim=1)
        gs = m._backward_soa(w, rep, None, eye)
        last["old"] = gs[n:].reshape(n, R, B).permute(2, 1, 0).contiguous()

    def acc_fwd():
        last["xdd"] = na.map_to_acc(w, m, S, A)

    def acc_fwd_bwd():
        s, a = S.clone().requires_grad_(True), A.clone().requires_grad_(True)
        na.map_to_acc(w, m, s, a).sum().backward()
        last["grads"] = (s.grad, a.grad)

    r = {"model": args.model, "B": B, "n": n, "rows": R, "reps": args.reps}
    for key, fn in (("task_jacobian", new_jacobian), ("old_jacobian", old_jacobian), ("map_to_acc_fwd", acc_fwd), ("map_to_acc_fwd_bwd", acc_fwd_bwd)):
        t = times_ms(fn, args.reps)
        r[key + "_ms"] = float(np.median(t))
        r[key + "_p10_p90_ms"] = [float(np.percentile(t, 10)), float(np.percentile(t, 90))]
    r["old_over_new_jacobian"] = r["old_jacobian_ms"] / r["task_jacobian_ms"]
    r["jacobian_agreement"] = float((last["new"] - last["old"]).abs().max())
    line = json.dumps(r)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
