"""Developer tool: time centroidal() next to what a user had to write before it existed, in one process on the same states.
    python tools/centroidal_bench.py [--reps 30] [--out FILE.json] [--model atlas20] [--batch 4096]
Two forward-plus-backward paths to the same four quantities (com, com_vel, ke, pe) with a scalar loss on them and the gradient to `state`:
  new         centroidal(world, state): one launch of k_centroidal, one of k_centroidal_vjp;
  workaround  one IKMapping with a linear entry at every body's local centre of mass, map_to_pos and map_to_vel (3 nb rows per world each),
              a mass-weighted reduction in torch, and mass_matrix (n^2 doubles per world) for the kinetic energy.  Its com_vel gradient to
              q is not the complete one (map_to_vel leaves d(J v)/dq out, like the reference's layer): it computes LESS.
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
from nimblephysics_amd.mapping import KIN_LINEAR


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


def com_mapping(w):
    """an IKMapping with one linear entry at the local centre of mass of every body of the World's model, and the masses"""
    m = na.IKMapping(w)
    targets, _ = w.description.weld_targets()
    masses = []
    for j, b in enumerate(w.model.bodies):
        T = np.eye(4)
        T[:3, 3] = np.asarray(b.com, dtype=np.float64)
        m._entries.append((KIN_LINEAR, targets.index(j), j, T))
        masses.append(float(b.mass))
    return m, masses


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
    rng = np.random.default_rng(0)
    S = torch.tensor(np.concatenate([rng.normal(0, 0.5, (B, n)), rng.normal(0, 1.0, (B, n))], 1), device=dev)
    mp, masses = com_mapping(w)
    nb = len(masses)
    mt = torch.tensor(masses, dtype=torch.float64, device=dev)
    Mtot = float(mt.sum())
    g = torch.tensor(np.asarray(md.gravity, dtype=np.float64), device=dev)
    last = {}

    def new():
        s = S.clone().requires_grad_(True)
        o = na.centroidal(w, s)
        (o.com.sum() + o.com_vel.sum() + o.ke.sum() + o.pe.sum()).backward()
        last["new"] = (o.com.detach(), o.com_vel.detach(), o.ke.detach(), s.grad)

    def workaround():
        s = S.clone().requires_grad_(True)
        x = na.map_to_pos(w, mp, s).reshape(B, nb, 3)
        xd = na.map_to_vel(w, mp, s).reshape(B, nb, 3)
        com = (mt[None, :, None] * x).sum(1) / Mtot
        cv = (mt[None, :, None] * xd).sum(1) / Mtot
        v = s[:, n:]
        ke = 0.5 * torch.einsum("bi,bij,bj->b", v, na.mass_matrix(w, s), v)
        pe = -Mtot * (com @ g)
        (com.sum() + cv.sum() + ke.sum() + pe.sum()).backward()
        last["old"] = (com.detach(), cv.detach(), ke.detach(), s.grad)

    r = {"model": args.model, "B": B, "n": n, "bodies": nb, "reps": args.reps}
    for key, fn in (("centroidal", new), ("workaround", workaround)):
        t = times_ms(fn, args.reps)
        r[key + "_ms"] = float(np.median(t))
        r[key + "_p10_p90_ms"] = [float(np.percentile(t, 10)), float(np.percentile(t, 90))]
    r["workaround_over_centroidal"] = r["workaround_ms"] / r["centroidal_ms"]
    # the two paths agree on what both compute (the springs of Atlas are zero; the workaround's d com_vel / dq is incomplete, so gradients are not compared)
    r["agreement"] = [float((a - b).abs().max()) for a, b in zip(last["new"][:3], last["old"][:3])]
    line = json.dumps(r)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
