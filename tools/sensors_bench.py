"""Developer tool: time imu_readings() next to the only route to a gyro reading that existed before it, in one process on the same states.
    python tools/sensors_bench.py [--reps 30] [--out FILE.json] [--model atlas20] [--batch 4096] [--sensors 8]
  imu         imu_readings(world, sensors, state, accel): gyro and accelerometer readings of --sensors IMUs from one launch of k_sensors, a
              scalar loss on both and the gradients to state and accel from one launch of k_sensors_vjp;
  gyro        gyro_readings alone, forward and backward: what the workaround computes;
  workaround  one IKMapping with a spatial entry per sensor body, map_to_pos and map_to_vel (6 rows per sensor and world each), the body
              rotation rebuilt from the log-map rows in torch (Rodrigues) and gyro = R_bs^T R^T w.  It has no accelerometer reading at all,
              and its gradient to q is not the complete one (map_to_vel leaves d(J v)/dq out): it computes LESS.
HIP events around each path through the public Python layer (transposes included on all sides), 5 warm-up calls, the median and the 10th /
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


def rodrigues(r):
    """exp of the rotation vectors r [..., 3] (torch)"""
    th = r.norm(dim=-1, keepdim=True).clamp_min(1e-12)[..., None]
    k = r / th[..., 0]
    z = torch.zeros_like(k[..., 0])
    K = torch.stack([torch.stack([z, -k[..., 2], k[..., 1]], -1), torch.stack([k[..., 2], z, -k[..., 0]], -1),
                     torch.stack([-k[..., 1], k[..., 0], z], -1)], -2)
    return torch.eye(3, dtype=r.dtype, device=r.device) + torch.sin(th) * K + (1 - torch.cos(th)) * K @ K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default="atlas20")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--sensors", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    md = na.atlas(args.model)
    n, B = md.num_dofs, args.batch
    w = na.World(md, device=dev)
    rng = np.random.default_rng(0)
    S = torch.tensor(np.concatenate([rng.normal(0, 0.5, (B, n)), rng.normal(0, 1.0, (B, n))], 1), device=dev)
    A = torch.tensor(rng.normal(0, 2.0, (B, n)), device=dev)
    movable = [i for i, b in enumerate(md.bodies) if b.joint_type != "weld"]
    bodies = [movable[(k * len(movable)) // args.sensors] for k in range(args.sensors)]
    sensors = []
    for i in bodies:                                               # a quarter turn about z and a small lever arm per IMU
        T = np.eye(4)
        T[:3, :3] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        T[:3, 3] = rng.normal(0, 0.05, 3)
        sensors.append((int(i), T))
    Rbs = torch.tensor(np.stack([T[:3, :3] for _, T in sensors]), device=dev)
    mp = na.IKMapping(w)
    for i in bodies:
        mp.addSpatialBodyNode(int(i))
    E = len(bodies)
    last = {}

    def imu():
        s, a = S.clone().requires_grad_(True), A.clone().requires_grad_(True)
        o = na.imu_readings(w, sensors, s, a)
        (o.gyro.sum() + o.acc.sum()).backward()
        last["imu"] = o.gyro.detach()

    def gyro():
        s = S.clone().requires_grad_(True)
        o = na.gyro_readings(w, sensors, s)
        o.sum().backward()
        last["gyro"] = o.detach()

    def workaround():
        s = S.clone().requires_grad_(True)
        pos = na.map_to_pos(w, mp, s).reshape(B, E, 6)
        vel = na.map_to_vel(w, mp, s).reshape(B, E, 6)
        R = rodrigues(pos[..., :3])
        o = torch.einsum("eji,bekj,bek->bei", Rbs, R, vel[..., :3]).reshape(B, 3 * E)
        o.sum().backward()
        last["old"] = o.detach()

    r = {"model": args.model, "B": B, "n": n, "sensors": E, "reps": args.reps}
    for key, fn in (("imu", imu), ("gyro", gyro), ("workaround", workaround)):
        t = times_ms(fn, args.reps)
        r[key + "_ms"] = float(np.median(t))
        r[key + "_p10_p90_ms"] = [float(np.percentile(t, 10)), float(np.percentile(t, 90))]
    r["workaround_over_gyro"] = r["workaround_ms"] / r["gyro_ms"]
    # the paths agree on the gyro readings (the workaround's gradient to q is incomplete, so gradients are not compared)
    r["agreement"] = [float((last["imu"] - last["old"]).abs().max()), float((last["gyro"] - last["old"]).abs().max())]
    line = json.dumps(r)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
