"""Developer tool: solves per second of the batched inverse kinematics (nbl_ik_solve) next to the host build of the same header.
    python tools/ik_bench.py [--reps 10] [--out FILE.json] [--batches 4096,32768] [--threads 16]
Atlas-20 with four spatial entries (pelvis, both feet, the left hand), IKMapping::setPositions' configuration (from zero, 500 steps),
targets = the rows of random configurations inside the limits.  Device: HIP events around every call on preallocated buffers, 3 warm-up
calls, the median of --reps.  Host: csrc/ik_dev.hpp compiled with g++ -O2 (tests/host_shim/ik_shim.cpp), the same problems shared by
--threads threads, the median wall time of 3 runs; minimum and maximum are reported next to each median.  The host figure is the SAME
header in the device's [slot][B] layout (a world's slots lie B doubles apart), built without -march=native: a like-for-like yardstick
for the kernel, not a tuned CPU solver.  One JSON line per batch; the number to read is `device_over_host`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import nimblephysics_amd as na


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="4096,32768")
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import ik_cases as ic
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    md, entries = ic.cases()["atlas20"]
    n = md.num_dofs
    host = ic.HostIK(ic.load_ik_shim(), md, entries)
    w = na.World(md, device=dev)
    m = na.IKMapping(w)
    for _, body in entries:
        m.addSpatialBodyNode(body)
    L, h, km = w._L, w._h, m._device_map(w)
    flat = md.flat()
    lo, hi = flat["pos_lo"], flat["pos_hi"]
    fin = np.isfinite(lo) & np.isfinite(hi)
    rows = []
    for B in (int(x) for x in args.batches.split(",")):
        rng = np.random.default_rng(0)
        q = rng.normal(0, 0.35, (B, n))
        q[:, fin] = (0.5 * (lo + hi) + 0.5 * (hi - lo) * rng.uniform(-0.9, 0.9, (B, n)))[:, fin]
        state = torch.tensor(np.concatenate([q, np.zeros_like(q)], 1), device=dev)
        targets = na.map_to_pos(w, m, state)                       # [B, P]
        t_soa = w.to_soa(targets)
        q_out = torch.empty((n, B), dtype=torch.float64, device=dev)
        loss = torch.empty(B, dtype=torch.float64, device=dev)
        steps = torch.empty(B, dtype=torch.int32, device=dev)
        need = L.nbl_ik_workspace_bytes(h, km, B)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        st = w._stream()
        run = lambda: L.nbl_ik_solve(h, km, B, p(t_soa), None, None, p(q_out), p(loss), p(steps), p(ws), need, st)
        for _ in range(3):
            assert run() == 0
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        dev_ms = float(np.median(ms))
        tn = targets.cpu().numpy()
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            hq, hl, hst = host.solve(tn, threads=args.threads, max_step_count=500)
            hs.append((time.perf_counter() - t0) * 1e3)
        host_ms = float(np.median(hs))
        dsteps = steps.cpu().numpy()
        r = {"model": "atlas20", "entries": "pelvis, l_foot, r_foot, l_hand (spatial)", "n": n, "P": m.getPosDim(), "B": B, "reps": args.reps,
             "device_ms": dev_ms, "device_ms_min": float(np.min(ms)), "device_ms_max": float(np.max(ms)), "host_ms_min": float(np.min(hs)),
             "host_ms_max": float(np.max(hs)), "device_solves_per_s": B / dev_ms * 1e3, "host_threads": args.threads, "host_ms": host_ms,
             "host_solves_per_s": B / host_ms * 1e3, "device_over_host": host_ms / dev_ms,
             "evaluations_mean": float(dsteps.mean()), "evaluations_max": int(dsteps.max()),
             "worlds_with_the_host_builds_evaluations": float((dsteps == hst).mean()), "workspace_MB": need / 2 ** 20}
        print(json.dumps(r), flush=True)
        rows.append(r)
        del ws
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
