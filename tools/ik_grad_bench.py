"""Developer tool: the reverse pass of the batched inverse kinematics (nbl_ik_solve_vjp) timed next to the solve it differentiates.
    python tools/ik_grad_bench.py [--reps 10] [--out profiles/ik_grad_bench.json] [--batches 4096,32768]
                                  [--resources profiles/ik_grad_kernel_resources.txt] [--resources-only]
Atlas-20 with four spatial entries (pelvis, both feet, the left hand) as tools/ik_bench.py sets it up: IKMapping::setPositions'
configuration (from zero, 500 steps), targets = the rows of random configurations inside the limits.  The VJP runs at the positions that
solve returned, with a random grad_q and grad_damping = 1e-9.  HIP events around every call on preallocated buffers, 3 warm-up calls, the
median of --reps; minimum and maximum next to it.  One JSON line per batch.  No threshold: the figures are recorded, not judged.
--resources: registers, scratch and LDS of k_ik_solve_vjp as the compiler reports them (gfx950, -Rpass-analysis=kernel-resource-usage on
the unit that holds the kernel; needs hipcc, no GPU)."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def kernel_resources(path):
    csrc = os.path.join(ROOT, "nimblephysics_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
           "-DNBL_NS=nbl_tree", "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "nimble_amd_tree.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, check=True).stderr.decode()
    keep, on = [], False
    for line in text.splitlines():
        m = re.search(r"remark: (Function Name: (\S+)|\s+.*)$", line.replace(" [-Rpass-analysis=kernel-resource-usage]", ""))
        if not m:
            continue
        if m.group(2):
            on = "k_ik_solve_vjp" in m.group(2) or re.search(r"\d+k_ik_solveE", m.group(2)) is not None
        if on:
            keep.append(m.group(1).rstrip())
    assert keep, "the compiler reported no k_ik_solve_vjp"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(keep) + "\n")
    print("\n".join(keep), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_grad_bench.json"))
    ap.add_argument("--batches", default="4096,32768")
    ap.add_argument("--resources", default=None)
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    if args.resources or args.resources_only:
        kernel_resources(args.resources or os.path.join(ROOT, "profiles", "ik_grad_kernel_resources.txt"))
    if args.resources_only:
        return
    import numpy as np
    import torch

    import ik_cases as ic
    import nimblephysics_amd as na
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    md, entries = ic.cases()["atlas20"]
    n = md.num_dofs
    w = na.World(md, device=dev)
    m = na.IKMapping(w)
    for _, body in entries:
        m.addSpatialBodyNode(body)
    L, h, km = w._L, w._h, m._device_map(w)
    P = m.getPosDim()
    flat = md.flat()
    lo, hi = flat["pos_lo"], flat["pos_hi"]
    fin = np.isfinite(lo) & np.isfinite(hi)

    def timed(run):
        for _ in range(3):
            assert run() == 0
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    rows = []
    for B in (int(x) for x in args.batches.split(",")):
        rng = np.random.default_rng(0)
        q = rng.normal(0, 0.35, (B, n))
        q[:, fin] = (0.5 * (lo + hi) + 0.5 * (hi - lo) * rng.uniform(-0.9, 0.9, (B, n)))[:, fin]
        state = torch.tensor(np.concatenate([q, np.zeros_like(q)], 1), device=dev)
        t_soa = w.to_soa(na.map_to_pos(w, m, state))
        q_out = torch.empty((n, B), dtype=torch.float64, device=dev)
        loss = torch.empty(B, dtype=torch.float64, device=dev)
        steps = torch.empty(B, dtype=torch.int32, device=dev)
        g_soa = torch.tensor(rng.normal(0, 1, (n, B)), device=dev)
        gt = torch.empty((P, B), dtype=torch.float64, device=dev)
        free = torch.empty(B, dtype=torch.int32, device=dev)
        need = max(L.nbl_ik_workspace_bytes(h, km, B), L.nbl_ik_grad_workspace_bytes(h, km, B))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        st = w._stream()
        solve = timed(lambda: L.nbl_ik_solve(h, km, B, p(t_soa), None, None, p(q_out), p(loss), p(steps), p(ws), need, st))
        vjp = timed(lambda: L.nbl_ik_solve_vjp(h, km, B, p(q_out), p(g_soa), 1e-9, p(gt), 0, p(free), p(ws), need, st))
        fc = free.cpu().numpy()
        r = {"model": "atlas20", "entries": "pelvis, l_foot, r_foot, l_hand (spatial)", "n": n, "P": P, "B": B, "reps": args.reps,
             "solve_ms": solve[0], "solve_ms_min": solve[1], "solve_ms_max": solve[2], "vjp_ms": vjp[0], "vjp_ms_min": vjp[1],
             "vjp_ms_max": vjp[2], "vjp_per_s": B / vjp[0] * 1e3, "solve_over_vjp": solve[0] / vjp[0],
             "evaluations_mean": float(steps.cpu().numpy().mean()), "free_count_mean": float(fc.mean()), "free_count_min": int(fc.min()),
             "grad_target_finite": bool(torch.isfinite(gt).all()), "workspace_MB": need / 2 ** 20}
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
