"""Developer tool: time the joint-space dynamics entry points next to the contact-free step, in one process on the same states.
    python tools/dynamics_bench.py [--reps 30] [--out FILE.json] [--models atlas20,atlas33] [--batches 4096,32768]
Atlas-20 and Atlas-33 at B = 4096 and 32768: nbl_inverse_dynamics_forward, nbl_inverse_dynamics_backward, nbl_mass_matrix, the n x B
reverse launch of mass_matrix's backward pass, nbl_step_forward (no colliders, record kept), then nbl_forward_dynamics_forward / _backward,
nbl_inv_mass_matrix and nbl_inv_mass_apply (R = 1) with their ratios to the inverse-dynamics (RNEA) call, next to the dense route to the
same results through the public functions: torch.linalg.solve(mass_matrix, tau - coriolis_and_gravity) and torch.linalg.inv(mass_matrix)
(with forward_dynamics / inv_mass_matrix through the same public layer beside them, transposes included on both sides), then the wrench
calls with a wrench set on the two feet (E = 2) - nbl_inverse_dynamics_wrench_forward / _backward, nbl_forward_dynamics_wrench_forward /
_backward in both frames of expression and nbl_contact_inverse_dynamics - each as a ratio to its counterpart without wrenches in the same
run (the kernels of those calls are the parent commit's: adding the wrench code left their instructions as they were).  HIP events around
every call on preallocated buffers, 5 warm-up calls, the median of --reps (the new rows also carry the 10th and 90th percentile); one
JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import nimblephysics_amd as na
from nimblephysics_amd.dynamics import CID_MIN_TORQUE, CID_NEAREST, ID_NO_GRAVITY, ID_NO_VELOCITY, WRENCH_WORLD, _fd_workspace, _workspace, _wr_workspace, wrench_set


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


def median_ms(fn, reps, warmup=5):
    return float(np.median(times_ms(fn, reps, warmup)))


def spread(r, key, fn, reps):
    """median into r[key + "_ms"], [p10, p90] into r[key + "_p10_p90_ms"]"""
    t = times_ms(fn, reps)
    r[key + "_ms"] = float(np.median(t))
    r[key + "_p10_p90_ms"] = [float(np.percentile(t, 10)), float(np.percentile(t, 90))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--models", default="atlas20,atlas33")
    ap.add_argument("--batches", default="4096,32768")     # (one model and one batch with few --reps: what a rocprofv3 --kernel-trace --stats run wants)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rows = []
    for variant in args.models.split(","):
        md = na.atlas(variant)
        n = md.num_dofs
        for B in (int(x) for x in args.batches.split(",")):
            w = na.World(md, device=dev)
            L, h = w._L, w._h
            rng = np.random.default_rng(0)
            s = torch.tensor(np.concatenate([rng.normal(0, 0.5, (n, B)), rng.normal(0, 1.0, (n, B))]), device=dev)
            a = torch.tensor(rng.normal(0, 2.0, (n, B)), device=dev)
            g = torch.tensor(rng.normal(0, 1.0, (n, B)), device=dev)
            tau, gs, ga = torch.empty_like(a), torch.empty_like(s), torch.empty_like(a)
            M = torch.empty((n * n, B), dtype=torch.float64, device=dev)
            ws = _workspace(w, n * B)
            st = w._stream()
            r = {"model": variant, "n": n, "B": B, "reps": args.reps}
            r["inverse_dynamics_forward_ms"] = median_ms(lambda: L.nbl_inverse_dynamics_forward(h, B, p(s), p(a), 0, p(tau), p(ws), ws.numel(), st), args.reps)
            r["inverse_dynamics_backward_ms"] = median_ms(lambda: L.nbl_inverse_dynamics_backward(h, B, p(s), p(a), 0, p(g), p(gs), p(ga), 0, p(ws), ws.numel(), st), args.reps)
            r["mass_matrix_ms"] = median_ms(lambda: L.nbl_mass_matrix(h, B, p(s), p(M), p(ws), ws.numel(), st), args.reps)
            rep, eye, gt = s.repeat(1, n), torch.eye(n, dtype=torch.float64, device=dev).repeat_interleave(B, dim=1), torch.randn((n, n * B), dtype=torch.float64, device=dev)
            gbig = torch.empty((2 * n, n * B), dtype=torch.float64, device=dev)
            r["mass_matrix_backward_launch_ms"] = median_ms(lambda: L.nbl_inverse_dynamics_backward(h, n * B, p(rep), p(eye), ID_NO_VELOCITY | ID_NO_GRAVITY, p(gt), p(gbig), None, 0, p(ws), ws.numel(), st), args.reps)
            del rep, eye, gt, gbig
            u = torch.zeros((w.k, B), dtype=torch.float64, device=dev)
            nxt, saved = torch.empty_like(s), torch.empty(w.saved_bytes(B), dtype=torch.uint8, device=dev)
            status = torch.empty(B, dtype=torch.int32, device=dev)
            r["step_forward_ms"] = median_ms(lambda: w.step_into(s, u, nxt, saved, status), args.reps)
            r["id_forward_over_step"] = r["inverse_dynamics_forward_ms"] / r["step_forward_ms"]
            # forward dynamics and M^-1 (articulated-body recursion), as ratios to the RNEA call at the same B
            acc, gt1, lam = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
            Mi = M                                                  # (same size; M is not needed any more)
            fws = _fd_workspace(w, B)
            spread(r, "forward_dynamics_forward", lambda: L.nbl_forward_dynamics_forward(h, B, p(s), p(a), 0, p(acc), p(fws), fws.numel(), st), args.reps)
            spread(r, "forward_dynamics_backward", lambda: L.nbl_forward_dynamics_backward(h, B, p(s), p(a), 0, p(g), p(gs), p(gt1), 0, p(fws), fws.numel(), st), args.reps)
            spread(r, "inv_mass_matrix", lambda: L.nbl_inv_mass_matrix(h, B, p(s), p(Mi), p(fws), fws.numel(), st), args.reps)
            spread(r, "inv_mass_apply_r1", lambda: L.nbl_inv_mass_apply(h, B, 1, p(s), p(g), p(lam), p(fws), fws.numel(), st), args.reps)
            for k in ("forward_dynamics_forward", "forward_dynamics_backward", "inv_mass_matrix", "inv_mass_apply_r1"):
                r[k + "_over_rnea"] = r[k + "_ms"] / r["inverse_dynamics_forward_ms"]
            # what the same results cost through the dense route of the public functions, and the tree route through the same layer
            sb, tb = s.t().contiguous(), a.t().contiguous()
            spread(r, "dense_solve_route", lambda: torch.linalg.solve(na.mass_matrix(w, sb), (tb - na.coriolis_and_gravity(w, sb)).unsqueeze(-1)), args.reps)
            spread(r, "public_forward_dynamics", lambda: na.forward_dynamics(w, sb, tb), args.reps)
            spread(r, "dense_inv_route", lambda: torch.linalg.inv(na.mass_matrix(w, sb)), args.reps)
            spread(r, "public_inv_mass_matrix", lambda: na.inv_mass_matrix(w, sb), args.reps)
            r["dense_solve_over_forward_dynamics"] = r["dense_solve_route_ms"] / r["public_forward_dynamics_ms"]
            r["dense_inv_over_inv_mass_matrix"] = r["dense_inv_route_ms"] / r["public_inv_mass_matrix_ms"]
            # wrenches on the two feet (E = 2), as ratios to the calls without wrenches above
            feet = wrench_set(w, ["l_foot", "r_foot"])
            km = feet._device_map(w)
            Wr = torch.tensor(rng.normal(0, 3.0, (12, B)), device=dev)
            gW, Wout = torch.empty_like(Wr), torch.empty_like(Wr)
            wws = _wr_workspace(w, km, B)
            for tag, fl in (("local", 0), ("world", WRENCH_WORLD)):
                spread(r, f"id_wrench_forward_{tag}", lambda: L.nbl_inverse_dynamics_wrench_forward(h, km, B, p(s), p(a), p(Wr), fl, p(tau), p(wws), wws.numel(), st), args.reps)
                spread(r, f"id_wrench_backward_{tag}", lambda: L.nbl_inverse_dynamics_wrench_backward(h, km, B, p(s), p(a), p(Wr), fl, p(g), p(gs), p(ga), p(gW), 0, p(wws), wws.numel(), st), args.reps)
                spread(r, f"fd_wrench_forward_{tag}", lambda: L.nbl_forward_dynamics_wrench_forward(h, km, B, p(s), p(a), p(Wr), fl, p(acc), p(wws), wws.numel(), st), args.reps)
                spread(r, f"fd_wrench_backward_{tag}", lambda: L.nbl_forward_dynamics_wrench_backward(h, km, B, p(s), p(a), p(Wr), fl, p(g), p(gs), p(gt1), p(gW), 0, p(wws), wws.numel(), st), args.reps)
                for k, base in (("id_wrench_forward", "inverse_dynamics_forward"), ("id_wrench_backward", "inverse_dynamics_backward"),
                                ("fd_wrench_forward", "forward_dynamics_forward"), ("fd_wrench_backward", "forward_dynamics_backward")):
                    r[f"{k}_{tag}_over_plain"] = r[f"{k}_{tag}_ms"] / r[base + "_ms"]
            spread(r, "contact_inverse_dynamics_nearest", lambda: L.nbl_contact_inverse_dynamics(h, km, B, p(s), p(a), p(Wr), CID_NEAREST, 0, p(Wout), p(tau), p(wws), wws.numel(), st), args.reps)
            spread(r, "contact_inverse_dynamics_min_torque", lambda: L.nbl_contact_inverse_dynamics(h, km, B, p(s), p(a), None, CID_MIN_TORQUE, 0, p(Wout), p(tau), p(wws), wws.numel(), st), args.reps)
            for k in ("contact_inverse_dynamics_nearest", "contact_inverse_dynamics_min_torque"):
                r[k + "_over_rnea"] = r[k + "_ms"] / r["inverse_dynamics_forward_ms"]
            print(json.dumps(r), flush=True)
            rows.append(r)
            del w, ws, fws, wws, feet
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
