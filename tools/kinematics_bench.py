"""Times nbl_kinematics_forward + nbl_kinematics_backward (csrc/kinematics.hip) with HIP events, next to one timestep (forward +
backward) at the same batch size for scale.  Atlas-20 standing on the ground box (the flagship model), four SPATIAL entries: the two
hands (welded to the forearms: offset entries) and the two feet.  B = 4096 (one step of a batch) and B = 65 x 4096 (the states of a T = 64
rollout mapped in one launch).  Prints one JSON line.

    python tools/kinematics_bench.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import nimblephysics_amd as na
    from nimblephysics_amd.mapping import _ptr
    dev = torch.device("cuda:0")
    md = na.atlas("atlas20", ground=True)
    w = na.World(md, device=dev)
    m = na.neural.IKMapping(w)
    for name in ("l_hand", "r_hand", "l_foot", "r_foot"):
        m.addSpatialBodyNode(name)
    P, n, k = m.getPosDim(), w.n, w.k
    out = {"model": "atlas20+ground", "entries": 4, "P": P, "results": []}
    for B in (4096, 65 * 4096):
        rng = np.random.default_rng(0)
        q = np.zeros((B, n)); q[:, 0] = -np.pi / 2; q[:, 4] = -0.01
        q[:, 6:] = rng.normal(0, 0.02, (B, n - 6))
        s = torch.tensor(np.concatenate([q, rng.normal(0, 0.01, (B, n))], 1), device=dev)
        st = w.to_soa(s)
        at = w.to_soa(torch.zeros((B, k), dtype=torch.float64, device=dev))
        pos = torch.empty((P, B), dtype=torch.float64, device=dev)
        vel = torch.empty((P, B), dtype=torch.float64, device=dev)
        g = torch.ones((P, B), dtype=torch.float64, device=dev)
        gs = torch.empty((2 * n, B), dtype=torch.float64, device=dev)
        km = m._device_map(w)
        L, h = w._L, w._h

        def fwd():
            na._lib.check(L.nbl_kinematics_forward(h, km, B, _ptr(st), _ptr(pos), _ptr(vel), w._stream()), "nbl_kinematics_forward")

        def bwd():
            na._lib.check(L.nbl_kinematics_backward(h, km, B, _ptr(st), _ptr(g), _ptr(g), _ptr(gs), 0, w._stream()), "nbl_kinematics_backward")

        t_fwd = _time(fwd, args.reps)
        t_bwd = _time(bwd, args.reps)
        _, saved, _ = w.step_soa(st, at, want_saved=True)

        def step():
            nxt, sv, _ = w.step_soa(st, at, want_saved=True)
            w.backward_soa(sv, nxt)
        t_step = _time(step, max(2, args.reps // 4), warmup=1)
        del saved
        out["results"].append({"B": B, "kin_forward_ms": t_fwd, "kin_backward_ms": t_bwd, "kin_total_ms": t_fwd + t_bwd,
                               "timestep_fwd_bwd_ms": t_step, "kin_fraction_of_timestep": (t_fwd + t_bwd) / t_step})
        w.reset_lcp_cache()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
