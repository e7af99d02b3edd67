"""Times nbl_contact_readout and nbl_contact_body_wrenches (csrc/contact_readout.hip) with HIP events on the launch stream, next to ONE
forward step of the same handle for scale.  The metric worlds: Atlas-20 standing on the ground box, 8 contacts, B = 4096; the wrenches
are read for the two feet.  Prints one JSON line (and writes it to --out when given).

    python tools/contact_readout_bench.py [--reps 50] [--out profiles/contact_readout_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, reps, warmup=5):
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import nimblephysics_amd as na
    from nimblephysics_amd import _abi
    from nimblephysics_amd._lib import check
    from nimblephysics_amd.mapping import _ptr, resolve_body
    dev = torch.device("cuda:0")
    md = na.atlas("atlas20", ground=True)
    w = na.World(md, device=dev)
    B, n, k, slots = args.B, w.n, w.k, md.max_contacts
    rng = np.random.default_rng(0)
    q = np.zeros((B, n)); q[:, 0] = -np.pi / 2; q[:, 4] = -0.01
    q[:, 6:] = rng.normal(0, 0.02, (B, n - 6))
    st = w.to_soa(torch.tensor(np.concatenate([q, rng.normal(0, 0.01, (B, n))], 1), device=dev))
    at = w.to_soa(torch.zeros((B, k), dtype=torch.float64, device=dev))
    _, saved, _ = w.step_soa(st, at, want_saved=True)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    nlim, nfr = torch.empty_like(count), torch.empty_like(count)
    table = torch.empty((_abi.CO_FIELDS, slots, B), dtype=torch.float64, device=dev)
    feet = np.asarray([resolve_body(md, name)[0] for name in ("l_foot", "r_foot")], dtype=np.int32)
    wrench = torch.empty((12, B), dtype=torch.float64, device=dev)
    L, h = w._L, w._h

    def readout():
        check(L.nbl_contact_readout(h, B, _ptr(saved), _ptr(count), _ptr(nlim), _ptr(nfr), _ptr(table), w._stream()), "nbl_contact_readout")

    def wrenches():
        check(L.nbl_contact_body_wrenches(h, B, _ptr(saved), 2, feet.ctypes.data_as(C.c_void_p), _ptr(wrench), w._stream()), "nbl_contact_body_wrenches")

    def step():
        w.reset_lcp_cache()
        w.step_soa(st, at, want_saved=True)

    t_step = _time(step, max(5, args.reps // 2), warmup=3)
    t_read, t_wr = _time(readout, args.reps), _time(wrenches, args.reps)
    moved = (1 + 22 * 8 + 2 * 24) * 8 * B + table.numel() * 8 + 3 * 4 * B   # the record rows read (count, 8 contacts, x, classes) + the table and counts written
    out = {"model": "atlas20+ground", "B": B, "contacts_per_world": float(count.float().mean()), "slots": slots,
           "forward_step_ms": t_step, "contact_readout_ms": t_read, "contact_body_wrenches_ms": t_wr, "wrench_bodies": 2,
           "readout_fraction_of_forward_step": t_read / t_step, "wrenches_fraction_of_forward_step": t_wr / t_step,
           "readout_bytes_moved_upper_bound": int(moved), "readout_GBps_upper_bound": moved / (t_read * 1e-3) / 1e9}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
