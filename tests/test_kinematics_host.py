"""The PRODUCT's world-space kinematics (nimblephysics_amd/csrc/kinematics_dev.hpp: IKMapping rows and their vector-Jacobian products,
the code k_kinematics_fwd / k_kinematics_vjp run per lane) compiled for the host with g++ (tests/host_shim/kin_shim.cpp) and checked on
every joint type of the device model against
  * the CPU oracle's body world transforms plus a logMap (positions, 1e-12),
  * a numpy statement of getWorldPositionJacobian / getWorldJacobian (tests/kin_numpy.py: the VJPs to 1e-10, J v to 1e-10),
  * central differences of the oracle's forward kinematics (eps 1e-6, to 1e-6): positions by stepping q, velocities by stepping
    integrate_positions(q, +-eps v / dt) (ball and free coordinates are not velocities' integrals).
States are sampled so that every entry's rotation stays at least 0.3 rad below theta = pi: the reference's dLogMap takes a special branch
above pi - 1e-6 that the device's logMap_vjp does not restate (the branch itself is not tested)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import nimblephysics_amd as na
from kin_numpy import ROWS, logmap, mapping_rows
from nimblephysics_amd.mapping import resolve_body
from oracle import OracleWorld

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "host_shim", "kin_shim.cpp")
    out = os.path.join(HERE, "host_shim", "libkin_shim.so")
    csrc = os.path.join(ROOT, "nimblephysics_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "nimble_amd.h")] + [os.path.join(csrc, f) for f in ("kinematics_dev.hpp", "spatial_dev.hpp", "model_dev.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(HERE, "host_shim"),
                               "-I", csrc, "-I", os.path.join(ROOT, "include"), "-o", out, src])
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.shim_kin_model.argtypes = [vp]
    lib.shim_kin_model.restype = vp
    lib.shim_kin_free.argtypes = [vp]
    lib.shim_kin_run.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    lib.shim_kin_run.restype = C.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class ShimMap:
    """An IKMapping over `entries` [(kind, body index of md)] evaluated by the host build of the device code on [2n][B] states."""

    def __init__(self, lib, md, entries):
        self.lib, self.md, self.entries = lib, md, entries
        dev = md.merge_welds() if md.has_welds() else md
        self.desc, self.keep = dev.to_desc()
        self.h = lib.shim_kin_model(C.addressof(self.desc))
        res = [resolve_body(md, e) for _, e in entries]
        self.kind = np.array([k for k, _ in entries], dtype=np.int32)
        self.body = np.array([r[0] for r in res], dtype=np.int32)
        self.T = np.ascontiguousarray(np.stack([np.concatenate([r[1][:3, :3].reshape(9), r[1][:3, 3]]) for r in res]))
        self.P = sum(ROWS[k] for k, _ in entries)
        self.n = md.num_dofs

    def __del__(self):
        self.lib.shim_kin_free(self.h)

    def run(self, S, want=("pos", "vel"), gpos=None, gvel=None):
        """S [2n][B] -> dict of pos / vel [P][B], and grad_state [2n][B] when a cotangent is given"""
        B = S.shape[1]
        S = np.ascontiguousarray(S)
        pos = np.full((self.P, B), np.nan) if "pos" in want else None
        vel = np.full((self.P, B), np.nan) if "vel" in want else None
        gs = np.full((2 * self.n, B), np.nan) if (gpos is not None or gvel is not None) else None
        gpos = None if gpos is None else np.ascontiguousarray(gpos)
        gvel = None if gvel is None else np.ascontiguousarray(gvel)
        P = self.lib.shim_kin_run(self.h, len(self.entries), _p(self.kind), _p(self.body), _p(self.T), B, _p(S), _p(pos), _p(vel),
                                  _p(gpos), _p(gvel), _p(gs))
        assert P == self.P
        return {"pos": pos, "vel": vel, "grad": gs}


def _json_model(name):
    return na.ModelDescription.from_json(json.load(open(os.path.join(ROOT, "nimblephysics_amd", "data", name + ".json"))))


def _models():
    from test_gpu_random_trees import random_tree
    from test_screw_joint import screw_arm
    out = [("pendulum", na.single_pendulum()), ("cartpole", na.cartpole()), ("atlas20", na.atlas("atlas20")), ("atlas33", na.atlas("atlas33")),
           ("serial_chain_ball_joint", _json_model("serial_chain_ball_joint")), ("tree_structure_ball_joint", _json_model("tree_structure_ball_joint")),
           ("box_stack", na.box_stack()), ("compound_joints", na.load_skel(os.path.join(HERE, "golden", "compound_joints.skel"))),
           ("screw_free_root", screw_arm(0)), ("screw_root", screw_arm(1, free_root=False))]
    for seed in range(3):
        rng = np.random.default_rng(900 + seed)
        out.append((f"random_tree{seed}", random_tree(rng, 9, ["chain", "star", "random"][seed], seed != 1, welds=0.2, balls=0.4)))
    return out


MODELS = _models()


def _entries(md, limit=64):
    """every BodyNode of the model (the massless links of compound joints are not), kinds cycling"""
    real = [i for i, b in enumerate(md.bodies) if "#v" not in b.name]
    return [(k % 3, i) for k, i in enumerate(real[:limit])]


def _states(md, ow, entries, B, seed):
    """B states [2n][B]; every entry's rotation at least 0.3 rad below pi"""
    rng = np.random.default_rng(seed)
    n = md.num_dofs
    out = []
    while len(out) < B:
        q = rng.normal(0, 0.35, n)
        v = rng.normal(0, 0.8, n)
        ok = all(np.arccos(np.clip(0.5 * (np.trace(ow.body_world_transform(q, e)[:3, :3]) - 1), -1, 1)) < np.pi - 0.3 for _, e in entries)
        if ok:
            out.append(np.concatenate([q, v]))
    return np.stack(out, 1)


def _frame(ow, md, q, e):
    return ow.body_world_transform(q, e)


@pytest.mark.parametrize("name,md", MODELS, ids=[m[0] for m in MODELS])
def test_rows_and_vjps_equal_the_oracle_and_the_numpy_jacobians(shim, name, md):
    ow = OracleWorld(md)
    entries = _entries(md)
    m = ShimMap(shim, md, entries)
    n, B = md.num_dofs, 6
    S = _states(md, ow, entries, B, 11)
    rng = np.random.default_rng(5)
    gp, gv = rng.normal(size=(m.P, B)), rng.normal(size=(m.P, B))
    fwd = m.run(S)
    gpos_only = m.run(S, want=(), gpos=gp)["grad"]
    gvel_only = m.run(S, want=(), gvel=gv)["grad"]
    both = m.run(S, want=(), gpos=gp, gvel=gv)["grad"]
    for b in range(B):
        q, v = S[:n, b], S[n:, b]
        pos, Jp, Jv = mapping_rows(ow, md, q, entries)
        assert np.abs(fwd["pos"][:, b] - pos).max() <= 1e-12 * max(1.0, np.abs(pos).max()), (name, b)
        ref_v = Jv @ v
        assert np.abs(fwd["vel"][:, b] - ref_v).max() <= 1e-10 * max(1.0, np.abs(ref_v).max()), (name, b)
        rp, rv = Jp.T @ gp[:, b], Jv.T @ gv[:, b]
        assert np.abs(gpos_only[:n, b] - rp).max() <= 1e-10 * max(1.0, np.abs(rp).max()), (name, b)
        assert not gpos_only[n:, b].any() and not gvel_only[:n, b].any()
        assert np.abs(gvel_only[n:, b] - rv).max() <= 1e-10 * max(1.0, np.abs(rv).max()), (name, b)
        assert np.array_equal(both[:n, b], gpos_only[:n, b]) and np.array_equal(both[n:, b], gvel_only[n:, b])


@pytest.mark.parametrize("name,md", MODELS, ids=[m[0] for m in MODELS])
def test_jacobians_equal_central_differences_of_the_oracle(shim, name, md):
    ow = OracleWorld(md)
    entries = _entries(md, limit=12)
    m = ShimMap(shim, md, entries)
    n, P = md.num_dofs, m.P
    S = _states(md, ow, entries, 2, 23)
    eps = 1e-6

    def rows(q):
        return np.concatenate([np.concatenate([logmap(T[:3, :3]), T[:3, 3]])[{0: slice(0, 6), 1: slice(3, 6), 2: slice(0, 3)}[k]]
                               for k, T in ((k, _frame(ow, md, q, e)) for k, e in entries)])

    def world_rates(qa, qb):
        """[w; v] rows of the motion qa -> qb over 2 eps (w from the rotation between the two frames)"""
        out = []
        for k, e in entries:
            Ta, Tb = _frame(ow, md, qa, e), _frame(ow, md, qb, e)
            w = logmap(Tb[:3, :3] @ Ta[:3, :3].T) / (2 * eps)
            u = (Tb[:3, 3] - Ta[:3, 3]) / (2 * eps)
            out.append(np.concatenate([w, u])[{0: slice(0, 6), 1: slice(3, 6), 2: slice(0, 3)}[k]])
        return np.concatenate(out)

    for b in range(S.shape[1]):
        q, v = S[:n, b], S[n:, b]
        # dense Jacobians of the device code: the VJP with unit cotangents, P worlds at the same state
        rep = np.repeat(S[:, b:b + 1], P, axis=1)
        Jp = m.run(rep, want=(), gpos=np.eye(P))["grad"][:n].T
        Jv = m.run(rep, want=(), gvel=np.eye(P))["grad"][n:].T
        fd = np.stack([(rows(q + eps * np.eye(n)[j]) - rows(q - eps * np.eye(n)[j])) / (2 * eps) for j in range(n)], 1)
        assert np.abs(Jp - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max()), (name, b, np.abs(Jp - fd).max())
        dt = md.dt
        fdv = world_rates(ow.integrate_positions(q, -eps * v / dt), ow.integrate_positions(q, eps * v / dt))
        assert np.abs(Jv @ v - fdv).max() <= 1e-6 * max(1.0, np.abs(fdv).max()), (name, b)
        assert np.abs(m.run(S[:, b:b + 1], want=("vel",))["vel"][:, 0] - Jv @ v).max() <= 1e-10 * max(1.0, np.abs(fdv).max())


def test_results_do_not_depend_on_the_batch(shim):
    """One world's rows and VJP are bit for bit the same alone, at any position of a batch, for any B."""
    md = na.atlas("atlas20")
    ow = OracleWorld(md)
    entries = _entries(md)
    m = ShimMap(shim, md, entries)
    S = _states(md, ow, entries, 5, 3)
    rng = np.random.default_rng(0)
    g = rng.normal(size=(m.P, 5))
    full = m.run(S, gpos=g, gvel=g)
    for b in range(5):
        one = m.run(S[:, b:b + 1], gpos=g[:, b:b + 1], gvel=g[:, b:b + 1])
        for key in ("pos", "vel", "grad"):
            assert np.array_equal(one[key][:, 0], full[key][:, b])


def test_a_welded_hand_is_its_merged_body_and_offset(shim):
    """atlas20's hands are welded to the forearms: their entries land on the merged body with the weld's fixed frame."""
    md = na.atlas("atlas20")
    ow = OracleWorld(md)
    hands = [i for i, b in enumerate(md.bodies) if b.name in ("l_hand", "r_hand")]
    assert len(hands) == 2 and all(md.bodies[i].joint_type == "weld" for i in hands)
    entries = [(0, i) for i in hands]
    m = ShimMap(shim, md, entries)
    assert not np.allclose(m.T[0], [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    S = _states(md, ow, entries, 3, 8)
    out = m.run(S, want=("pos",))["pos"]
    for b in range(3):
        for k, i in enumerate(hands):
            T = ow.body_world_transform(S[:md.num_dofs, b], i)
            assert np.abs(out[6 * k:6 * k + 6, b] - np.concatenate([logmap(T[:3, :3]), T[:3, 3]])).max() < 1e-12
