"""The PRODUCT's inertia-parameter gradient of inverse dynamics (idInertiaVjpWorld of nimblephysics_amd/csrc/dynamics_dev.hpp - the code
k_inverse_dynamics_inertia_vjp runs per lane) compiled for the host with g++ -O2 -ffp-contract=off (tests/host_shim/dynmass_shim.cpp) and
checked on every model of tests/test_dynamics_host.py (revolute, prismatic, screw, free, ball, compound chains, welds, a free joint below
the root, random trees) against exact central differences of the CPU oracle (tests/dynmass_ref.py):
    grad_params = D^T grad_tau,   D_p = [ID_o(theta + h_p e_p) - ID_o(theta - h_p e_p)] / (2 h_p),
held to max|x - ref| / max(1, |ref|) <= 1e-10 on every world and every parameter, after the reference has been held to itself (D at h
and at h / 2 agree to 1e-11 max(1, |D|)).  Per model up to three bodies - the root-most, a leaf, one in a ball or free chain - carry one
entry type each; the six types appear across the models.  B = 5; the flags 0 / NO_VELOCITY / NO_GRAVITY / JOINT_FORCES, accel = None,
accumulate on and off."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nimblephysics_amd.mass import WithRespectToMass
from dynmass_ref import ALL_TYPES, JOINT_FORCES, NO_GRAVITY, NO_VELOCITY, TOL, InertiaReference, on_the_mu_line, pick_entries, rel
from test_dynamics_host import MODELS as HOST_MODELS, ShimDynamics, _draw, _p

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B = 5


def load_shim():
    src = os.path.join(HERE, "host_shim", "dynmass_shim.cpp")
    out = os.path.join(HERE, "host_shim", "libdynmass_shim.so")
    csrc = os.path.join(ROOT, "nimblephysics_amd", "csrc")
    deps = [src, os.path.join(HERE, "host_shim", "dyn_shim.cpp"), os.path.join(ROOT, "include", "nimble_amd.h")] + \
        [os.path.join(csrc, f) for f in ("dynamics_dev.hpp", "kinematics_dev.hpp", "spatial_dev.hpp", "model_dev.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(HERE, "host_shim"),
                               "-I", csrc, "-I", os.path.join(ROOT, "include"), "-o", out, src])
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.shim_dyn_model.argtypes = [vp]
    lib.shim_dyn_model.restype = vp
    lib.shim_dyn_free.argtypes = [vp]
    lib.shim_dyn_run.argtypes = [vp, C.c_int64, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    lib.shim_dyn_run.restype = None
    lib.shim_dynmass_run.argtypes = [vp, C.c_int64, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int]
    lib.shim_dynmass_run.restype = None
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


class ShimInertia(ShimDynamics):
    """The host build on the model `md` with `entries` registered (the table WithRespectToMass.device_table() gives the device)."""

    def __init__(self, lib, md, entries):
        super().__init__(lib, md)
        w = WithRespectToMass(md)
        for b, t in entries:
            w.registerNode(b, t)
        self.bodies, self.dG = w.device_table()
        self.P = int(self.bodies.shape[0])

    def grad(self, S, A, g, flags=0, init=None):
        """grad_params [P][B]; init: accumulate onto it"""
        S = np.ascontiguousarray(S); A = None if A is None else np.ascontiguousarray(A); g = np.ascontiguousarray(g)
        out = np.full((self.P, S.shape[1]), np.nan) if init is None else init.copy()
        self.lib.shim_dynmass_run(self.h, S.shape[1], _p(S), _p(A), flags, _p(g), self.P, _p(np.ascontiguousarray(self.bodies)),
                                  _p(np.ascontiguousarray(self.dG)), _p(out), 0 if init is None else 1)
        return out


ENTRIES = [pick_entries(md, k) for k, (_, md) in enumerate(HOST_MODELS)]
# the models of tests/test_dynamics_host.py with their INERTIA_COM_MU bodies moved onto the line the entry moves them along
MU_MODELS = [(name, on_the_mu_line(md, e)) for (name, md), e in zip(HOST_MODELS, ENTRIES)]


def test_the_entries_cover_every_type_and_a_ball_or_free_chain():
    assert {t for e in ENTRIES for _, t in e} == set(ALL_TYPES)
    chain = [md.bodies[b].joint_type for (_, md), e in zip(MU_MODELS, ENTRIES) for b, _ in e if md.bodies[b].parent >= 0]
    assert "ball" in chain and "free" in chain


@pytest.mark.parametrize("k", range(len(MU_MODELS)), ids=[m[0] for m in MU_MODELS])
def test_the_inertia_gradient_equals_the_oracles_exact_differences(shim, k):
    name, md = MU_MODELS[k]
    entries = ENTRIES[k]
    ref = InertiaReference(md, entries)
    d = ShimInertia(shim, md, entries)
    n = md.num_dofs
    S, A, g = _draw(md, B, 61)
    assert d.P == ref.P > 0
    cases = [("0", 0, A), ("no velocity", NO_VELOCITY, A), ("no gravity", NO_GRAVITY, A), ("joint forces", JOINT_FORCES, A), ("accel None", 0, None)]
    got = {c: d.grad(S, a, g, fl) for c, fl, a in cases}
    init = np.random.default_rng(62).normal(size=(d.P, B))
    acc = d.grad(S, A, g, 0, init=init)
    assert np.abs(acc - (init + got["0"])).max() <= 1e-12 * max(1.0, np.abs(got["0"]).max())
    worst = {}
    for c, fl, a in cases:
        for b in range(B):
            D = ref.checked_D(S[:n, b], S[n:, b], None if a is None else a[:, b], fl)
            e = rel(got[c][:, b], D.T @ g[:, b])
            worst[c] = max(worst.get(c, 0.0), e)
            assert e <= TOL, (name, c, b, e, got[c][:, b], D.T @ g[:, b])
    print(name, [(b, t.name) for b, t in entries], worst)


def test_the_jacobian_by_unit_cotangents_is_d_and_the_euler_identity_holds(shim):
    """n worlds at one state with the cotangents e_i give D itself; with INERTIA_MASS on every body sum_p m_p D[:, p] = tau (tau is
    homogeneous of degree 1 in the masses), the product's own forward pass on the other side."""
    from nimblephysics_amd.mass import WrtMassBodyNodeEntryType as T
    name, md = next(m for m in MU_MODELS if m[0] == "free_below_root")
    entries = [(i, T.INERTIA_MASS) for i in range(len(md.bodies))]
    d = ShimInertia(shim, md, entries)
    ref = InertiaReference(md, entries)
    n = md.num_dofs
    S, A, _ = _draw(md, 1, 63)
    J = d.grad(np.repeat(S, n, 1), np.repeat(A, n, 1), np.eye(n)).T                   # [n (cotangent i), P]
    assert rel(J, ref.checked_D(S[:n, 0], S[n:, 0], A[:, 0])) <= TOL
    tau = d.tau(S, A)[:, 0]
    masses = np.array([b.mass for b in md.bodies])
    assert np.abs(J @ masses - tau).max() <= 1e-12 * max(1.0, np.abs(tau).max())


def test_results_do_not_depend_on_the_batch(shim):
    k = next(i for i, m in enumerate(MU_MODELS) if m[0] == "atlas20")
    md = MU_MODELS[k][1]
    d = ShimInertia(shim, md, ENTRIES[k])
    S, A, g = _draw(md, B, 64)
    all_ = d.grad(S, A, g)
    for b in range(B):
        assert np.array_equal(d.grad(S[:, b:b + 1], A[:, b:b + 1], g[:, b:b + 1])[:, 0], all_[:, b])
