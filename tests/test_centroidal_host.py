"""The PRODUCT's centre-of-mass family (nimblephysics_amd/csrc/centroidal_dev.hpp: the code k_centroidal and k_centroidal_vjp run per lane)
compiled for the host with g++ -O2 -ffp-contract=off (tests/host_shim/cen_shim.cpp) and held to tests/cen_numpy.py, the numpy statement
built on OracleWorld.body_world_transform, kin_numpy.joint_screws and the description's masses, on cartpole, the ball arm, the
compound-joint fixture, Atlas-20 and Atlas-20 on the ground (default set, a `skeleton=` set, the two feet), eight worlds each, states drawn
as in test_gpu_dynamics._states.

  1  every forward output, the mass and Jcom: |x - ref| / max(1, |ref|) <= 1e-10 (the dynamics tests' TOL against the same oracle); ke against
     BOTH numpy routes (v^T M v / 2 with OracleWorld.mass_matrix where the set is the whole model, and the body sum);
  2  the linear part of the momentum against M com_vel: 1e-13;
  3  the gradients the oracle has in closed form (com -> q, com_vel -> v, com_acc -> a, pe -> q, and for the whole model ke -> q, v): 1e-10;
  4  every gradient against central differences of the NUMPY reference (not of the code under test): the bound per quantity is 100 x the
     disagreement of the reference's own differences at the steps 1e-5 and 1e-6, floored at 1e-8 (the precedent of tests/cid_numpy.py /
     test_wrench_host.py);
  5  the potential energy's flags, subsets of outputs and cotangents (bit-identical to the full call), accumulation, independence of the
     batch, the body-set resolution and its refusals;
  6  a stand-alone program (tests/host_shim/cen_main.cpp, its own main) built with -fsanitize=address,undefined (the sanitizers' runtimes linked statically into it) runs the forward and the
     reverse pass on the ball arm and on Atlas-20 and ends clean.

MEASURED (this file's inputs; printed by the tests).  The two ke routes disagree by at most 6.0e-16 relative.  The reference's central
differences at 1e-5 and 1e-6 disagree by at most: com 2.3e-10, com_vel 5.1e-10, com_acc 8.6e-10, momentum 5.0e-10, ke 9.6e-10, pe 2.7e-10
(max over the models, relative to max(1, |gradient|)), so the bounds of item 4 lie between 1e-8 and 9.6e-8; the code under test is within
9.4e-10 of the 1e-6 differences for every quantity (forward outputs and closed-form gradients: within 2.2e-15)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nimblephysics_amd as na
import cen_numpy
from nimblephysics_amd.centroidal import CEN_NO_SPRINGS, CEN_PE_BODY_ORIGIN, origin_moments, resolve_body_set
from oracle import OracleWorld
from test_dynamics_host import ShimDynamics

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL = 1e-10
NAMES = cen_numpy.ORDER                       # com, com_vel, com_acc, momentum, ke, pe
ROWS = (3, 3, 3, 6, 1, 1)
B = 8


def _build(out, src, extra=()):
    csrc = os.path.join(ROOT, "nimblephysics_amd", "csrc")
    deps = [src, os.path.join(HERE, "host_shim", "cen_shim.cpp"), os.path.join(HERE, "host_shim", "dyn_shim.cpp"), os.path.join(ROOT, "include", "nimble_amd.h")] + \
        [os.path.join(csrc, f) for f in ("centroidal_dev.hpp", "dynamics_dev.hpp", "kinematics_dev.hpp", "spatial_dev.hpp", "model_dev.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", *extra, "-I", os.path.join(HERE, "host_shim"), "-I", csrc,
                               "-I", os.path.join(ROOT, "include"), "-o", out, src])


def load_shim():
    out = os.path.join(HERE, "host_shim", "libcen_shim.so")
    _build(out, os.path.join(HERE, "host_shim", "cen_shim.cpp"), ("-shared",))
    lib = C.CDLL(out)
    vp, i64, u64, ci = C.c_void_p, C.c_int64, C.c_uint64, C.c_int
    lib.shim_dyn_model.argtypes = [vp]
    lib.shim_dyn_model.restype = vp
    lib.shim_dyn_free.argtypes = [vp]
    lib.shim_cen_set.argtypes = [vp, ci, vp, vp, vp, vp]
    lib.shim_cen_set.restype = None
    lib.shim_cen_mass.argtypes = [vp, u64]
    lib.shim_cen_mass.restype = C.c_double
    lib.shim_cen_forward.argtypes = [vp, u64, u64, i64, vp, vp, ci] + [vp] * 8
    lib.shim_cen_forward.restype = None
    lib.shim_cen_vjp.argtypes = [vp, u64, u64, i64, vp, vp, ci] + [vp] * 9 + [ci]
    lib.shim_cen_vjp.restype = None
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


class ShimCentroidal(ShimDynamics):
    """The host build of the device code for the body set `idx` (bodies of md.merge_welds(), as resolve_body_set gives them; None: all)."""

    def __init__(self, lib, md, idx=None):
        super().__init__(lib, md)
        arr = np.asarray(idx if idx is not None else [], dtype=np.int32)
        masks = np.zeros(2, dtype=np.uint64)
        self.origin = np.zeros(3 * 64)
        mo = _c(origin_moments(md))                                  # what centroidal.py hands to nbl_body_set_origin_moments
        lib.shim_cen_set(self.h, int(arr.size), _p(arr) if arr.size else None, _p(masks), _p(mo), _p(self.origin))
        self.mass_mask, self.joint_mask = int(masks[0]), int(masks[1])

    def mass(self):
        return self.lib.shim_cen_mass(self.h, self.mass_mask)

    def forward(self, S, A=None, flags=0, want=(True,) * 6, jac=False):
        S, A = _c(S), _c(A)
        nB = S.shape[1]
        outs = [np.full((r, nB), np.nan) if w else None for r, w in zip(ROWS, want)]
        J = np.full((3 * self.n, nB), np.nan) if jac else None
        self.lib.shim_cen_forward(self.h, self.mass_mask, self.joint_mask, nB, _p(S), _p(A), flags, _p(self.origin), *[_p(o) for o in outs], _p(J))
        return [o for o in outs if o is not None], J

    def vjp(self, S, A, cots, flags=0, init=None):
        S, A = _c(S), _c(A)
        cots = [_c(c) for c in cots]
        nB = S.shape[1]
        gs = np.full((2 * self.n, nB), np.nan) if init is None else init[0].copy()
        ga = np.full((self.n, nB), np.nan) if init is None else init[1].copy()
        self.lib.shim_cen_vjp(self.h, self.mass_mask, self.joint_mask, nB, _p(S), _p(A), flags, _p(self.origin), *[_p(c) for c in cots], _p(gs), _p(ga),
                              0 if init is None else 1)
        return gs, ga


def _states(md, nB, seed):
    """as test_gpu_dynamics._states, transposed: positions N(0, 0.5^2), velocities N(0, 1), accelerations N(0, 2^2)"""
    rng = np.random.default_rng(seed)
    n = md.num_dofs
    return np.concatenate([rng.normal(0, 0.5, (nB, n)), rng.normal(0, 1.0, (nB, n))], 1).T.copy(), rng.normal(0, 2.0, (nB, n)).T.copy()


def _cases():
    from test_ball_joint import ball_model
    ground = na.atlas("atlas20", ground=True)
    skel = ground.body_skeletons()
    atlas_skel = skel[[b.name for b in ground.bodies].index("l_foot")]
    return [("cartpole", na.cartpole(), None, None), ("ball_arm", ball_model(2, True), None, None),
            ("compound_joints", na.load_skel(os.path.join(HERE, "golden", "compound_joints.skel")), None, None),
            ("atlas20", na.atlas("atlas20"), None, None), ("atlas20_ground", ground, None, None),
            ("atlas20_ground_skeleton", ground, None, atlas_skel), ("atlas20_ground_feet", ground, ["l_foot", "r_foot"], None)]


CASES = _cases()
IDS = [c[0] for c in CASES]


def _selection(md, bodies, skeleton):
    """(the set as bodies of the description for cen_numpy, as bodies of the merged model for the shim, whether it is the whole model)"""
    if bodies is not None:
        sel = [[i for i, b in enumerate(md.bodies) if b.name == nm][0] for nm in bodies]
    elif skeleton is not None:
        sk = md.body_skeletons()
        sel = [i for i in cen_numpy.default_set(md) if sk[i] == skeleton]
    else:
        sel = cen_numpy.default_set(md)
    return sel, resolve_body_set(md, bodies, skeleton), sorted(sel) == cen_numpy.default_set(md)


def _err(x, ref):
    return float(np.abs(x - ref).max() / max(1.0, np.abs(ref).max()))


def test_the_cases_cover_welds_ball_joints_springs_and_two_skeletons():
    ground = CASES[4][1]
    assert ground.has_welds() and len(set(ground.body_skeletons())) >= 2
    assert any(b.joint_type == "ball" for b in CASES[1][1].bodies) and any(b.joint_type == "free" for b in CASES[3][1].bodies)
    assert any(np.any(md.flat()["spring"] != 0) for _, md, _, _ in CASES)
    assert any(np.abs(np.asarray(b.com)).max() > 1e-3 for b in CASES[3][1].bodies)


@pytest.mark.parametrize("name,md,bodies,skeleton", CASES, ids=IDS)
def test_forward_outputs_equal_the_numpy_statement(shim, name, md, bodies, skeleton):
    ow = OracleWorld(md)
    sel, idx, whole = _selection(md, bodies, skeleton)
    d = ShimCentroidal(shim, md, idx)
    n = md.num_dofs
    S, A = _states(md, B, 51)
    outs, J = d.forward(S, A, jac=True)
    (pe_origin,), _ = d.forward(S, None, CEN_PE_BODY_ORIGIN, (False,) * 5 + (True,))
    (pe_nospring,), _ = d.forward(S, None, CEN_NO_SPRINGS, (False,) * 5 + (True,))
    worst, floor = {}, 0.0
    for b in range(B):
        q, v, a = S[:n, b], S[n:, b], A[:, b]
        ref = cen_numpy.outputs(ow, md, sel, q, v, a)
        k = cen_numpy.Kin(ow, md, q, sel)
        e = {nm: _err(o[:, b], ref[nm]) for nm, o in zip(NAMES, outs)}
        e["Jcom"] = _err(J[:, b].reshape(3, n), ref["Jcom"])
        e["mass"] = abs(d.mass() - ref["mass"]) / ref["mass"]
        e["pe origin"] = _err(pe_origin[:, b], k.pe(md.gravity, at_com=False))
        e["pe no springs"] = _err(pe_nospring[:, b], k.pe(md.gravity, springs=False))
        if whole:
            ke_M = 0.5 * v @ ow.mass_matrix(q) @ v
            floor = max(floor, abs(ke_M - ref["ke"][0]) / max(1.0, abs(ke_M)))
            e["ke (M)"] = _err(outs[4][:, b], ke_M)
        # the linear momentum, computed from G V, against M com_vel, computed from m (v + w x c)
        e13 = _err(outs[3][3:, b], d.mass() * outs[1][:, b])
        assert e13 <= 1e-13, (name, b, e13)
        for kk, x in e.items():
            worst[kk] = max(worst.get(kk, 0.0), x)
        assert max(e.values()) <= TOL, (name, b, e)
    print(name, "worst relative errors:", worst, "| the two ke routes disagree by", floor)


@pytest.mark.parametrize("name,md,bodies,skeleton", CASES, ids=IDS)
def test_gradients_equal_the_closed_forms_and_the_references_central_differences(shim, name, md, bodies, skeleton):
    """See the head of this file for the measured disagreement of the reference's differences at the two steps."""
    ow = OracleWorld(md)
    sel, idx, whole = _selection(md, bodies, skeleton)
    d = ShimCentroidal(shim, md, idx)
    n = md.num_dofs
    S, A = _states(md, B, 52)
    rng = np.random.default_rng(53)
    cots = [rng.normal(0, 1.0, (r, B)) for r in ROWS]
    grads = {}
    for k, nm in enumerate(NAMES):                                   # one cotangent at a time: the gradient of each output on its own
        gs, ga = d.vjp(S, A, [c if j == k else None for j, c in enumerate(cots)])
        grads[nm] = np.concatenate([gs, ga])
    gs_all, ga_all = d.vjp(S, A, cots)
    total = sum(grads.values())
    assert np.abs(np.concatenate([gs_all, ga_all]) - total).max() <= 1e-12 * max(1.0, np.abs(total).max())
    worst_cf, worst_fd, floors = {}, {k: 0.0 for k in NAMES}, {k: 0.0 for k in NAMES}
    for b in range(B):
        q, v, a = S[:n, b], S[n:, b], A[:, b]
        cot = {nm: c[:, b] for nm, c in zip(NAMES, cots)}
        cf = cen_numpy.closed_form_vjp(ow, md, sel, q, v, cot, whole)
        dev = {"com_q": grads["com"][:n, b], "com_vel_v": grads["com_vel"][n:2 * n, b], "com_acc_a": grads["com_acc"][2 * n:, b],
               "pe_q": grads["pe"][:n, b], "ke_v": grads["ke"][n:2 * n, b], "ke_q": grads["ke"][:n, b]}
        for kk, ref in cf.items():
            e = _err(dev[kk], ref)
            worst_cf[kk] = max(worst_cf.get(kk, 0.0), e)
            assert e <= TOL, (name, b, kk, e)
        assert not grads["com"][n:, b].any() and not grads["pe"][n:, b].any() and not grads["ke"][2 * n:, b].any()
        fd5 = cen_numpy.fd_vjp(ow, md, sel, q, v, a, cot, 1e-5)
        fd6 = cen_numpy.fd_vjp(ow, md, sel, q, v, a, cot, 1e-6)
        for nm in NAMES:
            two = _err(fd5[nm], fd6[nm])
            e = _err(grads[nm][:, b], fd6[nm])
            floors[nm], worst_fd[nm] = max(floors[nm], two), max(worst_fd[nm], e)
            bound = max(100.0 * two, 1e-8)
            assert e <= bound, (name, b, nm, e, bound)
    print(name, "closed forms:", worst_cf)
    print(name, "reference differences, 1e-5 against 1e-6:", floors)
    print(name, "code under test against the 1e-6 differences:", worst_fd)


def test_subsets_accumulation_and_the_batch_do_not_change_the_bits(shim):
    md = na.atlas("atlas20")
    d = ShimCentroidal(shim, md)
    S, A = _states(md, 5, 54)
    rng = np.random.default_rng(55)
    cots = [rng.normal(0, 1.0, (r, 5)) for r in ROWS]
    outs, J = d.forward(S, A, jac=True)
    gs, ga = d.vjp(S, A, cots)
    for k in range(6):                                               # one output alone: the same bits as in the full call
        (o,), _ = d.forward(S, A if k == 2 else None, 0, tuple(j == k for j in range(6)))
        assert np.array_equal(o, outs[k]), NAMES[k]
    _, J1 = d.forward(S, None, 0, (False,) * 6, jac=True)
    assert np.array_equal(J1, J)
    for b in range(5):                                               # a world alone: the same bits as in the batch
        sl = slice(b, b + 1)
        o1, j1 = d.forward(S[:, sl], A[:, sl], jac=True)
        assert all(np.array_equal(x[:, 0], y[:, b]) for x, y in zip(o1, outs)) and np.array_equal(j1[:, 0], J[:, b])
        g1 = d.vjp(S[:, sl], A[:, sl], [c[:, sl] for c in cots])
        assert np.array_equal(g1[0][:, 0], gs[:, b]) and np.array_equal(g1[1][:, 0], ga[:, b])
    acc = (rng.normal(size=gs.shape), rng.normal(size=ga.shape))
    gs2, ga2 = d.vjp(S, A, cots, init=acc)
    assert np.abs(gs2 - (acc[0] + gs)).max() <= 1e-12 * max(1.0, np.abs(gs).max()) and np.abs(ga2 - (acc[1] + ga)).max() <= 1e-12 * max(1.0, np.abs(ga).max())
    # Jcom: the columns of coordinates that move no body of the set are written as zeros (the buffer starts as NaN)
    feet = ShimCentroidal(shim, md, resolve_body_set(md, ["l_foot", "r_foot"]))
    _, Jf = feet.forward(S, None, 0, (False,) * 6, jac=True)
    Jf = Jf.reshape(3, md.num_dofs, 5)
    from kin_numpy import _ndof, dof_offsets
    moving = set()
    for nm in ("l_foot", "r_foot"):
        c = [i for i, bd in enumerate(md.bodies) if bd.name == nm][0]
        while c >= 0:
            moving.update(range(dof_offsets(md)[c], dof_offsets(md)[c] + _ndof(md.bodies[c])))
            c = md.bodies[c].parent
    still = [dd for dd in range(md.num_dofs) if dd not in moving]
    assert still and np.isfinite(Jf).all() and not Jf[:, still].any() and (np.abs(Jf[:, sorted(moving)]).max(axis=(0, 2)) > 0).all()


def test_body_set_resolution_and_its_refusals():
    md = na.atlas("atlas20")                                         # the hands are welded to the forearms
    targets, _ = md.weld_targets()
    names = [b.name for b in md.bodies]
    welded = [i for i, b in enumerate(md.bodies) if b.joint_type == "weld" and targets[i] >= 0]
    assert welded, "atlas20 has bodies welded into their parents"
    w = welded[0]
    carrier = [i for i, t in enumerate(targets) if t == targets[w] and md.bodies[i].joint_type != "weld"][0]
    group = [i for i, t in enumerate(targets) if t == targets[w]]
    assert resolve_body_set(md) is None
    assert resolve_body_set(md, group) == [targets[w]]
    assert resolve_body_set(md, [names[i] for i in group]) == [targets[w]]
    with pytest.raises(na.NimbleAmdError, match="welded into one body"):
        resolve_body_set(md, [names[w]])
    with pytest.raises(na.NimbleAmdError, match="welded into one body"):
        resolve_body_set(md, [carrier])
    with pytest.raises(na.NimbleAmdError, match="named twice"):
        resolve_body_set(md, ["l_foot", "l_foot"])
    with pytest.raises(ValueError):
        resolve_body_set(md, ["no_such_body"])
    with pytest.raises(ValueError):
        resolve_body_set(md, ["l_foot"], skeleton=0)
    ground = na.atlas("atlas20", ground=True)
    fixed = [i for i, t in enumerate(ground.weld_targets()[0]) if t < 0]
    assert fixed, "the ground link of atlas20 with ground is welded to the world"
    with pytest.raises(na.NimbleAmdError, match="welded to the world"):
        resolve_body_set(ground, [fixed[0]])
    with pytest.raises(ValueError, match="body set"):                 # the messages name the body set, not the mapping they are resolved with
        resolve_body_set(md, ["no_such_body"])
    sk = ground.body_skeletons()
    atlas_skel = sk[[b.name for b in ground.bodies].index("l_foot")]
    merged = ground.merge_welds()
    got = resolve_body_set(ground, skeleton=atlas_skel)
    assert got == sorted({t for i, t in enumerate(ground.weld_targets()[0]) if t >= 0 and sk[i] == atlas_skel}) and len(got) <= len(merged.bodies)
    with pytest.raises(na.NimbleAmdError, match="skeleton"):
        resolve_body_set(ground, skeleton=12345)


def _write_input(path, md, nB, seed):
    dev = md.merge_welds() if md.has_welds() else md
    fl, n = dev.flat(), dev.num_dofs
    S, A = _states(dev, nB, seed)
    cot = np.random.default_rng(seed + 1).normal(0, 1.0, (17, nB))
    from nimblephysics_amd import _abi
    with open(path, "w") as f:
        f.write(f"{len(dev.bodies)} {n} {nB}\n")
        f.write(" ".join(repr(float(x)) for x in list(dev.gravity) + [dev.dt]) + "\n")
        for i, b in enumerate(dev.bodies):
            f.write(f"{int(fl['parent'][i])} {int(fl['joint_type'][i])} {int(fl['dof_offset'][i])} {float(getattr(b, 'pitch', 0.1))!r}\n")
            for key in ("T_pj", "T_cj", "axis", "mass", "com", "inertia"):
                f.write(" ".join(repr(float(x)) for x in np.ravel(fl[key][i])) + "\n")
        for j in range(n):
            f.write(f"{float(fl['damping'][j])!r} {float(fl['spring'][j])!r} {float(fl['rest'][j])!r}\n")
        for arr in (S, A, cot):
            f.write(" ".join(repr(float(x)) for x in arr.ravel()) + "\n")
    assert _abi is not None


def test_a_stand_alone_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """cen_main.cpp has its own main and is never loaded into Python: the forward and the reverse pass on the ball arm and on Atlas-20."""
    from test_ball_joint import ball_model
    exe = os.path.join(HERE, "host_shim", "cen_main_san")
    _build(exe, os.path.join(HERE, "host_shim", "cen_main.cpp"), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                   "-static-libasan", "-static-libubsan"))   # the runtimes inside the executable
    for name, md in (("ball_arm", ball_model(2, True)), ("atlas20", na.atlas("atlas20"))):
        inp = str(tmp_path / (name + ".txt"))
        _write_input(inp, md, 3, 60)
        r = subprocess.run([exe, inp], capture_output=True, text=True, timeout=120)
        print(name, r.stdout.strip(), r.stderr.strip()[-2000:])
        assert r.returncode == 0 and "checksum" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (name, r.returncode, r.stderr[-2000:])
