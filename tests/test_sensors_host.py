"""The PRODUCT's inertial-sensor code (nimblephysics_amd/csrc/sensors_dev.hpp: what k_sensors and k_sensors_vjp run per lane) compiled for the
host with g++ -O2 -ffp-contract=off (tests/host_shim/sens_shim.cpp) and held to tests/sens_numpy.py, the numpy statement in world
coordinates, on cartpole, the ball arm, Atlas-20 on the ground and Atlas-33, eight worlds each, states drawn as in
test_gpu_dynamics._states, the field N(0, 1).

The sensor list of a model (sensor_list): identity on the root body; a general rotation + translation on a leaf; two different sensors
on one body; one on the world (-1); on Atlas one on a weld-merged body; on the ball arm one on a ball-jointed body (the z body of its triple).

  1  gyro, acc, mag: |x - ref| / max(1, |ref|) <= 1e-10;
  2  the closed-form blocks d gyro / dv, d acc / da, d mag / d field against the numpy Jacobians: 1e-10; the blocks that are identically
     zero (d gyro / da, d mag / dv, d mag / da, everything of the world sensor to state and accel) are exactly zero;
  3  every gradient against central differences of the NUMPY reference: the bound per output is 100 x the disagreement of the reference's
     own differences at the steps 1e-5 and 1e-6, floored at 1e-8 (the rule of tests/test_centroidal_host.py);
  4  subsets of outputs and cotangents (bit-identical to the full call), accumulation, independence of the batch;
  5  a stand-alone program (tests/host_shim/sens_main.cpp, its own main) built with -fsanitize=address,undefined (the sanitizers' runtimes
     linked statically into it) runs the forward and the reverse pass on the ball arm and on Atlas-20 and ends clean.

MEASURED (this file's inputs; printed by the tests).  Readings within 8.5e-16 of the numpy statement, closed-form blocks within 1.1e-15.
The reference's central differences at 1e-5 and 1e-6 disagree by at most: gyro 6.5e-10, acc 1.1e-9, mag 3.4e-10 (max over the models,
relative to max(1, |gradient|)), so the bounds of item 3 lie between 1e-8 and 1.1e-7; the code under test is within 1.1e-9 of the 1e-6
differences for every output."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nimblephysics_amd as na
import cen_numpy
import sens_numpy
from nimblephysics_amd.sensors import resolve_sensors
from oracle import OracleWorld
from test_dynamics_host import ShimDynamics

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL = 1e-10
NAMES = sens_numpy.ORDER                      # gyro, acc, mag
B = 8


def _build(out, src, extra=()):
    csrc = os.path.join(ROOT, "nimblephysics_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "nimble_amd.h")] + \
        [os.path.join(HERE, "host_shim", f) for f in ("sens_shim.cpp", "wrench_shim.cpp", "fdyn_shim.cpp", "dyn_shim.cpp")] + \
        [os.path.join(csrc, f) for f in ("sensors_dev.hpp", "centroidal_dev.hpp", "dynamics_dev.hpp", "kinematics_dev.hpp", "spatial_dev.hpp", "model_dev.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", *extra, "-I", os.path.join(HERE, "host_shim"), "-I", csrc,
                               "-I", os.path.join(ROOT, "include"), "-o", out, src])


def load_shim():
    out = os.path.join(HERE, "host_shim", "libsens_shim.so")
    _build(out, os.path.join(HERE, "host_shim", "sens_shim.cpp"), ("-shared",))
    lib = C.CDLL(out)
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    lib.shim_dyn_model.argtypes = [vp]
    lib.shim_dyn_model.restype = vp
    lib.shim_dyn_free.argtypes = [vp]
    lib.shim_wrench_set.argtypes = [vp, ci, vp, vp]
    lib.shim_wrench_set.restype = vp
    lib.shim_wrench_set_free.argtypes = [vp]
    lib.shim_sens_forward.argtypes = [vp, vp, i64] + [vp] * 6
    lib.shim_sens_forward.restype = None
    lib.shim_sens_vjp.argtypes = [vp, vp, i64] + [vp] * 9 + [ci]
    lib.shim_sens_vjp.restype = None
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def rigid(rng, spread):
    """a 4 x 4 transform: a rotation by a vector N(0, 0.8^2) per axis, a translation N(0, spread^2)"""
    r = rng.normal(0, 0.8, 3)
    th = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / th
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = rng.normal(0, spread, 3)
    return T


def sensor_list(md, seed=5):
    """[(index in md.bodies or -1, T 4 x 4 or None)]: see the head of this file"""
    rng = np.random.default_rng(seed)
    movable = cen_numpy.default_set(md)
    parents = {b.parent for b in md.bodies}
    leaves = [i for i in movable if i not in parents and md.bodies[i].joint_type != "weld"]
    mid = movable[len(movable) // 2]
    out = [(movable[0], None), (leaves[-1], rigid(rng, 0.2)), (mid, rigid(rng, 0.2)), (mid, rigid(rng, 0.2)), (-1, rigid(rng, 0.2))]
    welded = [i for i in movable if md.bodies[i].joint_type == "weld"]
    if welded:
        out.append((welded[0], rigid(rng, 0.1)))
    ball = [i for i in movable if md.bodies[i].joint_type == "ball"]
    if ball:
        out.append((ball[-1], rigid(rng, 0.1)))
    return out


def as_numpy_sensors(sensors):
    return [(i, np.eye(4) if T is None else T) for i, T in sensors]


class ShimSensors(ShimDynamics):
    """The host build of the device code for the sensor list `sensors` of md, resolved as nimblephysics_amd.sensors resolves it."""

    def __init__(self, lib, md, sensors):
        super().__init__(lib, md)
        res = resolve_sensors(md, sensors)
        self.S = len(res)
        body = np.array([mb for mb, _ in res], dtype=np.int32)
        T = _c(np.stack([np.concatenate([t[:3, :3].reshape(9), t[:3, 3]]) for _, t in res]))
        self.set = lib.shim_wrench_set(self.h, self.S, _p(body), _p(T))

    def __del__(self):
        self.lib.shim_wrench_set_free(self.set)
        super().__del__()

    def forward(self, S, A=None, F=None, want=(True, True, True)):
        S, A, F = _c(S), _c(A), _c(F)
        nB = S.shape[1]
        outs = [np.full((3 * self.S, nB), np.nan) if w else None for w in want]
        self.lib.shim_sens_forward(self.h, self.set, nB, _p(S), _p(A), _p(F), *[_p(o) for o in outs])
        return [o for o in outs if o is not None]

    def vjp(self, S, A, F, cots, init=None):
        """(grad_state [2n][B], grad_accel [n][B], grad_field [3][B]); init: accumulate onto these three"""
        S, A, F = _c(S), _c(A), _c(F)
        cots = [_c(c) for c in cots]
        nB = S.shape[1]
        g = [np.full((r, nB), np.nan) for r in (2 * self.n, self.n, 3)] if init is None else [x.copy() for x in init]
        self.lib.shim_sens_vjp(self.h, self.set, nB, _p(S), _p(A), _p(F), *[_p(c) for c in cots], *[_p(x) for x in g], 0 if init is None else 1)
        return g


def _states(md, nB, seed):
    """as test_gpu_dynamics._states, transposed, and a field N(0, 1): state [2n][B], accel [n][B], field [3][B]"""
    rng = np.random.default_rng(seed)
    n = md.num_dofs
    return (np.concatenate([rng.normal(0, 0.5, (nB, n)), rng.normal(0, 1.0, (nB, n))], 1).T.copy(), rng.normal(0, 2.0, (nB, n)).T.copy(),
            rng.normal(0, 1.0, (nB, 3)).T.copy())


def _cases():
    from test_ball_joint import ball_model
    return [("cartpole", na.cartpole()), ("ball_arm", ball_model(2, True)), ("atlas20_ground", na.atlas("atlas20", ground=True)),
            ("atlas33", na.atlas("atlas33"))]


CASES = _cases()
IDS = [c[0] for c in CASES]


def _err(x, ref):
    return float(np.abs(x - ref).max() / max(1.0, np.abs(ref).max()))


def test_the_sensor_lists_cover_welds_ball_joints_the_world_and_shared_bodies():
    lists = {name: sensor_list(md) for name, md in CASES}
    for name, md in CASES:
        s = lists[name]
        assert s[0][1] is None and s[2][0] == s[3][0] and any(i == -1 for i, _ in s), name
    assert any(CASES[2][1].bodies[i].joint_type == "weld" for i, _ in lists["atlas20_ground"] if i >= 0)
    assert any(CASES[3][1].bodies[i].joint_type == "weld" for i, _ in lists["atlas33"] if i >= 0)
    assert any(CASES[1][1].bodies[i].joint_type == "ball" for i, _ in lists["ball_arm"] if i >= 0)


@pytest.mark.parametrize("name,md", CASES, ids=IDS)
def test_readings_equal_the_numpy_statement(shim, name, md):
    ow = OracleWorld(md)
    sensors = sensor_list(md)
    ns = as_numpy_sensors(sensors)
    d = ShimSensors(shim, md, sensors)
    n = md.num_dofs
    S, A, F = _states(md, B, 51)
    outs = d.forward(S, A, F)
    worst = {}
    for b in range(B):
        ref = sens_numpy.readings(ow, md, ns, S[:n, b], S[n:, b], A[:, b], F[:, b])
        e = {nm: _err(o[:, b], ref[nm]) for nm, o in zip(NAMES, outs)}
        for kk, x in e.items():
            worst[kk] = max(worst.get(kk, 0.0), x)
        assert max(e.values()) <= TOL, (name, b, e)
    print(name, "worst relative errors:", worst)


@pytest.mark.parametrize("name,md", CASES, ids=IDS)
def test_gradients_equal_the_closed_forms_and_the_references_central_differences(shim, name, md):
    ow = OracleWorld(md)
    sensors = sensor_list(md)
    ns = as_numpy_sensors(sensors)
    d = ShimSensors(shim, md, sensors)
    n, P = md.num_dofs, 3 * len(sensors)
    S, A, F = _states(md, B, 52)
    rng = np.random.default_rng(53)
    cots = [rng.normal(0, 1.0, (P, B)) for _ in NAMES]
    grads = {}
    for k, nm in enumerate(NAMES):                                   # one cotangent at a time: the gradient of each output on its own
        grads[nm] = np.concatenate(d.vjp(S, A, F, [c if j == k else None for j, c in enumerate(cots)]))
    total = sum(grads.values())
    both = np.concatenate(d.vjp(S, A, F, cots))
    assert np.abs(both - total).max() <= 1e-12 * max(1.0, np.abs(total).max())
    worst_cf, worst_fd, floors = {}, {k: 0.0 for k in NAMES}, {k: 0.0 for k in NAMES}
    for b in range(B):
        q, v, a, m = S[:n, b], S[n:, b], A[:, b], F[:, b]
        cot = {nm: c[:, b] for nm, c in zip(NAMES, cots)}
        cf = sens_numpy.closed_form_jacobians(ow, md, ns, q)
        dev = {"gyro_v": (grads["gyro"][n:2 * n, b], cf["gyro_v"].T @ cot["gyro"]), "acc_a": (grads["acc"][2 * n:3 * n, b], cf["acc_a"].T @ cot["acc"]),
               "mag_m": (grads["mag"][3 * n:, b], cf["mag_m"].T @ cot["mag"])}
        for kk, (x, ref) in dev.items():
            e = _err(x, ref)
            worst_cf[kk] = max(worst_cf.get(kk, 0.0), e)
            assert e <= TOL, (name, b, kk, e)
        assert not grads["gyro"][2 * n:, b].any() and not grads["mag"][n:3 * n, b].any() and not grads["acc"][3 * n:, b].any()
        fd5 = sens_numpy.fd_vjp(ow, md, ns, q, v, a, m, cot, 1e-5)
        fd6 = sens_numpy.fd_vjp(ow, md, ns, q, v, a, m, cot, 1e-6)
        for nm in NAMES:
            two = _err(fd5[nm], fd6[nm])
            e = _err(grads[nm][:, b], fd6[nm])
            floors[nm], worst_fd[nm] = max(floors[nm], two), max(worst_fd[nm], e)
            bound = max(100.0 * two, 1e-8)
            assert e <= bound, (name, b, nm, e, bound)
    print(name, "closed forms:", worst_cf)
    print(name, "reference differences, 1e-5 against 1e-6:", floors)
    print(name, "code under test against the 1e-6 differences:", worst_fd)


def test_a_sensor_in_the_world_reads_the_constants_and_moves_no_gradient(shim):
    md = na.atlas("atlas20")
    T = rigid(np.random.default_rng(3), 0.3)
    d = ShimSensors(shim, md, [(-1, T)])
    S, A, F = _states(md, 3, 56)
    gyro, acc, mag = d.forward(S, A, F)
    R, g = T[:3, :3], np.asarray(md.gravity, dtype=np.float64)
    assert not gyro.any() and np.abs(acc - (-R.T @ g)[:, None]).max() <= 1e-15 and np.abs(mag - R.T @ F).max() <= 1e-15
    cots = [np.random.default_rng(4).normal(size=(3, 3)) for _ in NAMES]
    gs, ga, gf = d.vjp(S, A, F, cots)
    assert not gs.any() and not ga.any() and np.abs(gf - R @ cots[2]).max() <= 1e-15


def test_subsets_accumulation_and_the_batch_do_not_change_the_bits(shim):
    md = na.atlas("atlas20")
    sensors = sensor_list(md)
    d = ShimSensors(shim, md, sensors)
    S, A, F = _states(md, 5, 54)
    rng = np.random.default_rng(55)
    cots = [rng.normal(0, 1.0, (3 * len(sensors), 5)) for _ in NAMES]
    outs = d.forward(S, A, F)
    g = d.vjp(S, A, F, cots)
    for k in range(3):                                               # one output alone: the same bits as in the full call
        (o,) = d.forward(S, A if k == 1 else None, F if k == 2 else None, tuple(j == k for j in range(3)))
        assert np.array_equal(o, outs[k]), NAMES[k]
    for b in range(5):                                               # a world alone: the same bits as in the batch
        sl = slice(b, b + 1)
        o1 = d.forward(S[:, sl], A[:, sl], F[:, sl])
        assert all(np.array_equal(x[:, 0], y[:, b]) for x, y in zip(o1, outs))
        g1 = d.vjp(S[:, sl], A[:, sl], F[:, sl], [c[:, sl] for c in cots])
        assert all(np.array_equal(x[:, 0], y[:, b]) for x, y in zip(g1, g))
    acc = [rng.normal(size=x.shape) for x in g]
    g2 = d.vjp(S, A, F, cots, init=acc)
    for x2, x0, x in zip(g2, acc, g):
        assert np.abs(x2 - (x0 + x)).max() <= 1e-12 * max(1.0, np.abs(x).max())


def _write_input(path, md, sensors, nB, seed):
    dev = md.merge_welds() if md.has_welds() else md
    fl, n = dev.flat(), dev.num_dofs
    res = resolve_sensors(md, sensors)
    S, A, F = _states(dev, nB, seed)
    cot = np.random.default_rng(seed + 1).normal(0, 1.0, (9 * len(res), nB))
    with open(path, "w") as f:
        f.write(f"{len(dev.bodies)} {n} {nB} {len(res)}\n")
        f.write(" ".join(repr(float(x)) for x in list(dev.gravity) + [dev.dt]) + "\n")
        for i, b in enumerate(dev.bodies):
            f.write(f"{int(fl['parent'][i])} {int(fl['joint_type'][i])} {int(fl['dof_offset'][i])} {float(getattr(b, 'pitch', 0.1))!r}\n")
            for key in ("T_pj", "T_cj", "axis", "mass", "com", "inertia"):
                f.write(" ".join(repr(float(x)) for x in np.ravel(fl[key][i])) + "\n")
        for j in range(n):
            f.write(f"{float(fl['damping'][j])!r} {float(fl['spring'][j])!r} {float(fl['rest'][j])!r}\n")
        for mb, T in res:
            f.write(f"{int(mb)} " + " ".join(repr(float(x)) for x in np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])) + "\n")
        for arr in (S, A, F, cot):
            f.write(" ".join(repr(float(x)) for x in arr.ravel()) + "\n")


def test_a_stand_alone_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """sens_main.cpp has its own main and is never loaded into Python: the forward and the reverse pass on the ball arm and on Atlas-20."""
    from test_ball_joint import ball_model
    exe = os.path.join(HERE, "host_shim", "sens_main_san")
    _build(exe, os.path.join(HERE, "host_shim", "sens_main.cpp"), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                    "-static-libasan", "-static-libubsan"))   # the runtimes inside the executable
    for name, md in (("ball_arm", ball_model(2, True)), ("atlas20", na.atlas("atlas20"))):
        inp = str(tmp_path / (name + ".txt"))
        _write_input(inp, md, sensor_list(md), 3, 60)
        r = subprocess.run([exe, inp], capture_output=True, text=True, timeout=120)
        print(name, r.stdout.strip(), r.stderr.strip()[-2000:])
        assert r.returncode == 0 and "checksum" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (name, r.returncode, r.stderr[-2000:])
