"""What the 43 built-once calls (csrc/nimble_amd_tree.hip) REFUSE, and what they accept without launching: the return code and the
whole text of nbl_last_error() of every bad call below, as literals.  A characterisation table: it pins which mistake a call names, in
which words, and which mistake wins when two are made, so that the argument checks can be reorganised without a caller noticing.

One model (test_ball_joint.ball_model with ground: free root, ball joints, 16 DOFs) on a handle of the 8-slot and of the 16-slot build,
B = 2.  Every case would be harmless if it were wrongly accepted: every pointer is a full-size device buffer (inputs zero, outputs NaN),
only an integer, a size or the choice of map lies; a workspace "one byte short" is the full workspace with its size stated as need - 1.
Not here, because accepting them would launch on a null or oversized range: a null required pointer, "B too large for one launch".
No kernel runs in this file: the last test finds every output buffer still NaN."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, N, P = 2, 16, 9                       # worlds, DOFs of the model, rows of the map (one spatial entry, one linear)
BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
OTHER_MAP = "the kinematics map was made for another model"
OTHER_SET = "the body set was made for another model"
NEG_B = "B must not be negative (got -1)"


class _CIKConfig(C.Structure):           # nbl_ik_config
    _fields_ = [("convergence_threshold", C.c_double), ("max_step_count", C.c_int32), ("least_squares_damping", C.c_double),
                ("start_clamped", C.c_int32), ("line_search", C.c_int32), ("dont_exit_transpose", C.c_int32)]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Rig:
    def __init__(self):
        import nimblephysics_amd as na
        from nimblephysics_amd.centroidal import _body_set
        from test_ball_joint import ball_model
        md = ball_model(4, True, ground=True)
        ball = [i for i, b in enumerate(md.bodies) if b.joint_type == "ball"][0]
        last = len(md.bodies) - 1
        self.worlds = []
        for v in (0, 1):                 # read at every nbl_model_create
            os.environ["NBL_MIN_VARIANT"] = str(v)
            self.worlds.append(na.World(md, device=DEV))
        w0, w1 = self.worlds
        self.L, self.h, self.h1 = w0._L, w0._h, w1._h
        assert [self.L.nbl_model_max_contacts(w._h) for w in self.worlds] == [8, 16] and md.num_dofs == N and len(md.bodies) == 5
        self.keep = []

        def mapping(w, entries):
            m = na.IKMapping(w)
            for kind, body in entries:
                (m.addSpatialBodyNode, m.addLinearBodyNode)[kind](body)
            self.keep.append(m)
            return m._device_map(w)
        self.mixed = mapping(w0, [(0, ball), (1, last)])           # 9 rows; as a wrench or sensor set: entry 1 is not spatial
        self.one = mapping(w0, [(0, ball)])                        # a wrench / sensor / contact set of one frame
        self.two = mapping(w0, [(0, ball), (0, last)])             # ... of two frames
        self.mixed1 = mapping(w1, [(0, ball), (1, last)])          # the same maps on the handle of the other instantiation
        self.one1 = mapping(w1, [(0, ball)])
        assert self.L.nbl_kin_map_dim(self.mixed) == P
        self.sets = [_body_set(w0), _body_set(w1)]
        self.set, self.set1 = self.sets[0].ptr, self.sets[1].ptr
        self.outs = []
        L, h = self.L, self.h
        self.need = {"dyn": L.nbl_dynamics_workspace_bytes(h, B), "fdyn": L.nbl_forward_dynamics_workspace_bytes(h, B),
                     "wrench0": L.nbl_wrench_workspace_bytes(h, None, B), "wrench1": L.nbl_wrench_workspace_bytes(h, self.one, B),
                     "wrench2": L.nbl_wrench_workspace_bytes(h, self.two, B), "ik": L.nbl_ik_workspace_bytes(h, self.mixed, B),
                     "ikg": L.nbl_ik_grad_workspace_bytes(h, self.mixed, B), "cen": L.nbl_centroidal_workspace_bytes(h, B),
                     "sens": L.nbl_sensors_workspace_bytes(h, B), "task": L.nbl_task_workspace_bytes(h, B)}
        assert min(self.need.values()) > 0
        self.ws = torch.zeros(max(self.need.values()), dtype=torch.uint8, device=DEV)
        self.S, self.A, self.X = self.zeros(2 * N), self.zeros(N), self.zeros(N * N)
        self.W, self.F, self.T, self.G = self.zeros(12), self.zeros(3), self.zeros(P), self.zeros(P * N)

    def zeros(self, rows):
        return torch.zeros((rows, B), dtype=torch.float64, device=DEV)

    def out(self, rows, dtype=torch.float64):
        """an output buffer, NaN (or -1) until a kernel writes it"""
        t = torch.full((rows, B), float("nan") if dtype == torch.float64 else -1, dtype=dtype, device=DEV)
        self.outs.append(t)
        return _p(t)

    def cfg(self, steps=20, damping=0.01):
        """(a threshold every loss meets: were the call accepted, the solve would stop at once)"""
        self.keep.append(_CIKConfig(1e300, steps, damping, 0, 1, 0))
        return C.byref(self.keep[-1])


@pytest.fixture(scope="module")
def rig():
    mp = pytest.MonkeyPatch()
    mp.setenv("NBL_MIN_VARIANT", "0")
    yield Rig()
    mp.undo()


# ---- the calls, with the arguments a case may bend; everything else is valid ----
def kin_fwd(r, h="h", k="mixed", B=B, outputs=True):
    return r.L.nbl_kinematics_forward(_h(r, h), _k(r, k), B, _p(r.S), r.out(P) if outputs else None, r.out(P) if outputs else None, None)


def kin_bwd(r, h="h", k="mixed", B=B):
    return r.L.nbl_kinematics_backward(_h(r, h), _k(r, k), B, _p(r.S), _p(r.T), _p(r.T), r.out(2 * N), 0, None)


def id_fwd(r, h="h", B=B, flags=0, short=0):
    return r.L.nbl_inverse_dynamics_forward(_h(r, h), B, _p(r.S), _p(r.A), flags, r.out(N), _p(r.ws), r.need["dyn"] - short, None)


def id_bwd(r, h="h", B=B, flags=0, short=0, outputs=True):
    o = (r.out(2 * N), r.out(N)) if outputs else (None, None)
    return r.L.nbl_inverse_dynamics_backward(_h(r, h), B, _p(r.S), _p(r.A), flags, _p(r.A), o[0], o[1], 0, _p(r.ws), r.need["dyn"] - short, None)


def mass(r, h="h", B=B, short=0):
    return r.L.nbl_mass_matrix(_h(r, h), B, _p(r.S), r.out(N * N), _p(r.ws), r.need["dyn"] - short, None)


def id_inertia(r, h="h", B=B, flags=0, short=0):
    return r.L.nbl_inverse_dynamics_backward_inertia(_h(r, h), B, _p(r.S), _p(r.A), flags, _p(r.A), r.out(1), 0, _p(r.ws),
                                                     r.need["dyn"] - short, None)


def fd_fwd(r, h="h", B=B, flags=0, short=0):
    return r.L.nbl_forward_dynamics_forward(_h(r, h), B, _p(r.S), _p(r.A), flags, r.out(N), _p(r.ws), r.need["fdyn"] - short, None)


def fd_bwd(r, h="h", B=B, flags=0, short=0, outputs=True):
    o = (r.out(2 * N), r.out(N)) if outputs else (None, None)
    return r.L.nbl_forward_dynamics_backward(_h(r, h), B, _p(r.S), _p(r.A), flags, _p(r.A), o[0], o[1], 0, _p(r.ws), r.need["fdyn"] - short, None)


def minv_apply(r, h="h", B=B, R=N, X=True, short=0):
    return r.L.nbl_inv_mass_apply(_h(r, h), B, R, _p(r.S), _p(r.X) if X else None, r.out(N * N), _p(r.ws), r.need["fdyn"] - short, None)


def minv(r, h="h", B=B, short=0):
    return r.L.nbl_inv_mass_matrix(_h(r, h), B, _p(r.S), r.out(N * N), _p(r.ws), r.need["fdyn"] - short, None)


def _wneed(r, k):
    return r.need[{"none": "wrench0", "one": "wrench1", "two": "wrench2"}.get(k, "wrench2")]


def wrench_fwd(fn):
    def call(r, h="h", k="one", B=B, flags=0, short=0):
        return getattr(r.L, fn)(_h(r, h), _k(r, k), B, _p(r.S), _p(r.A), _p(r.W), flags, r.out(N), _p(r.ws), _wneed(r, k) - short, None)
    return call


def wrench_bwd(fn):
    def call(r, h="h", k="one", B=B, flags=0, short=0, outputs=True):
        o = (r.out(2 * N), r.out(N), r.out(12)) if outputs else (None, None, None)
        return getattr(r.L, fn)(_h(r, h), _k(r, k), B, _p(r.S), _p(r.A), _p(r.W), flags, _p(r.A), o[0], o[1], o[2], 0, _p(r.ws),
                                _wneed(r, k) - short, None)
    return call


idw_fwd, fdw_fwd = wrench_fwd("nbl_inverse_dynamics_wrench_forward"), wrench_fwd("nbl_forward_dynamics_wrench_forward")
idw_bwd, fdw_bwd = wrench_bwd("nbl_inverse_dynamics_wrench_backward"), wrench_bwd("nbl_forward_dynamics_wrench_backward")


def fd_inertia(r, h="h", k="one", B=B, flags=0, short=0):
    need = _wneed(r, k) if k != "none" else r.need["fdyn"]
    return r.L.nbl_forward_dynamics_backward_inertia(_h(r, h), _k(r, k), B, _p(r.S), _p(r.A), _p(r.W), flags, _p(r.A), r.out(1), 0, _p(r.ws),
                                                     need - short, None)


def cid(r, h="h", k="two", B=B, mode=2, flags=0, short=0):
    return r.L.nbl_contact_inverse_dynamics(_h(r, h), _k(r, k), B, _p(r.S), _p(r.A), _p(r.W), mode, flags, r.out(12), r.out(N), _p(r.ws),
                                            _wneed(r, k) - short, None)


def ik(r, h="h", k="mixed", B=B, steps=20, damping=0.01, short=0):
    return r.L.nbl_ik_solve(_h(r, h), _k(r, k), B, _p(r.T), _p(r.A), r.cfg(steps, damping), r.out(N), r.out(1), r.out(1, torch.int32), _p(r.ws),
                            r.need["ik"] - short, None)


def ik_vjp(r, h="h", k="mixed", B=B, mu=1e-9, short=0):
    return r.L.nbl_ik_solve_vjp(_h(r, h), _k(r, k), B, _p(r.A), _p(r.A), mu, r.out(P), 0, r.out(1, torch.int32), _p(r.ws), r.need["ikg"] - short,
                                None)


def cen_fwd(r, h="h", s="set", B=B, flags=0, short=0, accel=True, outputs=True, com_acc=True):
    o = [r.out(rows) for rows in (3, 3, 3, 6, 1, 1, 3 * N)] if outputs else [None] * 7
    o[2] = r.out(3) if com_acc else None                 # (com_acc alone is no output without accel: the call refuses first)
    return r.L.nbl_centroidal_forward(_h(r, h), _s(r, s), B, _p(r.S), _p(r.A) if accel else None, flags, *o, _p(r.ws), r.need["cen"] - short, None)


def cen_bwd(r, h="h", s="set", B=B, flags=0, short=0, accel=True, outputs=True):
    o = (r.out(2 * N), r.out(N)) if outputs else (None, None)
    g = [_p(r.zeros(rows)) for rows in (3, 3, 3, 6, 1, 1)]
    return r.L.nbl_centroidal_backward(_h(r, h), _s(r, s), B, _p(r.S), _p(r.A) if accel else None, flags, *g, o[0], o[1], 0, _p(r.ws),
                                       r.need["cen"] - short, None)


def sens_fwd(r, h="h", k="two", B=B, short=0, accel=True, field=True, outputs=("gyro", "acc", "mag")):
    o = [r.out(6) if nm in outputs else None for nm in ("gyro", "acc", "mag")]
    return r.L.nbl_sensors_forward(_h(r, h), _k(r, k), B, _p(r.S), _p(r.A) if accel else None, _p(r.F) if field else None, *o, _p(r.ws),
                                   r.need["sens"] - short, None)


def sens_bwd(r, h="h", k="two", B=B, short=0, accel=True, field=True, cots=("gyro", "acc", "mag"), outputs=True):
    g = [_p(r.zeros(6)) if nm in cots else None for nm in ("gyro", "acc", "mag")]
    o = (r.out(2 * N), r.out(N), r.out(3)) if outputs else (None, None, None)
    return r.L.nbl_sensors_backward(_h(r, h), _k(r, k), B, _p(r.S), _p(r.A) if accel else None, _p(r.F) if field else None, *g, *o, 0, _p(r.ws),
                                    r.need["sens"] - short, None)


def task_jac(fn):
    def call(r, h="h", k="mixed", B=B, rows=P, n=N):
        return getattr(r.L, fn)(_h(r, h), _k(r, k), B, rows, n, _p(r.S), r.out(P * N), None)
    return call


tj, tjd = task_jac("nbl_task_jacobian"), task_jac("nbl_task_jacobian_deriv")


def tj_vjp(r, h="h", k="mixed", B=B, rows=P, n=N):
    return r.L.nbl_task_jacobian_vjp(_h(r, h), _k(r, k), B, rows, n, _p(r.S), _p(r.G), r.out(N), 0, None)


def t_acc(r, h="h", k="mixed", B=B, rows=P, n=N, accel=True, outputs=True):
    o = (r.out(P), r.out(P)) if outputs else (None, None)
    return r.L.nbl_task_accel(_h(r, h), _k(r, k), B, rows, n, _p(r.S), _p(r.A) if accel else None, o[0], o[1], None)


def t_acc_vjp(r, h="h", k="mixed", B=B, rows=P, n=N, accel=True, outputs=True, short=0):
    o = (r.out(2 * N), r.out(N)) if outputs else (None, None)
    return r.L.nbl_task_accel_vjp(_h(r, h), _k(r, k), B, rows, n, _p(r.S), _p(r.A) if accel else None, _p(r.T), o[0], o[1], 0, _p(r.ws),
                                  r.need["task"] - short, None)


def _h(r, h):
    return {"h": r.h, "h1": r.h1, "null": None}[h]


def _k(r, k):
    return {"mixed": r.mixed, "one": r.one, "two": r.two, "mixed1": r.mixed1, "one1": r.one1, "none": None}[k]


def _s(r, s):
    return {"set": r.set, "set1": r.set1, "none": None}[s]


def _short(label, fn, key):
    return "%s workspace too small for B = 2: {%s-1} bytes given, %s() = {%s}" % (label, key, fn, key)


DYN_SHORT = _short("dynamics", "nbl_dynamics_workspace_bytes", "dyn")
FDYN_SHORT = _short("forward-dynamics", "nbl_forward_dynamics_workspace_bytes", "fdyn")
W1_SHORT = _short("wrench", "nbl_wrench_workspace_bytes", "wrench1")
W2_SHORT = _short("wrench", "nbl_wrench_workspace_bytes", "wrench2")
ID_FLAGS = "unknown flag bits 8 (NBL_ID_*)"
W_FLAGS = "unknown flag bits 16 (NBL_ID_*, NBL_WRENCH_WORLD)"
NOT_SPATIAL = "entry 1 of the wrench set is not NBL_KIN_SPATIAL: a wrench needs a whole frame"
SENS_NOT_SPATIAL = "entry 1 of the sensor set is not NBL_KIN_SPATIAL: a sensor needs a whole frame"

# (name, call, its bent arguments, return code, nbl_last_error(); {key} / {key-1}: the workspace size of that family / one byte less)
CASES = []


def case(name, fn, kw, rc, text=None):
    CASES.append(pytest.param(fn, kw, rc, text, id=name))


# -- a null model: every call that takes one
for _name, _fn in (("kinematics_forward", kin_fwd), ("kinematics_backward", kin_bwd), ("inverse_dynamics_forward", id_fwd),
                   ("inverse_dynamics_backward", id_bwd), ("mass_matrix", mass), ("inverse_dynamics_backward_inertia", id_inertia),
                   ("forward_dynamics_forward", fd_fwd), ("forward_dynamics_backward", fd_bwd), ("inv_mass_apply", minv_apply),
                   ("inv_mass_matrix", minv), ("inverse_dynamics_wrench_forward", idw_fwd), ("inverse_dynamics_wrench_backward", idw_bwd),
                   ("forward_dynamics_wrench_forward", fdw_fwd), ("forward_dynamics_wrench_backward", fdw_bwd),
                   ("forward_dynamics_backward_inertia", fd_inertia), ("contact_inverse_dynamics", cid), ("ik_solve", ik), ("ik_solve_vjp", ik_vjp),
                   ("centroidal_forward", cen_fwd), ("centroidal_backward", cen_bwd), ("sensors_forward", sens_fwd), ("sensors_backward", sens_bwd),
                   ("task_jacobian", tj), ("task_jacobian_deriv", tjd), ("task_jacobian_vjp", tj_vjp), ("task_accel", t_acc),
                   ("task_accel_vjp", t_acc_vjp)):
    case(_name + ": null model", _fn, {"h": "null"}, BADARG, "null model")

# -- kinematics (B = 0 is refused here, not a no-op)
for _name, _fn in (("kinematics_forward", kin_fwd), ("kinematics_backward", kin_bwd)):
    case(_name + ": null map", _fn, {"k": "none"}, BADARG, "null kinematics map")
    case(_name + ": null map and null model", _fn, {"k": "none", "h": "null"}, BADARG, "null kinematics map")
    case(_name + ": map of another instantiation", _fn, {"h": "h1"}, BADARG, OTHER_MAP)
    case(_name + ": B < 0", _fn, {"B": -1}, BADARG, "B must be positive")
    case(_name + ": B = 0", _fn, {"B": 0}, BADARG, "B must be positive")
case("kinematics_forward: no outputs", kin_fwd, {"outputs": False}, 0)

# -- inverse dynamics, mass matrix, their inertia gradient
for _name, _fn in (("inverse_dynamics_forward", id_fwd), ("inverse_dynamics_backward", id_bwd), ("inverse_dynamics_backward_inertia", id_inertia)):
    case(_name + ": B < 0", _fn, {"B": -1}, BADARG, NEG_B)
    case(_name + ": B < 0 and flags", _fn, {"B": -1, "flags": 8}, BADARG, NEG_B)
    case(_name + ": flags", _fn, {"flags": 8}, BADARG, ID_FLAGS)
    case(_name + ": flags 24", _fn, {"flags": 24 + 3}, BADARG, "unknown flag bits 24 (NBL_ID_*)")
    case(_name + ": flags at B = 0", _fn, {"B": 0, "flags": 8}, BADARG, ID_FLAGS)
    case(_name + ": workspace", _fn, {"short": 1}, WORKSPACE, DYN_SHORT)
    case(_name + ": workspace and flags", _fn, {"short": 1, "flags": 8}, WORKSPACE, DYN_SHORT)
    case(_name + ": B = 0", _fn, {"B": 0}, 0)
case("inverse_dynamics_backward: no outputs", id_bwd, {"outputs": False}, 0)
case("inverse_dynamics_backward: no outputs, flags", id_bwd, {"outputs": False, "flags": 8}, BADARG, ID_FLAGS)
case("inverse_dynamics_backward_inertia: none registered", id_inertia, {}, 0)
case("mass_matrix: B < 0", mass, {"B": -1}, BADARG, NEG_B)
case("mass_matrix: workspace", mass, {"short": 1}, WORKSPACE, DYN_SHORT)
case("mass_matrix: B = 0", mass, {"B": 0}, 0)

# -- forward dynamics, inverse mass matrix
for _name, _fn in (("forward_dynamics_forward", fd_fwd), ("forward_dynamics_backward", fd_bwd)):
    case(_name + ": B < 0", _fn, {"B": -1}, BADARG, NEG_B)
    case(_name + ": flags", _fn, {"flags": 8}, BADARG, ID_FLAGS)
    case(_name + ": flags at B = 0", _fn, {"B": 0, "flags": 8}, BADARG, ID_FLAGS)
    case(_name + ": workspace", _fn, {"short": 1}, WORKSPACE, FDYN_SHORT)
    case(_name + ": the inverse-dynamics workspace", _fn, {"short": "fdyn-dyn"}, WORKSPACE,
         "forward-dynamics workspace too small for B = 2: {dyn} bytes given, nbl_forward_dynamics_workspace_bytes() = {fdyn}")
    case(_name + ": workspace and flags", _fn, {"short": 1, "flags": 8}, WORKSPACE, FDYN_SHORT)
    case(_name + ": B = 0", _fn, {"B": 0}, 0)
case("forward_dynamics_backward: no outputs", fd_bwd, {"outputs": False}, 0)
case("inv_mass_apply: B < 0", minv_apply, {"B": -1}, BADARG, NEG_B)
case("inv_mass_apply: workspace", minv_apply, {"short": 1}, WORKSPACE, FDYN_SHORT)
case("inv_mass_apply: workspace and R", minv_apply, {"short": 1, "R": 0}, WORKSPACE, FDYN_SHORT)
case("inv_mass_apply: R = 0", minv_apply, {"R": 0}, BADARG, "R must be at least 1 (got 0)")
case("inv_mass_apply: R < 0 at B = 0", minv_apply, {"R": -3, "B": 0}, BADARG, "R must be at least 1 (got -3)")
case("inv_mass_apply: X null, R != n", minv_apply, {"R": N - 1, "X": False}, BADARG, "X may be null (the identity) only with R = n")
case("inv_mass_apply: X null, R != n at B = 0", minv_apply, {"R": N - 1, "X": False, "B": 0}, 0)
case("inv_mass_apply: B = 0", minv_apply, {"B": 0}, 0)
case("inv_mass_matrix: B < 0", minv, {"B": -1}, BADARG, NEG_B)
case("inv_mass_matrix: workspace", minv, {"short": 1}, WORKSPACE, FDYN_SHORT)
case("inv_mass_matrix: B = 0", minv, {"B": 0}, 0)

# -- wrenches in the dynamics calls
for _name, _fn in (("inverse_dynamics_wrench_forward", idw_fwd), ("inverse_dynamics_wrench_backward", idw_bwd),
                   ("forward_dynamics_wrench_forward", fdw_fwd), ("forward_dynamics_wrench_backward", fdw_bwd),
                   ("forward_dynamics_backward_inertia", fd_inertia)):
    case(_name + ": set of another instantiation", _fn, {"k": "one1"}, BADARG, OTHER_MAP)
    case(_name + ": set of another instantiation and null model", _fn, {"k": "one1", "h": "null"}, BADARG, "null model")
    case(_name + ": non-spatial entry", _fn, {"k": "mixed"}, BADARG, NOT_SPATIAL)
    case(_name + ": non-spatial entry and flags", _fn, {"k": "mixed", "flags": 16}, BADARG, NOT_SPATIAL)
    case(_name + ": flags", _fn, {"flags": 16}, BADARG, W_FLAGS)
    case(_name + ": flags and B < 0", _fn, {"flags": 16, "B": -1}, BADARG, W_FLAGS)
    case(_name + ": flags at B = 0", _fn, {"flags": 16, "B": 0}, BADARG, W_FLAGS)
    case(_name + ": B < 0", _fn, {"B": -1}, BADARG, NEG_B)
    case(_name + ": workspace", _fn, {"short": 1}, WORKSPACE, W1_SHORT)
    case(_name + ": B = 0", _fn, {"B": 0}, 0)
    case(_name + ": B = 0, world frame", _fn, {"B": 0, "flags": 8}, 0)
case("inverse_dynamics_wrench_backward: no outputs", idw_bwd, {"outputs": False}, 0)
case("forward_dynamics_wrench_backward: no outputs", fdw_bwd, {"outputs": False}, 0)
case("forward_dynamics_backward_inertia: none registered", fd_inertia, {}, 0)
case("forward_dynamics_backward_inertia, no set: none registered", fd_inertia, {"k": "none"}, 0)
case("forward_dynamics_backward_inertia, no set: B < 0", fd_inertia, {"k": "none", "B": -1}, BADARG, NEG_B)
case("forward_dynamics_backward_inertia, no set: flags", fd_inertia, {"k": "none", "flags": 8}, BADARG, ID_FLAGS)
case("forward_dynamics_backward_inertia, no set: workspace", fd_inertia, {"k": "none", "short": 1}, WORKSPACE, FDYN_SHORT)
case("forward_dynamics_backward_inertia, no set: workspace and flags", fd_inertia, {"k": "none", "short": 1, "flags": 8}, WORKSPACE, FDYN_SHORT)
case("forward_dynamics_backward_inertia, no set: B = 0", fd_inertia, {"k": "none", "B": 0}, 0)

# -- contact inverse dynamics
case("contact_inverse_dynamics: null map", cid, {"k": "none"}, BADARG, "null kinematics map: contact inverse dynamics needs at least one contact body")
case("contact_inverse_dynamics: map of another instantiation", cid, {"k": "one1"}, BADARG, OTHER_MAP)
case("contact_inverse_dynamics: mode", cid, {"mode": 3}, BADARG, "mode must be NBL_CID_SINGLE, NBL_CID_NEAREST or NBL_CID_MIN_TORQUE (got 3)")
case("contact_inverse_dynamics: mode and non-spatial entry", cid, {"mode": -1, "k": "mixed"}, BADARG,
     "mode must be NBL_CID_SINGLE, NBL_CID_NEAREST or NBL_CID_MIN_TORQUE (got -1)")
case("contact_inverse_dynamics: non-spatial entry", cid, {"k": "mixed"}, BADARG, NOT_SPATIAL)
case("contact_inverse_dynamics: world frame", cid, {"flags": 8}, BADARG, "unknown flag bits 8 (NBL_ID_*, NBL_WRENCH_WORLD)")
case("contact_inverse_dynamics: B < 0", cid, {"B": -1}, BADARG, NEG_B)
case("contact_inverse_dynamics: workspace", cid, {"short": 1}, WORKSPACE, W2_SHORT)
case("contact_inverse_dynamics: workspace and SINGLE with two", cid, {"short": 1, "mode": 0}, WORKSPACE, W2_SHORT)
case("contact_inverse_dynamics: SINGLE with two", cid, {"mode": 0}, BADARG, "NBL_CID_SINGLE takes one contact body (the set has 2)")
case("contact_inverse_dynamics: SINGLE with two at B = 0", cid, {"mode": 0, "B": 0}, BADARG, "NBL_CID_SINGLE takes one contact body (the set has 2)")
case("contact_inverse_dynamics: B = 0", cid, {"B": 0}, 0)
case("contact_inverse_dynamics: B = 0, SINGLE with one", cid, {"B": 0, "mode": 0, "k": "one"}, 0)

# -- inverse kinematics and its reverse pass
for _name, _fn in (("ik_solve", ik), ("ik_solve_vjp", ik_vjp)):
    case(_name + ": null map", _fn, {"k": "none"}, BADARG, "null kinematics map")
    case(_name + ": map of another instantiation", _fn, {"k": "mixed1"}, BADARG, OTHER_MAP)
    case(_name + ": B < 0", _fn, {"B": -1}, BADARG, NEG_B)
    case(_name + ": B = 0", _fn, {"B": 0}, 0)
case("ik_solve: null map and null model", ik, {"k": "none", "h": "null"}, BADARG, "null kinematics map")
case("ik_solve_vjp: null map and null model", ik_vjp, {"k": "none", "h": "null"}, BADARG, "null model")
case("ik_solve: max_step_count 0", ik, {"steps": 0}, BADARG, "max_step_count must be at least 1 (got 0)")
case("ik_solve: B < 0 and max_step_count 0", ik, {"steps": 0, "B": -1}, BADARG, NEG_B)
case("ik_solve: max_step_count 0 at B = 0", ik, {"steps": 0, "B": 0}, BADARG, "max_step_count must be at least 1 (got 0)")
case("ik_solve: max_step_count above the cap", ik, {"steps": 100001}, BADARG,
     "max_step_count above 100000 (got 100001): a lane runs its world's whole solve in one launch")
case("ik_solve: max_step_count at the cap, workspace", ik, {"steps": 100000, "short": 1}, WORKSPACE,
     _short("IK", "nbl_ik_workspace_bytes", "ik"))
case("ik_solve: negative damping", ik, {"damping": -0.5}, BADARG, "least_squares_damping and convergence_threshold must not be negative")
case("ik_solve: NaN damping", ik, {"damping": float("nan")}, BADARG, "least_squares_damping and convergence_threshold must not be negative")
case("ik_solve: damping 0", ik, {"damping": 0.0}, UNSUPPORTED,
     "least_squares_damping = 0 (the reference's complete orthogonal decomposition) is outside the device path")
case("ik_solve: damping 0 at B = 0", ik, {"damping": 0.0, "B": 0}, UNSUPPORTED,
     "least_squares_damping = 0 (the reference's complete orthogonal decomposition) is outside the device path")
case("ik_solve: workspace", ik, {"short": 1}, WORKSPACE, _short("IK", "nbl_ik_workspace_bytes", "ik"))
case("ik_solve: workspace and damping 0", ik, {"short": 1, "damping": 0.0}, UNSUPPORTED,
     "least_squares_damping = 0 (the reference's complete orthogonal decomposition) is outside the device path")
case("ik_solve_vjp: negative grad_damping", ik_vjp, {"mu": -1e-9}, BADARG, "grad_damping must not be negative")
case("ik_solve_vjp: B < 0 and negative grad_damping", ik_vjp, {"mu": -1e-9, "B": -1}, BADARG, NEG_B)
case("ik_solve_vjp: grad_damping 0", ik_vjp, {"mu": 0.0}, UNSUPPORTED,
     "grad_damping = 0 (a pseudo-inverse of a possibly singular Jacobian) is outside the device path")
case("ik_solve_vjp: grad_damping 0 at B = 0", ik_vjp, {"mu": 0.0, "B": 0}, UNSUPPORTED,
     "grad_damping = 0 (a pseudo-inverse of a possibly singular Jacobian) is outside the device path")
case("ik_solve_vjp: workspace", ik_vjp, {"short": 1}, WORKSPACE, _short("IK gradient", "nbl_ik_grad_workspace_bytes", "ikg"))
case("ik_solve_vjp: workspace and grad_damping 0", ik_vjp, {"short": 1, "mu": 0.0}, UNSUPPORTED,
     "grad_damping = 0 (a pseudo-inverse of a possibly singular Jacobian) is outside the device path")

# -- centroidal quantities
for _name, _fn, _acc in (("centroidal_forward", cen_fwd, "com_acc"), ("centroidal_backward", cen_bwd, "g_com_acc")):
    case(_name + ": null set", _fn, {"s": "none"}, BADARG, "null body set")
    case(_name + ": null set and null model", _fn, {"s": "none", "h": "null"}, BADARG, "null body set")
    case(_name + ": set of another instantiation", _fn, {"s": "set1"}, BADARG, OTHER_SET)
    case(_name + ": B < 0", _fn, {"B": -1}, BADARG, NEG_B)
    case(_name + ": B < 0 and flags", _fn, {"B": -1, "flags": 4}, BADARG, NEG_B)
    case(_name + ": flags", _fn, {"flags": 4}, BADARG, "unknown flag bits 4 (NBL_CEN_*)")
    case(_name + ": flags at B = 0", _fn, {"flags": 12 + 3, "B": 0}, BADARG, "unknown flag bits 12 (NBL_CEN_*)")
    case(_name + ": workspace", _fn, {"short": 1}, WORKSPACE, _short("centroidal", "nbl_centroidal_workspace_bytes", "cen"))
    case(_name + ": workspace and no accel", _fn, {"short": 1, "accel": False}, WORKSPACE,
         _short("centroidal", "nbl_centroidal_workspace_bytes", "cen"))
    case(_name + ": no accel", _fn, {"accel": False}, BADARG, _acc + " needs the accelerations (accel is null)")
    case(_name + ": no accel at B = 0", _fn, {"accel": False, "B": 0}, BADARG, _acc + " needs the accelerations (accel is null)")
    case(_name + ": no accel, no outputs", _fn, {"accel": False, "outputs": False}, BADARG, _acc + " needs the accelerations (accel is null)")
    case(_name + ": B = 0", _fn, {"B": 0}, 0)
case("centroidal_forward: no outputs", cen_fwd, {"outputs": False, "com_acc": False}, 0)
case("centroidal_forward: no accel, no com_acc", cen_fwd, {"accel": False, "com_acc": False, "B": 0}, 0)
case("centroidal_backward: no outputs", cen_bwd, {"outputs": False}, 0)

# -- sensors
for _name, _fn, _pre in (("sensors_forward", sens_fwd, ""), ("sensors_backward", sens_bwd, "g_")):
    case(_name + ": null set", _fn, {"k": "none"}, BADARG, "null sensor set")
    case(_name + ": set of another instantiation", _fn, {"k": "one1"}, BADARG, OTHER_MAP)
    case(_name + ": non-spatial entry", _fn, {"k": "mixed"}, BADARG, SENS_NOT_SPATIAL)
    case(_name + ": non-spatial entry and B < 0", _fn, {"k": "mixed", "B": -1}, BADARG, SENS_NOT_SPATIAL)
    case(_name + ": B < 0", _fn, {"B": -1}, BADARG, NEG_B)
    case(_name + ": workspace", _fn, {"short": 1}, WORKSPACE, _short("sensor", "nbl_sensors_workspace_bytes", "sens"))
    case(_name + ": workspace and no accel", _fn, {"short": 1, "accel": False}, WORKSPACE, _short("sensor", "nbl_sensors_workspace_bytes", "sens"))
    case(_name + ": no accel", _fn, {"accel": False}, BADARG, _pre + "acc needs the accelerations (accel is null)")
    case(_name + ": no accel, no field", _fn, {"accel": False, "field": False}, BADARG, _pre + "acc needs the accelerations (accel is null)")
    case(_name + ": no field", _fn, {"field": False}, BADARG, _pre + "mag needs the magnetic field (field is null)")
    case(_name + ": no field at B = 0", _fn, {"field": False, "B": 0}, BADARG, _pre + "mag needs the magnetic field (field is null)")
    case(_name + ": B = 0", _fn, {"B": 0}, 0)
case("sensors_forward: gyro alone, no accel, no field", sens_fwd, {"accel": False, "field": False, "outputs": ("gyro",), "B": 0}, 0)
case("sensors_forward: no outputs", sens_fwd, {"outputs": ()}, 0)
case("sensors_backward: g_gyro alone, no accel, no field", sens_bwd, {"accel": False, "field": False, "cots": ("gyro",), "B": 0}, 0)
case("sensors_backward: no outputs", sens_bwd, {"outputs": False}, 0)

# -- task-space Jacobians and accelerations
for _name, _fn in (("task_jacobian", tj), ("task_jacobian_deriv", tjd), ("task_jacobian_vjp", tj_vjp), ("task_accel", t_acc),
                   ("task_accel_vjp", t_acc_vjp)):
    case(_name + ": null map", _fn, {"k": "none"}, BADARG, "null kinematics map")
    case(_name + ": null map and null model", _fn, {"k": "none", "h": "null"}, BADARG, "null model")
    case(_name + ": map of another instantiation", _fn, {"k": "mixed1"}, BADARG, OTHER_MAP)
    case(_name + ": map of another instantiation and rows", _fn, {"k": "mixed1", "rows": 8}, BADARG, OTHER_MAP)
    case(_name + ": rows", _fn, {"rows": 8}, BADARG, "rows = 8, the kinematics map has 9")
    case(_name + ": rows and n", _fn, {"rows": 10, "n": 15}, BADARG, "rows = 10, the kinematics map has 9")
    case(_name + ": n", _fn, {"n": 15}, BADARG, "n = 15, the model has 16 DOFs")
    case(_name + ": n and B < 0", _fn, {"n": 17, "B": -1}, BADARG, "n = 17, the model has 16 DOFs")
    case(_name + ": n at B = 0", _fn, {"n": 0, "B": 0}, BADARG, "n = 0, the model has 16 DOFs")
    case(_name + ": B < 0", _fn, {"B": -1}, BADARG, NEG_B)
    case(_name + ": B = 0", _fn, {"B": 0}, 0)
case("task_accel: no accel", t_acc, {"accel": False}, BADARG, "xdd needs the accelerations (accel is null)")
case("task_accel: no accel at B = 0", t_acc, {"accel": False, "B": 0}, BADARG, "xdd needs the accelerations (accel is null)")
case("task_accel: no outputs", t_acc, {"outputs": False}, 0)
case("task_accel: no outputs, no accel", t_acc, {"outputs": False, "accel": False}, 0)
case("task_accel_vjp: no accel", t_acc_vjp, {"accel": False}, BADARG, "grad_accel needs the accelerations (accel is null)")
case("task_accel_vjp: no accel at B = 0", t_acc_vjp, {"accel": False, "B": 0}, BADARG, "grad_accel needs the accelerations (accel is null)")
case("task_accel_vjp: no accel and workspace", t_acc_vjp, {"accel": False, "short": 1}, BADARG, "grad_accel needs the accelerations (accel is null)")
case("task_accel_vjp: no outputs", t_acc_vjp, {"outputs": False}, 0)
case("task_accel_vjp: no outputs, workspace", t_acc_vjp, {"outputs": False, "short": 1}, 0)
case("task_accel_vjp: workspace", t_acc_vjp, {"short": 1}, WORKSPACE, _short("task-space", "nbl_task_workspace_bytes", "task"))


@pytest.mark.parametrize("fn, kw, rc, text", CASES)
def test_the_return_code_and_the_text_of_a_refusal(rig, fn, kw, rc, text):
    kw = dict(kw)
    if kw.get("short") == "fdyn-dyn":
        kw["short"] = rig.need["fdyn"] - rig.need["dyn"]
    assert fn(rig, **kw) == rc
    if rc != 0:
        sizes = {k: v for k, v in rig.need.items()}
        sizes.update({k + "-1": v - 1 for k, v in rig.need.items()})
        want = text
        for k, v in sizes.items():
            want = want.replace("{%s}" % k, str(v))
        assert rig.L.nbl_last_error().decode() == want


def test_workspace_sizes_of_a_null_handle_a_foreign_map_and_an_empty_batch_are_zero(rig):
    L, h, h1 = rig.L, rig.h, rig.h1
    for fn in (L.nbl_dynamics_workspace_bytes, L.nbl_forward_dynamics_workspace_bytes, L.nbl_centroidal_workspace_bytes,
               L.nbl_sensors_workspace_bytes, L.nbl_task_workspace_bytes):
        assert fn(None, B) == 0 and fn(h, 0) == 0 and fn(h, -1) == 0 and fn(h1, B) == fn(h, B) > 0
    for fn in (L.nbl_wrench_workspace_bytes, L.nbl_ik_workspace_bytes, L.nbl_ik_grad_workspace_bytes):
        assert fn(None, rig.one, B) == 0 and fn(h, rig.one1, B) == 0 and fn(h, rig.one, 0) == 0 and fn(h, rig.one, -1) == 0
        assert fn(h1, rig.one1, B) == fn(h, rig.one, B) > 0
    assert L.nbl_ik_workspace_bytes(h, None, B) == 0 and L.nbl_ik_grad_workspace_bytes(h, None, B) == 0
    assert L.nbl_wrench_workspace_bytes(h, None, B) > L.nbl_forward_dynamics_workspace_bytes(h, B)       # (a set with no entries)
    assert L.nbl_ik_grad_workspace_bytes(h, rig.mixed, B) == L.nbl_ik_workspace_bytes(h, rig.mixed, B)
    assert L.nbl_task_workspace_bytes(h, B) == L.nbl_sensors_workspace_bytes(h, B) == L.nbl_centroidal_workspace_bytes(h, B)


def test_maps_and_body_sets_refuse_at_registration(rig):
    L, h, h1 = rig.L, rig.h, rig.h1
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    km, bs = C.c_void_p(), C.c_void_p()

    def refused(rc, code, text):
        assert rc == code and L.nbl_last_error().decode() == text
    refused(L.nbl_kin_map_create(None, 1, i32(0), i32(0), None, C.byref(km)), BADARG, "null argument")
    refused(L.nbl_kin_map_create(h, 0, i32(0), i32(0), None, C.byref(km)), BADARG, "a kinematics map needs at least one entry")
    refused(L.nbl_kin_map_create(h, 65, i32(*[0] * 65), i32(*[0] * 65), None, C.byref(km)), BADARG,
            "a kinematics map holds at most 64 entries (384 rows); got 65")
    refused(L.nbl_kin_map_create(h, 2, i32(0, 3), i32(0, 0), None, C.byref(km)), BADARG,
            "entry 1: kind must be NBL_KIN_SPATIAL, NBL_KIN_LINEAR or NBL_KIN_ANGULAR")
    refused(L.nbl_kin_map_create(h, 1, i32(0), i32(-2), None, C.byref(km)), BADARG, "entry 0: body -2 out of range [-1, 5)")
    assert km.value is None and L.nbl_kin_map_dim(None) == 0
    refused(L.nbl_body_set_create(None, 0, None, C.byref(bs)), BADARG, "null argument")
    refused(L.nbl_body_set_create(h, -1, None, C.byref(bs)), BADARG, "a body set needs `count` body indices (or none: every body)")
    refused(L.nbl_body_set_create(h, 1, i32(5), C.byref(bs)), BADARG, "entry 0: body 5 out of range [0, 5)")
    refused(L.nbl_body_set_create(h, 2, i32(1, 1), C.byref(bs)), BADARG, "body 1 is named twice (entries 0 and 1)")
    assert bs.value is None
    mom = (C.c_double * 3)(0.0, 0.0, 0.0)
    refused(L.nbl_body_set_origin_moments(h, None, 0, None, None), BADARG, "null body set")
    refused(L.nbl_body_set_origin_moments(h1, rig.set, 1, i32(0), mom), BADARG, OTHER_SET)
    refused(L.nbl_body_set_origin_moments(None, rig.set, 1, i32(0), mom), BADARG, "null model")
    refused(L.nbl_body_set_origin_moments(h, rig.set, -1, i32(0), mom), BADARG, "null argument")
    refused(L.nbl_body_set_origin_moments(h, rig.set, 1, i32(5), mom), BADARG, "entry 0: body out of range")
    assert L.nbl_body_set_mass(h, rig.set) > 0
    assert L.nbl_body_set_mass(h1, rig.set) == 0.0 and L.nbl_last_error().decode() == OTHER_SET
    assert L.nbl_body_set_mass(h, None) == 0.0 and L.nbl_last_error().decode() == "null argument"


def test_no_case_above_launched_a_kernel(rig):
    """(last in the file) every output buffer handed to a call above is as it was allocated"""
    torch.cuda.synchronize()
    for t in rig.outs:
        assert (torch.isnan(t).all() if t.dtype == torch.float64 else (t == -1).all())
