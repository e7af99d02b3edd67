"""ctypes mirror of include/nimble_amd.h (struct nbl_model_desc and constants).

Pure declarations; nothing here touches a GPU or loads a library.
"""
import ctypes as C

JOINT_REVOLUTE = 0
JOINT_PRISMATIC = 1
JOINT_FREE = 2
JOINT_WELD = 3
JOINT_BALL = 4
JOINT_SCREW = 5
JOINT_NAMES = {"revolute": JOINT_REVOLUTE, "prismatic": JOINT_PRISMATIC, "free": JOINT_FREE, "weld": JOINT_WELD, "ball": JOINT_BALL,
               "screw": JOINT_SCREW}
JOINT_NDOF = {JOINT_REVOLUTE: 1, JOINT_PRISMATIC: 1, JOINT_FREE: 6, JOINT_WELD: 0, JOINT_BALL: 3, JOINT_SCREW: 1}

NBL_OK = 0
NBL_E_BADARG = -1
NBL_E_UNSUPPORTED = -2
NBL_E_HIP = -3
NBL_E_WORKSPACE = -4
NBL_E_NOGPU = -5

ID_NO_VELOCITY = 1   # NBL_ID_*: the flags of the inverse- and forward-dynamics calls
ID_NO_GRAVITY = 2
ID_JOINT_FORCES = 4
WRENCH_WORLD = 8      # NBL_WRENCH_WORLD: only the nbl_*_wrench_* calls take it
CID_SINGLE, CID_NEAREST, CID_MIN_TORQUE = 0, 1, 2   # NBL_CID_*

# NBL_CO_*: the rows of a contact slot in the table of nbl_contact_readout, in order, with their widths
CO_POINT, CO_NORMAL, CO_DEPTH, CO_TYPE, CO_COLLIDER_A, CO_COLLIDER_B, CO_BODY_A, CO_BODY_B = 0, 3, 6, 7, 8, 9, 10, 11
CO_IMPULSE, CO_CLASS, CO_FORCE, CO_FIELDS = 12, 15, 18, 21
CO_FIELD_LIST = (("point", 3), ("normal", 3), ("depth", 1), ("type", 1), ("collider_a", 1), ("collider_b", 1), ("body_a", 1), ("body_b", 1),
                 ("impulse", 3), ("row_class", 3), ("force", 3))
CO_CLASS_EMPTY = -1      # the tangent slots of a frictionless contact
CO_MAP_NONE = -4         # nbl_contact_readout_rows: mapping of a row past the world's live rows
CO_MAX_BODIES = 64
# nbl_centroidal_forward / _backward flags (NBL_CEN_*)
CEN_PE_BODY_ORIGIN, CEN_NO_SPRINGS = 1, 2

ST_CONTACT = 0x1
ST_LCP_STAGE0 = 0x2
ST_LCP_PIVOT = 0x4
ST_LCP_PGS = 0x8
ST_LCP_NOFRIC = 0x10
ST_LCP_FAILED = 0x20
ST_NAN = 0x40
ST_CONTACT_OVERFLOW = 0x80
ST_STANDARDIZED = 0x100

_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int32)


class ModelDesc(C.Structure):
    _fields_ = [
        ("n_bodies", C.c_int32),
        ("n_dofs", C.c_int32),
        ("parent", _pi),
        ("joint_type", _pi),
        ("dof_offset", _pi),
        ("T_pj", _pd),
        ("T_cj", _pd),
        ("axis", _pd),
        ("mass", _pd),
        ("com", _pd),
        ("inertia", _pd),
        ("damping", _pd),
        ("spring", _pd),
        ("rest", _pd),
        ("pos_lo", _pd),
        ("pos_hi", _pd),
        ("vel_lo", _pd),
        ("vel_hi", _pd),
        ("force_lo", _pd),
        ("force_hi", _pd),
        ("gravity", C.c_double * 3),
        ("dt", C.c_double),
        ("n_action", C.c_int32),
        ("action_map", _pi),
        ("n_boxes", C.c_int32),
        ("box_body", _pi),
        ("box_T", _pd),
        ("box_size", _pd),
        ("box_mu", _pd),
        ("max_contacts", C.c_int32),
        ("contact_clipping_depth", C.c_double),
        ("fallback_cfm", C.c_double),
        ("box_shape", _pi),
        ("box_restitution", _pd),
        ("penetration_correction", C.c_int32),
        ("body_skeleton", _pi),
        ("pitch", _pd),
        ("dof_limit_enforced", _pi),
        ("body_self_collision", _pi),
        ("box_node", _pi),
        ("box_node_parent", _pi),
        ("coulomb_friction", _pd),
    ]
