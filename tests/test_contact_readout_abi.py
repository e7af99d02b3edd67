"""The contact read-out entry points (nbl_contact_readout, nbl_contact_readout_rows, nbl_contact_body_wrenches) on a box without a GPU:
the header's NBL_CO_* constants against their Python mirror and the documented field list, the symbols in every build of the library
(csrc/abi_variants.h, like tests/test_ik_abi.py), the kernels' own offsets, and the argument errors the dispatch layer answers without a
device."""
import ctypes as C
import os
import re

import pytest

from nimblephysics_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nimblephysics_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "nimble_amd.h")).read()
NEW = ("nbl_contact_readout", "nbl_contact_readout_rows", "nbl_contact_body_wrenches")


def _defines(text, prefix):
    return {k: int(v) for k, v in re.findall(r"^#define (%s[A-Z_]+) (-?\d+)\s*$" % prefix, text, re.M)}


def test_header_constants_equal_the_python_mirror():
    d = _defines(HEADER, "NBL_CO_")
    mirror = {k: getattr(_abi, k[4:]) for k in d}
    assert d == mirror and len(d) == 15


def test_field_count_matches_the_documented_field_list():
    """point(3) normal(3) depth type collider A/B body A/B impulse(3) class(3) force(3), contiguous and in that order"""
    d = _defines(HEADER, "NBL_CO_")
    want = [("POINT", 3), ("NORMAL", 3), ("DEPTH", 1), ("TYPE", 1), ("COLLIDER_A", 1), ("COLLIDER_B", 1), ("BODY_A", 1), ("BODY_B", 1),
            ("IMPULSE", 3), ("CLASS", 3), ("FORCE", 3)]
    off = 0
    for (name, width), (pyname, pywidth) in zip(want, _abi.CO_FIELD_LIST):
        assert d["NBL_CO_" + name] == off and pywidth == width, name
        assert pyname == {"CLASS": "row_class"}.get(name, name.lower())
        off += width
    assert off == d["NBL_CO_FIELDS"] == _abi.CO_FIELDS == 21 and len(_abi.CO_FIELD_LIST) == len(want)
    for name, _ in want:                         # ... and every field is documented next to the call
        assert "NBL_CO_" + name in HEADER.split("nbl_contact_readout:")[1].split("#define NBL_CO_POINT")[0]


def test_the_kernels_use_the_header_offsets():
    src = open(os.path.join(CSRC, "contact_readout.hip")).read()
    k = {m[0]: int(m[1]) for m in re.findall(r"\b(CO_[A-Z_]+) = (-?\d+)", src)}
    d = _defines(HEADER, "NBL_CO_")
    for name in ("POINT", "NORMAL", "DEPTH", "TYPE", "COLLIDER_A", "COLLIDER_B", "BODY_A", "BODY_B", "IMPULSE", "CLASS", "FORCE", "FIELDS",
                 "MAP_NONE", "MAX_BODIES"):
        assert k["CO_" + name] == d["NBL_CO_" + name], name
    assert "static_assert(CO_POINT == NBL_CO_POINT" in open(os.path.join(CSRC, "nimble_amd.hip")).read()


def test_entry_points_exist_in_every_build():
    src = open(os.path.join(CSRC, "nimble_amd.hip")).read()
    src = src[src.index('extern "C" {'):]
    renamed = set(re.findall(r"#define (nbl_[a-z0-9_]+) NBL_V", open(os.path.join(CSRC, "abi_variants.h")).read()))
    disp = open(os.path.join(CSRC, "nimble_amd_dispatch.cpp")).read()
    for sym in NEW:
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"^int32_t %s\s*\(" % sym, src, re.M), sym
        assert sym in renamed
        assert re.search(r"^int32_t %s\s*\(" % sym, disp, re.M)
        assert re.search(r"\bX\(\s*S\s*,\s*int32_t\s*,\s*%s\s*," % sym[4:], disp), sym       # (in the one list of per-capacity entry points)
        assert re.search(r"^int32_t %s\(nbl_model\* m, int64_t B, const void\* saved," % sym, HEADER, re.M), sym
    import nimblephysics_amd as na
    for name in ("read_contacts", "body_contact_wrenches", "rollout_contacts", "rollout_body_contact_wrenches", "ContactReadout"):
        assert name in na.__all__


def test_argument_errors_without_a_device():
    """A null handle is refused by the dispatcher itself, before any instantiation or device is touched."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libnimble_amd.so not built (no hipcc in this environment)")
    L = C.CDLL(_lib.LIB_PATH)
    L.nbl_last_error.restype = C.c_char_p
    vp = C.c_void_p
    L.nbl_contact_readout.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.nbl_contact_readout_rows.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp]
    L.nbl_contact_body_wrenches.argtypes = [vp, C.c_int64, vp, C.c_int32, vp, vp, vp]
    for f in NEW:
        getattr(L, f).restype = C.c_int32
    buf = (C.c_int32 * 4)()
    assert L.nbl_contact_readout(None, 1, buf, buf, None, None, None, None) == _abi.NBL_E_BADARG
    assert b"null model" in L.nbl_last_error()
    assert L.nbl_contact_readout_rows(None, 1, buf, buf, None, None, None) == _abi.NBL_E_BADARG
    assert L.nbl_contact_body_wrenches(None, 1, buf, 1, buf, buf, None) == _abi.NBL_E_BADARG
    assert L.nbl_contact_body_wrenches(None, 0, None, 0, None, None, None) == _abi.NBL_E_BADARG      # even B = 0 needs a handle
