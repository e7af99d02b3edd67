"""Every function include/nimble_amd.h declares - nbl_ik_default_config included - exists in EVERY build of the library, and in exactly one
place.  The calls that depend on the contact capacity are defined in nimble_amd.hip and renamed per instantiation (csrc/abi_variants.h); the
43 contact-independent ones (kinematics, dynamics, IK and its reverse pass, centroidal, sensors, task space) are defined once, in
nimble_amd_tree.hip, under their public names: never renamed, never in the dispatcher's list of per-capacity entry points (NBL_PER_CAPACITY,
from which the prototypes, the table's members and its rows are expanded).  nimble_amd.hip alone, which then includes nimble_amd_tree.hip, is the whole library in its
8-contact form (the developer builds of tools/ compile it that way and load it through NBL_LIB_PATH)."""
import os
import re

from nimblephysics_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nimblephysics_amd", "csrc")


def _extern_c(text):
    return text[text.index('extern "C" {'):]


def _defines(sym, src):
    return re.search(r"^[a-z_0-9 *]*\b%s\s*\(" % sym, src, re.M) is not None


def test_every_public_symbol_is_defined_in_the_single_unit_library():
    per_capacity = _extern_c(open(os.path.join(CSRC, "nimble_amd.hip")).read())
    once = _extern_c(open(os.path.join(CSRC, "nimble_amd_tree.hip")).read())
    renamed = set(re.findall(r"#define (nbl_[a-z0-9_]+) NBL_V", open(os.path.join(CSRC, "abi_variants.h")).read()))
    disp = open(os.path.join(CSRC, "nimble_amd_dispatch.cpp")).read()
    n_once = 0
    for sym in _lib.EXPORTED_SYMBOLS:
        in_hip, in_tree = _defines(sym, per_capacity), _defines(sym, once)
        assert in_hip != in_tree, f"{sym} must be defined in nimble_amd.hip or in nimble_amd_tree.hip, and in one of them only"
        if in_hip:
            assert sym in renamed, f"{sym} is not renamed per instantiation in abi_variants.h"
        else:
            n_once += 1
            assert sym not in renamed, f"{sym} is built once (nimble_amd_tree.hip) but renamed in abi_variants.h"
            assert not re.search(r"\bX\(\s*S\s*,[^,]*,\s*%s\s*," % sym[4:], disp) and sym + "_c" not in disp and not _defines(sym, disp), \
                f"{sym} is built once but still passes through the dispatcher"
    assert n_once == 43
    for f in os.listdir(CSRC):                 # the forwards the task-space calls and the reverse pass of IK once went through
        assert not re.search(r"\btree(Task|Ik)", open(os.path.join(CSRC, f)).read()), f
    # the stand-alone library (nimble_amd.hip without NBL_VARIANT_SUFFIX) takes the rest from the same file
    assert re.search(r'^#else\n(//[^\n]*\n)*#define NBL_TREE_STANDALONE\n#include "nimble_amd_tree.hip"\n#endif', per_capacity, re.M)
    for sym in ("nbl_ik_default_config", "nbl_ik_workspace_bytes", "nbl_ik_solve"):
        assert sym in _lib.EXPORTED_SYMBOLS
