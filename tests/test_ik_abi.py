"""The inverse-kinematics entry points exist in EVERY build of the library: nimble_amd.hip alone is the whole library in its 8-contact
form (csrc/abi_variants.h; the developer builds of tools/ compile it that way and load it through NBL_LIB_PATH), so every function
include/nimble_amd.h declares - nbl_ik_default_config included - is defined there and renamed per instantiation, not in the dispatcher only."""
import os
import re

from nimblephysics_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nimblephysics_amd", "csrc")


def _extern_c(text):
    return text[text.index('extern "C" {'):]


def test_every_public_symbol_is_defined_in_the_single_unit_library():
    src = _extern_c(open(os.path.join(CSRC, "nimble_amd.hip")).read())
    renamed = set(re.findall(r"#define (nbl_[a-z0-9_]+) NBL_V", open(os.path.join(CSRC, "abi_variants.h")).read()))
    for sym in _lib.EXPORTED_SYMBOLS:
        assert re.search(r"^[a-z_0-9 *]*\b%s\s*\(" % sym, src, re.M), f"{sym} is not defined in nimble_amd.hip"
        assert sym in renamed, f"{sym} is not renamed per instantiation in abi_variants.h"
    for sym in ("nbl_ik_default_config", "nbl_ik_workspace_bytes", "nbl_ik_solve"):
        assert sym in _lib.EXPORTED_SYMBOLS
