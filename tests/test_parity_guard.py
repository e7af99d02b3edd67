"""tests/parity.py refuses a reference that the oracle computed without oracle/_ref (status bit 0x80000000): see DESIGN.md section 5."""
import numpy as np
import pytest

from parity import ORACLE_WITHOUT_REFERENCE_SOLVER, assert_match_or_reference_unstable, assert_reference_solver_present


def test_a_reference_without_the_reference_solver_is_refused():
    z = {"next": np.ones((3, 4)), "grad_state": np.ones((3, 4)), "grad_action": np.ones((3, 2))}
    ok = dict(z, status=np.array([0x105, 0x3, 0x111], np.uint32))
    assert_reference_solver_present("ok", ok)
    assert_reference_solver_present("no status", z)
    assert assert_match_or_reference_unstable("ok", None, None, None, None, z, ok, 1e-7, verbose=False) == (0, 0)
    flagged = dict(z, status=np.array([0x105, 0x80000111, 0x3], np.uint32))
    assert flagged["status"][1] & ORACLE_WITHOUT_REFERENCE_SOLVER
    with pytest.raises(AssertionError, match="libodelcp_ref"):
        assert_match_or_reference_unstable("flagged", None, None, None, None, z, flagged, 1e-7, verbose=False)
