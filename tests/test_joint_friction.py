"""Joint Coulomb friction on the host side: the loaders read it (the reference's own unit tests, test_SkelParser.cpp:415-444 and
test_DartLoader.cpp:171, on the reference's data files), the description carries it per DOF through compound-joint expansion, weld
merging, the flat arrays and JSON, and the live-World extraction reads Joint::getCoulombFriction."""
import os
import sys
import warnings

import numpy as np

import nimblephysics_amd as na
from nimblephysics_amd import loaders
from nimblephysics_amd.extract import model_from_nimble_world

DATA = os.path.join(os.path.dirname(__file__), "golden", "reference_data", "data")
sys.path.insert(0, os.path.dirname(__file__))


def _skel(name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return loaders.load_skel(os.path.join(DATA, "skel", "test", name))


def test_skel_dynamics_elements_friction_damping_spring_rest():
    """test_SkelParser.cpp:415-444 (DynamicsElements): joint0 f = 5, the translational joint1 f = 5 / 4 / 3 per axis; damping,
    spring stiffness and rest position read alongside."""
    md = _skel("joint_dynamics_elements_test.skel")
    fl = md.flat()
    assert fl["coulomb_friction"].tolist() == [5.0, 5.0, 4.0, 3.0]
    assert fl["damping"].tolist() == [1.0, 1.0, 2.0, 3.0]
    assert fl["spring"].tolist() == [3.0, 3.0, 2.0, 1.0]
    assert fl["rest"].tolist() == [0.1, 0.1, 0.2, 0.3]
    # the translational joint is expanded into its chain of 1-DOF joints: one value per link of the chain
    assert [tuple(b.coulomb_friction) for b in md.bodies] == [(5.0,), (5.0,), (4.0,), (3.0,)]
    assert md.num_friction_dofs() == 4


def test_skel_joint_friction_test_file_has_no_friction_of_its_own():
    """joint_friction_test.skel: the reference's test (test_Joints.cpp:617-720) sets the friction with setCoulombFriction."""
    md = _skel("joint_friction_test.skel")
    assert not md.flat()["coulomb_friction"].any() and md.num_friction_dofs() == 0


def test_urdf_dynamics_friction():
    """test_DartLoader.cpp:171: friction 2.3 (and damping 1.2) on both joints of joint_properties.urdf."""
    md = loaders.load_urdf(os.path.join(DATA, "urdf", "test", "joint_properties.urdf"))
    named = {b.joint_name: b for b in md.bodies if b.joint_type == "revolute"}
    assert set(named) == {"0_to_1", "1_to_2"}
    for b in named.values():
        assert tuple(b.coulomb_friction) == (2.3,) and tuple(b.damping) == (1.2,)
    # a model without colliders gets contact slots for its friction rows (one per friction DOF, at least 8)
    d, _keep = md.to_desc()
    assert d.max_contacts == 8 and bool(d.coulomb_friction)


def test_json_round_trip_keeps_friction_and_omits_zeros():
    md = _skel("joint_dynamics_elements_test.skel")
    js = md.to_json()
    back = na.ModelDescription.from_json(js)
    assert [tuple(b.coulomb_friction) for b in back.bodies] == [tuple(b.coulomb_friction) for b in md.bodies]
    assert np.array_equal(back.flat()["coulomb_friction"], md.flat()["coulomb_friction"])
    plain = na.cartpole()
    assert all("coulomb_friction" not in b for b in plain.to_json()["bodies"])
    plain.bodies[1].coulomb_friction = (0.0,)
    assert all("coulomb_friction" not in b for b in plain.to_json()["bodies"])


def test_compound_expansion_and_weld_merge_keep_per_dof_values():
    I = (0.01, 0.02, 0.03, 0, 0, 0)
    bodies = [na.BodySpec("a", -1, "revolute", "ja", mass=1.0, inertia=I, coulomb_friction=(0.7,)),
              na.BodySpec("w", 0, "weld", "jw", T_pj=na.make_transform((0.1, 0, 0)), mass=0.5, inertia=I),
              na.BodySpec("u", 1, "universal", "ju", axes=[(1, 0, 0), (0, 1, 0)], mass=0.4, inertia=I, coulomb_friction=(0.2, 0.3)),
              na.BodySpec("b", 2, "ball", "jb", mass=0.3, inertia=I, coulomb_friction=(1.0, 2.0, 3.0))]
    md = na.ModelDescription("fric_chain", bodies)
    assert [tuple(b.coulomb_friction) for b in md.bodies] == [(0.7,), (), (0.2,), (0.3,), (1.0, 2.0, 3.0)]
    merged = md.merge_welds()
    assert merged.flat()["coulomb_friction"].tolist() == [0.7, 0.2, 0.3, 1.0, 2.0, 3.0]
    assert merged.num_friction_dofs() == 6
    d, _keep = merged.to_desc()
    assert d.max_contacts == 8
    # without friction the description hands the library a NULL field (the behaviour before the field existed)
    d0, _keep0 = na.cartpole().to_desc()
    assert not bool(d0.coulomb_friction)


def test_slot_default_counts_friction_dofs():
    from util import limited_arm
    md = limited_arm(enforce=False)
    md.max_contacts = 0
    for b in md.bodies:
        b.coulomb_friction = (1.0,)
    assert md.suggest_max_contacts() == 8
    big = na.ModelDescription("many", [na.BodySpec(f"b{i}", i - 1, "revolute", f"j{i}", mass=1.0, coulomb_friction=(1.0,)) for i in range(20)])
    d, _keep = big.to_desc()
    assert d.max_contacts == 24 and big.suggest_max_contacts() == 24


def test_extraction_reads_coulomb_friction():
    from test_extract import StandInWorld, _Joint

    class _FricJoint(_Joint):
        def getCoulombFriction(self, k): return self._get("coulomb_friction", k, 0.0)

    import test_extract
    md = _skel("joint_dynamics_elements_test.skel")
    old = test_extract._Joint
    test_extract._Joint = _FricJoint
    try:
        got = model_from_nimble_world(StandInWorld(md), name=md.name, max_contacts=8)
    finally:
        test_extract._Joint = old
    assert got.flat()["coulomb_friction"].tolist() == [5.0, 5.0, 4.0, 3.0]
    # a joint class without the getter (the stand-in of tests/test_extract.py): no friction
    plain = model_from_nimble_world(StandInWorld(md), name=md.name, max_contacts=8)
    assert not plain.flat()["coulomb_friction"].any()
