"""nimblephysics_amd — MI355X-native batched differentiable timestep.

Drop-in for ONE hot path of nimblephysics: `timestep(world, state, action)`
(python/nimblephysics/timestep.py:63-69).  See DESIGN.md / INTEGRATION.md.
"""
from .model import (BodySpec, BoxSpec, CapsuleSpec, ModelDescription, SphereSpec, atlas, box_stack, cartpole,  # noqa: F401
                    make_transform, single_pendulum)

__all__ = ["ModelDescription", "BodySpec", "BoxSpec", "SphereSpec", "CapsuleSpec", "World", "timestep", "TimestepLayer", "rollout", "RolloutLayer", "single_pendulum", "cartpole",
           "atlas", "box_stack", "make_transform", "load_urdf", "load_skel", "with_ground", "load_model", "loadWorld", "model_from_nimble_world", "WrtMassBodyNodeEntryType", "GraphedStep", "GraphedRollout", "neural", "forwardPass", "BackpropSnapshot",
           "LossGradient", "LossGradientHighLevelAPI", "NimbleAmdError", "IKMapping", "map_to_pos", "map_to_vel", "MapToPosLayer",
           "MapToVelLayer", "inverse_dynamics", "coriolis_and_gravity", "mass_matrix", "forward_dynamics",
           "multiply_by_inv_mass_matrix", "inv_mass_matrix", "solve_ik", "solve_ik_vjp", "SolveIKLayer", "IKConfig", "contact_inverse_dynamics",
           "inverse_dynamics_from_predictions", "read_contacts", "body_contact_wrenches", "rollout_contacts",
           "rollout_body_contact_wrenches", "ContactReadout", "center_of_mass", "com_velocity", "com_acceleration", "centroidal_momentum",
           "kinetic_energy", "potential_energy", "com_jacobian", "centroidal", "Centroidal", "gyro_readings", "accelerometer_readings",
           "magnetometer_readings", "imu_readings", "IMUReadings", "gyro_jacobian", "accelerometer_jacobian", "magnetometer_jacobian",
           "inverse_dynamics_mass_gradient", "forward_dynamics_mass_gradient", "inverse_dynamics_mass_jacobian", "forward_dynamics_mass_jacobian",
           "task_jacobian", "task_jacobian_dot_times_v", "map_to_acc", "task_jacobian_deriv"]


def __getattr__(name):
    if name == "NimbleAmdError":                             # what every refused model / failed call raises
        from ._lib import NimbleAmdError
        return NimbleAmdError
    if name in ("GraphedStep", "GraphedRollout"):
        from . import graph as _g
        return getattr(_g, name)
    if name == "WrtMassBodyNodeEntryType":
        from .mass import WrtMassBodyNodeEntryType
        return WrtMassBodyNodeEntryType
    if name == "model_from_nimble_world":
        from .extract import model_from_nimble_world
        return model_from_nimble_world
    if name in ("load_urdf", "load_skel", "with_ground", "load_model", "loadWorld", "load_model", "loadWorld"):
        from . import loaders as _l
        return getattr(_l, name)
    if name in ("neural", "forwardPass", "BackpropSnapshot", "LossGradient", "LossGradientHighLevelAPI"):
        import importlib
        mod = importlib.import_module(".neural", __name__)
        return mod if name == "neural" else getattr(mod, name)
    # torch-dependent pieces are imported lazily so that model building works without a GPU stack
    if name in ("World",):
        from .world import World
        return World
    if name in ("IKMapping", "map_to_pos", "map_to_vel", "MapToPosLayer", "MapToVelLayer", "solve_ik", "solve_ik_vjp", "SolveIKLayer", "IKConfig"):
        from . import mapping as _m
        return getattr(_m, name)
    if name in ("inverse_dynamics", "coriolis_and_gravity", "mass_matrix", "forward_dynamics", "multiply_by_inv_mass_matrix", "inv_mass_matrix",
                "contact_inverse_dynamics", "inverse_dynamics_from_predictions", "inverse_dynamics_mass_gradient", "forward_dynamics_mass_gradient",
                "inverse_dynamics_mass_jacobian", "forward_dynamics_mass_jacobian"):
        from . import dynamics as _d
        return getattr(_d, name)
    if name in ("read_contacts", "body_contact_wrenches", "rollout_contacts", "rollout_body_contact_wrenches", "ContactReadout"):
        from . import contacts as _c
        return getattr(_c, name)
    if name in ("center_of_mass", "com_velocity", "com_acceleration", "centroidal_momentum", "kinetic_energy", "potential_energy", "com_jacobian",
                "centroidal", "Centroidal"):
        import importlib                                    # (not `from . import`: "centroidal" is also the name asked for here)
        _cen = importlib.import_module(".centroidal", __name__)
        return _cen if name == "centroidal" else getattr(_cen, name)       # the module answers a call like its function centroidal()
    if name in ("gyro_readings", "accelerometer_readings", "magnetometer_readings", "imu_readings", "IMUReadings", "gyro_jacobian",
                "accelerometer_jacobian", "magnetometer_jacobian"):
        from . import sensors as _s
        return getattr(_s, name)
    if name in ("task_jacobian", "task_jacobian_dot_times_v", "map_to_acc", "task_jacobian_deriv"):
        from . import taskspace as _ts
        return getattr(_ts, name)
    if name in ("timestep", "TimestepLayer", "rollout", "RolloutLayer"):
        from . import timestep as _t
        return getattr(_t, name)
    raise AttributeError(name)
