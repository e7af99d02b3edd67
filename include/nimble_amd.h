/*
 * nimble_amd.h — C ABI of the MI355X-native batched differentiable timestep.
 *
 * This is the drop-in boundary for ONE hot path of nimblephysics: the call
 *   nimble.timestep(world, state, action)                      python/nimblephysics/timestep.py:63-69
 * which in the reference goes through pybind11 into
 *   neural::forwardPass(world)                                  dart/neural/NeuralUtils.cpp:26-66
 *     -> World::step(true)                                      dart/simulation/World.cpp:221-254
 *   BackpropSnapshot::backpropState(world, grad)                dart/neural/BackpropSnapshot.cpp:382-420
 *
 * Everything here is plain C: pointers, sizes, ints.  No torch types.
 * All batched arrays are DEVICE pointers to fp64 in structure-of-arrays layout
 *   x[d * B + b]      d = DOF (or row) index, b = world index   ("[dof][B]")
 * so that one wavefront (64 consecutive worlds) reads one coalesced 512-byte line
 * per DOF.  The caller owns every buffer; the library owns only the model handle
 * and a workspace sized at nbl_workspace_bytes().
 *
 * Threading: one handle may be used from one host thread / one stream at a time
 * (the reference's World is not thread-safe either, World.cpp:114-172).
 * Multi-GPU: one handle per device, the batch is sharded by the caller.
 *
 * Return value of every int function: 0 = ok, <0 = error (see NBL_E_*).  This
 * replaces the reference's "print to std::cerr and ignore the call"
 * (World.cpp:2027-2033, 2063-2070) with a status the caller must check.
 */
#ifndef NIMBLE_AMD_H
#define NIMBLE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- joint types (dart/dynamics/{Revolute,Prismatic,Free,Weld}Joint.cpp) ---- */
#define NBL_JOINT_REVOLUTE 0
#define NBL_JOINT_PRISMATIC 1
#define NBL_JOINT_FREE 2 /* DART_USE_IDENTITY_JACOBIAN build: S = Ad(T_cj), FreeJoint.cpp:1049-1056.  Anywhere in the tree (as a tree root: the
                            fast path; below other bodies: six coincident single-axis joints internally, like NBL_JOINT_BALL) */
#define NBL_JOINT_WELD 3 /* 0 DOF. The GPU library requires welds to be merged into the parent
                            (host model builder does this); the CPU oracle accepts them. */
#define NBL_JOINT_SCREW 5 /* 1 DOF, ScrewJoint.cpp:160-232: rotation about `axis` coupled with a translation of `pitch` per turn along it,
                             S = Ad(T_cj) [axis; axis pitch / 2 pi], T = T_pj expMap(S_local q) T_cj^-1 */
#define NBL_JOINT_BALL 4 /* 3 DOF, BallJoint.cpp (DART_USE_IDENTITY_JACOBIAN build): positions = exponential-map vector of the joint
                            rotation, velocities = angular velocity in the child joint frame, S = Ad(T_cj)[:, 0:3] (:441-452),
                            q' = log(exp(q) exp(v dt)) (:333-349).  Anywhere in the tree.  The library runs it as three coincident
                            single-axis joints (x, y, z at zero angle, the first carrying exp(q)) - identical velocity-level dynamics -
                            and takes position derivatives through H(q) = [expMapJac(q)^T; 0] (:282-289); body indices of the
                            description stay valid in every entry point. */

/* ---- error codes ---- */
#define NBL_OK 0
#define NBL_E_BADARG -1
#define NBL_E_UNSUPPORTED -2 /* model feature outside the hot-path scope */
#define NBL_E_HIP -3         /* a HIP runtime call failed (nbl_last_error() has text) */
#define NBL_E_WORKSPACE -4   /* workspace too small for this B */
#define NBL_E_NOGPU -5

/* ---- per-lane status bits written to status[b] by nbl_step_forward ----
 * A world with several constrained groups (body_skeleton below) runs the solver once per group: STAGE0 and STANDARDIZED are set
 * when they hold for EVERY group, the other bits when they hold for ANY group. */
#define NBL_ST_CONTACT 0x1u       /* >=1 contact constraint was active */
#define NBL_ST_LCP_STAGE0 0x2u    /* warm-start / guess classification was a valid LCP solution (BoxedLcpConstraintSolver.cpp:434-457) */
#define NBL_ST_LCP_PIVOT 0x4u     /* pivoting (Dantzig-equivalent) stage used */
#define NBL_ST_LCP_PGS 0x8u       /* CFM + PGS fallback used */
#define NBL_ST_LCP_NOFRIC 0x10u   /* friction dropped fallback used */
#define NBL_ST_LCP_FAILED 0x20u   /* every stage failed its validity check: like the reference, the last stage's (frictionless PGS) iterate is applied as is
                                     (BoxedLcpConstraintSolver.cpp:590-676); the impulses are zeroed only if that iterate is non-finite (:678-687, NBL_ST_NAN) */
#define NBL_ST_NAN 0x40u          /* non-finite value seen: in the LCP stages, or in the world's next state (NaN / Inf inputs); other worlds are unaffected */
#define NBL_ST_CONTACT_OVERFLOW 0x80u /* more contacts (+ active joint-limit rows) than max_contacts: extra ones dropped; or a contact kept after
                                        2 x nbl_model_max_contacts() distinct points from the narrow phases (kept or dropped by the depth filter):
                                        the duplicate filter's memory */
#define NBL_ST_STANDARDIZED 0x100u /* least-squares standardized x replaced solver x (CGGM.cpp:321-332) */
#define NBL_ST_JOINT_LIMIT 0x400u  /* >=1 joint-limit constraint row was active (dof_limit_enforced) */
#define NBL_ST_JOINT_FRICTION 0x800u /* >=1 joint Coulomb friction row was active (coulomb_friction) */
#define NBL_ST_GRAD_PARTIAL 0x200u /* reserved (never set: the EDGE_EDGE contact-geometry gradient terms, DCC.cpp:397-424,
                                      700-735, are evaluated by the device backward) */

/*
 * Model description.  One model is shared by all B worlds of a batch; worlds differ only in
 * (q, v, tau) and the LCP warm start.  Bodies are listed parents-before-children.
 * Every body has exactly one parent joint.  Transforms are 12 doubles: R row-major (9) then p (3).
 */
typedef struct nbl_model_desc {
  int32_t n_bodies;
  int32_t n_dofs;
  const int32_t* parent;     /* [n_bodies] parent body index, -1 = world */
  const int32_t* joint_type; /* [n_bodies] NBL_JOINT_* */
  const int32_t* dof_offset; /* [n_bodies] first DOF of the parent joint */
  const double* T_pj;        /* [n_bodies][12] parent body -> joint  (Joint::mT_ParentBodyToJoint) */
  const double* T_cj;        /* [n_bodies][12] child body  -> joint  (Joint::mT_ChildBodyToJoint) */
  const double* axis;        /* [n_bodies][3] unit axis for revolute/prismatic */
  const double* mass;        /* [n_bodies] */
  const double* com;         /* [n_bodies][3] local COM (Inertia::mCenterOfMass) */
  const double* inertia;     /* [n_bodies][6] Ixx Iyy Izz Ixy Ixz Iyz about the COM (Inertia.cpp:1368-1383) */
  const double* damping;     /* [n_dofs] GenericJoint mDampingCoefficients */
  const double* spring;      /* [n_dofs] mSpringStiffnesses */
  const double* rest;        /* [n_dofs] mRestPositions */
  const double* pos_lo;      /* [n_dofs] limits, used only by clipLossGradientsToBounds (BackpropSnapshot.cpp:425-479) */
  const double* pos_hi;
  const double* vel_lo;
  const double* vel_hi;
  const double* force_lo;
  const double* force_hi;
  double gravity[3]; /* World::mGravity, default (0,-9.81,0) in the configs */
  double dt;         /* World::mTimeStep, default 1e-3 (World.cpp:76) */

  /* action space: tau[action_map[i]] = action[i], unmapped tau = 0 (World.cpp:2061-2086) */
  int32_t n_action;
  const int32_t* action_map; /* [n_action] */

  /* ---- contact: box colliders (dBoxBox, DARTCollide.cpp:764-1450) and spheres (box_shape below) ---- */
  int32_t n_boxes;
  const int32_t* box_body;  /* [n_boxes] body index, -1 = fixed to the world (immobile skeleton) */
  const double* box_T;      /* [n_boxes][12] shape transform in the body frame */
  const double* box_size;   /* [n_boxes][3] full side lengths */
  const double* box_mu;     /* [n_boxes] friction coefficient of the owning body (default 1, BodyNodeAspect.hpp:47) */
  int32_t max_contacts;     /* per world, <= 128; rows m = 3 * max_contacts.  The reference keeps every contact of every pair
                               (ConstraintSolver.cpp:563-606); a world with more than its model's slots is truncated and flagged
                               NBL_ST_CONTACT_OVERFLOW.  The library holds three instantiations of its contact stage: models with max_contacts
                               <= 8, <= 16 colliders and <= 32 collider pairs run the 24-row one (the fast one), up to 16 contacts / 32
                               colliders / 64 pairs the 48-row one, everything up to 64 contacts (192 rows) / 64 colliders / 512 pairs the
                               GENERAL one, whose dense kernels loop over the rows (since round 6 at 2 M world-steps/s on eight-contact worlds, 29 % of the 24-row
                               build's rate; on worlds that fill 12 - 16 slots the 48-row one is 2 - 3.7 x faster), roomy enough that a model can always be given
                               the slots its colliders can fill (a tower of ten cubes: 40 contacts in one constrained group).  A model that
                               asks for 65 .. 128 slots gets the same general code with 384 rows (four times the scratch and record per world:
                               ten cubes each turned against the next touch in clipped octagons, 80 contacts) */

  /* ---- options mirrored from the reference defaults ---- */
  double contact_clipping_depth; /* 0.03  World.cpp:86 */
  double fallback_cfm;           /* 1e-4  World.cpp:85 */

  /* ---- collider shapes (appended; NULL = every collider is a box) ----
   * [n_boxes] NBL_SHAPE_BOX | NBL_SHAPE_SPHERE | NBL_SHAPE_CAPSULE.  A sphere's radius is box_size[3*i]; sphere-box, box-sphere and
   * sphere-sphere pairs follow collideSphereBox / collideBoxSphere / collideSphereSphere (DARTCollide.cpp:1482-1880).
   * A capsule (CapsuleShape: axis = z of the shape frame) has radius box_size[3*i] and cylinder height box_size[3*i+1];
   * capsule-capsule, sphere-capsule and capsule-sphere pairs follow collideCapsuleCapsule / collideSphereCapsule /
   * collideCapsuleSphere (DARTCollide.cpp:4183-4420).  A model in which a capsule can meet a BOX is refused: that pair runs
   * libccd's MPR in the reference (DARTCollide.cpp:4422-4645), a third-party iterative algorithm outside this path. */
  const int32_t* box_shape;

  /* ---- restitution (appended; NULL = 0 everywhere, the reference's default BodyNodeAspect.hpp:48) ----
   * [n_boxes] restitution coefficient of the owning body.  A contact bounces when e = e_A * e_B > 1e-3 and e times its approach
   * speed exceeds 0.1 m/s: b_normal += min(e * b_normal, 100) (ContactConstraint.cpp:95-110, 395-442); the backward pass carries
   * the bounce diagonals 1 + e and the reference's bounce approximation of the position Jacobians
   * (BackpropSnapshot.cpp:1131-1226). */
  const double* box_restitution;

  /* ---- penetration correction (appended; 0 = off, the reference's default: ConstraintSolver.cpp:69-71, "it breaks our gradients") ----
   * World::setPenetrationCorrectionEnabled(true): b_normal += min(max(depth - 0, 0) * 0.01 / dt, 1e-3), unless the contact bounces
   * harder than that (ContactConstraint.cpp:393-441 with DART_ERROR_ALLOWANCE / DART_ERP / DART_MAX_ERV, :45-47).  Like the
   * reference's analytical Jacobians the backward pass treats the correction velocity as a constant. */
  int32_t penetration_correction;

  /* ---- skeletons (appended; NULL = every tree of the model is its own skeleton) ----
   * [n_bodies] index of the dart::dynamics::Skeleton a body belongs to.  The reference solves one LCP per CONSTRAINED GROUP: the
   * skeletons connected by contacts between two reactive bodies (ConstraintSolver.cpp:724-780, ContactConstraint.cpp:879-907;
   * contacts with world-fixed colliders do not connect anything).  Each group runs the solver cascade on its own, so one
   * object that needs the fallback stages does not change the solution of the others. */
  const int32_t* body_skeleton;

  /* ---- screw joints (appended; NULL = 0.1 for every screw joint, ScrewJointAspect's default) ----
   * [n_bodies] ScrewJoint::mPitch: translation along the axis per full turn; read for NBL_JOINT_SCREW bodies only. */
  const double* pitch;

  /* ---- joint-limit constraint rows (appended; NULL = none, the reference's default: Joint::isPositionLimitEnforced is false,
   * JointAspect.hpp:165) ----
   * [n_dofs] non-zero: the DOF's joint enforces its position limits (Joint::setPositionLimitEnforced).  A DOF at or beyond pos_lo /
   * pos_hi then adds one row to the LCP of its skeleton's constrained group, after the contact rows (JointLimitConstraint.cpp:182-290,
   * ConstraintSolver.cpp:641-696): unit impulse on the DOF, b = -qdot (error allowance 0), bounds [0, inf) at the lower and
   * (-inf, 0] at the upper limit.  Every joint type except the free-joint root (refused when such a coordinate has a finite limit);
   * a limit row takes one of the max_contacts contact slots.  The backward pass follows the reference's: its
   * DifferentiableContactConstraint gives a non-contact constraint a zero constraint-force column (DCC.cpp:51-99), so the row drops out
   * of every Jacobian. */
  const int32_t* dof_limit_enforced;

  /* ---- self-collision (appended; NULL = off, the reference's default: Skeleton::mEnabledSelfCollisionCheck is false) ----
   * [n_bodies] bit 0: the body's skeleton checks self-collisions (Skeleton::enableSelfCollisionCheck), bit 1: also between adjacent
   * bodies (enableAdjacentBodyCheck).  Two colliders of one skeleton are tested when bit 0 is set on both bodies and, unless bit 1
   * is set, neither body is the other's parent (BodyNodeCollisionFilter::ignoresCollision, CollisionFilter.cpp:105-154).  A DOF
   * above both bodies of such a contact moves it rigidly (DofContactType::SELF_COLLISION, DCC.cpp:116-130) and gets no
   * constraint force from it (getControlForceMultiple 0). */
  const int32_t* body_self_collision;
  /* [n_boxes] (appended; NULL = the collider's body and that body's parent) the BodyNode a collider belongs to and that node's parent, in
   * any numbering: "adjacent" above means box_node_parent[i] == box_node[j] or the reverse.  A caller that merges welded bodies before
   * nbl_model_create passes the identities of the unmerged BodyNodes here (a body welded to its neighbour's child is not adjacent to it). */
  const int32_t* box_node;
  const int32_t* box_node_parent;

  /* ---- joint Coulomb friction rows (appended; NULL = 0 everywhere, the reference's default: GenericJoint::mFrictions) ----
   * [n_dofs] Joint::getCoulombFriction of the DOF, >= 0.  A DOF with f != 0 whose pre-constraint velocity (after integrateVelocities)
   * is not exactly 0 adds one row to the LCP of its skeleton's constrained group, after the contact and the joint-limit rows
   * (JointCoulombFrictionConstraint.cpp:110-176, ConstraintSolver.cpp:636-716): unit impulse on the DOF, b = -qdot, fixed bounds
   * [-f dt, f dt], findex -1, no CFM (BoxedLcpConstraintSolver.cpp:291-299 asks for the velocity change without it).  Every joint type
   * except the free-joint root (refused when such a coordinate has f != 0, as for limits).  A friction row takes one of the max_contacts
   * contact slots (a full one: 3 rows, two of them empty), so a model with friction on k DOFs needs max_contacts >= contacts + limits + k
   * to never drop one; such a model always runs the GENERAL instantiation of the contact stage (nbl_model_max_contacts() >= 64).  The
   * backward pass treats a friction row as a limit row: the reference gives a non-contact constraint a zero constraint-force column
   * (DCC.cpp:51-99), so the row drops out of every Jacobian.  Rows are recreated every step (no per-constraint warm start: mLifeTime = 0);
   * the solver-level warm start (lcp_cache_in / out) carries them like every other row.
   * One difference in the row set: the reference makes one constraint per JOINT that has a DOF with f != 0 (ConstraintSolver.cpp:653-661)
   * and then activates every moving DOF of that joint (JointCoulombFrictionConstraint.cpp:107-147), so a DOF with f = 0 of such a joint
   * gets a row with bounds [0, 0]; here only DOFs with f != 0 get rows.  The impulse of a [0, 0] row is exactly 0, so the step is the
   * same, but for a multi-DOF joint with mixed friction (a ball joint with f = (1, 0, 0)) the row count m, the warm-start layout and the
   * slots used are smaller than the reference's.  (Compound joints reach the library as chains of single-DOF joints.) */
  const double* coulomb_friction;
} nbl_model_desc;

#define NBL_SHAPE_BOX 0
#define NBL_SHAPE_SPHERE 1
#define NBL_SHAPE_CAPSULE 2

typedef struct nbl_model nbl_model; /* opaque */

/* Human-readable text for the last error on this thread. */
const char* nbl_last_error(void);

/* Library/ABI version (major<<16 | minor).  The minor number counts the revisions that APPENDED fields to the model description struct: a NULL
 * pointer / zero in an appended field always means "the behaviour before that field existed"; a caller that zero-initialises
 * the struct and is compiled against this header keeps working, a caller compiled against minor k needs a library of minor >= k:
 *   minor 1: the struct up to and including pitch;
 *   minor 2: + dof_limit_enforced, body_self_collision, box_node, box_node_parent; NBL_SHAPE_CAPSULE; NBL_ST_JOINT_LIMIT;
 *   minor 3: max_contacts up to 16 (32 colliders, 64 pairs); + nbl_model_max_contacts, nbl_selftest_pinv_rows; the Dantzig self-test takes n <= 48.
 *   minor 4: max_contacts up to 64 (64 colliders, 512 pairs: the general instantiation); the Dantzig self-test takes n <= 192;
 *            nbl_workspace_bytes of such a model includes 1.5 MB of scratch matrices per world; max_contacts 65 .. 128: a second general
 *            instantiation of 384 rows (5.9 MB of scratch per world), the Dantzig self-test then takes n <= 384.
 *   minor 5: + nbl_set_deferred_join, nbl_slice_stream, nbl_fork_slices, nbl_join_slices (one handle, slices that are not joined per call);
 *            + nbl_kin_map_create, nbl_kin_map_destroy, nbl_kin_map_dim, nbl_kinematics_forward, nbl_kinematics_backward (world-space
 *            kinematics of body frames, below: added without a new minor number - a caller that needs them looks the symbols up);
 *            + coulomb_friction, NBL_ST_JOINT_FRICTION (appended without a new minor number, like the kinematics entries: a library
 *            built before the field ignores it, so a caller that depends on it checks for NBL_ST_JOINT_FRICTION in the status).
 *            + nbl_dynamics_workspace_bytes, nbl_inverse_dynamics_forward, nbl_inverse_dynamics_backward, nbl_mass_matrix (joint-space
 *            dynamics quantities, below: appended without a new minor number, like the kinematics entries - the model description did
 *            not change; a caller that needs them looks the symbols up).
 *            + nbl_ik_config, nbl_ik_default_config, nbl_ik_workspace_bytes, nbl_ik_solve (batched inverse kinematics, below: appended
 *            without a new minor number, like the kinematics and dynamics entries).
 *            + nbl_contact_readout, nbl_contact_readout_rows, nbl_contact_body_wrenches and the NBL_CO_* constants (read-out of a step's
 *            contacts, impulses and body contact wrenches from its saved record, below: appended without a new minor number, like the
 *            entries above - neither the model description nor any existing call changed; a caller that needs them looks the symbols up).
 *            + nbl_body_set_create, nbl_body_set_destroy, nbl_body_set_mass, nbl_body_set_origin_moments, nbl_centroidal_workspace_bytes,
 *            nbl_centroidal_forward, nbl_centroidal_backward and the NBL_CEN_* flags (centre of mass, momentum and energy of a body set,
 *            below: appended without a new minor number, like the entries above).
 *            + nbl_sensors_workspace_bytes, nbl_sensors_forward, nbl_sensors_backward (gyroscope, accelerometer and magnetometer readings
 *            of a sensor set, below: appended without a new minor number, like the entries above).
 *            + nbl_inverse_dynamics_backward_inertia, nbl_forward_dynamics_backward_inertia (gradients of the dynamics calls to the
 *            registered inertia parameters, below: appended without a new minor number, like the entries above).
 *            + nbl_ik_grad_workspace_bytes, nbl_ik_solve_vjp (the reverse pass of the inverse kinematics, below: appended without a new
 *            minor number, like the entries above - a caller that needs them looks the symbols up). */
#define NBL_ABI_MINOR 5
int32_t nbl_version(void);

/* Number of visible HIP devices (0 if none). */
int32_t nbl_device_count(void);

/*
 * Create a model on `device`.  Copies everything out of desc.
 * Replaces: constructing a nimble.simulation.World + skeletons (World.cpp:93-172).
 */
int32_t nbl_model_create(const nbl_model_desc* desc, int32_t device, nbl_model** out);
void nbl_model_destroy(nbl_model* m);

int32_t nbl_model_num_dofs(const nbl_model* m);
int32_t nbl_model_num_action(const nbl_model* m);
int32_t nbl_model_lcp_rows(const nbl_model* m); /* rows of the LCP warm-start buffer: 3 * nbl_model_max_contacts() impulses + 1 row holding the row count they belong to; 0 without colliders */
int32_t nbl_model_max_contacts(const nbl_model* m); /* contact slots per world of the instantiation the model runs on: 8, 16, 64 or 128 (>= desc.max_contacts); 0 without colliders */

/* Bytes of scratch the library needs for a batch of B worlds (forward or backward). */
size_t nbl_workspace_bytes(const nbl_model* m, int64_t B);

/*
 * Bytes of the per-step "saved for backward" record for B worlds: what the reference keeps in a
 * BackpropSnapshot (dart/neural/BackpropSnapshot.cpp:33-118): q_t, v_t, tau_t, the pre-step LCP
 * cache and the constraint-group results.  Caller-owned device memory.
 */
size_t nbl_saved_bytes(const nbl_model* m, int64_t B);

/*
 * One differentiable timestep for B worlds.
 *   state   [2n][B]  = [q; v]                              World::setState   World.cpp:2024-2036
 *   action  [k][B]                                          World::setAction  World.cpp:2061-2086
 *   lcp_cache_in  [m][B] or NULL (cold: guessSolution)      BoxedLcpConstraintSolver.cpp:202-208
 *   next_state [2n][B]                                      World::getState   World.cpp:2040-2047
 *   lcp_cache_out [m][B] or NULL
 *   saved      nbl_saved_bytes() bytes or NULL (no backward wanted)
 *   status     [B] uint32 or NULL
 * `stream` is a hipStream_t (void* so this header needs no HIP include); NULL = default stream.
 * Replaces: neural::forwardPass (NeuralUtils.cpp:26-66).
 */
int32_t nbl_step_forward(nbl_model* m, int64_t B, const double* state, const double* action,
                         const double* lcp_cache_in, double* next_state, double* lcp_cache_out,
                         void* saved, uint32_t* status, void* workspace, size_t workspace_bytes,
                         void* stream);

/*
 * Vector-Jacobian product of the step.
 *   grad_next_state [2n][B]  dL/d[q';v']
 *   grad_state      [2n][B]  dL/d[q;v]        (lossWrtState)
 *   grad_action     [k][B]   dL/daction       (lossWrtAction)
 * Replaces: BackpropSnapshot::backpropState (BackpropSnapshot.cpp:382-420), including
 * clipLossGradientsToBounds (:425-479).
 */
int32_t nbl_step_backward(nbl_model* m, int64_t B, const void* saved, const double* grad_next_state,
                          double* grad_state, double* grad_action, void* workspace,
                          size_t workspace_bytes, void* stream);

/*
 * Inertia ("mass") parameters: World::tuneMass / setMasses / lossWrtMass
 * (dart/simulation/World.cpp:1027-1035, 1821-1824; dart/neural/WithRespectToMass.cpp:50-140;
 *  dart/neural/BackpropSnapshot.cpp:153, 167-179, 580-640).
 *
 * nbl_set_body_inertia   replaces the inertial constants of one body (host pointers; com[3]; inertia[6] = Ixx Iyy Izz Ixy
 *                        Ixz Iyz about the COM, as in nbl_model_desc).  Synchronises the device: call it between steps.
 * nbl_set_inertia_params registers `count` scalar parameters theta_p: parameter p moves the spatial inertia of body
 *                        bodies[p] along dG[p] (6x6 row-major, symmetrised) - e.g. G/m for WrtMassBodyNodeEntryType::
 *                        INERTIA_MASS, whose setter scales the whole tensor (Inertia.cpp:157-179).  count = 0 clears them.
 * nbl_backward_inertia   grad_params [count][B]: dL/dtheta_p of every world for the step recorded in `saved`.  Call it
 *                        right after nbl_step_backward of the same record on the same stream and workspace (it uses the
 *                        adjoint joint rates that call leaves in the workspace).  accumulate != 0 adds to grad_params.
 *                        The reference finite-differences M^-1 and C for these parameters (Skeleton.cpp:1826-1829,
 *                        2078-2081); this is the closed form (csrc/inertia_backward.hip).
 */
int32_t nbl_set_body_inertia(nbl_model* m, int32_t body, double mass, const double* com, const double* inertia);
/* The same for `count` bodies at once (host pointers: bodies[count], mass[count], com[count][3], inertia[count][6]) as ONE
 * stream-ordered copy on `stream`: launches issued on that stream afterwards see the new constants; no device synchronisation
 * and the calling thread's current device is left as it was.  A backward pass reads the model's CURRENT constants: run the
 * backward of a step before changing the masses for the next one. */
int32_t nbl_set_body_inertias(nbl_model* m, int32_t count, const int32_t* bodies, const double* mass, const double* com,
                              const double* inertia, void* stream);
int32_t nbl_set_inertia_params(nbl_model* m, int32_t count, const int32_t* bodies, const double* dG);
/* The same, stream-ordered: a table of the size already registered (World::setMasses with new values) is ONE asynchronous copy on
 * `stream` - launches issued on that stream before the call read the old table, later ones the new one, no device synchronisation;
 * a table of another size is registration-time work and synchronises the device.  (nbl_set_inertia_params synchronises the device
 * around the copy in every case.) */
int32_t nbl_set_inertia_params_on(nbl_model* m, int32_t count, const int32_t* bodies, const double* dG, void* stream);
int32_t nbl_num_inertia_params(const nbl_model* m);
int32_t nbl_backward_inertia(nbl_model* m, int64_t B, const void* saved, double* grad_params, int32_t accumulate,
                             void* workspace, size_t workspace_bytes, void* stream);

/*
 * T-step trajectory rollout on the device: the loop of SingleShot::getStates /
 * SingleShot::backpropGradientWrt (dart/trajectory/SingleShot.cpp:539-598, 598-700) over forwardPass / backprop, without
 * a host round trip per step.
 *   forward:   states[0] = state0;  states[t+1] = step(states[t], actions[t])                       t = 0 .. T-1
 *     state0   [2n][B]
 *     actions  [T][k][B], or one [k][B] block used for every step when action_stride == 0 (else action_stride = k*B)
 *     states   [T+1][2n][B] out
 *     saved    T * nbl_saved_bytes(m, B) bytes (record t at byte offset t * nbl_saved_bytes), or NULL (no backward wanted)
 *     status   [T][B] uint32 or NULL
 *     warm_start != 0: step t starts the LCP from step t-1's solution (the reference's solver carries mX between steps,
 *                BoxedLcpConstraintSolver.cpp:176-187); 0: LCPUtils::guessSolution every step
 *   backward:  g_T = grad_states[T];  (g_t', grad_actions[t]) = step_backward(saved[t], g_{t+1});  g_t = g_t' + grad_states[t]
 *     grad_states  [T+1][2n][B]  dL/dstates[t] as it enters the loss directly (zeros where the loss does not look)
 *     grad_state0  [2n][B] out,  grad_actions [T][k][B] out
 * workspace: nbl_rollout_workspace_bytes(m, B) bytes.
 * Stream semantics: the slices of a rollout fork from `stream` and join into it before the call returns, on every handle.  Deferred
 * join (nbl_set_deferred_join) does not apply to the rollout entries, these and the checkpointed ones below: on such a handle they
 * also make `stream` wait for the slices of earlier nbl_step_forward / nbl_step_backward calls before they fork.
 */
size_t nbl_rollout_workspace_bytes(const nbl_model* m, int64_t B);
int32_t nbl_rollout_forward(nbl_model* m, int64_t B, int32_t T, const double* state0, const double* actions,
                            int64_t action_stride, double* states, void* saved, uint32_t* status, int32_t warm_start,
                            void* workspace, size_t workspace_bytes, void* stream);
int32_t nbl_rollout_backward(nbl_model* m, int64_t B, int32_t T, const void* saved, const double* grad_states,
                             double* grad_state0, double* grad_actions, void* workspace, size_t workspace_bytes,
                             void* stream);
/* The same with the inertia ("mass") parameters of nbl_set_inertia_params: grad_params [count][B] receives the sum over the T
 * steps of dL/dtheta_p (the masses are constant along the trajectory); NULL = nbl_rollout_backward. */
int32_t nbl_rollout_backward_inertia(nbl_model* m, int64_t B, int32_t T, const void* saved, const double* grad_states,
                                     double* grad_state0, double* grad_actions, double* grad_params, void* workspace,
                                     size_t workspace_bytes, void* stream);

/*
 * Checkpointed rollout: the saved records of `segment` steps are resident instead of T (a record is 26.7 kB per world-step on the
 * metric model - nbl_saved_bytes / B -, the states 16 n bytes).  The forward pass writes record t into slot t % segment of `saved`
 * (segment * nbl_saved_bytes(m, B) bytes) and keeps the LCP warm start entering every segment in `checkpoints`
 * (nbl_rollout_checkpoint_bytes(m, B, T, segment) bytes; may be NULL when warm_start == 0 or the model has no colliders).  The
 * backward pass walks the segments from the last to the first: it runs the steps of a segment again from states[k * segment] -
 * the forward kernels are bit-reproducible, so the records are the ones the forward call produced and the gradients are bit for
 * bit those of the unsegmented rollout - and then backpropagates through them.  The last segment is still resident and is not
 * recomputed; cost: one extra forward pass over the other T - segment steps.  (The role of the reference's re-simulation from
 * a stored state, RestorableSnapshot + forwardPass, for trajectories that do not fit.)
 *   segment == 0 (or >= T): exactly nbl_rollout_forward / nbl_rollout_backward_inertia.
 *   backward: `states`, `actions`, `action_stride`, `warm_start` as passed to / returned by the forward call (states[t0+1 .. t1] of
 *   a recomputed segment are rewritten with identical values); grad_params may be NULL.
 */
size_t nbl_rollout_checkpoint_bytes(const nbl_model* m, int64_t B, int32_t T, int32_t segment);
int32_t nbl_rollout_forward_checkpointed(nbl_model* m, int64_t B, int32_t T, int32_t segment, const double* state0, const double* actions,
                                         int64_t action_stride, double* states, void* saved, void* checkpoints, uint32_t* status,
                                         int32_t warm_start, void* workspace, size_t workspace_bytes, void* stream);
int32_t nbl_rollout_backward_checkpointed(nbl_model* m, int64_t B, int32_t T, int32_t segment, double* states, const double* actions,
                                          int64_t action_stride, void* saved, const void* checkpoints, int32_t warm_start,
                                          const double* grad_states, double* grad_state0, double* grad_actions, double* grad_params,
                                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- self-test ----
 * Runs the library's device restatement of the reference's Dantzig driver (dSolveLCP, dart/external/odelcpsolver/lcp.cpp:780-1113,
 * nub = 0, earlyTermination = true; the stage-1 code of the LCP cascade) on `count` caller-supplied n-row problems, one wavefront
 * per problem.  HOST pointers: A [count][n*n] row-major (only the lower triangles are read), b / lo / hi / findex [count][n] with
 * the bounds as DantzigBoxedLcpSolver::solve hands them over (friction rows: lo = -mu, hi = mu, findex = their normal row);
 * outputs x [count][n] and rc [count] (1 solved, 0 early termination, -1 NaN step).  n <= 48 (n <= 24 runs the 24-row instantiation's
 * code, larger n the 48-row one's).  Synchronous; for tests: on identical
 * inputs x and rc are bit-identical to the reference solver's. */
int32_t nbl_selftest_lcp_dantzig(int32_t count, int32_t n, const double* A, const double* b, const double* lo, const double* hi,
                                 const int32_t* findex, double* x, int32_t* rc);
/* The same, launched `reps` times back to back between two HIP events (after one untimed launch): *ms_per_launch = average duration of
 * one launch over the `count` problems (NULL: not timed).  The micro-benchmark of the stage-1 solver (tools/dantzig_bench.py). */
int32_t nbl_selftest_lcp_dantzig_timed(int32_t count, int32_t n, const double* A, const double* b, const double* lo, const double* hi,
                                       const int32_t* findex, double* x, int32_t* rc, int32_t reps, double* ms_per_launch);
/* The solver cascade of the GENERAL instantiation (csrc/gen_lcp_dev.hpp, gen_dantzig_dev.hpp: what a model with max_contacts > 16 runs) on
 * caller-supplied contact LCPs (HOST pointers): `count` problems of m = 3 * contacts rows each (m <= 192): A [count][m][m], b [count][m],
 * mu [count][m / 3], x_cache [count][m] (the warm start; have_cache = 0: LCPUtils::guessSolution instead), on [count][m] bytes (NULL: every
 * row; else the rows of the constrained group at hand).  Per problem: stage 0 and, if that fails, stages 1-3 in the reference's order, then
 * the classification / standardisation: x [count][m], row classes cls [count][m] (0 / 1 / 2), status bits st [count] (NBL_ST_* of the LCP:
 * 0x2 stage 0, 0x4 Dantzig, 0x8 CFM + PGS, 0x10 friction dropped, 0x20 PGS not converged, 0x40 NaN, 0x100 standardised), cfm [count].
 * Exactly the device code of k_contact_solve_gen; tests/test_gpu_general.py compares it with the same code compiled for the host. */
int32_t nbl_selftest_lcp_cascade(int32_t count, int32_t m, const double* A, const double* b, const double* mu, int32_t have_cache,
                                 const double* x_cache, const uint8_t* on, double fallback_cfm, double* x, int32_t* cls, uint32_t* st, double* cfm);
/* The same with the two kinds of joint pseudo-contact a step of the general instantiation carries next to its contacts, per SLOT of three rows
 * (HOST pointers, each [count][m / 3]; NULL: none - then this is nbl_selftest_lcp_cascade): lim 1 = a joint-limit row ([0, inf), no tangent
 * rows), 2 = one the step carries negated (the caller hands in the negated row: A_dev = S A S, b_dev = S b, x = S x_dev with S = -1 there);
 * bound > 0 = a joint Coulomb friction row with the FIXED bounds [-bound, bound] and findex -1 on the slot's first row (b = -qdot of the
 * DOF), its tangent rows empty; mu of such slots is ignored.  When any bound is > 0 the kernel is the instantiation of models with joint
 * friction (the JF = true text of genValid, genClassify, genLoadProblem and the stages), otherwise the one nbl_selftest_lcp_cascade runs.
 * Outputs as there.  For tests (tests/test_gpu_lcp_box_rows.py: against the same code on the host and the reference's isLCPSolutionValid);
 * added within minor 5. */
int32_t nbl_selftest_lcp_cascade_rows(int32_t count, int32_t m, const double* A, const double* b, const double* mu, const double* bound,
                                      const uint8_t* lim, int32_t have_cache, const double* x_cache, const uint8_t* on, double fallback_cfm,
                                      double* x, int32_t* cls, uint32_t* st, double* cfm);

/* Runs the library's device pseudo-inverses on `count` caller-supplied 24 x 24 matrices (HOST pointers: Q [count][24*24] row-major,
 * rows / columns outside the block of interest zero; cTrue [count] = size of that block, Eigen's `size` in the rank threshold), one
 * wavefront per matrix: route 0 = column-pivoted Householder QR + complete orthogonal decomposition (any matrix; what
 * CGGM.cpp:280 / LCPUtils.cpp:113 get from Eigen), route 1 = two Cholesky factorisations (symmetric positive semi-definite input:
 * A restricted to the guess rows, Q without upper-bound rows).  Outputs P [count][24*24] and rank [count]; launched `reps` times
 * between two HIP events, *ms_per_launch (may be NULL) = average launch duration.  For tests and tools/pinv_bench.py. */
int32_t nbl_selftest_pinv(int32_t count, const double* Q, const int32_t* cTrue, int32_t route, double* P, int32_t* rank, int32_t reps,
                          double* ms_per_launch);
/* The same on rows x rows matrices, rows = 24 or 48: the pseudo-inverses of the 24-row and of the 48-row instantiation of the contact stage. */
int32_t nbl_selftest_pinv_rows(int32_t count, int32_t rows, const double* Q, const int32_t* cTrue, int32_t route, double* P, int32_t* rank,
                               int32_t reps, double* ms_per_launch);
/* Stage 0 of the LCP cascade and its standardisation loop (coopStage0 / coopStandardizeLoop: classify, build Q, pseudo-inverse, apply,
 * isLCPSolutionValid) on `count` caller-supplied contact LCPs (HOST pointers), one wavefront per problem, rows = 24 or 48: A [count][rows*rows]
 * row-major, b and x_cache [count][rows], mu [count][rows / 3]; per problem the 64-bit words mask (the rows of the constrained group at
 * hand; the problem's size is the whole contacts up to its last bit), lim_mask (joint-limit rows) and neg_mask (the ones carried negated);
 * cfm [count]: 0 = stage 0 (have_cache [count]: start from x_cache instead of the guess), otherwise the standardisation loop alone on
 * x_cache with that constant on the diagonal, as after stages 2 / 3.  Outputs x, x0 (the pre-solve x), cls (0 / 1 / 2), e_out (the +-mu of
 * an upper-bound row) [count][rows], ok [count] (bit 0: standardised valid solution, bit 1: pinv is Q^+ of the final classification) and
 * pinv [count][rows*rows] (zero without bit 1).  For tests (tests/test_gpu_stage0_selftest.py); added within minor 5. */
int32_t nbl_selftest_stage0_rows(int32_t count, int32_t rows, const double* A, const double* b, const double* mu, const uint64_t* mask,
                                 const uint64_t* lim_mask, const uint64_t* neg_mask, const double* cfm, const int32_t* have_cache,
                                 const double* x_cache, double* x, double* x0, int32_t* cls, double* e_out, int32_t* ok, double* pinv);

/*
 * Layout helpers: the Python surface takes world-major tensors [B][d] like a stack of the
 * reference's 1-D state vectors; these transpose to/from the library's [d][B] layout on device.
 */
int32_t nbl_transpose_to_soa(const double* src_bd, double* dst_db, int64_t B, int32_t d, void* stream);
int32_t nbl_transpose_from_soa(const double* src_db, double* dst_bd, int64_t B, int32_t d, void* stream);

/* Average duration (ms) of the last timed launches, measured with HIP events on the launch stream. */
/* Launch shape of the one-world-per-lane tree kernels (models over 64 bodies / DOFs, NBL_COOP_TREE=0, the narrow phase):
 * worlds per workgroup, a power of two <= 64; 0 = default (16 below 65536 worlds, else 64).  Results do not depend on it;
 * environment NBL_TREE_LANES sets the initial value.  lcp_lanes is accepted for source compatibility and ignored: the
 * dense contact kernels are one world per wavefront. */
int32_t nbl_set_launch_lanes(nbl_model* m, int32_t tree_lanes, int32_t lcp_lanes);
/* Batch slicing: the worlds of a call are processed as `slices` contiguous ranges whose kernels overlap on internal HIP
 * streams forked from / joined into the caller's stream (0 = default: 2 from 4096 worlds on for a model with colliders, else 1;
 * max 8; environment NBL_SLICES).  Results do not depend on it; every call joins before it returns, so a caller who owns the whole
 * forward + backward loop gets more from one model handle per slice on its own stream.  nbl_slices_for: the number a
 * call with B worlds will use. */
int32_t nbl_set_slices(nbl_model* m, int32_t slices);
int32_t nbl_slices_for(const nbl_model* m, int64_t B);
/* Deferred join (ABI minor 5): with it enabled nbl_step_forward / nbl_step_backward return with their slices in flight: slice 0 on the
 * `stream` of the call (always hand in the same one), the others on internal streams of the handle, none waiting for another and
 * nothing recorded or awaited on `stream` per call (four busy streams is what the hardware runs side by side: the caller's is one
 * of them).  The forward pass of one slice overlaps the
 * backward pass of another across consecutive calls on ONE handle (what a caller otherwise gets from one handle per slice on its
 * own stream; the reference has no counterpart: its World::step is synchronous on one CPU thread).  Ordering against the caller's
 * streams is explicit: nbl_fork_slices(m, stream) makes every slice stream wait for what `stream` holds (after uploading inputs
 * there), nbl_join_slices(m, stream) makes `stream` wait for everything the slices hold (before consuming results there).  A result
 * can also be consumed on its slice's own stream: nbl_slice_stream gives the stream (a hipStream_t; NULL for slice 0: the calls' own) and the world range
 * [first_world, end_world) of slice `slice` of a call with B worlds - enqueue the per-slice loss there.  The buffers of a call must
 * stay valid until its slices have run.  nbl_slices_for(m, B) is the slice count (4 from 4096 worlds on).  Results are bit for bit
 * those of the joined calls.
 * THE MODE COVERS nbl_step_forward AND nbl_step_backward ONLY.  Every other entry behaves on such a handle as on a joined one.  The
 * rollout entries (nbl_rollout_forward / _backward / _backward_inertia and the _checkpointed pair) first make `stream` wait for the
 * slices still in flight from earlier step calls (what nbl_join_slices does), then fork their slices from `stream` and join them into
 * it before they return: inputs produced on `stream` are seen by every slice, results are safe to read on `stream`, and neither
 * nbl_fork_slices nor nbl_join_slices is needed around them.  The entries that run on `stream` alone (nbl_backward_inertia, the
 * kinematics, dynamics, sensor and read-out calls) do not look at the slice streams: after deferred step calls, nbl_join_slices first. */
int32_t nbl_set_deferred_join(nbl_model* m, int32_t enabled);
int32_t nbl_slice_stream(nbl_model* m, int64_t B, int32_t slice, void** stream, int64_t* first_world, int64_t* end_world);
int32_t nbl_fork_slices(nbl_model* m, void* stream);
int32_t nbl_join_slices(nbl_model* m, void* stream);
/*
 * World-space kinematics of body frames: the reference's IKMapping (dart/neural/IKMapping.{hpp,cpp}) and the vector-Jacobian products
 * of nimble.map_to_pos / nimble.map_to_vel (python/nimblephysics/mapping.py:8-101), for B worlds at once.
 *
 * A map is a list of ENTRIES made against a model; several maps may coexist on one handle.  An entry is a frame F fixed in one body of
 * the description the model was created from (`body`: its index there - the description has no welds: a welded body is its merged
 * body plus a constant offset; -1 = the world: a constant entry), F = W_body T_offset.  The library resolves its internal bodies (the
 * entry sits on the body that carries T_cj: the z body of a ball triple, the last body of a free chain).  Its rows, concatenated in
 * the order of the entries (IKMapping::getPositionsInPlace / getVelocitiesInPlace, IKMapping.cpp:146-232):
 *   NBL_KIN_SPATIAL  6 rows  position: logMap(R_F), then p_F     velocity: [w; v] = getSpatialVelocity(World, World) (Frame.cpp:163-178)
 *   NBL_KIN_LINEAR   3 rows  position: p_F                        velocity: v, the velocity of F's origin in world coordinates
 *   NBL_KIN_ANGULAR  3 rows  position: logMap(R_F)                velocity: w, the angular velocity in world coordinates
 * (IKMapping's COM entries have no public constructor in the reference and are not offered.)  At most 64 entries (P <= 384 rows):
 * more is NBL_E_BADARG.  T_offset: [count][12], R row-major then p; NULL = identity for every entry.  Registration uploads the entries
 * once (synchronous); destroy a map before the model it was made for.
 */
#define NBL_KIN_SPATIAL 0 /* 6 rows: logMap(R) then p */
#define NBL_KIN_LINEAR 1  /* 3 rows: p */
#define NBL_KIN_ANGULAR 2 /* 3 rows: logMap(R) */
typedef struct nbl_kin_map nbl_kin_map; /* opaque */
int32_t nbl_kin_map_create(nbl_model* m, int32_t count, const int32_t* kind, const int32_t* body, const double* T_offset,
                           nbl_kin_map** out);
void nbl_kin_map_destroy(nbl_kin_map* k);
int32_t nbl_kin_map_dim(const nbl_kin_map* k); /* P: the rows of the mapped vector (IKMapping::getPosDim = getVelDim) */
/* The mapped positions pos [P][B] and / or velocities vel [P][B] (either may be NULL) of the states state [2n][B] (DEVICE pointers, the
 * layout of nbl_step_forward; B may be (T + 1) x worlds: a whole rollout in one call).  Replaces IKMapping::getPositions /
 * getVelocities after World::setState.  Stream-ordered on `stream`, no device synchronisation, no workspace; it does not use the
 * handle's slices (deferred join does not apply).  Bit-reproducible, independent of B and of a world's place in the batch. */
int32_t nbl_kinematics_forward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, double* pos, double* vel, void* stream);
/* The vector-Jacobian products: grad_state [2n][B] = (accumulate: +=) [Jpos^T grad_pos; Jvel^T grad_vel].  Jpos =
 * IKMapping::getPosJacobian (IKMapping.cpp:371-416: Skeleton::getWorldPositionJacobian, Skeleton.cpp:11010-11060 - the joints' position
 * screws, the angular rows through dLogMap: the exact derivative of the rows above), Jvel = getVelJacobian (:429-473, getWorldJacobian).
 * A NULL grad_pos / grad_vel contributes nothing to its block.  As MapToPosLayer / MapToVelLayer (mapping.py:34-44, 81-92), the velocity
 * block carries Jvel^T grad_vel only: the dependence of J v on the positions is left out.  The angular rows follow logMap's regular
 * branch up to theta = pi - 1e-6 (dLogMap's special branch there, Geometry.cpp:764-, is not restated).  Stream-ordered like
 * nbl_kinematics_forward; no atomics: bit-reproducible. */
int32_t nbl_kinematics_backward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* grad_pos,
                                const double* grad_vel, double* grad_state, int32_t accumulate, void* stream);
/* ---- joint-space dynamics quantities (csrc/dynamics.hip) -------------------------------------------------------------------------------
 * Inverse dynamics  tau = M(q) a + C(q, v)  by the recursive Newton-Euler algorithm (Skeleton::getInverseDynamics, Skeleton.cpp:9658-9666),
 * the Coriolis-and-gravity vector C(q, v) (a = 0; World::getCoriolisAndGravityForces, World.cpp:1965-1986) and the mass matrix M(q)
 * (World::getMassMatrix, World.cpp:1943-1963; composite-rigid-body algorithm) of B worlds, one world per lane, with the exact
 * vector-Jacobian product of the first.  They read the handle's CURRENT body inertias (nbl_set_body_inertia(s), nbl_set_inertia_params).
 * state [2n][B] = [q; v], accel / tau / grad_* [n][B], M [n * n][B] (row-major n x n per world), device pointers, SoA like the step's.
 * B may be (T + 1) x worlds: a whole rollout in one launch.  workspace: device scratch of nbl_dynamics_workspace_bytes(m, B) bytes (one
 * size serves the three calls); calls that share a workspace must be ordered on one stream.  Stream-ordered, no synchronisation, no
 * atomics: bit-reproducible.  External wrenches on bodies, Skeleton::getContactInverseDynamics, getMultipleContactInverseDynamics and what
 * getInverseDynamicsFromPredictions needs are covered by the nbl_*_wrench_* calls and nbl_contact_inverse_dynamics further down.  Not
 * covered: the ...NearCoP variant of the contact solve (createMultipleContactInverseDynamicsNearCoPProblem), the ...OverTime variant, and
 * gradients through the contact solve. */
#define NBL_ID_NO_VELOCITY 1  /* take v as 0 */
#define NBL_ID_NO_GRAVITY 2   /* leave gravity out */
#define NBL_ID_JOINT_FORCES 4 /* + damping v + spring (q - rest + dt v) per DOF: the terms nbl_step_forward puts on the right-hand side, so
                                 that tau fed to the step as the joint torques reproduces a */
size_t nbl_dynamics_workspace_bytes(const nbl_model* m, int64_t B);
/* tau = M(q) a + C(q, v).  accel NULL: a = 0 (tau = C).  Errors: NBL_E_BADARG (null handle / state / tau / workspace, B < 0, unknown
 * flag bits), NBL_E_WORKSPACE (workspace_bytes < nbl_dynamics_workspace_bytes(m, B)).  B = 0 is a no-op. */
int32_t nbl_inverse_dynamics_forward(nbl_model* m, int64_t B, const double* state, const double* accel, int32_t flags, double* tau,
                                     void* workspace, size_t workspace_bytes, void* stream);
/* The reverse pass: grad_state [2n][B] = (accumulate: +=) (d tau / d [q; v])^T grad_tau, grad_accel [n][B] = (+=) M^T grad_tau; either may
 * be NULL.  Both blocks of grad_state are exact (with NBL_ID_NO_VELOCITY the velocity block receives nothing); free and ball coordinates
 * are differentiated analytically through expMapJac (FreeJoint.cpp:790-823, BallJoint.cpp:282-289). */
int32_t nbl_inverse_dynamics_backward(nbl_model* m, int64_t B, const double* state, const double* accel, int32_t flags,
                                      const double* grad_tau, double* grad_state, double* grad_accel, int32_t accumulate, void* workspace,
                                      size_t workspace_bytes, void* stream);
/* M(q): symmetric, both triangles written (M[i][j] and M[j][i] are the same bits).  Only the position block of state is read. */
int32_t nbl_mass_matrix(nbl_model* m, int64_t B, const double* state, double* M, void* workspace, size_t workspace_bytes, void* stream);
/* ---- forward dynamics and the inverse mass matrix (csrc/dynamics.hip) ---------------------------------------------------------------------
 * a = M(q)^-1 (tau - C(q, v))  by the articulated-body algorithm (Skeleton::computeForwardDynamics, Skeleton.cpp:13296-13314) and
 * Y = M(q)^-1 X  /  M(q)^-1 itself (World::getInvMassMatrix; the recursion of Skeleton::updateInvMassMatrix, Skeleton.cpp:12573-12660)
 * of B worlds, one world per lane: O(n) per right-hand side, M is never formed.  The flags are the NBL_ID_* of inverse dynamics, and under
 * the same flags nbl_forward_dynamics_forward and nbl_inverse_dynamics_forward are inverse functions of each other (with
 * NBL_ID_JOINT_FORCES the right-hand side carries - damping v - spring (q - rest + dt v) exactly as nbl_step_forward has it: a is then
 * (v' - v) / dt of a contact-free step).  Conventions as for the nbl_inverse_dynamics_* calls: device pointers, SoA, state [2n][B],
 * tau / accel / grad_* [n][B], B may be (T + 1) x worlds, the handle's CURRENT inertias are read, the handle's slices are not used,
 * stream-ordered, no synchronisation, no atomics, bit-reproducible and independent of B and of a world's place in the batch.
 * workspace: nbl_forward_dynamics_workspace_bytes(m, B) bytes of device scratch (84 doubles per body and world, plus 2 n per world for the
 * reverse pass; one size serves the four calls); calls that share a workspace must be ordered on one stream.
 * Errors: NBL_E_BADARG (null handle / state / output / workspace, B < 0, R < 1, unknown flag bits), NBL_E_WORKSPACE (workspace too small);
 * nothing is launched then.  B = 0 is a no-op. */
size_t nbl_forward_dynamics_workspace_bytes(const nbl_model* m, int64_t B);
/* accel = M(q)^-1 (tau - C(q, v)).  tau NULL: 0. */
int32_t nbl_forward_dynamics_forward(nbl_model* m, int64_t B, const double* state, const double* tau, int32_t flags, double* accel,
                                     void* workspace, size_t workspace_bytes, void* stream);
/* The exact reverse pass, two launches: a is recomputed and lambda = M^-1 grad_accel; grad_tau [n][B] = (accumulate: +=) lambda;
 * grad_state [2n][B] = (+=) -(d ID / d [q; v])^T lambda at (q, v, a) under the same flags, through the reverse kernel of
 * nbl_inverse_dynamics_backward.  Either output may be NULL. */
int32_t nbl_forward_dynamics_backward(nbl_model* m, int64_t B, const double* state, const double* tau, int32_t flags, const double* grad_accel,
                                      double* grad_state, double* grad_tau, int32_t accumulate, void* workspace, size_t workspace_bytes,
                                      void* stream);
/* Y [R][n][B] = M(q)^-1 X [R][n][B]: the articulated inertias once per world, two sweeps per right-hand side.  Only the position block of
 * state is read.  X NULL with R = n: the identity (nothing is read) - nbl_inv_mass_matrix. */
int32_t nbl_inv_mass_apply(nbl_model* m, int64_t B, int32_t R, const double* state, const double* X, double* Y, void* workspace,
                           size_t workspace_bytes, void* stream);
/* Minv [n * n][B] (row-major n x n per world) = M(q)^-1: one triangle is computed and mirrored, Minv[i][j] and Minv[j][i] are the same bits. */
int32_t nbl_inv_mass_matrix(nbl_model* m, int64_t B, const double* state, double* Minv, void* workspace, size_t workspace_bytes, void* stream);
/* ---- wrenches on bodies in the dynamics calls, contact inverse dynamics (csrc/dynamics.hip) ---------------------------------------------------
 * A WRENCH SET is an nbl_kin_map whose entries are all NBL_KIN_SPATIAL (any other kind: NBL_E_BADARG): entry e names the frame
 * F_e = W_body T_offset, and rows 6 e .. 6 e + 5 of wrench [6 E][B] (SoA, device pointer) are [torque(3); force(3)] on it - expressed in
 * F_e and acting at its origin (BodyNode::setExtWrench; the local Jacobian of Skeleton::getJacobian(body)), or, with NBL_WRENCH_WORLD, in
 * world coordinates, acting at the origin of F_e.  The generalized force of a set is tau_ext = sum_e J_e^T W_e, and
 *   nbl_inverse_dynamics_wrench_forward:  tau = M(q) a + C(q, v) - tau_ext        nbl_forward_dynamics_wrench_forward:  a = M(q)^-1 (tau + tau_ext - C(q, v))
 * (plus the NBL_ID_JOINT_FORCES terms): inverse functions of each other under equal flags and wrenches.  The argument lists are those of
 * the calls without wrenches with (k, wrench) added, and grad_wrench [6 E][B] in the reverse passes: grad_wrench = (accumulate: +=)
 * -J grad_tau (inverse dynamics) / J lambda, lambda = M^-1 grad_accel (forward dynamics), in the coordinates the wrenches came in;
 * grad_state is exact in both frames (with NBL_WRENCH_WORLD it includes how R_F^T turns with the ancestors' coordinates).  k NULL: a set
 * with no entries (wrench, grad_wrench unused) - the results of the calls without wrenches, bit for bit; so are those of an all-zero
 * wrench array.  An entry fixed in the world (body -1) moves nothing.  NBL_WRENCH_WORLD is a flag of these four calls only.
 * workspace: nbl_wrench_workspace_bytes(m, k, B) bytes of device scratch (the forward-dynamics workspace plus 3 doubles per body and 12 per
 * entry, per world; one size serves all six calls); calls that share a workspace must be ordered on one stream.  Errors as for the
 * dynamics calls: NBL_E_BADARG (null handle / state / output / workspace, a null wrench array for a set with entries, B < 0, unknown
 * flag bits, a map made for another model, a non-spatial entry), NBL_E_WORKSPACE; nothing is launched then.  B = 0 is a no-op.
 * Stream-ordered, no synchronisation, no atomics, bit-reproducible and independent of B and of a world's place in the batch. */
#define NBL_WRENCH_WORLD 8 /* wrenches in world coordinates, acting at the origin of their entry's frame */
size_t nbl_wrench_workspace_bytes(const nbl_model* m, const nbl_kin_map* k, int64_t B);
int32_t nbl_inverse_dynamics_wrench_forward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* accel,
                                            const double* wrench, int32_t flags, double* tau, void* workspace, size_t workspace_bytes,
                                            void* stream);
int32_t nbl_inverse_dynamics_wrench_backward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* accel,
                                             const double* wrench, int32_t flags, const double* grad_tau, double* grad_state, double* grad_accel,
                                             double* grad_wrench, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
int32_t nbl_forward_dynamics_wrench_forward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* tau,
                                            const double* wrench, int32_t flags, double* accel, void* workspace, size_t workspace_bytes,
                                            void* stream);
int32_t nbl_forward_dynamics_wrench_backward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* tau,
                                             const double* wrench, int32_t flags, const double* grad_accel, double* grad_state, double* grad_tau,
                                             double* grad_wrench, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* ---- gradients of the dynamics calls to the registered inertia parameters (csrc/dynamics.hip) -------------------------------------------
 * Skeleton::getJacobianOfID / getJacobianOfC / getJacobianOfM / getJacobianOfMinv / getJacobianOfFD with a WithRespectTo that is the mass
 * vector (dart/dynamics/Skeleton.hpp:650-718; the reference finite-differences them), as vector-Jacobian products for B worlds.  The
 * parameters are the table of nbl_set_inertia_params[_on] (count = nbl_num_inertia_params(m)); inverse dynamics is linear in every body's
 * spatial inertia G_i, so with V_i, A_i the body's twist and acceleration (gravity carried as the base acceleration -g) and Fb_i the
 * twist field the cotangent generates,
 *   d(grad_tau^T tau) / d theta_p = Fb_i . (dG_p A_i) - ad(V_i, Fb_i) . (dG_p V_i),   i = the body of parameter p:
 * one root -> leaf sweep and one contraction per parameter, one world per lane, in closed form.
 *   nbl_inverse_dynamics_backward_inertia: grad_params [count][B] = (accumulate: +=) (d tau / d theta)^T grad_tau of
 *     nbl_inverse_dynamics_forward under the same state, accel (NULL: a = 0) and flags.  The NBL_ID_JOINT_FORCES terms and wrenches on
 *     bodies do not depend on the inertias: the call serves nbl_inverse_dynamics_wrench_forward unchanged.
 *     workspace: nbl_dynamics_workspace_bytes(m, B).
 *   nbl_forward_dynamics_backward_inertia: grad_params = (+=) (d a / d theta)^T grad_accel = -(d ID / d theta)^T lambda at (q, v, a),
 *     lambda = M^-1 grad_accel, of nbl_forward_dynamics_forward (k NULL: wrench is not read) or nbl_forward_dynamics_wrench_forward
 *     (k, wrench as there; NBL_WRENCH_WORLD accepted): two launches, a and lambda by the articulated-body recursion, then the contraction.
 *     workspace: nbl_forward_dynamics_workspace_bytes(m, B), or nbl_wrench_workspace_bytes(m, k, B) when k is given.
 * Both are self-contained (no preceding backward call, unlike nbl_backward_inertia), read the handle's CURRENT inertias, are stream-ordered
 * on `stream` without synchronisation, do not use the handle's slices, use no atomics and are bit-reproducible and independent of B and
 * of a world's place in the batch; B may be (T + 1) x worlds.  Per-world results: the caller sums over b for a loss over the batch.
 * No parameter registered, or B = 0: a no-op that returns NBL_OK.  Errors as for the calls they differentiate (NBL_E_BADARG, also for a
 * NULL grad_params when count > 0; NBL_E_WORKSPACE): nothing is launched then. */
int32_t nbl_inverse_dynamics_backward_inertia(nbl_model* m, int64_t B, const double* state, const double* accel, int32_t flags,
                                              const double* grad_tau, double* grad_params, int32_t accumulate, void* workspace,
                                              size_t workspace_bytes, void* stream);
int32_t nbl_forward_dynamics_backward_inertia(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* tau,
                                              const double* wrench, int32_t flags, const double* grad_accel, double* grad_params,
                                              int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* Contact inverse dynamics (Skeleton::getContactInverseDynamics, getMultipleContactInverseDynamics; Skeleton.cpp:9705-9949): the wrenches
 * wrench_out [6 E][B] on the entries' frames (local coordinates) under which the accelerations accel [n][B] need NO torque on the six
 * coordinates of the free root joint above them, and the joint torques tau [n][B] = M a + C - J^T W that go with them (the root's six rows
 * are set to 0).  With r = the root's rows of M a + C (flags: NBL_ID_*, as in nbl_inverse_dynamics_forward) and A = J[:, root]^T (6 x 6 E):
 *   NBL_CID_SINGLE      E = 1:  W = A^-1 r                                              (getContactInverseDynamics)
 *   NBL_CID_NEAREST     W = W0 + A^T (A A^T)^-1 (r - A W0), W0 = wrench_guess [6 E][B]: the solution nearest to the guesses, what the
 *                       reference's complete orthogonal decomposition returns for a full-row-rank A
 *   NBL_CID_MIN_TORQUE  W = B^-1 A^T (A B^-1 A^T)^-1 r, B = diag(1, 1, 1, 0.01, 0.01, 0.01) per body: the closed form of the reference's
 *                       KKT system for an empty guess list (wrench_guess is not read)
 * through the LDL^T factorisation of the 6 x 6 matrix A D A^T per world; a pivot that is not positive (a rank-deficient A) writes NaN to
 * that world's outputs only.  Every entry must hang below ONE body whose joint is the free joint at the root of its tree: otherwise
 * NBL_E_UNSUPPORTED (the reference prints an error and returns zeros).  NBL_WRENCH_WORLD is not accepted (NBL_E_BADARG): the reference's
 * wrenches are local.  Other errors as above, plus NBL_E_BADARG for an unknown mode, NBL_CID_SINGLE with E != 1 and NBL_CID_NEAREST without
 * guesses.  No gradients flow through the solve (the reference has none).  Not offered: the ...NearCoP and ...OverTime variants. */
#define NBL_CID_SINGLE 0
#define NBL_CID_NEAREST 1
#define NBL_CID_MIN_TORQUE 2
int32_t nbl_contact_inverse_dynamics(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* accel,
                                     const double* wrench_guess, int32_t mode, int32_t flags, double* wrench_out, double* tau, void* workspace,
                                     size_t workspace_bytes, void* stream);
/* ---- batched inverse kinematics (csrc/ik.hip) --------------------------------------------------------------------------------------------
 * IKMapping::setPositions (dart/neural/IKMapping.cpp:86-119) for B independent worlds: find joint positions whose mapped rows (the rows
 * of nbl_kinematics_forward) meet `target`.  The kernel restates math::solveIK with ONE restart and math::refineIK
 * (dart/math/IKSolver.cpp:195-493) operation by operation, one world per lane: refineIK for 20 steps from q_init (unclamped unless
 * start_clamped), then refineIK for max_step_count steps from that result; refineIK's ladder on errorChange (the 1e-21 stop, halving of
 * lr with the switch to transpose mode below 1e-4, the line search back to the last iterate, the vanishing-lr stop below 1e-10, the
 * convergence branch that goes to transpose mode with lr <= 5e-5, then turns clamping on, then stops, lr *= 1.1 otherwise), clamping
 * forced on the last steps (i > max_step_count - 5), the update pos <- clamp?(pos - lr delta).  J is IKMapping::getPosJacobian, the exact
 * derivative nbl_kinematics_backward applies, built densely per world.  Clamping is Skeleton::clampPositionsToLimits
 * (dart/dynamics/Skeleton.cpp:3642-3740) on the model's pos_lo / pos_hi: the clamp per coordinate (the routine's 2 pi candidates for
 * revolute coordinates never change its result: csrc/ik_dev.hpp), then logMap(expMapRot(.)) of the rotation coordinates of free and ball
 * joints.  Random restarts are not offered (setPositions' own restart callback is assert(false)).
 * Two departures from the reference:
 *   1. the damped-least-squares step.  The reference factors J J^T + lambda I when n < P and J^T J + lambda I otherwise - the LARGER of
 *      the two, up to 384 x 384.  The two give the same step in exact arithmetic, J^T (J J^T + lambda I)^-1 = (J^T J + lambda I)^-1 J^T;
 *      the kernel factors the SMALLER one (min(P, n) <= 64 on a side) by an in-place Cholesky and two triangular solves.
 *      least_squares_damping = 0 (the reference's complete orthogonal decomposition) is NBL_E_UNSUPPORTED;
 *   2. `loss` is |rows(q_out) - target|^2 AT the returned positions, from one evaluation after the loop (refineIK's lastError belongs to
 *      an earlier iterate, and solveIK returns the 20-step phase's loss).
 * target [P][B], q_init / q_out [n][B], loss [B], steps [B] (the number of eval calls over both phases): DEVICE pointers, SoA like
 * the step's.  q_init NULL: zeros (setPositions).  config NULL: setPositions' configuration (the defaults with max_step_count = 500).
 * workspace: nbl_ik_workspace_bytes(m, k, B) bytes of device scratch (3 n + P + min(P, n) + P n + min(P, n)^2 doubles per world).
 * Errors: NBL_E_BADARG (null handle / map / target / q_out / workspace, B < 0, max_step_count < 1 or > 100000, negative damping or threshold),
 * NBL_E_WORKSPACE (workspace too small), NBL_E_UNSUPPORTED (damping = 0); nothing is launched then.  B = 0 is a no-op.  Stream-ordered
 * on `stream`, no synchronisation, no atomics; it does not use the handle's slices.  Results do not depend on B or on a world's place
 * in the batch.  The reference has no gradient of the solve; nbl_ik_solve_vjp below gives the one this library defines. */
typedef struct {
  double convergence_threshold;   /* 1e-7 */
  int32_t max_step_count;         /* 100; IKMapping::setPositions passes 500 */
  double least_squares_damping;   /* 0.01 */
  int32_t start_clamped;          /* 0 */
  int32_t line_search;            /* 1 */
  int32_t dont_exit_transpose;    /* 0 */
} nbl_ik_config;
void nbl_ik_default_config(nbl_ik_config* config); /* math::IKConfig's defaults (IKSolver.hpp:31-38) */
size_t nbl_ik_workspace_bytes(const nbl_model* m, const nbl_kin_map* k, int64_t B);
int32_t nbl_ik_solve(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* target, const double* q_init, const nbl_ik_config* config,
                     double* q_out, double* loss, int32_t* steps, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the reverse pass of inverse kinematics (csrc/ik_grad.hip) ---------------------------------------------------------------------------
 * grad_target = (d q / d target)^T grad_q at the positions q nbl_ik_solve returned: what a loss on q contributes to the gradient of the
 * targets.  The reference has no such gradient; this is the library's own convention.  Let J = IKMapping::getPosJacobian at q (the dense
 * Jacobian the solver builds, the exact derivative nbl_kinematics_backward applies) and F the FREE coordinates: a coordinate is clamped
 * when q_i equals a finite pos_lo_i or pos_hi_i bit for bit - what the solver's clamp leaves behind -, free otherwise (always, for an
 * infinite limit).  With J_F the columns of J in F,
 *     grad_target = J_F (J_F^T J_F + mu I)^-1 (grad_q)_F  =  (J_F J_F^T + mu I)^-1 J_F (grad_q)_F,
 * the Gauss-Newton sensitivity of min |rows(q) - target|^2 over the free coordinates.  Clamped coordinates contribute nothing; with no
 * free coordinate grad_target is 0.  mu = grad_damping > 0 is a Tikhonov term of the gradient alone (NOT the solver's
 * least_squares_damping; 1e-9 is a good default); grad_damping = 0 is NBL_E_UNSUPPORTED, as the solver refuses damping 0.  The kernel
 * factors the SMALLER of the two forms, min(P, |F|) <= 64 on a side, by the solver's in-place Cholesky and two triangular solves.
 * Two limits of the convention:
 *   1. the second-order term sum_k (rows(q) - target)_k grad^2 rows_k is left out: the result is the derivative of the solve where the
 *      target is met (and the solve converged), and the Gauss-Newton approximation of it elsewhere;
 *   2. there is no gradient with respect to q_init.
 * q, grad_q [n][B], grad_target [P][B] (accumulate != 0: added to), free_count [B] int32 = |F| per world (may be NULL): DEVICE pointers,
 * SoA.  workspace: nbl_ik_grad_workspace_bytes(m, k, B) bytes of device scratch (the solver's layout).  Errors: NBL_E_BADARG (null handle
 * / map / q / grad_q / grad_target / workspace, B < 0, negative grad_damping), NBL_E_WORKSPACE (workspace too small), NBL_E_UNSUPPORTED
 * (grad_damping = 0); nothing is launched then.  B = 0 is a no-op.  Stream-ordered on `stream`, no synchronisation, no atomics; it does
 * not use the handle's slices.  Results are bit-reproducible and do not depend on B or on a world's place in the batch. */
size_t nbl_ik_grad_workspace_bytes(const nbl_model* m, const nbl_kin_map* k, int64_t B);
int32_t nbl_ik_solve_vjp(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* q, const double* grad_q, double grad_damping,
                         double* grad_target, int32_t accumulate, int32_t* free_count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- read-out of a step's contacts, impulses and body contact wrenches (csrc/contact_readout.hip) -----------------------------------------
 * What the contacts of a step WERE, decoded from its saved record (`saved`: the nbl_saved_bytes(m, B) bytes nbl_step_forward wrote; the T
 * records of a rollout are read with T calls at the byte offsets t * nbl_saved_bytes(m, B) - the rows of a record are interleaved over ITS
 * B worlds, so one launch cannot take T x B worlds): World::getLastCollisionResult (dart/collision/Contact.hpp:90-147), Contact::force as
 * ContactConstraint::applyImpulse fills it (ContactConstraint.cpp:630-684), BackpropSnapshot::getContactConstraintImpulses / Mappings.
 * The calls only read the record: the step, its records and its results are untouched.  All outputs are DEVICE pointers, SoA.
 *
 * nbl_contact_readout: count[b] (int32) = the collider contacts of world b.  The pseudo-contacts the record appends after them are not
 * counted: n_limit_rows[b] joint-limit rows and n_friction_rows[b] joint Coulomb friction rows (either may be NULL).  contacts (may be
 * NULL) is the table [NBL_CO_FIELDS][C][B], entry ((field * C + slot) * B + b), C = desc.max_contacts of the model (0 when <= 0):
 *   NBL_CO_POINT (3), NBL_CO_NORMAL (3), NBL_CO_DEPTH, NBL_CO_TYPE (the narrow phase's contact type code)
 *   NBL_CO_COLLIDER_A, NBL_CO_COLLIDER_B   indices into the description's collider list (box_*)
 *   NBL_CO_BODY_A, NBL_CO_BODY_B           the colliders' bodies as indices of the description (nbl_kin_map_create's `body`), -1 = the world
 *   NBL_CO_IMPULSE (3)                     the LCP impulses: normal, tangent 1, tangent 2
 *   NBL_CO_CLASS (3)                       their row classes: 0 not clamping, 1 clamping, +2 / -2 a friction row on its upper / lower bound
 *   NBL_CO_FORCE (3)                       (n l0 + t1 l1 + t2 l2) / dt, world coordinates, t1 / t2 = ContactConstraint::getTangentBasisMatrixODE(n)
 * all as doubles.  A frictionless contact (min(mu_A, mu_B) <= 1e-3) has one LCP row: its tangent impulses read 0 and their classes
 * NBL_CO_CLASS_EMPTY (-1); its force is along the normal.  Slots at or above count[b] are all zeros.
 *
 * nbl_contact_readout_rows: the live LCP rows of every world in the reference's order - constraint by constraint, 3 rows for a contact
 * with friction, 1 for a frictionless contact, a joint-limit row and a joint-friction row - compacted: n_rows[b] (int32), impulse
 * [3 C][B] (the reference's sign: a row at an upper joint limit is negative) and mapping [3 C][B] (int32; neural::ConstraintMapping):
 * -1 clamping, -2 not clamping, >= 0 a friction row on its bound: the compacted index of its contact's normal row.  A joint-limit row
 * that carries an impulse is clamping; a joint-friction row on its fixed bound has no normal row to point to and reads not clamping.
 * Rows at or above n_rows[b]: impulse 0, mapping NBL_CO_MAP_NONE.  impulse / mapping may be NULL.
 *
 * nbl_contact_body_wrenches: wrench [6 E][B] for E <= NBL_CO_MAX_BODIES bodies of the description (`bodies`, HOST pointer, read during the
 * call): rows 6 e .. 6 e + 5 = [torque(3); force(3)] in world coordinates, acting at the origin of body e's frame = the sum over the
 * world's collider contacts of + NBL_CO_FORCE on the body of collider A and - NBL_CO_FORCE on the body of collider B, each with the
 * moment (point - p_body) x force.  These are the wrenches nbl_forward_dynamics_wrench_forward takes with NBL_WRENCH_WORLD for an all-
 * NBL_KIN_SPATIAL set with identity offsets on the same bodies.  A body no contact touches gets zeros; a self-collision contact gives
 * + and - to its two bodies.  Joint-limit and joint-friction rows are generalized forces, not body wrenches: they contribute nothing.
 * The bodies' world positions are recomputed from the record's q (forward kinematics down each body's ancestor chain), so the call does
 * not depend on whether or how the record carries tree state (NBL_SAVE_TREE, compact or lane-interleaved).
 *
 * A model without a contact stage: count 0, zero tables and wrenches; nothing reads the record.  Errors: NBL_E_BADARG for a null handle,
 * record or required output (count; n_rows; wrench and bodies when E > 0), B < 0, E < 0 or > NBL_CO_MAX_BODIES, a body index outside
 * [0, n_bodies) or named twice; nothing is launched then.  B = 0 is a no-op.  Stream-ordered on `stream`, no synchronisation, no atomics,
 * no workspace; bit-reproducible and independent of B and of a world's place in the batch.  The calls do not use the handle's slices: with
 * deferred join on, nbl_join_slices first.  No gradients flow through the read-outs (the reference has none there either). */
#define NBL_CO_POINT 0
#define NBL_CO_NORMAL 3
#define NBL_CO_DEPTH 6
#define NBL_CO_TYPE 7
#define NBL_CO_COLLIDER_A 8
#define NBL_CO_COLLIDER_B 9
#define NBL_CO_BODY_A 10
#define NBL_CO_BODY_B 11
#define NBL_CO_IMPULSE 12
#define NBL_CO_CLASS 15
#define NBL_CO_FORCE 18
#define NBL_CO_FIELDS 21
#define NBL_CO_CLASS_EMPTY -1
#define NBL_CO_MAP_NONE -4
#define NBL_CO_MAX_BODIES 64
int32_t nbl_contact_readout(nbl_model* m, int64_t B, const void* saved, int32_t* count, int32_t* n_limit_rows, int32_t* n_friction_rows,
                            double* contacts, void* stream);
int32_t nbl_contact_readout_rows(nbl_model* m, int64_t B, const void* saved, int32_t* n_rows, double* impulse, int32_t* mapping, void* stream);
int32_t nbl_contact_body_wrenches(nbl_model* m, int64_t B, const void* saved, int32_t E, const int32_t* bodies, double* wrench, void* stream);

/* ---- centre of mass, momentum and energy of a body set (csrc/centroidal.hip) -----------------------------------------------------------------
 * The whole-body quantities of Skeleton (dart/dynamics/Skeleton.cpp:13598-13810; python/_nimblephysics/dynamics/Skeleton.cpp:1873-2035)
 * for B worlds, one world per lane, one launch for whichever outputs are asked for, and their exact vector-Jacobian product.  Appended
 * within ABI minor 5 like the entries above: a caller that needs them looks the symbols up.
 *
 * A BODY SET (nbl_body_set_create) names bodies of the description the model was created from (`bodies`: `count` indices there, each at
 * most once; NULL with count 0: every body of the model - a Skeleton of the reference is the set of its bodies).  The library resolves its
 * internal bodies (a ball / free chain carries its mass on the body that carries T_cj).  A model of more than 64 internal bodies is
 * NBL_E_UNSUPPORTED; an index out of range or named twice, and a set whose total mass is 0, are NBL_E_BADARG.  Destroy a set before the
 * model it was made for.  nbl_body_set_mass: the set's total mass at the handle's CURRENT inertias (Skeleton::getMass, Skeleton.cpp:11310).
 * A null handle or a set made for another model: 0 and nbl_last_error() says why.
 *
 * nbl_centroidal_forward writes every output that is not NULL (device pointers, SoA like the step's; state [2n][B] = [q; v]):
 *   com      [3][B]    sum m_i (p_i + R_i c_i) / M                                          Skeleton::getCOM (Skeleton.cpp:13645-13658)
 *   com_vel  [3][B]    sum m_i d/dt(p_i + R_i c_i) / M, world coordinates                   getCOMLinearVelocity(World, World) (:13695-13701)
 *   com_acc  [3][B]    sum m_i d2/dt2(p_i + R_i c_i) / M at the accelerations accel [n][B]: the classical linear acceleration of every
 *                      body's centre of mass (BodyNode::getCOMLinearAcceleration); gravity is NOT part of it  getCOMLinearAcceleration (:13714-13720)
 *   momentum [6][B]    [angular momentum about the set's centre of mass; linear momentum], world coordinates.  The reference has the momenta
 *                      PER BODY only (BodyNode::getLinearMomentum / getAngularMomentum, BodyNode.cpp:2378-2391): their sum over the set is
 *                      this library's extension.  The linear part equals M com_vel and is computed independently from G_i V_i.
 *   ke       [B]       sum V_i^T G_i V_i / 2                                                computeKineticEnergy (:13598-13607; BodyNode.cpp:2357-2363)
 *   pe       [B]       - sum m_i g . (p_i + R_i c_i) + sum_d k_d (q_d - rest_d)^2 / 2 over the coordinates of the set's joints
 *                      (computePotentialEnergy, :13610-13621; GenericJoint.hpp:1598-1610).  NBL_CEN_PE_BODY_ORIGIN: - sum m_i g . p_i instead, the reference's number
 *                      (BodyNode::computePotentialEnergy, BodyNode.cpp:2372-2375, takes the body frame's origin, not its centre of mass);
 *                      NBL_CEN_NO_SPRINGS leaves the spring energy out.
 *   Jcom     [3 n][B]  row-major 3 x n per world: getCOMLinearJacobian in world coordinates (:13783-13790), com_vel = Jcom v.  The columns
 *                      of coordinates that move no body of the set are zeros, written by the kernel (no host zero-fill).
 * All read the handle's CURRENT inertias (nbl_set_body_inertia(s), nbl_set_inertia_params).  accel may be NULL unless com_acc is asked for.
 *
 * nbl_centroidal_backward: grad_state [2n][B] and grad_accel [n][B] (either may be NULL) = (accumulate: +=) the cotangents g_* (any may be
 * NULL: it contributes nothing) pulled back.  Exact in both blocks of the state: the velocity- and acceleration-level outputs carry their
 * full dependence on the positions; free and ball coordinates are differentiated analytically through expMapJac.  Jcom has no cotangent.
 *
 * workspace: nbl_centroidal_workspace_bytes(m, B) bytes of device scratch (54 doubles per body and world; one size serves both calls);
 * calls that share a workspace must be ordered on one stream.  Errors: NBL_E_BADARG (null handle / set / state / workspace, a set made for
 * another model, B < 0, unknown flag bits, com_acc or g_com_acc without accel, a set whose mass has become 0), NBL_E_WORKSPACE; nothing is
 * launched then.  B = 0 is a no-op.  B may be (T + 1) x worlds.  Stream-ordered on `stream`, no synchronisation, no atomics, no LDS:
 * bit-reproducible and independent of B and of a world's place in the batch.  The calls do not use the handle's slices. */
#define NBL_CEN_PE_BODY_ORIGIN 1 /* pe from the body frames' origins (the reference's rule) instead of the bodies' centres of mass */
#define NBL_CEN_NO_SPRINGS 2     /* pe without the joint spring energy */
typedef struct nbl_body_set nbl_body_set; /* opaque */
int32_t nbl_body_set_create(nbl_model* m, int32_t count, const int32_t* bodies, nbl_body_set** out);
void nbl_body_set_destroy(nbl_body_set* s);
double nbl_body_set_mass(nbl_model* m, const nbl_body_set* s);
/* For a caller that merged welded BodyNodes before nbl_model_create and wants NBL_CEN_PE_BODY_ORIGIN to give the reference's number on
 * them: moments [count][3] (HOST pointer) = for each of `bodies`, sum_k m_k o_k over the BodyNodes merged into it, o_k the origin of
 * BodyNode k's frame in the merged body's frame.  pe then reads - sum g . (m_i p_i + R_i moment_i).  Default: zeros (the body's own origin).
 * Takes effect for the calls issued afterwards; the caller repeats it when those masses change. */
int32_t nbl_body_set_origin_moments(nbl_model* m, nbl_body_set* s, int32_t count, const int32_t* bodies, const double* moments);
size_t nbl_centroidal_workspace_bytes(const nbl_model* m, int64_t B);
int32_t nbl_centroidal_forward(nbl_model* m, const nbl_body_set* s, int64_t B, const double* state, const double* accel, int32_t flags,
                               double* com, double* com_vel, double* com_acc, double* momentum, double* ke, double* pe, double* Jcom,
                               void* workspace, size_t workspace_bytes, void* stream);
int32_t nbl_centroidal_backward(nbl_model* m, const nbl_body_set* s, int64_t B, const double* state, const double* accel, int32_t flags,
                                const double* g_com, const double* g_com_vel, const double* g_com_acc, const double* g_momentum,
                                const double* g_ke, const double* g_pe, double* grad_state, double* grad_accel, int32_t accumulate,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ---- gyroscope, accelerometer and magnetometer readings (csrc/sensors.hip) -----------------------------------------------------------------------
 * Skeleton::getGyroReadings / getAccelerometerReadings / getMagnetometerReadings (dart/dynamics/Skeleton.cpp:8082-8460) for B worlds, and
 * their exact vector-Jacobian product.
 *
 * A SENSOR SET is an nbl_kin_map whose entries are all NBL_KIN_SPATIAL (any other kind: NBL_E_BADARG), like a wrench set: entry e names
 * the sensor frame T_bs = (R_bs, p_bs) = T_offset[e] fixed in body[e] (at most 64 entries; body -1: a sensor fixed in the world).  With the
 * body's spatial velocity [w; v] and spatial acceleration [al; a] in body coordinates (no gravity in it), its world rotation R, the
 * model's gravity g and a world-frame magnetic field m, rows 3 e .. 3 e + 2 of the outputs are
 *   gyro = R_bs^T w          acc = R_bs^T (a + al x p_bs + w x (v + w x p_bs) - R^T g)          mag = R_bs^T R^T m
 * (a sensor in the world: gyro 0, acc -R_bs^T g, mag R_bs^T m).  Body scales do not exist here: they are 1.
 *
 * nbl_sensors_forward writes every output that is not NULL (device pointers, SoA: state [2n][B] = [q; v], accel [n][B], field [3][B],
 * gyro / acc / mag [3 count][B]).  acc without accel and mag without field: NBL_E_BADARG.
 * nbl_sensors_backward: grad_state [2n][B], grad_accel [n][B] and grad_field [3][B] (any may be NULL) = (accumulate: +=) the cotangents
 * g_gyro, g_acc, g_mag [3 count][B] (any may be NULL: zero) pulled back through the forward function, exactly, in the library's own
 * coordinates: the dependence of the velocity products on q and v and of R^T g on q is included; ball and free coordinates go through
 * expMapJac.  g_acc needs accel, g_mag needs field.
 * workspace: nbl_sensors_workspace_bytes(m, B) bytes of device scratch (54 doubles per body and world; one size serves both calls).
 * Stream-ordered, no device synchronisation, no use of the handle's slices; B may be (T + 1) x worlds. */
size_t nbl_sensors_workspace_bytes(const nbl_model* m, int64_t B);
int32_t nbl_sensors_forward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* accel, const double* field,
                            double* gyro, double* acc, double* mag, void* workspace, size_t workspace_bytes, void* stream);
int32_t nbl_sensors_backward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* accel, const double* field,
                             const double* g_gyro, const double* g_acc, const double* g_mag, double* grad_state, double* grad_accel,
                             double* grad_field, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* enabled = 0: off (and reset); 1: HIP events around every kernel launch; N > 1: around the launches of every N-th forward /
 * backward call only (sampling keeps the perturbation of a timed region below 1 %). */
int32_t nbl_set_timing(nbl_model* m, int32_t enabled);
int32_t nbl_get_timing(nbl_model* m, double* fwd_ms_sum, int64_t* fwd_count, double* bwd_ms_sum,
                       int64_t* bwd_count);
/* Per-kernel breakdown of the same measurements (names match the rocprofv3 kernel trace). */
int32_t nbl_kernel_count(void);
const char* nbl_kernel_name(int32_t i);
int32_t nbl_kernel_timing(nbl_model* m, int32_t i, double* ms_sum, int64_t* count);

/* ---- task-space Jacobians, their time derivative and task-space accelerations (csrc/taskspace.hip) ---------------------------------------------
 * Second-order world-space kinematics of the rows of a kinematics map, entries of any kind (the rows, their order and their frames are those of
 * nbl_kinematics_forward's vel), for B worlds: BodyNode::getJacobian / getJacobianClassicDeriv / getLinearJacobianDeriv /
 * getAngularJacobianDeriv of the reference, batched.  With R = nbl_kin_map_dim(k) and n the DOFs:
 *   J    [R n][B]  row-major R x n per world: vel = J v.  One pass per entry, every column written (zero where a coordinate is no ancestor's).
 *   Jdot [R n][B]  d/dt J along the motion (q moving with v), so that Jdot v = bias.  Forward only.
 *   bias [R][B]    Jdot v
 *   xdd  [R][B]    J accel + Jdot v: for linear rows the classical acceleration of the frame's origin, for angular rows the angular
 *                  acceleration, each the time derivative of the vel row; ball and free joints carry their Sdot v term.  No gravity.
 * nbl_task_accel writes bias and / or xdd (either may be NULL; xdd needs accel).
 * nbl_task_jacobian_vjp: grad_q [n][B] = (accumulate: +=) d<G, J>/dq for a cotangent G [R n][B], exactly.
 * nbl_task_accel_vjp: grad_state [2n][B] and grad_accel [n][B] (either may be NULL) = (accumulate: +=) the cotangent g_out [R][B] of xdd -
 * accel NULL: of bias - pulled back exactly; the dependence of J accel + Jdot v on q is included.
 * `rows` and `n` are the caller's R and n, checked against the map and the model: NBL_E_BADARG on a mismatch, as on a null handle, map,
 * state or required output, a map made for another model, B < 0; NBL_E_WORKSPACE.  B = 0 is a no-op.  All pointers are device pointers, SoA,
 * state [2n][B] = [q; v], accel [n][B].  Only nbl_task_accel_vjp needs a workspace: nbl_task_workspace_bytes(m, B) bytes of device scratch
 * (54 doubles per body and world).  Stream-ordered on `stream`, no synchronisation, no atomics, no LDS: bit-reproducible and independent
 * of B and of a world's place in the batch; B may be (T + 1) x worlds.  The calls do not use the handle's slices. */
size_t nbl_task_workspace_bytes(const nbl_model* m, int64_t B);
int32_t nbl_task_jacobian(nbl_model* m, const nbl_kin_map* k, int64_t B, int32_t rows, int32_t n, const double* state, double* J, void* stream);
int32_t nbl_task_accel(nbl_model* m, const nbl_kin_map* k, int64_t B, int32_t rows, int32_t n, const double* state, const double* accel,
                       double* bias, double* xdd, void* stream);
int32_t nbl_task_accel_vjp(nbl_model* m, const nbl_kin_map* k, int64_t B, int32_t rows, int32_t n, const double* state, const double* accel,
                           const double* g_out, double* grad_state, double* grad_accel, int32_t accumulate, void* workspace,
                           size_t workspace_bytes, void* stream);
int32_t nbl_task_jacobian_vjp(nbl_model* m, const nbl_kin_map* k, int64_t B, int32_t rows, int32_t n, const double* state, const double* G,
                              double* grad_q, int32_t accumulate, void* stream);
int32_t nbl_task_jacobian_deriv(nbl_model* m, const nbl_kin_map* k, int64_t B, int32_t rows, int32_t n, const double* state, double* Jdot,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NIMBLE_AMD_H */
