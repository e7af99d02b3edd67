"""URDF subset loader: builds a `ModelDescription` from the URDF features the hot path covers.

Conventions follow the reference's dart/utils/urdf/DartLoader.cpp (parameters only; nothing is copied):
  * root link != "world"  -> FreeJoint root (:224-248); a root link named "world" is not a body (:196-222)
  * joint origin -> T_ParentBodyToJoint, T_ChildBodyToJoint = identity (:399-400)
  * inertial origin xyz -> local COM, inertia rotated by the inertial rpy (:527-545)
  * limits/damping per :403-437; `fixed` -> WeldJoint (:482-486), merged into the parent by ModelDescription.merge_welds
  * children are visited depth-first in joint-NAME order (urdfdom keeps joints in a std::map and builds child_links
    from it), which fixes the DOF order of the skeleton
  * collision boxes -> box colliders with the collision origin as the shape's relative transform (:612-616);
    mesh / capsule / cylinder colliders (libccd path, not vendored) raise, or are dropped on request
Revolute, continuous, prismatic, fixed, floating and planar joints (every type DartLoader::createDartJoint knows); joint Coulomb friction (`<dynamics friction=...>`) is read into BodySpec.coulomb_friction.
"""
import os
import xml.etree.ElementTree as ET

import numpy as np

from .model import BodySpec, BoxSpec, ModelDescription, make_transform


def _floats(s, n=3, default=0.0):
    if s is None:
        return [default] * n
    return [float(x) for x in s.split()]


def _origin(el):
    o = el.find("origin") if el is not None else None
    if o is None:
        return make_transform()
    return make_transform(_floats(o.get("xyz")), _floats(o.get("rpy")))


def load_urdf(path, name=None, weld_joints=(), drop_unsupported_colliders=False):
    """Parse `path`; joints named in `weld_joints` are frozen at 0 (welded), e.g. the arms of the 20-DOF Atlas.  Collision geometry other
    than boxes and spheres raises unless `drop_unsupported_colliders` (the link is then loaded without that collider)."""
    root = ET.parse(path).getroot()
    if name is None:
        name = root.get("name", "model")
    links = {l.get("name"): l for l in root.findall("link")}
    joints = {j.get("name"): j for j in root.findall("joint")}
    link_names = {ln_.get("name") for ln_ in root.findall("link")}
    for jn_, j_ in joints.items():
        for end in ("parent", "child"):                                      # (urdfdom refuses such a file: DartLoader returns no skeleton)
            if j_.find(end) is None or j_.find(end).get("link") not in link_names:
                raise ValueError(f"{path}: joint {jn_} refers to a {end} link that the file does not define")
        if j_.find("mimic") is not None:
            # DartLoader::addMimicJointsRecursive (DartLoader.cpp:318-380): the joint becomes a MIMIC actuator driven by another joint
            raise ValueError(f"{path}: joint {jn_} is a mimic joint: kinematically driven joints are outside the hot-path scope")
    child_of = {}
    children = {ln: [] for ln in links}
    for jn in sorted(joints):  # std::map order
        j = joints[jn]
        p, c = j.find("parent").get("link"), j.find("child").get("link")
        child_of[c] = jn
        children[p].append(jn)
    roots = [ln for ln in links if ln not in child_of]
    assert len(roots) == 1, roots
    bodies, boxes = [], []

    def link_inertial(ln):
        inert = links[ln].find("inertial")
        if inert is None:
            return 1.0, (0, 0, 0), (1, 1, 1, 0, 0, 0)  # BodyNode defaults (Inertia.cpp ctor: mass 1, identity moment)
        mass = float(inert.find("mass").get("value"))
        o = inert.find("origin")
        xyz = _floats(o.get("xyz")) if o is not None else [0, 0, 0]
        rpy = _floats(o.get("rpy")) if o is not None else [0, 0, 0]
        i = inert.find("inertia")
        J = np.array([[float(i.get("ixx")), float(i.get("ixy")), float(i.get("ixz"))],
                      [float(i.get("ixy")), float(i.get("iyy")), float(i.get("iyz"))],
                      [float(i.get("ixz")), float(i.get("iyz")), float(i.get("izz"))]])
        R = make_transform((0, 0, 0), rpy)[:3, :3]
        J = R @ J @ R.T
        return mass, tuple(xyz), (J[0, 0], J[1, 1], J[2, 2], J[0, 1], J[0, 2], J[1, 2])

    def add_shapes(ln, body_index):
        for col in links[ln].findall("collision"):
            geom = col.find("geometry")
            box = geom.find("box") if geom is not None else None
            sph = geom.find("sphere") if geom is not None else None
            if box is not None:
                boxes.append(BoxSpec(body_index, _origin(col), tuple(_floats(box.get("size"))), 1.0))
            elif sph is not None:
                r = float(sph.get("radius"))
                boxes.append(BoxSpec(body_index, _origin(col), (r, r, r), 1.0, "sphere"))
            elif geom is not None and len(geom) and not drop_unsupported_colliders:
                # mesh / capsule / cylinder: outside the analytic box / sphere narrow phases (the reference: libccd / its mesh code)
                raise ValueError(f"{path}: {geom[0].tag} collider on link {ln} is outside the analytic narrow phases (box, sphere); "
                                 "drop_unsupported_colliders=True loads the model without it")

    def recurse(ln, parent_index):
        for jn in children[ln]:
            j = joints[jn]
            c = j.find("child").get("link")
            jt = j.get("type")
            mass, com, inertia = link_inertial(c)
            kw = {}
            if jt in ("revolute", "continuous", "prismatic") and jn not in weld_joints:
                jtype = "prismatic" if jt == "prismatic" else "revolute"
                lim = j.find("limit")
                if lim is not None and jt != "continuous":
                    kw["pos_lo"] = (float(lim.get("lower", 0.0)),)
                    kw["pos_hi"] = (float(lim.get("upper", 0.0)),)
                if lim is not None:
                    if lim.get("velocity") is not None:
                        kw["vel_lo"] = (-float(lim.get("velocity")),)
                        kw["vel_hi"] = (float(lim.get("velocity")),)
                    if lim.get("effort") is not None:
                        kw["force_lo"] = (-float(lim.get("effort")),)
                        kw["force_hi"] = (float(lim.get("effort")),)
                    lo, hi = float(lim.get("lower", 0.0)), float(lim.get("upper", 0.0))
                    if jt != "continuous" and (lo > 0 or hi < 0):
                        kw["rest"] = ((lo + hi) / 2.0,)  # DartLoader.cpp:414-431
                dyn = j.find("dynamics")
                if dyn is not None:
                    kw["damping"] = (float(dyn.get("damping", 0.0)),)
                    if float(dyn.get("friction", 0.0)) != 0.0:
                        kw["coulomb_friction"] = (float(dyn.get("friction")),)   # DartLoader.cpp:436
                axis = _floats(j.find("axis").get("xyz")) if j.find("axis") is not None else [1, 0, 0]
            elif jt == "fixed" or jn in weld_joints:
                jtype, axis = "weld", [0, 0, 1]
            elif jt == "floating":                       # FreeJoint with the basic properties only (DartLoader.cpp:487-494)
                jtype, axis = "free", [0, 0, 1]
            elif jt == "planar":                         # PlanarJoint with its default XY plane; URDF limits are not read (:495-503)
                jtype, axis = "planar", [0, 0, 1]
                kw["axes"] = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]
            else:
                raise ValueError(f"{jn}: joint type {jt} outside scope")
            bodies.append(BodySpec(c, parent_index, jtype, jn, axis=tuple(axis), T_pj=_origin(j), mass=mass, com=com,
                                   inertia=inertia, **kw))
            idx = len(bodies) - 1
            add_shapes(c, idx)
            recurse(c, idx)

    rl = roots[0]
    if rl == "world":
        recurse(rl, -1)
    else:
        mass, com, inertia = link_inertial(rl)
        bodies.append(BodySpec(rl, -1, "free", "rootJoint", mass=mass, com=com, inertia=inertia))
        add_shapes(rl, 0)
        recurse(rl, 0)
    return ModelDescription(name, bodies, boxes)


def with_ground(model, ground):
    """One world from two skeletons (the reference loads the robot and the ground URDF into the same World)."""
    nb = len(model.bodies)
    boxes = list(model.boxes)
    # skeleton ids: both descriptions number their skeletons from 0 (or not at all): resolve each on its own, then put the ground's
    # after the model's - otherwise two mobile skeletons with the same id would never collide (CollisionFilter.cpp:105-154)
    ids_m, ids_g = model.body_skeletons(), ground.body_skeletons()
    dense_m = {v: k for k, v in enumerate(sorted(set(ids_m)))}
    dense_g = {v: k + len(dense_m) for k, v in enumerate(sorted(set(ids_g)))}
    bodies = []
    for b, sk in zip(model.bodies, ids_m):
        nbdy = BodySpec(**{**b.__dict__})
        nbdy.skeleton = dense_m[sk]
        bodies.append(nbdy)
    for b, sk in zip(ground.bodies, ids_g):
        nbdy = BodySpec(**{**b.__dict__})
        nbdy.parent = b.parent + nb if b.parent >= 0 else -1
        nbdy.skeleton = dense_g[sk]
        bodies.append(nbdy)
    for bx in ground.boxes:
        boxes.append(BoxSpec(bx.body + nb if bx.body >= 0 else -1, bx.T, bx.size, bx.mu, bx.shape, bx.restitution))
    return ModelDescription(model.name + "_ground", bodies, boxes, model.gravity, model.dt, None, max_contacts=8)




# ---------------------------------------------------------------------------------------------------------------------
# SKEL subset loader (conventions of dart/utils/SkelParser.cpp; parameters only, nothing is copied)
# ---------------------------------------------------------------------------------------------------------------------
def euler_xyz_to_matrix(a):
    """math::eulerXYZToMatrix (dart/math/Geometry.cpp:1767-1797): R = Rx(a0) Ry(a1) Rz(a2), the rotation part of every
    <transformation>x y z a0 a1 a2</transformation> of a SKEL file (XmlHelpers.cpp:346-379)."""
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    return np.array([[cy * cz, -cy * sz, sy],
                     [cx * sz + cz * sx * sy, cx * cz - sx * sy * sz, -cy * sx],
                     [sx * sz - cx * cz * sy, cz * sx + cx * sy * sz, cx * cy]])


def _skel_T(el, tag="transformation"):
    t = el.find(tag) if el is not None else None
    if t is None or t.text is None:
        return np.eye(4)
    v = [float(x) for x in t.text.split()]
    return make_transform(v[:3], R=euler_xyz_to_matrix(v[3:6]))


def _text(el, tag, default=None, cast=float):
    t = el.find(tag) if el is not None else None
    return default if t is None or t.text is None else cast(t.text.strip())


def _shape_inertia(geom, mass):
    """Diagonal of Shape::computeInertia(mass) for a SKEL <geometry> element, shape kinds in readShape's order of tests
    (SkelParser.cpp:1277-1316); None for a kind outside the list (plane, multi_sphere, mesh...)."""
    def nums(e, tag):
        return [float(x) for x in e.find(tag).text.split()]
    e = geom.find("sphere")
    if e is not None:                                # SphereShape.cpp:91-100
        r, = nums(e, "radius")
        return (2.0 / 5.0 * mass * r ** 2,) * 3
    e = geom.find("box")
    if e is not None:                                # BoxShape.cpp:74-83
        x, y, z = nums(e, "size")
        return (mass / 12.0 * (y ** 2 + z ** 2), mass / 12.0 * (x ** 2 + z ** 2), mass / 12.0 * (x ** 2 + y ** 2))
    e = geom.find("ellipsoid")
    if e is not None:                                # EllipsoidShape.cpp:125-140 (size = diameters)
        a, bb, c = (x ** 2 for x in nums(e, "size"))
        return (mass / 20.0 * (bb + c), mass / 20.0 * (a + c), mass / 20.0 * (a + bb))
    e = geom.find("cylinder")
    if e is not None:                                # CylinderShape.cpp:104-113
        (r,), (h,) = nums(e, "radius"), nums(e, "height")
        ixx = mass * (3.0 * r ** 2 + h ** 2) / 12.0
        return (ixx, ixx, 0.5 * mass * r * r)
    e = geom.find("capsule")
    if e is not None:                                # CapsuleShape.cpp:107-131
        (r,), (h,) = nums(e, "radius"), nums(e, "height")
        v_cyl, v_sph = np.pi * r * r * h, 4.0 / 3.0 * np.pi * r ** 3
        m_cyl, m_sph = mass * v_cyl / (v_cyl + v_sph), mass * v_sph / (v_cyl + v_sph)
        ixx = m_cyl * (h * h / 12.0 + r * r / 4.0) + m_sph * (h * h + 3.0 / 8.0 * h * r + 0.4 * r * r)
        return (ixx, ixx, m_cyl * (r * r / 2.0) + m_sph * (0.4 * r * r))
    e = geom.find("cone")
    if e is not None:                                # ConeShape.cpp:106-117
        (r,), (h,) = nums(e, "radius"), nums(e, "height")
        ixx = (3.0 / 20.0) * mass * (r * r + (2.0 / 3.0) * h * h)
        return (ixx, ixx, (3.0 / 10.0) * mass * r * r)
    return None


def load_skel(path, name=None, skeletons=None, max_contacts=None, drop_unsupported_colliders=False, immobile="weld"):
    """Parse a SKEL world (`<skel><world>`: physics + skeletons) into ONE ModelDescription (all skeletons of the world in one
    model, like `with_ground`).  `skeletons`: names of the skeletons to keep (default: all), in file order.  Collision shapes other than
    boxes, spheres (isotropic ellipsoids) and capsules that only meet capsules / spheres raise unless `drop_unsupported_colliders` (the body is then loaded without that collider).

    Subset, following SkelParser.cpp: <physics> time_step / gravity (:520-560); per <body> name, <transformation> = the body's
    WORLD transform at the zero configuration (:1082-1092), <inertia> mass / offset / moment_of_inertia (:1095-1128; without a
    moment the first shape's inertia for that mass, :618-645; without <inertia> the BodyNode defaults mass 1, I = 1),
    <collision_shape> box / isotropic ellipsoid (= sphere) with its <transformation> in the body frame; per <joint> type
    weld / revolute / prismatic / free and the compound types euler (xyz, zyx) / universal / translational / translational2d /
    planar (expanded into 1-DOF chains by ModelDescription), <parent> ("world" = none) / <child>, <transformation> = T_ChildBodyToJoint and
    T_ParentBodyToJoint = parentWorld^-1 childWorld childToJoint (:1540-1552), <axis> xyz, damping (under <axis> or
    <axis><dynamics>), spring_stiffness / spring_rest_position, <limit> lower / upper (:1870-1960).  Bodies are emitted
    parents-before-children in the file's joint order, which is the skeleton's DOF order.  Ball joints and the
    <dof> elements of every joint type are read too; a file without <world> is a skeleton file.  Soft bodies, meshes, screw joints and
    <init_pos> / <init_vel> (a state, not a model constant) are outside the subset: unsupported joints raise.
    `immobile`: a skeleton with <mobile>false</mobile> (Skeleton::setMobile, SkelParser.cpp:958-964: World::step skips its dynamics,
    World.cpp:221-254, and its bodies are not reactive in contacts, BodyNode.cpp:2394-2400 - the ground of cartpole.skel / fullbody1.skel) is
    loaded WELDED to the world at its zero configuration ("weld": what the reference's world does with it as long as nobody gives it a
    velocity; its joint coordinates are then not part of the state vector, the one difference to the reference's World) or refused ("error").
    `max_contacts`: contact slots per world (<= 128: up to 8 the 24-row build, up to 16 the 48-row build, beyond that the general one with 64 or 128 slots);
    None = ModelDescription.suggest_max_contacts() (by what the collider pairs can hold)."""
    root = ET.parse(path).getroot()
    world = root.find("world")
    if world is None:
        # a skeleton file (SkelParser::readSkeleton, :433-460): <skeleton> elements directly under <skel>; the world they are added to has the
        # defaults of World's constructor (dt 1e-3, gravity (0, -9.81, 0), World.cpp:76-99)
        if root.find("skeleton") is None:
            raise ValueError(f"{path}: neither a <world> nor a <skeleton>")
        world = root
    phys = world.find("physics")
    dt = _text(phys, "time_step", 1e-3)
    g = phys.find("gravity") if phys is not None else None
    gravity = tuple(float(x) for x in g.text.split()) if g is not None else (0.0, -9.81, 0.0)
    bodies, boxes = [], []
    welded_dofs = []      # (skeleton, joint, DOFs) of every joint of an immobile skeleton: coordinates the reference's state vector has and this one does not
    ref_dof_mobile = []   # the reference World's coordinates in ITS order (skeleton by skeleton, joint by joint): True = one of this model's
    immobile_skeletons = []   # skeleton ids (BodySpec.skeleton) of the immobile skeletons: their bodies carry no entry of an IKMapping (mapping.py)
    for sk_index, sk in enumerate(world.findall("skeleton")):
        if skeletons is not None and sk.get("name") not in skeletons:
            continue
        skel_T = _skel_T(sk)                                     # optional skeleton frame (:948-955)
        mob = sk.find("mobile")
        is_mobile = mob is None or (mob.text or "").strip().lower() not in ("false", "0")   # (an empty <mobile/> reads as mobile, like the reference's default)
        if not is_mobile and immobile != "weld":
            raise ValueError(f"{path}: skeleton {sk.get('name')} is immobile (<mobile>false</mobile>); immobile=\"weld\" loads it welded to the world")
        if not is_mobile:
            immobile_skeletons.append(sk_index)
        bel = {b.get("name"): b for b in sk.findall("body")}
        for bn, b_ in bel.items():
            if b_.find("soft_shape") is not None:
                # readSoftBodyNode (SkelParser.cpp:285-, called from :972): a SoftBodyNode with point masses and its own dynamics, nothing of it is rigid-body ABA
                raise ValueError(f"{path}: body {bn} is a soft body (<soft_shape>): outside the hot-path scope")
        Tw = {n: skel_T @ _skel_T(b) for n, b in bel.items()}
        joints = sk.findall("joint")
        child_joint = {j.find("child").text.strip(): j for j in joints}
        index = {}

        def shapes_of(b):
            out = []
            for cs in b.findall("collision_shape"):
                geom = cs.find("geometry")
                box = geom.find("box") if geom is not None else None
                ell = geom.find("ellipsoid") if geom is not None else None
                sph = geom.find("sphere") if geom is not None else None
                cap = geom.find("capsule") if geom is not None else None
                if box is not None:
                    out.append(("box", tuple(float(x) for x in box.find("size").text.split()), _skel_T(cs)))
                elif cap is not None:      # CapsuleShape(radius, height), axis = z of the shape frame (SkelParser.cpp:1302-1308)
                    out.append(("capsule", (float(cap.find("radius").text), float(cap.find("height").text), 0.0), _skel_T(cs)))
                elif sph is not None:
                    r = float(sph.find("radius").text)
                    out.append(("sphere", (r, r, r), _skel_T(cs)))
                elif ell is not None:
                    d = tuple(float(x) for x in ell.find("size").text.split())
                    if max(d) - min(d) > 1e-12 * max(d):
                        raise ValueError(f"{path}: anisotropic ellipsoid collider outside the analytic narrow phase")
                    out.append(("sphere", (d[0] / 2,) * 3, _skel_T(cs)))
                elif geom is not None and len(geom) and not drop_unsupported_colliders:
                    # cylinder / mesh / ...: the reference collides them through libccd or its mesh code; loading the body without
                    # its collider would silently change the physics (it falls through the ground)
                    raise ValueError(f"{path}: {geom[0].tag} collider on body {b.get('name')} is outside the analytic narrow phases (box, sphere); "
                                     "drop_unsupported_colliders=True loads the model without it")
            return out

        def inertial(b):
            ine = b.find("inertia")
            if ine is None:
                return 1.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)
            mass = _text(ine, "mass", 1.0)
            off = ine.find("offset")
            com = tuple(float(x) for x in off.text.split()) if off is not None else (0.0, 0.0, 0.0)
            moi = ine.find("moment_of_inertia")
            if moi is not None:
                I6 = tuple(_text(moi, k, 0.0) for k in ("ixx", "iyy", "izz", "ixy", "ixz", "iyz"))
            else:
                I6 = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)
                # the inertia of the body's FIRST ShapeNode for this mass (:618-645); visualization shapes are read before collision
                # shapes (:612-616), so that is the first <visualization_shape> when there is one - whether or not the shape is one
                # the device can collide
                first = b.find("visualization_shape")
                if first is None:
                    first = b.find("collision_shape")
                geom = first.find("geometry") if first is not None else None
                if geom is not None:
                    d = _shape_inertia(geom, mass)
                    if d is None and len(geom):
                        raise ValueError(f"{path}: default inertia of body {b.get('name')} from a {geom[0].tag} shape is outside the subset")
                    if d is not None:
                        I6 = d + (0.0, 0.0, 0.0)
            return mass, com, I6

        # Assembly order = body and DOF order of the reference (readSkeleton :999-1040 with getNextJointAndNodePair :753-805): take the
        # lowest remaining joint in file order; if its parent body does not exist yet, create the parent's joint first (and that one's
        # missing ancestors before it), then go on from the lowest remaining joint.
        pending = list(joints)
        creating = set()
        while pending:
            j = pending[0]
            while True:                                          # hoist the missing ancestors
                pn = j.find("parent").text.strip()
                if pn == "world" or pn in index:
                    break
                if pn not in child_joint or pn in creating:
                    raise ValueError(f"{path}: joints of skeleton {sk.get('name')} do not form a tree rooted in the world "
                                     f"(parent body {pn} of joint {j.get('name')})")
                creating.add(pn)
                j = child_joint[pn]
            creating.clear()
            if True:
                pn = j.find("parent").text.strip()
                cn = j.find("child").text.strip()
                jt = j.get("type")
                c2j = _skel_T(j)
                parentW = np.eye(4) if pn == "world" else Tw[pn]
                T_pj = np.linalg.inv(parentW) @ Tw[cn] @ c2j
                kw = {}

                def axis_props(k):
                    """damping / spring / rest / limits of <axis>, <axis2>, ... (readJointDynamicsAndLimit, :1870-1960): per-DOF
                    lists of length k with the reference's defaults where an element is missing."""
                    inf = float("inf")
                    P = {"damping": [0.0] * k, "spring": [0.0] * k, "rest": [0.0] * k, "pos_lo": [-inf] * k, "pos_hi": [inf] * k,
                         "coulomb_friction": [0.0] * k}
                    for i in range(k):
                        ax = j.find("axis" if i == 0 else f"axis{i + 1}")
                        if ax is None:
                            continue
                        damp = _text(ax, "damping", None)
                        dyn = ax.find("dynamics")
                        if dyn is not None:
                            damp = _text(dyn, "damping", damp)
                            P["coulomb_friction"][i] = _text(dyn, "friction", 0.0)   # (SkelParser.cpp:1921-1925)
                            P["spring"][i] = _text(dyn, "spring_stiffness", 0.0)
                            P["rest"][i] = _text(dyn, "spring_rest_position", 0.0)
                        if damp is not None:
                            P["damping"][i] = damp
                        lim = ax.find("limit")
                        if lim is not None:
                            P["pos_lo"][i] = _text(lim, "lower", -inf)
                            P["pos_hi"][i] = _text(lim, "upper", inf)
                    dflt = {"damping": 0.0, "spring": 0.0, "rest": 0.0, "pos_lo": -inf, "pos_hi": inf, "coulomb_friction": 0.0}
                    return {key: tuple(v) for key, v in P.items() if any(x != dflt[key] for x in v)}   # all-default: leave unset

                def plane_axes():
                    """<plane type="xy|yz|zx|arbitrary"> of planar / translational2d joints (:2351-2500; missing: the XY plane)"""
                    pl = j.find("plane")
                    kind = pl.get("type") if pl is not None else "xy"
                    E = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0)}
                    if kind == "arbitrary":
                        return [tuple(float(x) for x in pl.find(f"translation_axis{i}/xyz").text.split()) for i in (1, 2)]
                    return [E[kind[0]], E[kind[1]]] if kind in ("xy", "yz", "zx") else [E["x"], E["y"]]

                axis = (0.0, 0.0, 1.0)
                if jt in ("revolute", "prismatic"):
                    ax = j.find("axis")
                    axis = tuple(float(x) for x in ax.find("xyz").text.split())
                    kw.update(axis_props(1))
                    jtype = jt
                elif jt == "euler":
                    order = j.find("axis_order").text.strip().lower()
                    if order not in ("xyz", "zyx"):
                        raise ValueError(f"{j.get('name')}: Euler axis order {order} (the reference's SKEL reader knows xyz and zyx, :2259-2283)")
                    jtype = "euler_" + order
                    kw.update(axis_props(3))
                elif jt == "universal":
                    jtype = "universal"
                    kw["axes"] = [tuple(float(x) for x in j.find(a).find("xyz").text.split()) for a in ("axis", "axis2")]
                    kw.update(axis_props(2))
                elif jt == "translational":
                    jtype = "translational"
                    kw.update(axis_props(3))
                elif jt in ("translational2d", "planar"):
                    jtype = jt
                    kw["axes"] = plane_axes()
                    kw.update(axis_props(2 if jt == "translational2d" else 3))
                elif jt == "weld":
                    jtype = "weld"
                elif jt == "free":
                    jtype = "free"
                elif jt == "screw":
                    ax = j.find("axis")                      # readScrewJoint (:2085-2150): <axis><xyz/><pitch/> + the per-axis dynamics
                    axis = tuple(float(x) for x in ax.find("xyz").text.split())
                    kw.update(axis_props(1))
                    if ax.find("pitch") is not None:
                        kw["pitch"] = float(ax.find("pitch").text)
                    jtype = "screw"
                elif jt == "ball":
                    jtype = "ball"              # readBallJoint (:2226-2256): init_pos / init_vel (states are the caller's here) + <dof> elements
                else:
                    raise ValueError(f"{j.get('name')}: joint type {jt} outside scope")
                # <dof local_index="i"> elements (readAllDegreesOfFreedom / readDegreeOfFreedom, :1713-1866) are read last and override the
                # per-axis values: limits as attributes of <position> / <velocity> / <force>, damping / spring as child elements
                ndofs = {"weld": 0, "free": 6, "ball": 3, "universal": 2, "translational": 3, "translational2d": 2, "planar": 3}.get(
                    jtype, 3 if jtype.startswith("euler_") else 1)
                dofs = j.findall("dof")
                if dofs and ndofs > 0:
                    inf = float("inf")
                    dflt = {"damping": 0.0, "spring": 0.0, "rest": 0.0, "pos_lo": -inf, "pos_hi": inf, "vel_lo": -inf, "vel_hi": inf,
                            "force_lo": -inf, "force_hi": inf, "coulomb_friction": 0.0}
                    P = {key: list(kw.get(key, ())) or [dflt[key]] * ndofs for key in dflt}
                    for de in dofs:
                        li = de.get("local_index")
                        if li is None:
                            if ndofs > 1:
                                continue                                  # the reference reports an error and skips the element
                            li = 0
                        li = int(li)
                        if li >= ndofs:
                            continue
                        for tag, lo, hi in (("position", "pos_lo", "pos_hi"), ("velocity", "vel_lo", "vel_hi"), ("force", "force_lo", "force_hi")):
                            el = de.find(tag)
                            if el is not None:
                                if el.get("lower") is not None:
                                    P[lo][li] = float(el.get("lower"))
                                if el.get("upper") is not None:
                                    P[hi][li] = float(el.get("upper"))
                        for tag, key in (("damping", "damping"), ("spring_rest_position", "rest"), ("spring_stiffness", "spring")):
                            if de.find(tag) is not None:
                                P[key][li] = float(de.find(tag).text)
                        if de.find("friction") is not None:                # (SkelParser.cpp:1858-1859)
                            P["coulomb_friction"][li] = float(de.find("friction").text)
                    for key, vals in P.items():
                        if any(x != dflt[key] for x in vals):
                            kw[key] = tuple(vals)
                        else:
                            kw.pop(key, None)
                ref_dof_mobile.extend([bool(is_mobile)] * int(ndofs))
                if not is_mobile:                 # an immobile skeleton: every joint frozen at its zero configuration
                    if ndofs:
                        welded_dofs.append((sk.get("name"), j.get("name"), int(ndofs)))
                    jtype, kw, axis = "weld", {}, (0.0, 0.0, 1.0)
                mass, com, I6 = inertial(bel[cn])
                base = len(bodies)
                bodies.append(BodySpec(cn, -1 if pn == "world" else index[pn], jtype, j.get("name"), axis=axis, T_pj=T_pj, T_cj=c2j,
                                       mass=mass, com=com, inertia=I6, skeleton=sk_index, **kw))
                index[cn] = base
                for kind, size, Ts in shapes_of(bel[cn]):
                    boxes.append(BoxSpec(base, Ts, size, 1.0, kind))
                pending.remove(j)
        missing = set(bel) - set(child_joint)
        if missing:
            raise ValueError(f"{path}: bodies without a parent joint: {sorted(missing)}")
    if name is None:
        name = os.path.splitext(os.path.basename(path))[0]
    md = ModelDescription(name, bodies, boxes, gravity, dt, None, max_contacts=(max_contacts or 0) if boxes else 0)
    # coordinates of immobile skeletons: part of the reference World's getPositions() / state vector, NOT of this model's (loaded welded).
    # Callers porting reference state vectors must drop them: md.welded_dofs lists them in the reference's order; warned about once per load.
    # Round 6: they STAY in the drop-in surface's state vector (World.getStateSize / setState / getState, timestep(): the reference's layout,
    # nimblephysics_amd/ref_layout.py) as frozen coordinates - identity rows of the step's Jacobians - which must sit at zero, where the
    # skeleton was welded; only the raw SoA entry points (step_soa, ...) see the device's shorter vector.
    md.welded_dofs = welded_dofs
    md.ref_dof_mobile = ref_dof_mobile if welded_dofs else None
    md.immobile_skeletons = immobile_skeletons
    if welded_dofs:
        import warnings
        warnings.warn(f"{path}: {sum(d for _, _, d in welded_dofs)} coordinate(s) of immobile skeleton(s) "
                      f"{sorted({s_ for s_, _, _ in welded_dofs})} are frozen at zero: part of the state vector of World / timestep() like in the "
                      "reference (ModelDescription.welded_dofs, ref_dof_mobile), not of the device's SoA entry points", stacklevel=2)
    if boxes and max_contacts is None:          # (not said: by what the collider pairs of the world can hold, ModelDescription.suggest_max_contacts)
        md.max_contacts = md.suggest_max_contacts()
    if md.capsule_meets_box():
        # capsule-capsule and capsule-sphere pairs are closed form (DARTCollide.cpp:4183-4420); capsule-box is libccd's MPR (:4422-4645)
        if not drop_unsupported_colliders:
            raise ValueError(f"{path}: a capsule collider can meet a box collider, a pair outside the analytic narrow phases; "
                             "drop_unsupported_colliders=True loads the model without its capsule colliders")
        md.boxes = [bx for bx in md.boxes if bx.shape != "capsule"]
    return md


def load_model(path, **kw):
    """A ModelDescription from a .skel or .urdf file, by extension (the file kinds nimble.loadWorld / UniversalLoader accept on this path)."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".skel":
        return load_skel(path, **kw)
    if ext == ".urdf":
        return load_urdf(path, **kw)
    raise ValueError(f"{path}: unknown model file type {ext!r} (.skel, .urdf)")


def loadWorld(path, device="cuda:0", **kw):
    """nimble.loadWorld(path) for this path: the batched World of the file's model on `device`."""
    from .world import World
    return World(load_model(path, **kw), device=device)

