"""TEST INFRASTRUCTURE: an independent reference of the rigid-body physics, in
np.longdouble, built on tests/mjcf_indep.py (world-frame quantities at qpos0).
It never reads the product's compiled record and shares no recursion with the
oracle (oracle/mjsub.c) or the device code: no body-frame recursion, no
composite-rigid-body pass, no recursive Newton-Euler, no sparse LDL.

  kinematics   product of exponentials in the world frame: a body's pose at q is
               its qpos0 pose moved by the screw of each ancestor dof, root to leaf
  Jacobians    world frame, column by column; the free joint follows MuJoCo's
               convention (linear velocity in the world frame, angular in the body frame);
               a ball joint is three rotational dofs about the axes of its body's frame,
               anchored at the joint's world position, all carried by the ancestors' dofs
               and by the ball's own rotation
  M(q)         sum_b m_b Jp_b'Jp_b + Jr_b' I_b(q) Jr_b + diag(armature)
  c(q, v)      sum_b m_b Jp_b'(Jp_b_dot v - g) + Jr_b'(I_b Jr_b_dot v + w_b x I_b w_b)
  qacc_smooth  M^-1 tau by Gaussian elimination with partial pivoting
  integrators  Euler with MuJoCo's implicit damping, RK4 stage by stage (valid
               only while no constraint is active; asserted); free and ball quaternions
               advance by the exponential of the body-frame angular velocity
  collisions   plane/sphere/capsule pairs; capsule-capsule by enumeration
  constraints  limit and contact rows, D, aref; the convex cost and its exact
               minimiser by an active-set Newton iteration

Every function works in the dtype the Ref was made with, so the same formulas
run in float64 measure the reference's own rounding (E64 in the tests).

MuJoCo conventions that are not physics are restated here and marked
"convention": a ball joint carries damping and armature but neither a spring
nor a limit (the product refuses both), the contact point at half the penetration, the tangent frame of a
contact, two contacts for exactly parallel capsules, the order of rows.
"""
import numpy as np

import mjcf_indep as mi

MINVAL = 1e-15           # MuJoCo's mjMINVAL
MINIMP, MAXIMP = 1e-4, 0.9999


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]],
                    dtype=a.dtype)


def rodrigues(axis, angle):
    """rotation by angle about the unit axis"""
    dt = axis.dtype
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=dt)
    return np.eye(3, dtype=dt) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def solve(A, b):
    """A x = b by Gaussian elimination with partial pivoting, in A's dtype"""
    A = np.array(A, dtype=A.dtype)
    x = np.array(b, dtype=A.dtype)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            x[[k, p]] = x[[p, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            if f != 0:
                A[i, k:] -= f * A[k, k:]
                x[i] -= f * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def segment_segment(c1, a1, c2, a2):
    """closest points of the segments c1 + s a1 and c2 + t a2, s, t in [-1, 1],
    by enumeration: the interior stationary point, the four edges (one parameter
    at a bound, the other stationary inside), the four corners.  The squared
    distance is convex, so the smallest valid candidate is the minimum.
    Returns (s, t, region); region is one of "interior", "edge_s+", "edge_s-",
    "edge_t+", "edge_t-", "corner_++", "corner_+-", "corner_-+", "corner_--"."""
    d = c1 - c2
    A, B, Cc = a1 @ a1, a1 @ a2, a2 @ a2
    u, w = a1 @ d, a2 @ d
    cand = []
    det = A * Cc - B * B
    if det != 0:
        s, t = (B * w - Cc * u) / det, (A * w - B * u) / det
        if abs(s) < 1 and abs(t) < 1:
            cand.append((s, t, "interior"))
    one = A / A
    for sg, nm in ((one, "+"), (-one, "-")):
        t = (w + sg * B) / Cc       # d/dt |d + sg a1 - t a2|^2 = 0
        if abs(t) < 1:
            cand.append((sg, t, "edge_s" + nm))
        s = (sg * B - u) / A        # d/ds |d + s a1 - sg a2|^2 = 0
        if abs(s) < 1:
            cand.append((s, sg, "edge_t" + nm))
        for tg, nm2 in ((one, "+"), (-one, "-")):
            cand.append((sg, tg, "corner_" + nm + nm2))
    best = None
    for s, t, nm in cand:
        r = d + s * a1 - t * a2
        f = r @ r
        if best is None or f < best[0]:
            best = (f, s, t, nm)
    return best[1], best[2], best[3]


class Ref:
    def __init__(self, C, dtype=np.longdouble):
        self.C, self.dt = C, dtype
        T = self.T = lambda x: np.array(x, dtype=dtype)
        self.nb, self.nv, self.nq = C.nbody, C.nv, C.nq
        self.parent = [b["parent"] for b in C.bodies]
        self.mass, self.com0, self.I0 = T(C.body_mass), T(C.body_com), T(C.body_I)
        self.bpos0 = T([b["gpos"] for b in C.bodies])
        self.grav, self.h = T(C.gravity), dtype(C.timestep)
        self.qpos0 = T(C.qpos0)
        # joints: qpos / dof address; dofs: the chain that carries each axis
        self.jq, self.jd, self.bjoints = [], [], [[] for _ in range(self.nb)]
        aq = ad = 0
        for ji, j in enumerate(C.joints):
            assert j["type"] in ("free", "ball", "hinge", "slide")
            if j["type"] == "ball":   # convention: the product simulates neither, and refuses both
                assert not j["limited"] and j["stiffness"] == 0, "a ball joint with a limit or a spring"
            self.jq.append(aq)
            self.jd.append(ad)
            self.bjoints[j["body"]].append(ji)
            aq += {"free": 7, "ball": 4}.get(j["type"], 1)
            ad += {"free": 6, "ball": 3}.get(j["type"], 1)
        self.R0 = T([mi.qmat(b["gquat"]) for b in C.bodies])   # body frames at qpos0, world
        self.chain = [[] for _ in range(self.nb)]   # dofs that move body b, root to leaf
        self.carr = [None] * self.nv                # dofs that move the axis / anchor of dof i
        self.rot = [False] * self.nv
        for b in range(1, self.nb):
            ch = list(self.chain[self.parent[b]])
            for ji in self.bjoints[b]:
                d0 = self.jd[ji]
                if C.joints[ji]["type"] == "free":
                    for k in range(3):       # world axes: carried by nothing
                        self.carr[d0 + k] = list(ch)
                    for k in range(3, 6):    # body axes: carried by the whole joint
                        self.carr[d0 + k] = ch + list(range(d0, d0 + 6))
                        self.rot[d0 + k] = True
                    ch += list(range(d0, d0 + 6))
                elif C.joints[ji]["type"] == "ball":
                    # the body's frame after the joint's rotation: no later joint may turn it again
                    assert ji == self.bjoints[b][-1], "a ball joint must be the last joint of its body"
                    ch += list(range(d0, d0 + 3))
                    for k in range(3):       # body axes: carried by the ancestors and the ball itself
                        self.carr[d0 + k] = list(ch)
                        self.rot[d0 + k] = True
                else:
                    ch.append(d0)
                    self.carr[d0] = list(ch)
                    self.rot[d0] = C.joints[ji]["type"] == "hinge"
            self.chain[b] = ch
        self.armature = T([C.joints[j]["armature"] for j in C.dof_joint])
        self.damping = T([C.joints[j]["damping"] for j in C.dof_joint])
        # welded bodies (no joint of their own) collide as their ancestor
        self.weld = [0] * self.nb
        for b in range(1, self.nb):
            self.weld[b] = b if self.bjoints[b] else self.weld[self.parent[b]]
        self.gaxis0 = T([mi.qmat(g["gquat"])[:, 2] for g in C.geoms])
        self.gpos0 = T([g["gpos"] for g in C.geoms])

    # ---------------------------------------------------------------- kinematics
    def kin(self, q):
        """poses as displacements (R, p) of the qpos0 configuration: a point x0
        of body b at qpos0 is at R[b] x0 + p[b]"""
        dt, C = self.dt, self.C
        q = self.T(q)
        R = [np.eye(3, dtype=dt) for _ in range(self.nb)]
        p = [np.zeros(3, dtype=dt) for _ in range(self.nb)]
        ax = [None] * self.nv
        an = [None] * self.nv
        for b in range(1, self.nb):
            Rb, pb = R[self.parent[b]], p[self.parent[b]]
            for ji in self.bjoints[b]:
                j, qa, da = C.joints[ji], self.jq[ji], self.jd[ji]
                if j["type"] == "free":
                    Rq = mi.qmat(q[qa + 3:qa + 7])
                    Rb = Rq @ mi.qmat(self.qpos0[qa + 3:qa + 7]).T
                    pb = q[qa:qa + 3] - Rb @ self.qpos0[qa:qa + 3]
                    for k in range(3):
                        ax[da + k] = np.eye(3, dtype=dt)[k]
                        an[da + k] = q[qa:qa + 3].copy()
                        ax[da + 3 + k] = Rq[:, k].copy()
                        an[da + 3 + k] = q[qa:qa + 3].copy()
                    continue
                if j["type"] == "ball":    # T <- T o E0, E0 the body-frame rotation about r0, seen at qpos0
                    r0, R0 = self.T(j["gpos"]), self.R0[b]
                    quat = q[qa:qa + 4] / np.sqrt(q[qa:qa + 4] @ q[qa:qa + 4])
                    E = R0 @ mi.qmat(quat).astype(dt) @ R0.T
                    anchor = Rb @ r0 + pb
                    pb = Rb @ (r0 - E @ r0) + pb
                    Rb = Rb @ E
                    for k in range(3):
                        ax[da + k], an[da + k] = (Rb @ R0)[:, k].copy(), anchor.copy()
                    continue
                a0, r0 = self.T(j["gaxis"]), self.T(j["gpos"])
                a0 = a0 / np.sqrt(a0 @ a0)
                ax[da], an[da] = Rb @ a0, Rb @ r0 + pb
                th = q[qa] - self.qpos0[qa]
                if j["type"] == "hinge":   # T <- T o E0, E0 the rotation about (a0, r0)
                    E = rodrigues(a0, th)
                    pb = Rb @ (r0 - E @ r0) + pb
                    Rb = Rb @ E
                else:
                    pb = pb + (Rb @ a0) * th
            R[b], p[b] = Rb, pb
        K = type("Kin", (), {})()
        K.R, K.p, K.ax, K.an = R, p, ax, an
        K.com = [R[b] @ self.com0[b] + p[b] for b in range(self.nb)]
        K.xpos = [R[b] @ self.bpos0[b] + p[b] for b in range(self.nb)]
        K.I = [R[b] @ self.I0[b] @ R[b].T for b in range(self.nb)]
        return K

    def jac(self, K, b, x):
        """(Jp, Jr) of the point x carried by body b"""
        Jp, Jr = np.zeros((3, self.nv), dtype=self.dt), np.zeros((3, self.nv), dtype=self.dt)
        for i in self.chain[b]:
            if self.rot[i]:
                Jr[:, i] = K.ax[i]
                Jp[:, i] = cross(K.ax[i], x - K.an[i])
            else:
                Jp[:, i] = K.ax[i]
        return Jp, Jr

    def axis_rates(self, K, v):
        """per dof: the rate of its axis (w x a, w the angular velocity of what
        carries it) and the velocity of its anchor"""
        adot, rdot = [None] * self.nv, [None] * self.nv
        for i in range(self.nv):
            w, rd = np.zeros(3, dtype=self.dt), np.zeros(3, dtype=self.dt)
            for j in self.carr[i]:
                if self.rot[j]:
                    w = w + K.ax[j] * v[j]
                    rd = rd + cross(K.ax[j], K.an[i] - K.an[j]) * v[j]
                else:
                    rd = rd + K.ax[j] * v[j]
            adot[i], rdot[i] = cross(w, K.ax[i]), rd
        return adot, rdot

    def jac_dot(self, K, rates, b, x, xdot):
        """closed-form time derivative of jac(K, b, x), the point moving with b at xdot"""
        adot, rdot = rates
        Jpd, Jrd = np.zeros((3, self.nv), dtype=self.dt), np.zeros((3, self.nv), dtype=self.dt)
        for i in self.chain[b]:
            if self.rot[i]:
                Jrd[:, i] = adot[i]
                Jpd[:, i] = cross(adot[i], x - K.an[i]) + cross(K.ax[i], xdot - rdot[i])
            else:
                Jpd[:, i] = adot[i]
        return Jpd, Jrd

    # ---------------------------------------------------------------- dynamics
    def mass_matrix(self, K):
        M = np.diag(self.armature).astype(self.dt)
        for b in range(1, self.nb):
            Jp, Jr = self.jac(K, b, K.com[b])
            M = M + self.mass[b] * (Jp.T @ Jp) + Jr.T @ K.I[b] @ Jr
        return M

    def bias(self, K, v):
        v = self.T(v)
        c = np.zeros(self.nv, dtype=self.dt)
        rates = self.axis_rates(K, v)
        for b in range(1, self.nb):
            Jp, Jr = self.jac(K, b, K.com[b])
            Jpd, Jrd = self.jac_dot(K, rates, b, K.com[b], Jp @ v)
            w = Jr @ v
            c = c + self.mass[b] * (Jp.T @ (Jpd @ v - self.grav)) + Jr.T @ (K.I[b] @ (Jrd @ v) + cross(w, K.I[b] @ w))
        return c

    def passive(self, q, v):
        """-k (q - q_spring) - d v; MJCF's springref is the joint value at which
        the spring rests (a hinge's in the compiler's angle unit), not an offset from ref"""
        q, v = self.T(q), self.T(v)
        f = -self.damping * v
        for ji, j in enumerate(self.C.joints):
            if j["type"] in ("free", "ball") or j["stiffness"] == 0:
                continue
            spring = self.dt(j["springref"] * (self.C.angle_unit if j["type"] == "hinge" else 1.0))
            f[self.jd[ji]] -= self.dt(j["stiffness"]) * (q[self.jq[ji]] - spring)
        return f

    def actuation(self, ctrl):
        f = np.zeros(self.nv, dtype=self.dt)
        for a, u in zip(self.C.act, self.T(ctrl)):
            if a["ctrllimited"]:
                u = min(max(u, self.dt(a["ctrlrange"][0])), self.dt(a["ctrlrange"][1]))
            frc = self.dt(a["gear"][0]) * u
            if a["forcelimited"]:
                frc = min(max(frc, self.dt(a["forcerange"][0])), self.dt(a["forcerange"][1]))
            f[self.jd[a["joint"]]] += frc
        return f

    def applied(self, K, qfrc_applied, xfrc_applied):
        """qfrc_applied plus xfrc_applied: per body a force at the COM and a torque, world frame"""
        f = np.zeros(self.nv, dtype=self.dt) if qfrc_applied is None else self.T(qfrc_applied).copy()
        if xfrc_applied is not None:
            X = self.T(xfrc_applied).reshape(self.nb, 6)
            for b in range(1, self.nb):
                if np.any(X[b] != 0):
                    Jp, Jr = self.jac(K, b, K.com[b])
                    f = f + Jp.T @ X[b, :3] + Jr.T @ X[b, 3:]
        return f

    def forward(self, q, v, ctrl, qfrc_applied=None, xfrc_applied=None):
        """the unconstrained dynamics at one state"""
        K = self.kin(q)
        o = type("Fwd", (), {})()
        o.K, o.q, o.v = K, self.T(q), self.T(v)
        o.xpos = np.array(K.xpos, dtype=self.dt)
        o.M = self.mass_matrix(K)
        o.bias = self.bias(K, v)
        o.tau = (-o.bias + self.passive(q, v) + self.actuation(ctrl)
                 + self.applied(K, qfrc_applied, xfrc_applied))
        o.qacc_smooth = solve(o.M, o.tau)
        return o

    # ---------------------------------------------------------------- integration
    def integrate_pos(self, q, v, h):
        """q (+) h v; a free or ball joint's quaternion by the exponential of the body-frame angular velocity"""
        q, v = self.T(q).copy(), self.T(v)
        for ji, j in enumerate(self.C.joints):
            qa, da = self.jq[ji], self.jd[ji]
            if j["type"] not in ("free", "ball"):
                q[qa] += h * v[da]
                continue
            if j["type"] == "free":
                q[qa:qa + 3] += h * v[da:da + 3]
                qa, da = qa + 3, da + 3
            w = v[da:da + 3]
            n = np.sqrt(w @ w)
            quat = q[qa:qa + 4] / np.sqrt(q[qa:qa + 4] @ q[qa:qa + 4])
            if n > 0:
                ang = h * n
                quat = mi.qmul(quat, np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * w / n]).astype(self.dt))
            q[qa:qa + 4] = quat
        return q

    def _free_qacc(self, q, v, ctrl, qf, xf):
        nl, con = self.active(q)
        assert nl == 0 and con == 0, f"the reference integrator met a constraint ({nl} limit rows, {con} contacts)"
        return self.forward(q, v, ctrl, qf, xf)

    def step(self, q, v, ctrl, qfrc_applied=None, xfrc_applied=None, nstep=1):
        """nstep steps of the model's integrator; asserts that no constraint is ever active"""
        q, v, h = self.T(q), self.T(v), self.h
        for _ in range(nstep):
            if self.C.integrator == 0:
                f = self._free_qacc(q, v, ctrl, qfrc_applied, xfrc_applied)
                # implicit in the joint damping: (M + h D) dv = h M qacc
                v = v + h * solve(f.M + h * np.diag(self.damping), f.M @ f.qacc_smooth)
                q = self.integrate_pos(q, v, h)
            else:
                a1 = self._free_qacc(q, v, ctrl, qfrc_applied, xfrc_applied).qacc_smooth
                v2 = v + (h / 2) * a1
                a2 = self._free_qacc(self.integrate_pos(q, v, h / 2), v2, ctrl, qfrc_applied, xfrc_applied).qacc_smooth
                v3 = v + (h / 2) * a2
                a3 = self._free_qacc(self.integrate_pos(q, v2, h / 2), v3, ctrl, qfrc_applied, xfrc_applied).qacc_smooth
                v4 = v + h * a3
                a4 = self._free_qacc(self.integrate_pos(q, v3, h), v4, ctrl, qfrc_applied, xfrc_applied).qacc_smooth
                q = self.integrate_pos(q, (v + 2 * v2 + 2 * v3 + v4) / 6, h)
                v = v + h * (a1 + 2 * a2 + 2 * a3 + a4) / 6
        return q, v

    # ---------------------------------------------------------------- collisions
    def geom_pose(self, K, g):
        b = self.C.geoms[g]["body"]
        return K.R[b] @ self.gpos0[g] + K.p[b], K.R[b] @ self.gaxis0[g]

    def pair_allowed(self, g1, g2):
        G = self.C.geoms
        w1, w2 = self.weld[G[g1]["body"]], self.weld[G[g2]["body"]]
        if w1 == w2:
            return False
        if w1 and w2 and (w1 == self.weld[self.parent[w2]] or w2 == self.weld[self.parent[w1]]):
            return False
        return bool((int(G[g1]["contype"]) & int(G[g2]["conaffinity"]))
                    or (int(G[g2]["contype"]) & int(G[g1]["conaffinity"])))

    def _sphere_sphere(self, c1, r1, c2, r2):
        d = c2 - c1
        n = np.sqrt(d @ d)
        dist = n - r1 - r2
        # convention: the contact point lies halfway between the two surfaces
        return dist, d / n, c1 + (d / n) * (r1 + dist / 2)

    def _plane_sphere(self, p0, n, c, r):
        dist = n @ (c - p0) - r
        return dist, n, c - n * (r + dist / 2)

    def pair_geometry(self, K, g1, g2):
        """every candidate contact of the pair (lower geom type first, as MuJoCo
        orders them; the normal points from the first geom to the second):
        a list of (dist, normal, point, kind)"""
        G, dt = self.C.geoms, self.dt
        order = {"plane": 0, "sphere": 2, "capsule": 3}
        if order[G[g1]["type"]] > order[G[g2]["type"]]:
            g1, g2 = g2, g1
        t1, t2 = G[g1]["type"], G[g2]["type"]
        c1, z1 = self.geom_pose(K, g1)
        c2, z2 = self.geom_pose(K, g2)
        s1, s2 = self.T(G[g1]["size"]), self.T(G[g2]["size"])
        out = []
        if t1 == "plane" and t2 == "sphere":
            out.append(self._plane_sphere(c1, z1, c2, s2[0]) + ("plane-sphere",))
        elif t1 == "plane" and t2 == "capsule":
            for sg in (1, -1):  # convention: the +axis end sphere first
                out.append(self._plane_sphere(c1, z1, c2 + sg * s2[1] * z2, s2[0]) + ("plane-capsule",))
        elif t1 == "sphere" and t2 == "sphere":
            out.append(self._sphere_sphere(c1, s1[0], c2, s2[0]) + ("sphere-sphere",))
        elif t1 == "sphere" and t2 == "capsule":
            x = z2 @ (c1 - c2)
            kind = "sphere-capsule interior" if abs(x) < s2[1] else "sphere-capsule end"
            x = min(max(x, -s2[1]), s2[1])
            out.append(self._sphere_sphere(c1, s1[0], c2 + x * z2, s2[0]) + (kind,))
        elif t1 == "capsule" and t2 == "capsule":
            a1, a2 = z1 * s1[1], z2 * s2[1]
            det = (a1 @ a1) * (a2 @ a2) - (a1 @ a2) ** 2
            if abs(det) < dt(MINVAL):
                # convention, not geometry: for parallel capsules MuJoCo reports two
                # contacts, each end of the first against the nearest point of the second
                for sg in (1, -1):
                    e = c1 + sg * a1
                    t = min(max((a2 @ (e - c2)) / (a2 @ a2), -dt(1)), dt(1))
                    out.append(self._sphere_sphere(e, s1[0], c2 + t * a2, s2[0]) + ("capsule-capsule parallel",))
            else:
                s, t, region = segment_segment(c1, a1, c2, a2)
                out.append(self._sphere_sphere(c1 + s * a1, s1[0], c2 + t * a2, s2[0])
                           + ("capsule-capsule " + region.split("_")[0],))
        elif t1 == "plane" and t2 == "plane":
            pass
        else:
            raise NotImplementedError((t1, t2))
        return g1, g2, out

    def contacts(self, q, K=None):
        """(contacts within their margin, smallest dist - margin over all pairs)"""
        K = K or self.kin(q)
        G, res, clear = self.C.geoms, [], None
        for g1 in range(len(G)):
            for g2 in range(g1 + 1, len(G)):
                if not self.pair_allowed(g1, g2):
                    continue
                margin = self.dt(max(G[g1]["margin"], G[g2]["margin"]))
                ga, gb, cands = self.pair_geometry(K, g1, g2)
                for dist, n, pos, kind in cands:
                    clear = dist - margin if clear is None else min(clear, dist - margin)
                    if dist <= margin:
                        res.append(dict(g1=ga, g2=gb, dist=dist, normal=n, pos=pos, kind=kind, margin=margin))
        return res, clear

    def limit_rows(self, q):
        """(joint, side, dist) of every limited hinge / slide joint inside its margin;
        convention: the lower side first"""
        q, rows = self.T(q), []
        for ji, j in enumerate(self.C.joints):
            if not j["limited"] or j["type"] in ("free", "ball"):
                continue
            for side, dist in ((+1, q[self.jq[ji]] - self.dt(j["range"][0])), (-1, self.dt(j["range"][1]) - q[self.jq[ji]])):
                if dist < self.dt(j["margin"]):
                    rows.append((ji, side, dist))
        return rows

    def active(self, q):
        return len(self.limit_rows(q)), len(self.contacts(q)[0])

    def limit_clearance(self, q):
        """smallest distance of a limited joint to either end of its range"""
        q, out = self.T(q), None
        for ji, j in enumerate(self.C.joints):
            if j["limited"] and j["type"] not in ("free", "ball"):
                d = min(q[self.jq[ji]] - self.dt(j["range"][0]), self.dt(j["range"][1]) - q[self.jq[ji]])
                out = d if out is None else min(out, d)
        return out

    # ---------------------------------------------------------------- constraints
    def _impedance(self, solimp, x):
        """MuJoCo's impedance d(|pos - margin| / width): a sigmoid from dmin to dmax"""
        dt = self.dt
        dmin, dmax = (min(max(dt(s), dt(MINIMP)), dt(MAXIMP)) for s in solimp[:2])
        width, mid, power = dt(solimp[2]), dt(solimp[3]), dt(solimp[4])
        if dmin == dmax or width <= MINVAL:
            return (dmin + dmax) / 2
        x = abs(x) / width
        if x >= 1:
            return dmax
        if x <= 0:
            return dmin
        if x <= mid:
            y = x ** power / mid ** (power - 1)
        else:
            y = 1 - (1 - x) ** power / (1 - mid) ** (power - 1)
        return min(max(dmin + y * (dmax - dmin), dt(MINIMP)), dt(MAXIMP))

    def _kb(self, solref, solimp):
        dt = self.dt
        dmax = min(max(dt(solimp[1]), dt(MINIMP)), dt(MAXIMP))
        tc, dr = dt(solref[0]), dt(solref[1])
        if tc > 0:
            tc = max(tc, 2 * self.h)   # the spring may not be faster than two time steps
            return 1 / (dmax * dmax * tc * tc * dr * dr), 2 / (dmax * tc)
        return -tc / (dmax * dmax), -dr / dmax

    @staticmethod
    def _tangents(n):
        """convention (mju_makeFrame): the first tangent is y, or z when the normal is
        mostly along y, made orthogonal to the normal; the second completes the frame"""
        t = np.zeros(3, dtype=n.dtype)
        t[1 if abs(n[1]) < 0.5 else 2] = 1
        t = t - n * (n @ t)
        t = t / np.sqrt(t @ t)
        return t, cross(n, t)

    def problem(self, q, v, ctrl, qfrc_applied=None, xfrc_applied=None):
        """the constraint problem at a state: rows J, D, aref (limit rows, then the
        contacts in pair order), the contacts, M and the unconstrained acceleration"""
        C, dt = self.C, self.dt
        f = self.forward(q, v, ctrl, qfrc_applied, xfrc_applied)
        K, v = f.K, self.T(v)
        J, D, aref, pos, kind = [], [], [], [], []

        def add(row, p, margin, solref, solimp, dA):
            imp = self._impedance(solimp, p - margin)
            Kk, B = self._kb(solref, solimp)
            R = max(dt(MINVAL), (1 - imp) * dA / imp)
            J.append(row)
            D.append(1 / R)
            pos.append(p)
            aref.append(-B * (row @ v) - Kk * imp * (p - margin))

        for ji, side, dist in self.limit_rows(q):
            j = C.joints[ji]
            row = np.zeros(self.nv, dtype=dt)
            row[self.jd[ji]] = side
            add(row, dist, dt(j["margin"]), j["solreflimit"], j["solimplimit"], dt(C.dof_invweight0[self.jd[ji]]))
            kind.append("limit")
        cons, _ = self.contacts(q, K)
        for c in cons:
            G1, G2 = C.geoms[c["g1"]], C.geoms[c["g2"]]
            b1, b2 = G1["body"], G2["body"]
            s1, s2 = G1["solmix"], G2["solmix"]
            mix = 0.5 if (s1 < MINVAL and s2 < MINVAL) else 0.0 if s1 < MINVAL else 1.0 if s2 < MINVAL else s1 / (s1 + s2)
            mix = dt(mix)
            solref = [mix * dt(a) + (1 - mix) * dt(b) for a, b in zip(G1["solref"], G2["solref"])]
            solimp = [mix * dt(a) + (1 - mix) * dt(b) for a, b in zip(G1["solimp"], G2["solimp"])]
            margin = c["margin"] - dt(max(G1["gap"], G2["gap"]))
            dim = c["dim"] = int(max(G1["condim"], G2["condim"]))
            assert dim in (1, 3), "condim 1 and 3 only"
            Jc = self.jac(K, b2, c["pos"])[0] - self.jac(K, b1, c["pos"])[0]
            tran = dt(C.body_invweight0[b1][0]) + dt(C.body_invweight0[b2][0])
            n = c["normal"]
            c["row"] = len(J)
            if dim == 1:
                add(n @ Jc, c["dist"], margin, solref, solimp, tran)
                kind.append("contact")
            else:
                mu = dt(max(G1["friction"][0], G2["friction"][0]))
                for t in self._tangents(n):
                    for sg in (1, -1):  # the pyramid's edges n +- mu t
                        add(n @ Jc + sg * mu * (t @ Jc), c["dist"], margin, solref, solimp, tran + mu * mu * tran)
                        kind.append("contact")
        P = type("Problem", (), {})()
        P.f, P.M, P.a_s, P.contacts, P.kind = f, f.M, f.qacc_smooth, cons, kind
        P.J = np.array(J, dtype=dt).reshape(len(J), self.nv)
        P.D, P.aref, P.pos = (np.array(x, dtype=dt) for x in (D, aref, pos))
        P.scale = 1 / (dt(C.stat_meaninertia) * max(1, self.nv))
        return P

    def cost(self, P, a):
        """1/2 (a - a_s)' M (a - a_s) + 1/2 sum_i D_i min(0, J_i a - aref_i)^2"""
        a = self.T(a)
        e = a - P.a_s
        r = np.minimum(0, P.J @ a - P.aref) if len(P.D) else np.zeros(0, dtype=self.dt)
        return (e @ (P.M @ e)) / 2 + (P.D * r) @ r / 2

    def grad(self, P, a):
        r = np.minimum(0, P.J @ a - P.aref)
        return P.M @ (a - P.a_s) + P.J.T @ (P.D * r)

    def grad_scale(self, P, a):
        """the size of the terms the gradient at a is summed from: rounding a to the
        working dtype alone moves the gradient by eps |H| |a|"""
        res = P.J @ a - P.aref
        act = res < 0
        H = P.M + (P.J[act].T * P.D[act]) @ P.J[act]
        return (np.abs(P.M) @ np.abs(a - P.a_s) + np.abs(P.J.T) @ np.abs(P.D * np.where(act, res, 0))
                + np.abs(H) @ np.abs(a))

    def minimise(self, P, maxiter=200):
        """the minimiser of cost(): exact Newton on the active set with an exact
        line search.  cost is strictly convex and piecewise quadratic, so along a
        line its slope is piecewise linear and its zero is found exactly between two
        breakpoints; once the active set stops changing one step lands on the
        minimiser.  Stops when the gradient is at the rounding of the terms it is summed
        from, 64 eps grad_scale: with longdouble's 64-bit mantissa (eps 1.1e-19) that is
        the smallest gradient that can be told from zero; 1e-25 of the problem's scale
        would take a wider format than any NumPy has on x86-64."""
        dt = self.dt
        a = P.a_s.copy()
        if not len(P.D):
            return a
        eps = np.finfo(dt).eps
        for it in range(maxiter):
            res = P.J @ a - P.aref
            act = res < 0
            fr = P.D * np.where(act, res, 0)
            g = P.M @ (a - P.a_s) + P.J.T @ fr
            H = P.M + (P.J[act].T * P.D[act]) @ P.J[act]
            if np.all(np.abs(g) <= 64 * eps * self.grad_scale(P, a)):
                return a
            p = solve(H, -g)
            Jp = P.J @ p

            def slope(al):  # d cost / d alpha along a + alpha p
                r = np.minimum(0, res + al * Jp)
                return p @ (P.M @ (a + al * p - P.a_s)) + (P.D * Jp) @ r

            bk = sorted(set([dt(0)] + [-res[i] / Jp[i] for i in range(len(res)) if Jp[i] != 0 and -res[i] / Jp[i] > 0]))
            lo, slo = bk[0], slope(bk[0])
            alpha = None
            for hi in bk[1:]:
                shi = slope(hi)
                if shi >= 0:
                    alpha = lo if shi == slo else lo - slo * (hi - lo) / (shi - slo)
                    break
                lo, slo = hi, shi
            if alpha is None:  # past the last breakpoint the slope is linear
                alpha = lo - slo / (slope(lo + 1) - slo)
            a = a + alpha * p
        raise AssertionError("the reference minimiser did not converge")
