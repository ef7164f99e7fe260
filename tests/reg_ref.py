"""Reference of the regularisation mode (ilqg_solver_set_regularization): the
mu / dmu schedule, the acceptance rule and the restarting backward pass in
plain Python floats, every expression in the order the header writes it.  A
helper: not collected.

    increase:  dmu = max(dmu f, f);  mu = max(mu dmu, mu_min);  mu >= mu_max: status = 2
    decrease:  dmu = min(dmu / f, 1 / f);  t = mu dmu;  mu = t > mu_min ? t : 0
    candidate a acceptable:  actual = cost_nom - cost[a] > 0  and  actual >= zmin expected,
                             expected = -(alpha_a dV1 + alpha_a alpha_a dV2)

RegRef composes one seed's loop from std_ref.StdRef: the oracle rollout through
forward_candidates, the records through sweep, recursion_f64 / recursion_ld.  A
rejected step puts the oracle's trajectory back: the snapshot taken before the
rollout is written point by point through il.point(n).set_state, then
il.set_dinit(il.point(N)).  In replay mode the gains, dV and restart count are
the device's (handed to backward()), so that candidate costs, decisions, mu and
trajectories compare bit for bit and only the gains carry a tolerance."""
import contextlib
import math

import numpy as np

import std_ref as sr

NAN = float("nan")
DEFAULTS = dict(factor=1.6, mu_min=1e-6, mu_max=1e10, zmin=0.0, tol_cost=0.0, max_retry=16, trace_len=0)


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def increase(o, mu, dmu, status):
    f = float(o["factor"])
    d = dmu * f
    dmu = d if d > f else f
    t = mu * dmu
    mu = t if t > o["mu_min"] else float(o["mu_min"])
    if mu >= o["mu_max"]:
        status = 2
    return mu, dmu, status


def decrease(o, mu, dmu):
    f = float(o["factor"])
    d, i = dmu / f, 1.0 / f
    dmu = d if d < i else i
    t = mu * dmu
    mu = t if t > o["mu_min"] else 0.0
    return mu, dmu


def plain_select(costs, mode):
    """k_select: the lowest cost (a NaN never wins over a number), or candidate 0"""
    best = 0
    if mode == 1:
        bc = costs[0]
        for a in range(1, len(costs)):
            c = costs[a]
            if c < bc or (bc != bc and c == c):
                bc, best = c, a
    return best


def expected(alpha, dV):
    return -(alpha * dV[0] + alpha * alpha * dV[1])


def decide(o, st, costs, alphas, dV, mode):
    """one acceptance on the state dict st (mu, dmu, cost_nom, valid, status);
    -> (pick, trace fields 0..5, per-candidate actual / expected of the tested one)"""
    costs = [float(c) for c in costs]
    best = plain_select(costs, mode)
    mu0 = st["mu"]
    t0 = t3 = NAN
    pick, ratio = -1, NAN
    if not st["valid"]:
        pick = best
        st["valid"] = 1
    else:
        cn = st["cost_nom"]
        t0, t3 = cn, expected(alphas[best], dV)
        ratio = (cn - costs[best]) / t3 if t3 != 0 else NAN
        if st["status"] == 0:
            pc = 0.0
            for a in range(len(costs) if mode == 1 else 1):
                actual = cn - costs[a]
                if actual > 0 and actual >= o["zmin"] * expected(alphas[a], dV) and (pick < 0 or costs[a] < pc):
                    pick, pc = a, costs[a]
            if pick >= 0:
                t3 = expected(alphas[pick], dV)
                ratio = (cn - costs[pick]) / t3 if t3 != 0 else NAN
                st["mu"], st["dmu"] = decrease(o, st["mu"], st["dmu"])
                if cn - costs[pick] < o["tol_cost"]:
                    st["status"] = 1
            else:
                st["mu"], st["dmu"], st["status"] = increase(o, st["mu"], st["dmu"], st["status"])
    if pick >= 0:
        st["cost_nom"] = costs[pick]
    return pick, [t0, costs[best], float(pick), t3, mu0, st["mu"]], ratio


@contextlib.contextmanager
def _record_pivots(log):
    """std_ref's recursions report each step's Quu_r pivots through _pivots:
    keep (largest |diagonal| of the matrix, its pivots) per step"""
    orig = sr._pivots

    def rec(M, zero):
        out = orig(M, zero)
        log.append((max(abs(float(M[i][i])) for i in range(len(M))), [float(d) for d in out]))
        return out
    sr._pivots = rec
    try:
        yield
    finally:
        sr._pivots = orig


def backward_restart(o, st, rec, nv, nu, dt, layout, lxx, luu, V0=None, v0=None, f=None):
    """the restarting pass on the state dict st (mu, dmu, status): -> (the last
    attempt's std_ref dict, retries, [mu tried], the smallest |pivot| / largest
    |diagonal| over every step factored in any attempt)"""
    f = f or sr.recursion_f64
    retries, tried, margin = 0, [], math.inf
    while True:
        log = []
        with _record_pivots(log):
            out = f(rec, nv, nu, dt, st["mu"], layout, lxx, luu, V0, v0)
        tried.append(st["mu"])
        for big, piv in log:
            if big > 0 and all(d == d for d in piv):
                margin = min(margin, min(abs(d) for d in piv) / big)
        if out["first_bad"] >= 0 and retries < o["max_retry"] and st["status"] == 0:
            st["mu"], st["dmu"], st["status"] = increase(o, st["mu"], st["dmu"], st["status"])
            retries += 1
            continue
        return out, retries, tried, margin


class RegRef:
    """one seed's outer loop on the oracle.  ref: a std_ref.StdRef (its mu is
    overwritten per pass); mode: select_mode (1 min_cost, 0 reference)"""

    def __init__(self, ref, opts, mu0, replay=False):
        self.ref, self.o, self.replay = ref, opts, replay
        self.mode = 1 if ref.select == "min_cost" else 0
        self.st = dict(mu=float(mu0), dmu=1.0, cost_nom=0.0, valid=0, status=0)
        self.retries = 0
        self.dV = [0.0, 0.0]
        self.trace, self.ratios = [], []

    def invalidate(self):
        self.st["valid"] = 0

    def _restore(self, snap):
        il, N = self.ref.il, self.ref.N
        for n in range(N + 1):
            il.point(n).set_state(time=snap["time"][n], qpos=snap["qpos"][n], qvel=snap["qvel"][n],
                                  warm=snap["warm"][n], ctrl=snap["ctrl"][n])
        il.set_dinit(il.point(N))

    def forward(self):
        """-> (candidate costs, pick or -1)"""
        il = self.ref.il
        snap = il.traj()
        costs, sel = self.ref.forward()
        pick, fields, ratio = decide(self.o, self.st, costs, self.ref.alphas, self.dV, self.mode)
        if pick < 0:
            self._restore(snap)
        elif pick != sel:
            # an acceptable candidate that is not the plain selection's: rolled out alone
            self._restore(snap)
            c1, _ = il.forward_candidates((self.ref.alphas[pick],), "min_cost")
            assert c1[0] == costs[pick]
        self.trace.append(fields + [NAN, NAN])
        self.ratios.append(ratio)
        return np.array(costs), pick

    def backward(self, dev=None, rec=None, V0=None, v0=None):
        """the backward pass behind forward(): the reference's own (with restarts),
        or in replay mode the device's K, k, dV, retries (dict dev)"""
        if self.replay:
            for _ in range(int(dev["retries"])):
                self.st["mu"], self.st["dmu"], self.st["status"] = increase(self.o, self.st["mu"], self.st["dmu"],
                                                                            self.st["status"])
            self.retries = int(dev["retries"])
            self.dV = [float(dev["dV"][0]), float(dev["dV"][1])]
            self.ref.il.set_gains(np.asarray(dev["K"], dtype=np.float64), np.asarray(dev["k"], dtype=np.float64))
            out = None
        else:
            r = self.ref
            rec = r.sweep() if rec is None else rec
            out, self.retries, _, _ = backward_restart(self.o, self.st, rec, r.m.nv, r.m.nu, r.m.timestep, r.layout,
                                                       r.lxx, r.luu, V0, v0,
                                                       sr.recursion_ld if r.precise else sr.recursion_f64)
            self.dV = [float(out["dV"][0]), float(out["dV"][1])]
            r.il.set_gains(np.asarray(out["K"], dtype=np.float64), np.asarray(out["k"], dtype=np.float64))
        if self.trace:
            self.trace[-1][6] = self.st["mu"]
            self.trace[-1][7] = float(self.retries + 100 * self.st["status"])
        return out

    def iterate(self):
        costs, pick = self.forward()
        self.backward()
        return costs, pick

    def traj(self):
        return self.ref.il.traj()
