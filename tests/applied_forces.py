"""Inputs of tests/test_applied_forces.py: the seeded force sets, the states, the
solver runs on both sides and the flat result dictionaries they are compared in.

Run as a program (python applied_forces.py MODEL OUT.npz) it makes the GPU run
of test_iterate in a process of its own and saves the results: the rollout
kernel set (ILQG_DUAL) is chosen once per process, at the first rollout launch.
"""
import io
import os
import sys

import numpy as np

MODELS = ("inverted_pendulum", "hopper", "chain", "humanoid")
HORIZON = {"inverted_pendulum": 8, "hopper": 8, "chain": 6, "humanoid": 6}
ALPHAS4 = tuple(2.0 ** -i for i in range(4))
# the rows of the force set a model's solver runs with
ROWS = {"inverted_pendulum": (0, 1, 2, 3), "hopper": (0, 1, 2, 3), "chain": (0, 1, 2, 3), "humanoid": (2, 3)}
FIELDS = ("costs", "sel", "qpos", "qvel", "warm", "ctrl", "deriv", "K", "k", "V", "v")
ITERS = 2


def _compiled(name):
    import mjcf_indep as mi
    from conftest import model_path
    from test_riccati_cases import chain_xml
    return mi.compile_mjcf(io.StringIO(chain_xml())) if name == "chain" else mi.compile_mjcf(model_path(name))


_sets = {}


def force_set(name):
    """(qf[4, nv], xf[4, nbody, 6]): row 0 zero; row 1 qfrc_applied alone; row 2
    xfrc_applied alone, on a leaf (force and torque; the humanoid's with index
    >= 11, so that its row lies past the 64th double) and a force on one other
    body; row 3 qfrc_applied, a wrench on the last body, the world body's row
    filled (never applied) and one -0.0 in an otherwise empty row"""
    if name in _sets:
        return _sets[name]
    C = _compiled(name)
    nv, nb = C.nv, C.nbody
    rng = np.random.default_rng([20261020, MODELS.index(name)])

    def wrench():
        return np.concatenate([rng.normal(0, 3.0, 3), rng.normal(0, 0.2, 3)])
    qf, xf = np.zeros((4, nv)), np.zeros((4, nb, 6))
    qf[1] = rng.normal(0, 0.5, nv)
    parents = [b["parent"] for b in C.bodies[1:]]
    leaves = [b for b in range(1, nb) if b not in parents]
    high = [b for b in leaves if 6 * b >= 64]
    leaf = high[0] if high else leaves[int(rng.integers(len(leaves)))]
    others = [b for b in range(1, nb) if b != leaf]
    xf[2, leaf] = wrench()
    xf[2, others[int(rng.integers(len(others)))], :3] = rng.normal(0, 3.0, 3)
    qf[3] = rng.normal(0, 0.5, nv)
    xf[3, nb - 1] = wrench()
    xf[3, 0] = wrench()
    if name == "humanoid":
        qf *= 0.3
        xf *= 0.3
    assert nb > 2
    xf[3, 1, 4] = -0.0
    _sets[name] = (qf, xf)
    return qf, xf


def world_only(name):
    """xfrc_applied on the world body alone, in every seed: zero forces to the physics"""
    qf, xf = force_set(name)
    w = np.zeros_like(xf)
    w[:, 0] = xf[3, 0] * (1 + np.arange(4))[:, None]
    return np.zeros_like(qf), w


def forces(name):
    """the rows of the force set the model's solver carries, one per seed"""
    qf, xf = force_set(name)
    r = list(ROWS[name])
    return np.ascontiguousarray(qf[r]), np.ascontiguousarray(xf[r])


# ------------------------------------------------------------------ the device side
def model(ia, name):
    from conftest import model_path
    from test_riccati_cases import chain_xml
    return ia.Model.from_string(chain_xml()) if name == "chain" else ia.Model.load(model_path(name))


def cost(ia, name):
    return {"inverted_pendulum": ia.PENDULUM_COST, "hopper": ia.HOPPER_COST, "humanoid": ia.HUMANOID_COST,
            "chain": ia.Cost(wq=[1.0] * 9, wv=[0.1] * 9, wu=[0.01] * 7)}[name]


def states(ia, m, name):
    """the solver's states: one per row of ROWS (built with the device's own physics)"""
    import workloads
    S = len(ROWS[name])
    if name == "inverted_pendulum":
        st = workloads.pendulum_dmain(m, S)
        st.qpos[:, 1] += 0.01 * np.arange(S)
        return st
    if name == "hopper":
        return workloads.hopper_dmain(m, S, sigma=0.01)   # cfg 3's state: in contact
    st = m.reset_state(S)
    if name == "humanoid":
        st.qpos[:, 2] = 1.4
    else:
        st.qpos[:] = 0.05 * (1 + np.arange(m.nq)) + 0.01 * np.arange(S)[:, None]
    return st


def sub(ia, st, idx):
    idx = np.atleast_1d(idx)
    return ia.State(st.time[idx], st.qpos[idx], st.qvel[idx], st.warm[idx], st.ctrl[idx])


def line_search(name):
    """(alphas, select) of the model's solver: the humanoid runs one candidate"""
    return ((1.0,), "reference") if name == "humanoid" else (ALPHAS4, "min_cost")


def solver(ia, m, name, st, qf, xf, H=None, alphas=None, select=None):
    a, sel = line_search(name)
    return ia.ILQR(m, st, H or HORIZON[name], cost(ia, name), alphas=alphas or a, select=select or sel,
                   qfrc_applied=qf, xfrc_applied=xf)


def results(g):
    """every result of the last iterate(), seed-major"""
    g.synchronize()
    S, P = g.S, g.P
    t, (K, k), (V, v), (c, sel) = g.traj(), g.gains(), g.value(), g.costs()
    dV, bad = g.expected()
    mask, info = g.clamped()
    return dict(costs=c, sel=sel.astype(np.int64), qpos=t.qpos.reshape(S, P, -1), qvel=t.qvel.reshape(S, P, -1),
                warm=t.warm.reshape(S, P, -1), ctrl=t.ctrl.reshape(S, P, -1), deriv=g.deriv(), K=K, k=k, V=V, v=v,
                dV=dV, first_bad=bad, clamp_mask=mask, clamp_info=info)


def run(ia, name, qf, xf, iters=ITERS, prepare=None, st=None, m=None):
    """a solver of the model's states with the given forces: results after each iterate()"""
    m = m or model(ia, name)
    g = solver(ia, m, name, states(ia, m, name) if st is None else st, qf, xf)
    if prepare:
        prepare(g)
    out = []
    for _ in range(iters):
        g.iterate()
        out.append(results(g))
    return out


# ------------------------------------------------------------------ the oracle side
def oracle_model(ia, ora, name, m=None):
    """(product model, oracle model) with the model's cost installed as the oracle's cost descriptor"""
    m = m or model(ia, name)
    om = ora.OModel(m.blob())
    om.lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(cost(ia, name), m.nq, m.nv, m.nu))
    om.lib.L.ora_set_nthread(1)
    return m, om


def oracle_data(om, state, qf, xf):
    d = om.make_data()
    d.set_state(**state)
    d.arr("qfrc_applied")[:] = 0.0 if qf is None else qf
    d.xfrc()[:] = 0.0 if xf is None else np.ravel(xf)
    return d


def oracle_solver(ora, om, state, qf, xf, H):
    d = oracle_data(om, state, qf, xf)
    il = ora.OILQR(om, d, H, cost_fn="ora_cost_desc_fn")
    il.set_dinit(d)
    return il


def oracle_iterate(il, alphas, select):
    """one iterate_ls: the results of one seed in the layout of results()[f][s]"""
    c, sel = il.iterate_ls(alphas, select)
    t, a = il.traj(), il.arrays()
    return dict(costs=c, sel=np.int64(sel), qpos=t["qpos"], qvel=t["qvel"], warm=t["warm"], ctrl=t["ctrl"],
                deriv=a["deriv"], K=a["K"], k=a["k"], V=a["V"], v=a["v"])


def state_dict(st, s):
    return dict(time=st.time[s], qpos=st.qpos[s], qvel=st.qvel[s], warm=st.warm[s], ctrl=st.ctrl[s])


def oracle_run(ia, ora, name, st, qf, xf, iters=ITERS, m=None, H=None):
    """out[iteration][seed]: the oracle's solver of every seed, each carrying its own forces"""
    m, om = oracle_model(ia, ora, name, m)
    alphas, select = line_search(name)
    out = [[] for _ in range(iters)]
    for s in range(st.qpos.shape[0]):
        il = oracle_solver(ora, om, state_dict(st, s), None if qf is None else qf[s], None if xf is None else xf[s],
                           H or HORIZON[name])
        for it in range(iters):
            out[it].append(oracle_iterate(il, alphas, select))
    return out


def hopper_states_oracle(ora, om, S):
    """workloads.hopper_dmain(m, S, sigma=0.01) with the oracle's physics: no device"""
    import workloads
    d = om.make_data()
    d.step(500)
    d.arr("ctrl")[:] -= 0.1
    base = d.state()
    out = []
    for s in range(S):
        z = workloads.normals(s, om.nq + om.nv)
        st = {k: np.copy(v) for k, v in base.items()}
        st["qpos"] = st["qpos"] + 0.01 * z[:om.nq]
        st["qvel"] = st["qvel"] + 0.01 * z[om.nq:]
        out.append(st)
    return out


# ------------------------------------------------------------------ the child process
def _main(name, path):
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import conftest  # noqa: F401  (the package's and the oracle's directories)
    import ilqg_amd as ia
    qf, xf = forces(name)
    out = run(ia, name, qf, xf)
    np.savez(path, **{f"{f}{it}": r[f] for it, r in enumerate(out) for f in FIELDS})


if __name__ == "__main__":
    _main(sys.argv[1], sys.argv[2])
