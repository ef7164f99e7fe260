"""ilqg_solver_refresh_nominal: what the calls cost, and what they buy in a
closed loop (DESIGN.md "Nominal refresh").  Needs a GPU.

  python3 tools/refresh_nominal_study.py cost    # HIP-event times on the bench workload
  python3 tools/refresh_nominal_study.py loop    # the closed-loop experiment, with and without the refresh

cost: hopper H = 500, 8 seeds x 8 alphas, three iterate() to warm up, then nine
repetitions of refresh_nominal('cost'), forward_pass() and
refresh_nominal('reroll'), each timed by ilqg_solver_set_timing's events
(index 0 rollout, 1 select / the cost kernel); medians.

loop: hopper H = 100, 4 seeds x 4 alphas, corrected layout, STANDARD, the
regularisation mode on (mu from 0), a target height that moves with the
absolute step, one iterate() per tick, 30 ticks.  The plant is stepped with the
nominal's first control and a velocity disturbance the solver does not know.
Tick: shift_cost_schedule; shift_horizon(1); set_dinit(measured) -- then
refresh_nominal('reroll', resume=True), or nothing -- and iterate().  Reported
per run: rejected steps, the range of mu, the summed selected cost.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ilqg-mujoco_amd"))

import torch  # noqa: E402,F401  (its HIP runtime initialises first: ilqg_amd.lib)

import ilqg_amd as ia  # noqa: E402
import workloads  # noqa: E402
from seed_shard import device_view  # noqa: E402

ALPHAS8 = tuple(2.0 ** -i for i in range(8))


def med(x):
    return float(np.median(np.asarray(x)))


def cost_of_calls(reps=9):
    m = ia.Model.load(workloads.model_file("hopper"))
    S, H = 8, 500
    g = ia.ILQR(m, workloads.hopper_dmain(m, S, sigma=0.01), H, ia.HOPPER_COST, alphas=ALPHAS8, select="min_cost")
    for _ in range(3):
        g.iterate()
    g.set_timing(True)
    g.synchronize()
    g.timing()
    rows = {k: [] for k in ("cost: cost kernel", "forward: rollout (8 x 8 candidates)", "forward: k_select",
                            "reroll: rollout (8 x 1 candidates)", "reroll: epilogue")}
    for _ in range(reps):
        g.refresh_nominal("cost")
        t = g.timing()
        assert t["select"][1] == 1 and t["rollout"][1] == 0
        rows["cost: cost kernel"].append(t["select"][0])
        g.forward_pass()
        t = g.timing()
        rows["forward: rollout (8 x 8 candidates)"].append(t["rollout"][0])
        rows["forward: k_select"].append(t["select"][0])
        g.refresh_nominal("reroll")
        t = g.timing()
        assert t["select"][1] == 1 and t["rollout"][1] == 1
        rows["reroll: rollout (8 x 1 candidates)"].append(t["rollout"][0])
        rows["reroll: epilogue"].append(t["select"][0])
    print(f"cost of the calls: hopper H={H}, {S} seeds x {len(ALPHAS8)} alphas, after 3 iterate(); HIP events, ms, "
          f"{reps} repetitions in run order")
    for k, v in rows.items():
        print(f"  {k:38s}" + " ".join(f"{x:8.4f}" for x in v) + f"   median {med(v):.4f}")


def row(m, t):
    """the cost row of absolute step t: the hopper's cost with a torso height target that moves"""
    c = ia.HOPPER_COST
    tq = list(c.tq)
    tq[1] = 1.25 + 0.1 * math.sin(0.05 * t)
    return ia.Cost(wq=c.wq, tq=tq, wv=c.wv, wu=c.wu).row(m.nq, m.nv, m.nu)


def closed_loop(refresh, ticks=30):
    m = ia.Model.load(workloads.model_file("hopper"))
    S, H, alphas = 4, 100, ALPHAS8[:4]
    plant = workloads.hopper_dmain(m, S, sigma=0.01)
    g = ia.ILQR(m, plant, H, ia.HOPPER_COST, alphas=alphas, select="min_cost", mu=0.0)
    g.set_layout("corrected")
    g.set_recursion("standard")
    # point p of the window that starts at step k is absolute step k + (H - p)
    g.set_cost_schedule(np.stack([row(m, H - p) for p in range(H + 1)]))
    g.set_regularization(True, trace_len=ticks)
    csel = device_view(g.device_costs_ptr(), S)
    rejected, mus, total, per_tick = 0, [], 0.0, []
    for k in range(ticks):
        if k > 0:
            # the plant takes the first control, and a disturbance
            t = g.traj()
            plant.ctrl[:] = t.ctrl.reshape(S, H + 1, -1)[:, H]
            m.step(plant, 1)
            z = np.stack([workloads.normals(1000 * k + s, m.nv) for s in range(S)])
            plant.qvel[:] += 0.05 * z
            g.shift_cost_schedule(row(m, k + H)[None], 1)
            g.shift_horizon(1)
            g.set_dinit(plant)
            if refresh:
                g.refresh_nominal("reroll", resume=True)
        g.iterate()
        g.synchronize()
        sel = g.costs()[1]
        st = g.reg_state()
        c = csel.cpu().numpy()
        rejected += int(np.sum(sel < 0))
        mus += [float(x) for x in st["mu"]]
        total += float(np.mean(c))
        per_tick.append(float(np.mean(c)))
    what = "set_dinit + refresh_nominal(REROLL | RESUME)" if refresh else "set_dinit, no refresh"
    print(f"closed loop, {what}: hopper H={H}, {S} seeds x {len(alphas)} alphas, {ticks} ticks")
    print(f"  rejected steps {rejected} of {ticks * S}; mu {min(mus):.4g} .. {max(mus):.4g}; "
          f"summed selected cost (mean over seeds per tick) {total:.6g}")
    print("  per tick: " + " ".join(f"{x:.4g}" for x in per_tick))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "cost"
    if what == "cost":
        cost_of_calls()
    else:
        closed_loop(True)
        closed_loop(False)
