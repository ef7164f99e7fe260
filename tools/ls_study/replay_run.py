"""Newton replay study (tools/ls_study/replay_study.c): the FD sweeps of the
bench workload (hopper, cfg-4 seeds, 8 line-search candidates, min-cost
selection) on the CPU oracle, counting per iteration the Newton iterations of
the sweep that repeat the one before them bit for bit -- the iterations the
device's replay exit (ILQG_NT_REPLAY, dcoop_impl.h) leaves out.

  python3 tools/ls_study/replay_run.py [seeds] [iterations] [horizon]
"""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "ilqg-mujoco_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
LIB = os.path.join(HERE, "liboracle_replaystudy.so")


def build(lib=LIB):
    o = os.path.join(ROOT, "oracle")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-fopenmp",
                    "-DORA_NT_STUDY", "-I" + os.path.join(o, "include"), "-I" + os.path.join(ROOT, "include"),
                    "-shared", "-o", lib, os.path.join(o, "mjsub.c"), os.path.join(o, "ilqr_ora.c"),
                    os.path.join(o, "ora_api.c"), os.path.join(HERE, "replay_study.c"), "-lm"], check=True)
    return lib


def sweep_counts(S=2, iters=2, H=20, lib_path=LIB):
    """One dict per iteration: the study's counts over the FD sweeps (the
    backward passes) of all S seeds; the rollouts before them are not counted."""
    import ilqg_amd as ia
    import oracle as ora
    import workloads
    m = ia.Model.load(workloads.model_file("hopper"))
    lib = ora.Lib(lib_path)
    om = ora.OModel(m.blob(), lib=lib)
    lib.L.ora_set_cost_desc(ora.CostDesc.from_cost(ia.HOPPER_COST, m.nq, m.nv, m.nu))
    lib.L.ora_set_nthread(1)
    ils = []
    for s in range(S):
        # workloads.hopper_dmain(m, S, sigma=0.01) on the oracle's physics (no GPU): cfg 3's
        # state + cfg 4's perturbation of seed s
        d = om.make_data()
        d.step(500)
        d.arr("ctrl")[:] -= 0.1
        z = workloads.normals(s, m.nq + m.nv)
        d.arr("qpos")[:] += 0.01 * z[: m.nq]
        d.arr("qvel")[:] += 0.01 * z[m.nq:]
        il = ora.OILQR(om, d, H, cost_fn="ora_cost_desc_fn")
        il.set_dinit(d)
        ils.append(il)
    buf = ctypes.create_string_buffer(1024)
    out = []
    for it in range(iters):
        lib.L.ora_nt_study_reset()
        for il in ils:
            # iterate_ls in its three parts (ora_ilqr_iterate_ls), the study reset between
            # the rollouts and the sweep: each seed's counts are added up by hand
            il.forward_candidates(workloads.LINESEARCH_ALPHAS, "min_cost")
        tot = {}
        for il in ils:
            lib.L.ora_nt_study_reset()
            il.set_dinit(il.point(H))
            il.backward_pass()
            lib.L.ora_nt_study_report(buf, 1024)
            for k, v in json.loads(buf.value.decode()).items():
                tot[k] = tot.get(k, 0) + v
        out.append(dict(tot, iteration=it + 1, seeds=S, horizon=H))
    return out


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 500
    build()
    for r in sweep_counts(S, iters, H):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
