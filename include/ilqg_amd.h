/*
 * ilqg_amd -- MI355X-native iLQR hot path (FD derivative sweep, Riccati
 * backward pass, forward rollout) behind a plain C ABI.
 *
 * Every entry point takes plain pointers and sizes and returns an int status
 * (ILQG_OK == 0).  Host buffers are row-major float64.  Each entry point names
 * the reference interface it replaces (paths under /root/reference).
 *
 * Trajectory record (the per-point state contract of cpMjData, src/util.cpp:4-14),
 * per seed s and point p = 0..N (p = N is the initial state, p = 0 the terminal
 * one, inc/ilqr.h:52):
 *   time[s][p], qpos[s][p][nq], qvel[s][p][nv], warm[s][p][nv] (qacc_warmstart),
 *   ctrl[s][p][nu]
 * qfrc_applied / xfrc_applied are per-seed constants (the reference never
 * changes them along a trajectory).
 *
 * FD record per point (src/mjderivative.cpp:88,107,120,138,174,202), D =
 * nv*(2nv+nu) + 2nv + nu doubles, written exactly as the reference writes it:
 *   [i + j*nv]            d qacc_j / d qpos_i
 *   [nv^2 + i + j*nv]     d qacc_j / d qvel_i
 *   [2nv^2 + i + j*nu]    d qacc_j / d ctrl_i
 *   [2nv^2+nv*nu + i]     d cost / d qpos_i   (then qvel, then ctrl)
 * Gains: K[s][p] is nu x 2nv column-major (Eigen layout, inc/ilqr.h:130),
 * k[s][p] is nu.
 */
#ifndef ILQG_AMD_H
#define ILQG_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ILQG_OK 0
#define ILQG_ERR_ARG 1
#define ILQG_ERR_MODEL 2
#define ILQG_ERR_HIP 3
#define ILQG_ERR_UNSUPPORTED 4
#define ILQG_ERR_NODEVICE 5

typedef struct ilqg_model ilqg_model;
typedef struct ilqg_solver ilqg_solver;

/* Diagonal-quadratic + linear step cost over (qpos, qvel, ctrl), evaluated on
   the device inside the sweep and the rollout.  Replaces the host callback
   stepCostFn_t (inc/mjderivative.h:5) on the batched path:
     c = sum_i wq_i (qpos_i - tq_i)^2 + lq_i qpos_i  + (same for qvel, ctrl)
   accumulated in (q, v, u) order, index ascending.  inc/inverted_pendulum/
   cost.h:7-17 is wq = {1,10}, wv = {1,10}, wu = {1}.  NULL arrays mean 0. */
typedef struct ilqg_cost {
  const double *wq, *tq, *lq;
  const double *wv, *tv, *lv;
  const double *wu, *tu, *lu;
} ilqg_cost;

typedef struct ilqg_solver_opts {
  int horizon;          /* N; N+1 trajectory points (inc/ilqr.h:14 template N) */
  int nseed;            /* independent trajectories (MPC seeds) on this device */
  int nalpha;           /* rollout candidates per seed; alphas[0] == 1 is the reference rollout */
  const double* alphas; /* feed-forward scales: u = K(x - x*) + alpha*k + u* */
  int select_mode;      /* 0: keep alphas[0] (reference semantics); 1: lowest trajectory cost */
  double mu;            /* Levenberg-Marquardt constant, 1000 in inc/ilqr.h:65 */
  int device;           /* HIP device ordinal */
} ilqg_solver_opts;

const char* ilqg_last_error(void);
int ilqg_version(void);
int ilqg_device_count(int* count);

/* ---- model: replaces mj_loadXML / mj_deleteModel (cmd/basic.cpp:123) ----
   Model-size limit: every device path runs one physics evaluation per
   workgroup with its workspace (mjData equivalent) in LDS, so the workspace
   must fit one CU's 160 KB (the bundled humanoid, nv = 27 with 12 contact
   slots, uses 147 KB).  A larger model is refused at load with
   ILQG_ERR_UNSUPPORTED; the reference's CPU path has no such limit. */
int ilqg_model_load_xml(const char* path, ilqg_model** out);
int ilqg_model_load_xml_string(const char* xml, ilqg_model** out);
void ilqg_model_free(ilqg_model* m);
/* sizes[10] = nq nv nu nbody njnt ngeom maxcon maxefc nconmax njmax */
int ilqg_model_sizes(const ilqg_model* m, int* sizes);
int ilqg_model_timestep(const ilqg_model* m, double* dt);
int ilqg_model_qpos0(const ilqg_model* m, double* qpos0);
/* the actuators' control ranges (mjModel.actuator_ctrlrange, which mj_fwdActuation
   clips to where actuator_ctrllimited): lo[a], hi[a] (nu doubles each) where
   actuator a is ctrllimited, else -inf / +inf.  The reference never reads them
   on the optimiser's side (no counterpart call); see ilqg_solver_set_ctrl_limits. */
int ilqg_model_ctrlrange(const ilqg_model* m, double* lo, double* hi);
/* compiled-model record (include/ilqg_model_blob.h); needed = bytes required */
int ilqg_model_blob(const ilqg_model* m, void* buf, size_t cap, size_t* needed);
/* specialisation key: the integer data (sizes, topology, static collision
   pairs, device-image layout) that model-specific kernels compile in
   (tools/gen_static_models.py); n = entries written (or required if key is
   NULL).  static_id: the compiled specialisation this model runs on, 0 = the
   generic kernels.  Results are identical either way. */
int ilqg_model_static_key(const ilqg_model* m, int* key, int cap, int* n);
int ilqg_model_static_id(const ilqg_model* m, int* id);

/* ---- batched single-point physics (device) ----
   n independent states; host buffers (n x nq etc.).  step: mj_step
   (inc/ilqr.h:86,128, src/update.cpp:8-11) -- advances time/qpos/qvel/warm in
   place; forward: mj_forward -> qacc (n x nv), warm updated in place. */
int ilqg_step_batch(const ilqg_model* m, int n, int nstep, double* time, double* qpos, double* qvel,
                    double* warm, const double* ctrl, const double* qfrc_applied,
                    const double* xfrc_applied);
int ilqg_forward_batch(const ilqg_model* m, int n, const double* qpos, const double* qvel,
                       double* warm, const double* ctrl, const double* qfrc_applied,
                       const double* xfrc_applied, double* qacc);
/* calcMJDerivatives (src/mjderivative.cpp:212-255) at n independent points;
   deriv is n x D.  cost may be NULL (cost-gradient entries then 0). */
int ilqg_fd_batch(const ilqg_model* m, int n, const double* qpos, const double* qvel,
                  const double* warm, const double* ctrl, const double* qfrc_applied,
                  const double* xfrc_applied, const ilqg_cost* cost, double* deriv);

/* ---- the iLQR solver context (ILQR<nv,nu,N>, inc/ilqr.h:14-188) ---- */
int ilqg_solver_create(const ilqg_model* m, const ilqg_solver_opts* opts, const ilqg_cost* cost,
                       ilqg_solver** out);
void ilqg_solver_free(ilqg_solver* s);
/* ILQR ctor (inc/ilqr.h:69-97): per seed, d = dmain; initial passive rollout
   with constant ctrl fills the trajectory; then setDInit(dmain).  dmain
   arrays are nseed x {1, nq, nv, nv, nu}; applied forces may be NULL (zero,
   also when an earlier call on the same solver passed forces). */
int ilqg_solver_init(ilqg_solver* s, const double* time, const double* qpos, const double* qvel,
                     const double* warm, const double* ctrl, const double* qfrc_applied,
                     const double* xfrc_applied);
/* setDInit (inc/ilqr.h:110-113) per seed */
int ilqg_solver_set_dinit(ilqg_solver* s, const double* time, const double* qpos, const double* qvel,
                          const double* warm, const double* ctrl);
int ilqg_solver_set_traj(ilqg_solver* s, const double* time, const double* qpos, const double* qvel,
                         const double* warm, const double* ctrl);
int ilqg_solver_get_traj(ilqg_solver* s, double* time, double* qpos, double* qvel, double* warm,
                         double* ctrl);
int ilqg_solver_set_gains(ilqg_solver* s, const double* K, const double* k);
int ilqg_solver_get_gains(ilqg_solver* s, double* K, double* k);
int ilqg_solver_get_deriv(ilqg_solver* s, double* deriv);     /* nseed x (N+1) x D */
/* one FD record (D doubles) of seed `seed` at point `point` (0 = terminal) */
int ilqg_solver_get_deriv_point(ilqg_solver* s, int seed, int point, double* deriv);
/* overwrite the FD records before ilqg_backward, e.g. with cost-gradient
   entries from a host cost callback (stepCostFn_t, inc/mjderivative.h:5) */
int ilqg_solver_set_deriv(ilqg_solver* s, const double* deriv);
int ilqg_solver_get_value(ilqg_solver* s, double* V, double* v); /* nseed x nx x nx (col-major), nseed x nx */
/* per-seed trajectory cost of every candidate (nseed x nalpha) and the selected index */
int ilqg_solver_get_costs(ilqg_solver* s, double* cost, int* selected);

/* hot path, enqueued on the solver's stream (asynchronous) */
int ilqg_forward(ilqg_solver* s);   /* forwardPass over all candidates + selection (inc/ilqr.h:116-130) */
int ilqg_fd_sweep(ilqg_solver* s);  /* calcMJDerivatives at every point of every seed */
int ilqg_backward(ilqg_solver* s);  /* initV + Riccati n = 1..N (inc/ilqr.h:100-107,133-176) */
/* calcMJDerivatives at points p0 .. p0+np-1 of every seed (one rank's share
   of a point-sharded sweep, src/mjderivative.cpp:212-255 per point; records
   identical to ilqg_fd_sweep's).  With the records of the other points
   written into the buffer ilqg_solver_device_deriv exposes (an all-gather),
   ilqg_backward then runs the recursion over all of them. */
int ilqg_fd_sweep_range(ilqg_solver* s, int p0, int np);
/* One seed's iteration point-sharded over `world` ranks, pipelined
   (BASELINE.json configs[4]: one humanoid seed on 8 GPUs).  Every rank runs
   the whole rollout (forwardPass, inc/ilqr.h:116-130, in the pipelined
   iterate's chunks) and, behind each chunk, calcMJDerivatives
   (src/mjderivative.cpp:212-255) at the points it owns (point_owners), then
   selection / setDInit (inc/ilqr.h:110-113); the solver's stream is left
   behind every sweep launch.  The caller then gathers the other ranks'
   records into ilqg_solver_device_deriv's buffer and calls ilqg_backward.
   ILQG_ERR_UNSUPPORTED unless the solver pipelines its iterate (one candidate
   per seed, the unfused sweep: fp32 FD or the MFMA recursion).  world = 1 is
   ilqg_iterate without the backward pass. */
int ilqg_forward_sharded(ilqg_solver* s, int rank, int world);
/* owner[p] (p = 0 .. npoint-1, 0 = terminal) = the rank that differentiates
   point p under ilqg_forward_sharded: the pipelined rollout's chunks of
   `chunk` points (launch order: descending from npoint - 1) dealt round-robin,
   the last two chunks' points in contiguous blocks over every rank.  Pure host
   logic (no device).  solver_point_owners: the same for a solver's chunking. */
int ilqg_point_owners(int npoint, int chunk, int world, int* owner);
int ilqg_solver_point_owners(ilqg_solver* s, int world, int* owner);
int ilqg_iterate(ilqg_solver* s);   /* forwardPass; setDInit(dArray[N]); backwardPass (inc/ilqr.h:179-186) */
/* waits for every launch; returns ILQG_ERR_HIP once if a fused sweep's
   hand-off wait timed out since the last call (the report is cleared by it) */
int ilqg_synchronize(ilqg_solver* s);
/* test hook: preset the fault report word that ilqg_synchronize reads */
int ilqg_solver_debug_set_fault(ilqg_solver* s, unsigned value);
/* test hook: run the fused sweep's ticket planner on the durations the last
   sweep recorded and copy out the schedule (slot -> FD item) and the
   durations; nitems = the sweep's FD item count (0: no fused sweep) */
int ilqg_solver_debug_plan(ilqg_solver* s, unsigned* order, unsigned* dur, int* nitems);
/* test hook: the next fused sweep's ticket map (planned, or the identity) gets
   order[slot] = item before it is validated (calls accumulate until then).  Every map is checked on the
   device (items in range, none repeated, every column behind its centre); an
   invalid one is replaced by the identity, the sweep runs normally, and
   ilqg_synchronize returns ILQG_ERR_HIP once ("invalid ticket schedule") */
int ilqg_solver_debug_plant_schedule(ilqg_solver* s, unsigned slot, unsigned item);
void* ilqg_solver_stream(ilqg_solver* s); /* hipStream_t */
/* enqueue subsequent hot-path launches on an external stream (hipStream_t,
   e.g. torch's current stream) instead of the solver's own; NULL restores it */
int ilqg_solver_set_stream(ilqg_solver* s, void* stream);
/* per-kernel HIP-event timing of the hot path, recorded on the launch stream:
   index 0 rollout, 1 select, 2 fd_centre, 3 fd_cols (or the fused sweep run
   alone), 4 backward, 5 fd_backward (the fused sweep with the backward pass
   streamed behind it: ilqg_iterate on cooperative models) */
#define ILQG_NKERNEL 6
int ilqg_solver_set_timing(ilqg_solver* s, int enable);
/* synchronises; returns summed device ms and launch counts per kernel, then resets */
int ilqg_solver_get_timing(ilqg_solver* s, double* ms, int* launches);
/* How the Riccati recursion reads the FD records (Differentiator::
   updateDerivatives, inc/differentiator.h:85-93).  REFERENCE (default): as the
   reference does -- Eigen column-major maps of the row-major deriv blocks
   (differentiator.h:57-59), i.e. A's lower blocks are
   dt J^T and B's lower block is a permutation of dt J_u when nu > 1.
   CORRECTED: the true linearisation, A lower = [dt J_q, I + dt J_v], B lower =
   dt J_u (SURVEY.md Appendix A Q1 "provide a corrected mode").  The FD records
   themselves (ilqg_solver_get_deriv) are the reference's either way. */
#define ILQG_LAYOUT_REFERENCE 0
#define ILQG_LAYOUT_CORRECTED 1
int ilqg_solver_set_layout(ilqg_solver* s, int layout);
/* initV override (virtual ILQR::initV, inc/ilqr.h:100-107,142): the next
   backward pass (ilqg_backward or ilqg_iterate) starts its recursion from
   these V0 (nseed x nx x nx, column-major) and v0 (nseed x nx) instead of the
   terminal point's v = dgdx, V = v'v.  One-shot: later passes use initV. */
int ilqg_solver_set_value(ilqg_solver* s, const double* V, const double* v);
/* Levenberg-Marquardt constant mu (the public ILQR::mu, inc/ilqr.h:65, read
   by every backward step at inc/ilqr.h:166): used by every backward pass
   enqueued after the call (opts.mu at creation until then).  NaN is refused. */
int ilqg_solver_set_mu(ilqg_solver* s, double mu);
/* Control limits: a box-constrained backward pass and a clamped rollout.  The
   reference has no counterpart (inc/ilqr.h solves the unconstrained
   Quu k = ..., stores u unclamped and leaves any clipping to the physics); an
   extension in the spirit of ILQG_LAYOUT_CORRECTED, off by default.
   lo, hi: nu doubles each, lo <= hi, +-inf = unbounded on that side.  Both
   NULL switches the feature off again (ilqg_iterate is then the solver's as
   created, the fused sweep included).  ILQG_ERR_ARG: lo[a] > hi[a], any NaN,
   exactly one of lo, hi NULL.  Synchronises like ilqg_solver_set_mu and applies
   to every launch enqueued after it.  With limits on:
   - ilqg_backward (and the backward pass ilqg_iterate ends in) solves, per
     step, min 1/2 k'Quu k + Qu'k over lo - u* <= k <= hi - u* by projected
     Newton (Tassa, Mansard & Todorov 2014); clamped controls get zero rows of
     K, free ones the free block's gains; a step whose unconstrained k lies
     inside the box is the exact engine's, bit for bit.  A free block that is
     not definite (mu = 0 rank-one cases) or an exhausted iteration cap takes
     the fallback: k = clip(unconstrained k), zero K rows where it clipped.
   - ilqg_forward stores and charges u = clip(K(x - x*) + alpha k + u*); the
     constructor's passive rollout and the FD sweep are untouched.
   - ilqg_iterate runs rollout, selection, sweep, ilqg_backward unfused.
   ILQG_ERR_UNSUPPORTED, from whichever call comes second: with the MFMA
   engine, with seed groups > 1, and from the forward calls when ILQG_DUAL=0
   selects a rollout kernel without a clamped variant.  fp32 FD, both layouts,
   set_value, set_mu, set_deriv and ilqg_forward_sharded compose with limits.
   Limits wider than a ctrllimited model's own ctrlrange leave the physics
   clipping inside them: pass ilqg_model_ctrlrange's arrays. */
int ilqg_solver_set_ctrl_limits(ilqg_solver* s, const double* lo, const double* hi);
/* the limits in force (-inf / +inf when off) and whether they are on; any
   pointer may be NULL.  No counterpart in the reference. */
int ilqg_solver_get_ctrl_limits(ilqg_solver* s, double* lo, double* hi, int* enabled);
/* after a backward pass with limits, per (seed, point) (nseed x (N+1) words
   each, either may be NULL): mask, bit a = control a clamped in that step's
   solution; info, the step's QP iterations, bit 31 = the fallback was taken.
   Point 0 (no step) and every entry after a pass without limits read 0.
   Synchronises.  No counterpart in the reference. */
int ilqg_solver_get_clamped(ilqg_solver* s, unsigned* mask, unsigned* info);
/* Cost schedule: one cost row per trajectory point, resident on the device and
   shared by every seed (ilqg_solver_set_cost_schedule_seeds below: a table per
   seed); off by default.  No counterpart in the reference: it
   stands in for a stepCostFn_t (inc/mjderivative.h:5) that reads d->time, i.e.
   a running cost that moves over the horizon, and a terminal cost of its own.
   rows: (N+1) x C doubles, C = 3 (nq + nv + nu); row p, the cost of point p, is
   the ilqg_cost arrays packed as wq[nq] tq[nq] lq[nq] wv[nv] tv[nv] lv[nv]
   wu[nu] tu[nu] lu[nu].  Point 0 is the terminal point (initV reads its
   record, so row 0 is the terminal cost) and point N the first applied control.
   NULL switches the feature off: the solver is then exactly as created.  Any
   non-finite entry is ILQG_ERR_ARG.  Synchronises like ilqg_solver_set_mu and
   applies to every launch enqueued after it.  With a schedule on:
   - ilqg_forward (and the rollout inside ilqg_iterate / ilqg_forward_sharded)
     charges a candidate with sum_n step_cost(row n; x_n, u_n), n = N .. 0, the
     terms of a point in ilqg_cost's order; selection works on these costs.
   - the FD sweep (fused, unfused, ilqg_fd_sweep_range, fp32) takes costCenter
     and every perturbed cost of point p from row p.
   - the Riccati engines consume records and are unchanged; the constructor's
     passive rollout, ilqg_fd_batch and the legacy layer keep the creation cost.
   Composes with both layouts, set_mu, set_value, set_deriv, control limits,
   fp32 FD, the MFMA engine, seed groups (every group reads the same rows) and
   ilqg_forward_sharded.  ILQG_ERR_UNSUPPORTED, from whichever call comes
   second: from the forward calls when ILQG_DUAL=0 selects a rollout kernel
   without a scheduled variant.
   On a solver with a per-seed schedule this call replaces it by the shared
   one, and NULL switches it off. */
int ilqg_solver_set_cost_schedule(ilqg_solver* s, const double* rows);
/* the rows in force, (N+1) x C, and whether a schedule is on; either pointer
   may be NULL.  While off every row reads as the creation cost.  No counterpart
   in the reference (it stands in for reading back such a stepCostFn_t's state).
   While a per-seed schedule is in force enabled reads 1 and a non-NULL rows is
   ILQG_ERR_ARG: there is no single table to return. */
int ilqg_solver_get_cost_schedule(ilqg_solver* s, double* rows, int* enabled);
/* the receding-horizon tick of a schedule: the window advances n steps, row p
   takes row p - n for p >= n and rows 0 .. n-1 take new_rows (n x C).  No
   counterpart in the reference: a stepCostFn_t that reads d->time follows the
   advancing clock by itself.  ILQG_ERR_ARG while the schedule is off, for
   n < 1 or n > N+1, and for new_rows NULL or non-finite.  Synchronises.
   While a per-seed schedule is in force every seed's table advances and takes
   the same n new rows. */
int ilqg_solver_shift_cost_schedule(ilqg_solver* s, int n, const double* new_rows);
/* Per-seed cost schedule: every seed, an MPC problem of its own, tracks a
   reference of its own.  rows: nseed x (N+1) x C doubles, seed s's table at
   rows + s (N+1) C; the row packing and the point indexing are those of
   ilqg_solver_set_cost_schedule, row [s][0] is seed s's terminal cost.  It
   replaces a shared schedule if one is set; NULL switches every schedule off
   (the solver is then exactly as created); a non-finite entry is ILQG_ERR_ARG.
   Synchronises like ilqg_solver_set_mu, invalidates the regularisation mode's
   nominal cost, and keeps two nseed x (N+1) x C tables on the device.
   Everywhere a shared schedule reads row p, seed s now reads row [s][p]: the
   rollout, every FD sweep (fused, unfused, ilqg_fd_sweep_range, fp32, the tail
   records of ilqg_solver_shift_horizon) and the STANDARD recursion's lxx / luu,
   with s the solver's seed index in every launch -- a seed group reads its own
   seeds' rows, and under ilqg_forward_sharded every rank holds the full table.
   Composes with whatever the shared schedule composes with, the same
   ILQG_DUAL=0 refusal included; the constructor's passive rollout,
   ilqg_fd_batch and the legacy layer keep the creation cost.  No counterpart
   in the reference. */
int ilqg_solver_set_cost_schedule_seeds(ilqg_solver* s, const double* rows);
/* every seed's rows in force, nseed x (N+1) x C, and whether a per-seed table
   is in force; either pointer may be NULL.  per_seed = 0 with a shared
   schedule (each seed's block then reads as the shared rows) and while off
   (each block reads as the creation cost). */
int ilqg_solver_get_cost_schedule_seeds(ilqg_solver* s, double* rows, int* per_seed);
/* the per-seed receding-horizon tick: for every seed s, row [s][p] takes row
   [s][p - n] for p >= n and rows [s][0 .. n-1] take new_rows[s] (new_rows:
   nseed x n x C).  The argument checks of ilqg_solver_shift_cost_schedule;
   ILQG_ERR_ARG unless a per-seed table is in force.  Synchronises. */
int ilqg_solver_shift_cost_schedule_seeds(ilqg_solver* s, int n, const double* new_rows);
/* Horizon shift: the receding-horizon tick of the nominal trajectory, the gains
   and the FD records, on the device.  The reference has no counterpart: its
   driver reuses dArray unshifted as the next nominal.  Per seed,
   with points indexed as everywhere (p = N now, p = 0 terminal):
   1. move: for p = N .. n every per-point array takes the entry of old point
      p - n -- the trajectory's five fields, K[p] and k[p], the FD record p (its
      whole padded slot) -- in place: the pointers ilqg_solver_device_traj,
      ilqg_solver_device_deriv and ilqg_solver_device_costs hand out stay valid;
   2. tail: points n-1 .. 0 continue the rollout past the old terminal point
      holding its control: from new point n one mj_step with the stored ctrl[n]
      (forwardPass after storing a point, inc/ilqr.h:127-128), the resulting
      time, qpos, qvel, qacc_warmstart stored as point n-1 with ctrl[n-1] =
      ctrl[n], and so on down to point 0.  The seed's qfrc_applied /
      xfrc_applied apply; control limits do not re-clamp the held control (it
      was stored clamped).  K[p] = 0 and k[p] = 0 for p < n;
   3. tail records: the FD records of points 0 .. n-1 are swept behind the
      tail on the same stream, by the kernels of ilqg_fd_sweep_range(s, 0, n)
      launched once for every seed (the same records): the FD precision that
      is set and the cost rows in force at that moment, seed by seed -- with a
      schedule the tick is ilqg_solver_shift_cost_schedule (or its _seeds
      form), then this call, and a moved
      record is still the record of its point under its row;
   4. dinit takes new point N, the nominal's prediction of "now", so that
      ilqg_iterate can follow with no host call; a later ilqg_solver_set_dinit
      overrides it as ever.
   Enqueued on the solver's stream: no synchronisation, nothing copied to or
   from the host (the first call on a solver allocates the tail's staging
   buffers, a second trajectory and record array, zeroed in stream).
   Seed groups wait for it as for ilqg_fd_sweep_range; under
   ilqg_forward_sharded every rank shifts identically and sweeps the n tail
   points itself.  Stale by construction afterwards: ilqg_solver_get_value and
   ilqg_solver_get_costs keep the last pass's values, ilqg_solver_get_clamped
   reads 0 until the next boxed pass, and in the regularisation mode the nominal
   cost is invalid (mu, dmu, status and the trace are untouched;
   ilqg_solver_refresh_nominal recomputes the shifted nominal's cost on the
   device and makes it valid again).  With ilqg_solver_set_timing
   the move and the tail's store count under index 1, the tail's rollout under
   0, the tail sweep under 3.
   ILQG_ERR_ARG: s NULL or not initialised, n < 1, n > N, tail not
   ILQG_TAIL_HOLD (the only tail built; a zero-control tail is not).  Composes
   with both layouts and recursions, limits, the cost schedule, fp32 FD, the
   MFMA engine and seed groups, and changes no refusal. */
#define ILQG_TAIL_HOLD 0
int ilqg_solver_shift_horizon(ilqg_solver* s, int n, int tail);
/* Nominal refresh: the stored nominal trajectory's cost, valid again on the
   device -- what the regularisation mode's accept test needs after a
   receding-horizon tick, where every step is the first one after a shift.  The
   reference has no counterpart: its forwardPass (inc/ilqr.h:116-130) keeps no
   trajectory cost and accepts every step.  Works with the regularisation mode
   on or off.  Enqueued on the solver's stream: no synchronisation, nothing
   copied to or from the host (REROLL's first call allocates one double,
   zeroed in stream).
   ILQG_NOMINAL_COST: per seed s, the cost of the stored nominal under the cost
   rows in force at that moment -- row [s][n] of a per-seed schedule, row n of a
   shared one, else the creation cost -- summed exactly as the rollout charges
   a candidate: c = 0; for n = N .. 0: c += step_cost(row n; qpos_n, qvel_n,
   ctrl_n), a point's terms in ilqg_cost's order.  It is, bit for bit, what
   ilqg_forward wrote for the candidate that became this nominal.  Written to
   the selected-cost buffer (ilqg_solver_device_costs) always, and in the
   regularisation mode to cost_nom[s] with valid[s] = 1.  Untouched: the
   trajectory, dinit, the gains, the FD records, the selection and the
   candidate costs (ilqg_solver_get_costs), dV, mu, dmu, retries and the trace
   (it does not advance).
   ILQG_NOMINAL_REROLL: the stored policy rolled out from dinit with
   feed-forward scale 0, u_n = K_n (x_n - x*_n) + 0 k_n + u*_n, clamped while
   control limits are on, charged under the rows in force, the seed's applied
   forces applied; the result becomes the nominal unconditionally.  Every array
   comes out as ilqg_forward leaves it on a solver created with nalpha = 1,
   alphas = {0.0}, select_mode = 0 and given the same nominal, gains and dinit:
   the trajectory's five fields, dinit (= new point N) and the selected cost,
   bit for bit; then cost_nom / valid as under COST.  The gains stay; the FD
   records are now those of the old nominal -- ilqg_iterate sweeps again behind
   its own rollout, ilqg_backward alone would read stale records.  The
   ILQG_DUAL=0 refusals of the forward calls apply.  After
   ilqg_solver_set_dinit(measured state) this is the nominal the accept test
   must compare against.
   ILQG_NOMINAL_RESUME (a flag, with COST or REROLL; needs the regularisation
   mode on): a seed
   whose status is 1 (converged on the window that has moved on) runs again,
   status 0; status 2, mu and dmu stay.  Without the flag the status is kept.
   ILQG_ERR_ARG, nothing changed: s NULL or not initialised, an unknown mode or
   flag bit, RESUME while the regularisation mode is off.
   Seed groups wait for it as for ilqg_solver_shift_horizon; under
   ilqg_forward_sharded every rank calls it identically.  With
   ilqg_solver_set_timing the cost kernel counts under index 1, REROLL's
   rollout under 0.  Composes with both layouts and recursions, control limits,
   both cost schedules, fp32 FD, the MFMA engine, seed groups and models with
   nq != nv, and lifts no refusal. */
#define ILQG_NOMINAL_COST 0
#define ILQG_NOMINAL_REROLL 1
#define ILQG_NOMINAL_RESUME 1u
int ilqg_solver_refresh_nominal(ilqg_solver* s, int mode, unsigned flags);
/* Recursion mode.  REFERENCE (default): the backward step of inc/ilqr.h:157-174
   as the reference wrote it (outer products of the FD cost gradients for
   Hessians, mu added to V and kept, factors of 2: SURVEY.md Appendix A Q13,
   Q15, Q16).  STANDARD replaces inc/ilqr.h:157-174 by the textbook iLQR step
   in deviation coordinates about the nominal trajectory (no c term); the
   reference has no counterpart.  For step n = 1..N, with A, B assembled from
   record n as today (either layout), q = dgdx, r = dgdu of record n,
   lxx = 2 diag(wq, wv) and luu = 2 diag(wu) the exact Hessians of ilqg_cost
   (row n of the cost schedule when one is on, else the creation cost; with
   set_deriv still the solver's cost) and mu from opts.mu / set_mu:
     Qx = q + A'v   Qu = r + B'v   Qxx = lxx + A'VA   Qux = B'VA   Quu = luu + B'VB
     Quu_r = luu + B'(V + mu I)B   Qux_r = B'(V + mu I)A   (Tassa, Erez & Todorov 2012, eq. 10)
     k = -Quu_r^-1 Qu   K = -Quu_r^-1 Qux_r   dV1 += k'Qu   dV2 += 1/2 k'Quu k
     v <- Qx + K'Quu k + K'Qu + Qux'k
     V <- Qxx + K'Quu K + K'Qux + Qux'K ;  V <- (V + V')/2
   (evaluated in the algebraically equal closed-loop form V = lxx + K'luu K +
   (A+BK)'V(A+BK)); the regulariser does not enter the value update.  The
   recursion starts from v = dgdx of record 0 and V = lxx of row 0, or from
   ilqg_solver_set_value's arrays for one pass.  K, k keep their layouts: the
   rollout's law u = K(x - x*) + alpha k + u* is the one this step assumes.
   Indefinite step: Quu_r is factored by the pivoted LDLT; a pivot <= 0 or NaN
   (or a non-finite gain) makes the step take K = 0, k = 0 and add nothing to
   dV -- V, v go on as for an uncontrolled step -- and flags it.
   Meant for ILQG_LAYOUT_CORRECTED: in the reference layout with nu > 1 the
   step reads permuted Jacobians and the cost rises (not enforced).
   Synchronises like ilqg_solver_set_mu and applies to every backward pass
   enqueued after it; any other mode is ILQG_ERR_ARG.  With STANDARD on,
   ilqg_iterate runs rollout, selection, sweep, ilqg_backward unfused (as with
   control limits); REFERENCE restores the solver exactly as created, the
   fused sweep included.  Composes with both layouts, set_mu, set_value,
   set_deriv, fp32 FD, the cost schedule, select_mode 0 and 1, and
   ilqg_forward_sharded.  Not built here -- ILQG_ERR_UNSUPPORTED, from whichever
   call comes second: a model with nq != nv (the humanoid: the tangent-space
   Hessian of a quaternion term is not diagonal), the MFMA engine, control
   limits, seed groups > 1.  Also not built: a fused/streamed or register
   formulation, the semi-implicit top block of A (Q10).  The mu schedule and
   the accept test are ilqg_solver_set_regularization below. */
#define ILQG_RECURSION_REFERENCE 0
#define ILQG_RECURSION_STANDARD 1
int ilqg_solver_set_recursion(ilqg_solver* s, int mode);
/* the last backward pass's expected change of the trajectory cost, per seed:
   dV[nseed][2] = dV1 (linear term, sum of k'Qu) and dV2 (quadratic term, sum of
   1/2 k'Quu k), so a step of feed-forward scale alpha is expected to change
   the cost by alpha dV1 + alpha^2 dV2 (accept test: the actual change over
   that, both negative); first_bad[nseed] = the smallest step n that took the
   indefinite-step fallback, or -1.  Either pointer may be NULL.  After a
   REFERENCE pass dV reads 0 and first_bad -1: inc/ilqr.h:157-174, which the
   STANDARD step replaces, reports neither (no counterpart).  Synchronises. */
int ilqg_solver_get_expected(ilqg_solver* s, double* dV, int* first_bad);
/* Regularisation mode: the iLQR outer loop (Tassa, Erez & Todorov 2012, II-F)
   on the device, per seed and without a host sync -- step acceptance, the
   mu / dmu schedule, a backward pass that restarts at a larger mu, a stop.
   Off by default; needs ILQG_RECURSION_STANDARD; the reference has no
   counterpart.  Per seed the device keeps mu, dmu, the nominal trajectory's
   cost and whether it is valid, a status (0 running, 1 converged, 2 mu reached
   mu_max) and the restart count of the last backward pass.  Every expression
   below is fp64, evaluated in the order written (f = factor):
     increase:  dmu = max(dmu f, f);  mu = max(mu dmu, mu_min);  mu >= mu_max: status = 2
     decrease:  dmu = min(dmu / f, 1 / f);  t = mu dmu;  mu = t > mu_min ? t : 0
   ilqg_solver_set_regularization(s, opts) switches the mode on: mu[s] = the
   solver's mu (opts.mu at creation or the last ilqg_solver_set_mu), dmu = 1,
   status 0, the nominal cost invalid, the trace empty.  NULL switches it off:
   the solver is then exactly as it was before.  ILQG_ERR_ARG unless
   factor > 1, mu_min >= 0, mu_max > mu_min, zmin >= 0, tol_cost >= 0,
   0 <= max_retry <= ILQG_REG_MAXRETRY, 0 <= trace_len <= ILQG_REG_MAXTRACE.
   Synchronises like ilqg_solver_set_mu.  With the mode on:
   - ilqg_forward (and the one inside ilqg_iterate) decides the step per seed.
     For candidate a, actual = cost_nom - cost[a] and expected =
     -(alpha_a dV1 + alpha_a alpha_a dV2) with the last backward pass's dV; a is
     acceptable when actual > 0 && actual >= zmin expected (a NaN fails both).
     select_mode 1 takes the acceptable candidate of lowest cost (a tie: the
     lower index), select_mode 0 tests candidate 0 only.  Accepted: the
     candidate becomes the nominal trajectory and dinit, cost_nom its cost, the
     decrease is applied, and status becomes 1 when actual < tol_cost.
     Rejected: the nominal trajectory, dinit and the selected cost
     (ilqg_solver_device_costs) are untouched, ilqg_solver_get_costs reports
     selected = -1 (only in this mode), and the increase is applied.  A seed
     whose status is not 0 is frozen: every step is rejected and mu stays.
     While the nominal cost is invalid the choice is the plain selection's,
     unconditionally, and mu stays; it is invalid after enabling the mode and
     after ilqg_solver_init, set_traj, set_dinit, set_gains,
     set_cost_schedule, shift_cost_schedule (and their _seeds forms) and
     shift_horizon; ilqg_solver_refresh_nominal makes it valid again.
   - ilqg_backward (and the one inside ilqg_iterate) reads mu[s].  A step that
     is indefinite by the STANDARD test raises mu (the increase) and restarts
     the recursion from step 1, from the same V0, v0 (ilqg_solver_set_value's
     on every attempt of that pass), while fewer than max_retry restarts were
     used and status is 0; otherwise the pass completes with the STANDARD
     fallback and first_bad.  dV and first_bad are the last attempt's.  A pass
     costs at most max_retry + 1 plain ones.
   - ilqg_iterate runs rollout, acceptance, sweep, ilqg_backward unfused.  The
     sweep of a rejected seed is not skipped: it reproduces its records.
   - ilqg_solver_set_mu sets every seed's mu (dmu = 1, status = 0).
   Composes with both layouts, the cost schedule, fp32 FD, set_value,
   set_deriv and both select_modes.  ILQG_ERR_UNSUPPORTED, from whichever call
   comes second: ILQG_RECURSION_REFERENCE (so also everything STANDARD
   refuses), and ilqg_forward_sharded while the mode is on. */
#define ILQG_REG_MAXRETRY 16
#define ILQG_REG_MAXTRACE 1024
#define ILQG_REG_TRACE 8
typedef struct ilqg_reg_opts {
  double factor;   /* f > 1 (Tassa: 1.6) */
  double mu_min;   /* >= 0 (1e-6) */
  double mu_max;   /* > mu_min (1e10) */
  double zmin;     /* >= 0: the least accepted actual / expected */
  double tol_cost; /* >= 0, absolute: an accepted reduction below it ends the seed (status 1) */
  int max_retry;   /* restarts of one backward pass, 0 .. ILQG_REG_MAXRETRY */
  int trace_len;   /* iterations kept in the trace ring, 0 .. ILQG_REG_MAXTRACE */
} ilqg_reg_opts;
int ilqg_solver_set_regularization(ilqg_solver* s, const ilqg_reg_opts* opts);
/* the options in force (zeros while off) and whether the mode is on; either
   pointer may be NULL */
int ilqg_solver_get_regularization(ilqg_solver* s, ilqg_reg_opts* opts, int* enabled);
/* the per-seed state, nseed entries each, any pointer may be NULL; valid:
   whether cost_nom is the nominal trajectory's cost.  ILQG_ERR_ARG while the
   mode is off.  Synchronises. */
int ilqg_solver_get_reg_state(ilqg_solver* s, double* mu, double* dmu, double* cost_nom, int* valid, int* status,
                              int* retries);
/* mu per seed (nseed values, finite and >= 0); resets dmu to 1 and status to 0.
   ILQG_ERR_ARG while the mode is off.  Synchronises. */
int ilqg_solver_set_reg_mu(ilqg_solver* s, const double* mu);
/* the trace, oldest iteration first: *len iterations (at most trace_len) of
   nseed x ILQG_REG_TRACE doubles; trace may be NULL (the length alone) and
   must hold trace_len iterations otherwise.  One iteration = one ilqg_forward
   and the ilqg_backward after it.  Per (iteration, seed):
     0 the nominal cost before (NaN while invalid)   1 the best candidate's cost
     2 the chosen index, or -1                       3 the expected reduction of the
     4 mu before the decision                          tested candidate (NaN while invalid)
     5 mu after it                                   6 mu after the backward pass
     7 restarts + 100 status after the backward pass (6, 7: NaN until it ran)
   so N ilqg_iterate calls can be enqueued back to back and the history read
   once.  ILQG_ERR_ARG while the mode is off.  Synchronises. */
int ilqg_solver_get_reg_trace(ilqg_solver* s, double* trace, int* len);
/* Riccati recursion (inc/ilqr.h:133-176) engine.  EXACT (default): the
   oracle's loops, bit-identical K, k, V, v (streamed behind the FD sweep on
   cooperative models).  MFMA: every matrix product (B'V, Quu = -2B'VB - 2R,
   Qux = B'VA, A + BK, (A+BK)'V(A+BK), K'RK) on the fp64 matrix cores
   (v_mfma_f64_16x16x4_f64), four wavefronts per seed -- the north star's
   "MFMA on the Quu/Qux block products" for large nu x nx (humanoid 21 x 54);
   results agree with EXACT to rounding (product sums in the matrix core's
   order).  BASELINE.json configs[4]. */
#define ILQG_RICCATI_EXACT 0
#define ILQG_RICCATI_MFMA 1
int ilqg_solver_set_riccati(ilqg_solver* s, int mode);
/* FD sweep precision (calcMJDerivatives, src/mjderivative.cpp:212-255).  F64
   (default): the reference's fp64 arithmetic and eps = 1e-6, bit-identical to
   the oracle.  F32: BASELINE.json configs[4]'s "fp32 FD with fp64 Riccati" --
   the physics of every FD evaluation in fp32 (workspace, state and arithmetic;
   the model stays fp64), eps = ILQG_FD32_EPS (1e-6 is below fp32 resolution,
   SURVEY.md §7(g)), fp64 records for the fp64 (exact or MFMA) recursion.
   Agrees with the fp64 oracle at the same eps to the tolerance stated in
   tests/test_gpu_parity.py (fp32 rounding amplified by 1/(2 eps)). */
#define ILQG_FD_F64 0
#define ILQG_FD_F32 1
#define ILQG_FD32_EPS 1e-3
int ilqg_solver_set_fd_precision(ilqg_solver* s, int prec);
/* Seed groups: ilqg_iterate runs the seeds as ngroups (1..4, <= nseed)
   contiguous ranges, software-pipelined -- each group's rollout on a stream
   CU-masked to XCDs of its own, its fused FD sweep + recursion on a stream
   masked to the rest, and group g's rollout of an iteration behind group
   g - 1's, so one group's sweep runs beside the next group's (latency-bound)
   rollout.  Every seed's launches and results are the ungrouped iterate's (bit
   for bit); only the overlap between independent seeds changes.  Work enqueued
   on the solver's stream after ilqg_iterate waits for every group; the groups
   wait for work on that stream only when it came through this API (ilqg_forward,
   ilqg_fd_sweep, ilqg_backward, set_stream, join_stream ...) -- work of your
   own enqueued there (a collective reading the costs) must be followed by
   ilqg_solver_join_stream before the next ilqg_iterate.  The seeds of MahanFathi/iLQG-MuJoCo's
   driver are independent (one ILQR per MPC problem, inc/ilqr.h:52-71), so
   the reference has no counterpart call.  ILQG_ERR_UNSUPPORTED unless the fused
   sweep is in use (fp64 FD, exact recursion, cooperative model); 1 restores
   the ungrouped iterate.  get_groups: the count and the CUs of each group's
   rollout mask (0: unmasked). */
int ilqg_solver_set_groups(ilqg_solver* s, int ngroups);
int ilqg_solver_get_groups(ilqg_solver* s, int* ngroups, int* rollout_cus);
/* the next ilqg_iterate's seed groups wait for everything enqueued on the
   solver's stream up to now (work of the caller's own, e.g. the RCCL cost
   all-gather, which reads the buffers the next rollout writes); without
   groups every launch is on that stream anyway and this is a no-op */
int ilqg_solver_join_stream(ilqg_solver* s);
/* sha256 prefix (16 hex digits) of the sources this library was built from
   (all of csrc, Makefile; the same digest as ilqg_amd.source_sha()): the host
   refuses a library whose digest differs from the sources beside it */
const char* ilqg_source_sha(void);
/* device pointer to the per-seed selected-candidate cost (nseed doubles), for
   an in-stream collective (RCCL all-gather) without a host round trip */
int ilqg_solver_device_costs(ilqg_solver* s, double** dptr);
/* device pointer to the resident FD records, [nseed][N+1][stride] doubles
   (stride >= D: each record padded to whole 128-byte lines) */
int ilqg_solver_device_deriv(ilqg_solver* s, double** dptr, int* stride);
/* device pointer to the resident nominal trajectory (field 0 time, 1 qpos,
   2 qvel, 3 warm, 4 ctrl; seed-major [nseed][N+1][...], point N = the first
   applied control): the multi-GPU MPC broadcast of the winning seed's first
   control reads it in place */
int ilqg_solver_device_traj(ilqg_solver* s, int field, double** dptr);
/* test hook: q[i] = a[i] / b[i] (host arrays, n <= 2^24) through the device's
   split fp64 division (divisor reciprocal computed ahead, dsmall.h rcp_ref /
   div_ref), both the every-lane and the one-lane form; q2 may be NULL.  The
   physics kernels use it for the Cholesky solve and the line search, so it
   must equal IEEE division bit for bit */
int ilqg_selftest_div(const double* a, const double* b, double* q, double* q2, int n);
#ifdef __cplusplus
}
#endif
#endif
