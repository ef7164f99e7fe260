// Launch interface of the hot-path kernels (kernels_rollout.hip, kernels_fd.hip, riccati.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "dmodel.h"

namespace ilqg {

// trajectory / state arrays on the device, [point][field]
struct TrajDev {
  double* time;
  double* qpos;
  double* qvel;
  double* warm;
  double* ctrl;
};

// a rollout launch over points n_hi .. n_lo (descending) of the horizon: the
// whole trajectory (n_hi < 0, the default), or one chunk of a chunked rollout
// whose FD sweep runs behind it (ilqg_iterate's pipelined path).  A chunk that
// does not start at point P-1 takes its state from carry[candidate] and adds
// to the candidate's cost already in cost_cand; one that does not end at
// point 0 leaves its state in carry[candidate].
struct RollChunk {
  TrajDev carry{};
  int n_hi = -1, n_lo = 0;
  // set by launch_rollout_coop (two-wave generic kernel): the nominal record
  // double-buffered in LDS past the team's workspace, the next point's copied
  // by the helper wave while the primary runs the constraint solve
  int dbuf = 0;
  // control limits (ilqg_solver_set_ctrl_limits): lo[nu] then hi[nu] on the
  // device, read by the clamped rollout kernels only; null = no limits
  const double* ulim = nullptr;
};

// device cost descriptor (all 9 arrays present, zero where unused)
struct CostDev {
  const double *wq, *tq, *lq, *wv, *tv, *lv, *wu, *tu, *lu;
};
// Cost schedule (ilqg_solver_set_cost_schedule): the descriptor's arrays are
// row 0 of a [point][3 (nq + nv + nu)] table, packed wq tq lq wv tv lv wu tu lu,
// and point p is charged with the row `stride` doubles further on per point.
// The launches below take the stride as `cstride` (0 = one stationary cost:
// the kernels they always launched); != 0 launches the kernels' scheduled
// instances (<.., int, int>), which carry it as an extra kernel argument.
// Per-seed schedule (ilqg_solver_set_cost_schedule_seeds): a second stride,
// `sstride`, the doubles from one seed's table to the next (0 = one table shared
// by every seed), the scheduled instances' last argument.  Row (s, p) is
// cost_at(c, p, cstride) advanced by s * sstride, s the GLOBAL seed: a launch
// over seeds s0 .. takes the descriptor of seed s0's table, as it takes every
// other per-seed array from seed s0 on, and its kernels advance by their own
// seed index.
__host__ __device__ inline CostDev cost_at(const CostDev& c, int p, int stride) {
  const size_t o = (size_t)p * (size_t)stride;
  return CostDev{c.wq + o, c.tq + o, c.lq + o, c.wv + o, c.tv + o, c.lv + o, c.wu + o, c.tu + o, c.lu + o};
}
__host__ __device__ inline CostDev cost_at(const CostDev& c, int s, int sstride, int p, int stride) {
  const size_t o = (size_t)s * (size_t)sstride + (size_t)p * (size_t)stride;
  return CostDev{c.wq + o, c.tq + o, c.lq + o, c.wv + o, c.tv + o, c.lv + o, c.wu + o, c.tu + o, c.lu + o};
}

// How the Riccati recursion reads an FD record (ilqg_solver_set_layout).
// The record is always the reference's (row-major by output, mjderivative.cpp:
// 107,138,202).  REFERENCE: A's lower blocks and B are Eigen column-major maps
// of those row-major blocks (differentiator.h:57-59,89-92, quirk Q1: dt J^T,
// and a permuted dt J_u for nu > 1).  CORRECTED: the true Jacobians, dt J and
// dt J_u.  The recursion stages entry e of a record from record index
// rec_src(e): identity in the reference layout, the three Jacobian blocks
// transposed in the corrected one.
struct RicFlags {
  int layout;  // 0 reference, 1 corrected
  int vinit;   // 1: V0 / v0 are read from V / v instead of initV's (inc/ilqr.h:100-107)
  int ldlt_lds = 0;  // k_backward_mfma<27, 21>: 1 the LDS-resident LDLT instead of ldlt_factor_reg_t, 2 its pivot replay forced (ILQG_LDLT_REG)
};
__host__ __device__ inline int rec_src(int e, int nv, int nu, int layout) {
  if (!layout) return e;
  const int nn = nv * nv;
  if (e < 2 * nn) {  // A block b (0 qpos, 1 qvel): staged (r + c nv) <- record (c + r nv)
    const int b = e >= nn, f = e - b * nn, r = f % nv, c = f / nv;
    return b * nn + c + r * nv;
  }
  if (e < 2 * nn + nv * nu) {  // B: staged (r + a nv) <- record (a + r nu)
    const int f = e - 2 * nn, r = f % nv, a = f / nv;
    return 2 * nn + a + r * nu;
  }
  return e;  // cost gradients
}

// candidate selection + setDInit(dArray[N])
hipError_t launch_selftest_div(const double* a, const double* b, double* q, double* q2, int n, hipStream_t st);
hipError_t launch_select(const DevModel& m, int S, int A, int P, int mode, int copy_cand, const double* cost_cand,
                         int* sel, double* cost_sel, TrajDev cand, TrajDev nominal, TrajDev dinit, hipStream_t st);
// Riccati backward pass, one workgroup per seed
// deriv records at stride Ds (>= D) doubles
hipError_t launch_backward(const DevModel& m, int S, int P, double mu, const double* deriv, int Ds, TrajDev tr,
                           double* K, double* k, double* V, double* v, RicFlags fl, hipStream_t st);
size_t backward_lds_bytes(int nv, int nu);
// the boxed recursion (ilqg_solver_set_ctrl_limits; riccati.h backward_seed
// with BOX): each step's feed-forward solves min 1/2 k'(-Mm)k + col'k over
// lo - u* <= k <= hi - u* by projected Newton, the clamped controls' gain rows
// are zero.  lo, hi: nu doubles each on the device; mask, info: [S][P] words
// (bit a of mask = control a clamped; info = QP iterations, bit 31 = fallback)
struct BoxDev {
  const double* lo = nullptr;
  const double* hi = nullptr;
  unsigned* mask = nullptr;
  unsigned* info = nullptr;
};
hipError_t launch_backward_box(const DevModel& m, int S, int P, double mu, const double* deriv, int Ds, TrajDev tr,
                               double* K, double* k, double* V, double* v, RicFlags fl, BoxDev bx, hipStream_t st);
size_t backward_box_lds_bytes(int nv, int nu);
// the standard recursion (ilqg_solver_set_recursion; riccati.h backward_seed
// with STD): exact diagonal cost Hessians from the cost row of each step's
// point (seed s: cost_at(cost, s, sstride, n, cstride)), mu in Quu / Qux only, no c term.  dV:
// [S][2], the expected reduction's linear and quadratic terms; bad: [S], the
// first step that took the indefinite-step fallback (K = 0, k = 0), or -1.
// Models with nq == nv only (the caller checks).
struct StdDev {
  CostDev cost{};
  int cstride = 0;
  int sstride = 0;
  double* dV = nullptr;
  int* bad = nullptr;
};
hipError_t launch_backward_std(const DevModel& m, int S, int P, double mu, const double* deriv, int Ds, TrajDev tr,
                               double* K, double* k, double* V, double* v, RicFlags fl, StdDev sd, hipStream_t st);
size_t backward_std_lds_bytes(int nv, int nu);
// the regularisation mode (ilqg_solver_set_regularization; "Reg" here is the
// Levenberg-Marquardt schedule, not riccati_reg.h's register formulation):
// per-seed state resident on the device, [S] each.  k_accept (kernels_rollout.hip)
// decides a step from cost_nom and the last pass's dV and moves mu; the STD
// recursion's restarting instances (k_backward_std_reg) read mu[s] and raise it
// when a step is indefinite.  Every expression of the schedule is fp64 in the
// order written in reg_increase / reg_decrease: the host reference evaluates
// the same expressions and the decisions agree bit for bit.
constexpr int REG_MAXRETRY = 16;  // ILQG_REG_MAXRETRY: restarts of one backward pass, at most
constexpr int REG_TRACE = 8;      // doubles per (iteration, seed) of the trace
struct RegDev {
  double* mu = nullptr;
  double* dmu = nullptr;
  double* cost_nom = nullptr;  // the nominal trajectory's cost, meaningful while valid[s]
  int* valid = nullptr;
  int* status = nullptr;       // 0 running, 1 converged, 2 mu reached mu_max
  int* retries = nullptr;      // restarts of the last backward pass
  double* trace = nullptr;     // this iteration's [S][REG_TRACE] slot of the ring, or null
  double factor = 0, mu_min = 0, mu_max = 0, zmin = 0, tol_cost = 0;
  int max_retry = 0;
};
// dmu = max(dmu f, f); mu = max(mu dmu, mu_min); status 2 once mu >= mu_max
__host__ __device__ inline void reg_increase(const RegDev& r, double& mu, double& dmu, int& status) {
  const double d = dmu * r.factor;
  dmu = d > r.factor ? d : r.factor;
  const double t = mu * dmu;
  mu = t > r.mu_min ? t : r.mu_min;
  if (mu >= r.mu_max) status = 2;
}
// dmu = min(dmu / f, 1 / f); mu = mu dmu, or 0 when that is not above mu_min
__host__ __device__ inline void reg_decrease(const RegDev& r, double& mu, double& dmu) {
  const double d = dmu / r.factor, i = 1.0 / r.factor;
  dmu = d < i ? d : i;
  const double t = mu * dmu;
  mu = t > r.mu_min ? t : 0.0;
}
// launch_backward_std with a restart: mu from rg.mu[s]; an indefinite step
// raises it and restarts the recursion, at most min(rg.max_retry, REG_MAXRETRY)
// times per pass and only while rg.status[s] == 0
hipError_t launch_backward_std_reg(const DevModel& m, int S, int P, const double* deriv, int Ds, TrajDev tr, double* K,
                                   double* k, double* V, double* v, RicFlags fl, StdDev sd, RegDev rg, hipStream_t st);
// launch_select's place in the regularisation mode: the step is accepted (the
// candidate copied to the nominal trajectory and dinit, mu lowered) or rejected
// (nothing copied, sel = -1, mu raised).  cand is always a buffer of its own.
hipError_t launch_accept(const DevModel& m, int S, int A, int P, int mode, const double* cost_cand,
                         const double* alphas, const double* dV, int* sel, double* cost_sel, TrajDev cand,
                         TrajDev nominal, TrajDev dinit, RegDev rg, hipStream_t st);
// the reference recursion with the matrix products on the fp64 matrix cores
// (riccati_mfma.h): one 8-wave workgroup per seed; agrees with the oracle to
// rounding (the product sums run in the matrix core's order)
hipError_t launch_backward_mfma(const DevModel& m, int S, int P, double mu, const double* deriv, int Ds, TrajDev tr,
                                double* K, double* k, double* V, double* v, RicFlags fl, hipStream_t st);
size_t backward_mfma_lds_bytes(int nv, int nu);
bool backward_mfma_supported(int nv, int nu);

// Horizon shift (ilqg_solver_shift_horizon; kernels_shift.hip).
// k_shift_horizon: per seed and per-point array, point p takes point p - n for
// p = N .. n, in place.  arr[i]: [S][P][w[i]] doubles -- the trajectory's five
// fields (TrajDev order), then K, k and the FD records at their padded stride.
// Behind the move: K and k zero below n; dinit[f][s] = new point N and
// carry[f][s] = new point n of field f, the state the tail's passive rollout
// starts from.
// k_shift_store: the tail, computed compactly -- tail[f]: [S][n + 1][w[f]] for
// the five fields (a trajectory of n + 1 points per seed, its point n = new
// point n), tail[5]: their FD records [S][n + 1][w[ARR_DERIV]] -- into points
// n-1 .. 0 of the resident trajectory and records.
struct ShiftArgs {
  static constexpr int NARR = 8, ARR_K = 5, ARR_k = 6, ARR_DERIV = 7, NTAIL = 6;
  double* arr[NARR];
  int w[NARR];
  double* dinit[5];
  double* carry[5];
  const double* tail[NTAIL];
  int S, P, n;  // 1 <= n <= P - 1
};
hipError_t launch_shift_horizon(const ShiftArgs& a, hipStream_t st);
hipError_t launch_shift_store(const ShiftArgs& a, hipStream_t st);

// Nominal refresh (ilqg_solver_refresh_nominal; kernels_shift.hip k_nominal_cost),
// one workgroup per seed.  compute = 1: the cost of the nominal trajectory nom,
// [S][P] points, under the rows in force -- seed s, point n:
// cost_at(cost, s, sstride, n, cstride), both strides 0 for the creation cost
// -- summed exactly as the rollout charges a candidate, into cost_sel[s].
// compute = 0: cost_sel[s] already holds that cost (a rollout wrote it) and
// dinit takes point N of nom.  Either way, when rg.cost_nom is set (the
// regularisation mode): cost_nom[s] = that cost, valid[s] = 1, and with
// resume a status of 1 becomes 0.
struct NomCostArgs {
  int nq, nv, nu, S, P;
  TrajDev nom;
  TrajDev dinit{};  // compute = 0 only
  CostDev cost{};
  int cstride = 0, sstride = 0;
  double* cost_sel = nullptr;
  int compute = 1;
  int resume = 0;
  RegDev rg{};
};
hipError_t launch_nominal_cost(const NomCostArgs& a, hipStream_t st);

// fused FD sweep + streamed backward pass (kernels_fd.hip)
struct FdFused {
  TrajDev tr;
  int S, P;
  int nB;        // backward roles (S, or 0 for the sweep alone)
  int nv;        // qvel and qpos teams per point (one column each)
  int nut;       // ctrl teams per point, min(nu, nv) (mjderivative.cpp:78-82)
  int Dp, WCp;   // padded record strides (doubles, multiples of 16 = 128 B)
  const double* qfrc_applied;
  const double* xfrc_applied;
  CostDev cost;
  double* cw;      // [S*P][WCp]: centre warm start (nv) + centre cost
  double* deriv;   // [S*P][Dp]
  unsigned* sync;  // [4 + 2 S P]: ticket, pad, cflag[S*P], done[S*P]; zeroed before each launch
  unsigned* fault; // set by a timed-out wait
  double mu;
  double *K, *k, *V, *v;
  RicFlags fl;
  // ticket schedule (launch_fd_plan): slot -> FD item, null = identity; each
  // FD item's duration in this launch (s_memrealtime ticks), null = not kept
  const unsigned* order;
  unsigned* dur;
  // issue priority of the FD teams by ticket slot: slots >= prio1 run at
  // s_setprio 1, >= prio2 at 2 (the backward roles run at 3); ~0u = never
  unsigned prio1 = ~0u, prio2 = ~0u;
  // the centre team's workspace after its position and velocity stages, per
  // point ([S*P][snapd] doubles: the team's LDS ints, then the doubles the
  // column teams read, kernels_fd.hip snap_ranges), which the qvel and ctrl
  // teams load instead of recomputing those stages; null = every team
  // computes its own
  double* snap = nullptr;
  int snapd = 0;
  int poison = 0;  // tests (ILQG_SNAP_POISON): every double a snapshot does not carry reads as NaN
  // every column as two items, its + and - evaluations ([S*P][ntm][2][nv]
  // qacc exchange, [S*P][ntm] pair counters zeroed with sync); 0 = one item
  int halves = 0;
  double* xq = nullptr;
  unsigned* pairc = nullptr;
  // the FD teams' Newton loops end once their state repeats (dcoop_impl.h
  // ILQG_NT_REPLAY; the host reads the environment's ILQG_NT_REPLAY once);
  // 0 = every iteration runs.  The records are the same bits either way.
  int nt_replay = 1;
};
// Plan the fused sweep's ticket order from the previous launch's per-item
// durations (dur, all zero = no history: identity order).  Items of the first
// p0 points keep their slots; then, point-major, every (seed, point) with an
// item longer than kthr x the mean duration: its centre team and its long
// column teams; then the rest in identity order.  Every column team still
// follows its centre team, so the deadlock argument is unchanged.
hipError_t launch_fd_plan(int S, int P, int ntm, int p0, float kthr, const unsigned* dur, unsigned* order,
                          hipStream_t st);
// validates a ticket -> item map (nt items per (seed, point) besides its
// centre); replaces an invalid one by the identity and sets fault bit 1
hipError_t launch_fd_order_check(int S, int P, int nt, unsigned* order, unsigned* pos, unsigned* fault,
                                 hipStream_t st);

}  // namespace ilqg

// ---- cooperative (one wavefront per evaluation, LDS workspace) variants ----
namespace ilqg {
size_t coop_lds_bytes(const WsLayout& L, const coop::CoopLayout& C);
// an FD sweep over npts points, P per seed (kernels_fd.hip's two-kernel sweep,
// kernels_fd32.hip): centre warm starts and costs into warm_c / cost_c, the
// records into deriv at stride Ds
struct FdArgs {
  TrajDev tr;
  int npts, P;
  const double *qfrc_applied, *xfrc_applied;
  CostDev cost;
  int cstride;  // cost schedule (cost_at), 0 = none
  int sstride;  // its stride from seed to seed, 0 = shared
  double *warm_c, *cost_c;
  double* deriv;
  int Ds;
  hipStream_t st;
  int nt_replay = 1;  // as FdFused.nt_replay, a uniform argument of every kernel of the sweep
};
hipError_t launch_fd_centre_coop(const DevModel& m, const WsLayout& L, const coop::CoopLayout& C,
                                 const coop::CoopAux& X, const FdArgs& a);
hipError_t launch_fd_cols_coop(const DevModel& m, const WsLayout& L, const coop::CoopLayout& C,
                               const coop::CoopAux& X, const FdArgs& a);
// fp32 FD sweep (kernels_fd32.hip; BASELINE.json configs[4]): centre + column
// kernels on the fp32 physics, fp64 records; eps is the FD step (1e-3)
size_t coop_lds_bytes_f32(const WsLayout& L, const coop::CoopLayout& C);
hipError_t launch_fd_sweep_f32(const DevModel& m, const WsLayout& L, const coop::CoopLayout& C,
                               const coop::CoopAux& X, const FdArgs& a, double eps);
hipError_t launch_fd_fused_coop(const DevModel& m, const WsLayout& L, const coop::CoopLayout& C,
                                const coop::CoopAux& X, const FdFused& a, hipStream_t st, int cstride,
                                int sstride);
// a rollout of S seeds x A candidates over a P-point horizon (ch: the points)
struct RollArgs {
  int S, A, P;
  TrajDev nominal, out;
  int out_is_cand;
  const double *K, *k, *alphas;
  TrajDev dinit;
  const double *qfrc_applied, *xfrc_applied;
  int passive;
  CostDev cost;
  double* cost_cand;
  hipStream_t st;
  RollChunk ch;
  int cstride;  // cost schedule (cost_at), 0 = none
  int sstride = 0;  // its stride from seed to seed, 0 = shared
};
hipError_t launch_rollout_coop(const DevModel& m, const WsLayout& L, const coop::CoopLayout& C,
                               const coop::CoopAux& X, const RollArgs& a);
// whether the rollout kernel this process selects (ILQG_DUAL) has a clamped
// variant (RollChunk.ulim): launch_rollout_coop refuses limits otherwise
bool rollout_clamp_supported();
// the same for a cost schedule (cstride != 0): the scheduled variants re-stage
// the LDS cost copy per point
bool rollout_sched_supported();
// n independent states, one wavefront each: nstep mj_step (in place)
hipError_t launch_step_coop(const DevModel& m, const WsLayout& L, const coop::CoopLayout& C, const coop::CoopAux& X,
                            TrajDev stt, int n, int nstep, const double* qfrc_applied, const double* xfrc_applied,
                            hipStream_t st);
// n independent states, one wavefront each: mj_forward -> qacc, warm start updated
hipError_t launch_forward_coop(const DevModel& m, const WsLayout& L, const coop::CoopLayout& C,
                               const coop::CoopAux& X, TrajDev stt, int n, const double* qfrc_applied,
                               const double* xfrc_applied, double* qacc, hipStream_t st);
}  // namespace ilqg
