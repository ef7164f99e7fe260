// Legacy-boundary check program (tests/test_legacy.py): a caller that touches
// every public type, member and method SURVEY.md §8b lists for
// Differentiator<nv,nu> (/root/reference/inc/differentiator.h:14-93) and
// ILQR<nv,nu,N> (/root/reference/inc/ilqr.h:19-186), and an ILQR subclass that
// overrides the virtual initV (inc/ilqr.h:100,142).  Built against
// include/legacy and libilqg_mujoco.so by ilqg-mujoco_amd/Makefile.
//
//   legacy_members model.xml members   reference semantics of the members (GPU)
//   legacy_members model.xml initv N   N iterate() of the initV-override subclass;
//                                      prints K, k, V, v and the trajectory as hex
//   legacy_members model.xml mu X N    N iterate() of a plain ILQR whose public mu
//                                      was set to X first (inc/ilqr.h:65,166); same output
//   legacy_members model.xml mutate    one iterate() of a subclass whose initV changes
//                                      dArray[N/2] after the default; same output
// and three modes that are not tied to the pendulum's nv = 2, nu = 1 (any model;
// every number read or printed is a C hex float, so nothing is rounded on the way):
//   legacy_members - quat seed count   mju_quatIntegrate on `count` seeded cases; prints
//                                      "case quat[4] vel[3] scale" and "out quat[4]" rows (CPU)
//   legacy_members model.xml costcols cases.txt
//                                      host_cost_columns at every state of the file with the
//                                      file's cost descriptor as the host callback; "g" rows (CPU)
//   legacy_members model.xml fd cases.txt [--device-cost]
//                                      calcMJDerivatives at every state with the host callback,
//                                      or with the descriptor registered for it; "deriv" rows (GPU)
// cases.txt: rows "wq|tq|lq|wv|tv|lv|wu|tu|lu values..." (absent rows are zero) and rows
// "state time qpos[nq] qvel[nv] warm[nv] ctrl[nu]".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "differentiator.h"
#include "ilqg_amd.h"
#include "ilqg_legacy.h"
#include "ilqr.h"
#include "mjderivative.h"
#include "mujoco/mujoco.h"
#include "update.h"
#include "util.h"

namespace {

constexpr int kNv = 2, kNu = 1, kN = 20;

// inc/inverted_pendulum/cost.h:7-17
mjtNum stepCost(const mjData* d) {
  return 1.0 * d->qpos[0] * d->qpos[0] + 10.0 * d->qpos[1] * d->qpos[1] + 1.0 * d->qvel[0] * d->qvel[0] +
         10.0 * d->qvel[1] * d->qvel[1] + 1.0 * d->ctrl[0] * d->ctrl[0];
}

// the terminal value an override installs: V0(i, j) = 0.5 (i + 1) delta_ij + 0.125 (i + j), v0(i) = i - 1.5
template <int nv, int nu, int N>
class FixedTerminal : public ILQR<nv, nu, N> {
 public:
  using Base = ILQR<nv, nu, N>;
  FixedTerminal(mjModel* m, mjData* d, stepCostFn_t& fn) : Base(m, d, fn) {}
  int calls = 0;
  void initV() override {
    calls++;
    for (int j = 0; j < 2 * nv; j++) {
      (*this->v)(0, j) = j - 1.5;
      for (int i = 0; i < 2 * nv; i++) (*this->V)(i, j) = (i == j ? 0.5 * (i + 1) : 0.0) + 0.125 * (i + j);
    }
  }
};

// the default terminal value, then a later point changed (qvel[0] of
// dArray[N / 2] += 1e-3): the recursion must differentiate that point at its
// new state, as the reference's loop would (inc/ilqr.h:142-154)
template <int nv, int nu, int N>
class MutatingTerminal : public ILQR<nv, nu, N> {
 public:
  using Base = ILQR<nv, nu, N>;
  MutatingTerminal(mjModel* m, mjData* d, stepCostFn_t& fn) : Base(m, d, fn) {}
  void initV() override {
    Base::initV();
    this->dArray[N / 2]->qvel[0] += 1e-3;
  }
};

int fails = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "FAIL: %s\n", what);
    fails++;
  }
}

void hex(const char* tag, const mjtNum* a, int n) {
  printf("%s", tag);
  for (int i = 0; i < n; i++) printf(" %a", a[i]);
  printf("\n");
}

int members(mjModel* m, mjData* d0) {
  stepCostFn_t fn = stepCost;
  // ---- Differentiator<nv,nu>: typedefs, members, methods ----
  using D = Differentiator<kNv, kNu>;
  D::A_t a0;
  D::B_t b0;
  D::x_t x0;
  D::u_t u0;
  (void)a0; (void)b0; (void)x0; (void)u0;
  D* df = new D(m, d0, fn);
  expect(df->m == m && df->d == d0, "Differentiator m / d");
  expect(df->x->data() == d0->qpos && df->u->data() == d0->ctrl, "Differentiator x / u bound to d");
  expect(df->stepCostFn == fn, "Differentiator stepCostFn is the caller's");
  expect(df->dqaccdq->data() == df->deriv && df->dqaccdqvel->data() == df->deriv + kNv * kNv &&
             df->dqaccdctrl->data() == df->deriv + 2 * kNv * kNv &&
             df->dgdx->data() == df->deriv + 2 * kNv * kNv + kNv * kNu &&
             df->dgdu->data() == df->dgdx->data() + 2 * kNv,
         "Differentiator maps into deriv (differentiator.h:57-61)");
  df->updateDerivatives();
  const mjtNum dt = m->opt.timestep;
  for (int i = 0; i < kNv; i++)
    for (int j = 0; j < kNv; j++) {
      expect((*df->A)(kNv + i, j) == (*df->dqaccdq)(i, j) * dt, "A lower-left = dt * col-major dqaccdq (Q1)");
      expect((*df->A)(i, j) == (i == j ? 1 : 0) && (*df->A)(i, kNv + j) == (i == j ? dt : 0), "A top = [I, dt I]");
    }
  for (int i = 0; i < kNv; i++) expect((*df->B)(kNv + i, 0) == (*df->dqaccdctrl)(i, 0) * dt, "B lower");
  mjData* d1 = mj_makeData(m);
  cpMjData(m, d1, d0);
  mj_step(m, d1);
  df->setMJData(d1);
  expect(df->d == d1 && df->x->data() == d1->qpos && df->u->data() == d1->ctrl, "setMJData re-seats x / u");
  ilqg_legacy::Map<1, 2 * kNv> q(df->deriv + 2 * kNv * kNv + kNv * kNu);
  (void)q;
  delete df;

  // ---- ILQR<nv,nu,N>: typedefs, members, methods ----
  using L = ILQR<kNv, kNu, kN>;
  L::A_t la; L::B_t lb; L::x_t lx; L::u_t lu; L::Q_t lq; L::R_t lr;
  L::K_t lK; L::k_t lk; L::V_t lV; L::v_t lv;
  (void)la; (void)lb; (void)lx; (void)lu; (void)lq; (void)lr; (void)lK; (void)lk; (void)lV; (void)lv;
  L::dqdq_mt* mp = nullptr; L::dqdu_mt* mu_ = nullptr; L::qpos_mt* mq = nullptr; L::qvel_mt* mv = nullptr;
  L::ctrl_mt* mc = nullptr; L::x_mt* mx = nullptr; L::u_mt* mu2 = nullptr; L::q_mt* mq2 = nullptr;
  L::r_mt* mr = nullptr;
  (void)mp; (void)mu_; (void)mq; (void)mv; (void)mc; (void)mx; (void)mu2; (void)mq2; (void)mr;
  L* il = new L(m, d0, fn);
  expect(il->m == m && il->mu == 1000.0, "ILQR m / mu");
  expect(il->x->data() == il->d->qpos && il->u->data() == il->d->ctrl, "ILQR x / u bound to d (ilqr.h:90-91)");
  expect(il->xStar->data() == il->d->qpos && il->uStar->data() == il->d->ctrl, "ILQR xStar / uStar after ctor");
  // after the ctor d is one step past dArray[0] (ilqr.h:82-87)
  mjData* t = mj_makeData(m);
  cpMjData(m, t, il->dArray[0]);
  mj_step(m, t);
  expect(!memcmp(t->qpos, il->d->qpos, sizeof(mjtNum) * m->nq) && !memcmp(t->qvel, il->d->qvel, sizeof(mjtNum) * m->nv),
         "ctor leaves d one step past the terminal point");
  il->setDInit(d0);
  il->forwardPass();
  expect(il->xStar->data() == il->dArray[0]->qpos && il->uStar->data() == il->dArray[0]->ctrl,
         "forwardPass leaves xStar / uStar on dArray[0] (ilqr.h:124-125)");
  il->setDInit(il->dArray[kN]);
  il->backwardPass();
  expect(il->differentiator->d == il->dArray[kN], "backwardPass leaves the differentiator at dArray[N]");
  // the differentiator's A / B are dArray[N]'s linearisation: recompute it
  L::A_t Aend = *il->differentiator->A;
  L::B_t Bend = *il->differentiator->B;
  il->differentiator->updateDerivatives();
  expect(!memcmp(Aend.data(), il->differentiator->A->data(), sizeof(Aend)) &&
             !memcmp(Bend.data(), il->differentiator->B->data(), sizeof(Bend)),
         "differentiator A / B after backwardPass = updateDerivatives at dArray[N]");
  il->initV();  // the base initV is callable
  il->iterate();
  for (int n = 1; n <= kN; n++) expect(il->K[n](0, 0) == il->K[n](0, 0), "K finite");
  expect((*il->V)(0, 0) == (*il->V)(0, 0) && (*il->v)(0, 0) == (*il->v)(0, 0), "V / v finite");
  delete il;
  mj_deleteData(t);
  mj_deleteData(d1);
  if (!fails) printf("members ok\n");
  return fails ? 1 : 0;
}

template <class IL>
void dump(const mjModel* m, IL& il) {
  for (int n = 0; n <= kN; n++) hex("K", il.K[n].data(), kNu * 2 * kNv);
  for (int n = 0; n <= kN; n++) hex("k", il.k[n].data(), kNu);
  hex("V", il.V->data(), 4 * kNv * kNv);
  hex("v", il.v->data(), 2 * kNv);
  for (int n = 0; n <= kN; n++) {
    hex("qpos", il.dArray[n]->qpos, m->nq);
    hex("qvel", il.dArray[n]->qvel, m->nv);
    hex("ctrl", il.dArray[n]->ctrl, m->nu);
  }
}

int initv(mjModel* m, mjData* d0, int iters) {
  stepCostFn_t fn = stepCost;
  FixedTerminal<kNv, kNu, kN> il(m, d0, fn);
  il.setDInit(d0);
  for (int i = 0; i < iters; i++) il.iterate();
  if (il.calls != iters) {
    fprintf(stderr, "FAIL: backwardPass called initV %d times for %d iterations\n", il.calls, iters);
    return 1;
  }
  dump(m, il);
  return 0;
}

int mutate(mjModel* m, mjData* d0) {
  stepCostFn_t fn = stepCost;
  MutatingTerminal<kNv, kNu, kN> il(m, d0, fn);
  il.setDInit(d0);
  il.iterate();
  dump(m, il);
  return 0;
}

int mu(mjModel* m, mjData* d0, mjtNum value, int iters) {
  stepCostFn_t fn = stepCost;
  ILQR<kNv, kNu, kN> il(m, d0, fn);
  il.mu = value;  // the public member, read by every backwardPass
  il.setDInit(d0);
  for (int i = 0; i < iters; i++) il.iterate();
  dump(m, il);
  return 0;
}

// ---- modes for any model ----
// splitmix64: the seeded cases of the quat mode
uint64_t g_rng = 0;
uint64_t next64() {
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double uniform(double lo, double hi) { return lo + (hi - lo) * ((next64() >> 11) * (1.0 / 9007199254740992.0)); }

// a third exactly the identity, the rest seeded unit quaternions: as numpy-style
// rounding leaves them (|norm - 1| of a few 1e-16), scaled by 1 +- a few 1e-16
// (inside normalize4's window of 1e-15 or just around it), or denormalised by 1e-12;
// each with +-1e-6 e_k and with general velocities at scales 0.002 and 1
int quat_cases(uint64_t seed, int count) {
  g_rng = seed;
  for (int c = 0; c < count; c++) {
    mjtNum q[4] = {1, 0, 0, 0};
    const int kind = c % 6;  // 0, 1: identity
    if (kind >= 2) {
      mjtNum n = 0;
      for (int i = 0; i < 4; i++) { q[i] = uniform(-1, 1); n += q[i] * q[i]; }
      n = std::sqrt(n);
      for (int i = 0; i < 4; i++) q[i] /= n;
      const mjtNum f = kind == 3 ? 1 + uniform(1e-16, 1e-15) : kind == 4 ? 1 - uniform(1e-16, 1e-15)
                       : kind == 5 ? 1 + (c % 12 == 5 ? 1e-12 : -1e-12) : 1.0;
      for (int i = 0; i < 4; i++) q[i] *= f;
    }
    mjtNum vel[3] = {0, 0, 0}, scale = 1;
    const int vk = (c / 6) % 8;
    if (vk < 6) {
      vel[vk % 3] = vk < 3 ? 1e-6 : -1e-6;  // the FD sweep's own perturbation
    } else {
      for (int i = 0; i < 3; i++) vel[i] = uniform(-4, 4);
      scale = vk == 6 ? 0.002 : 1.0;
    }
    printf("case %a %a %a %a %a %a %a %a\n", q[0], q[1], q[2], q[3], vel[0], vel[1], vel[2], scale);
    mju_quatIntegrate(q, vel, scale);
    hex("out", q, 4);
  }
  return 0;
}

struct Cases {
  std::vector<mjtNum> a[9];  // wq tq lq wv tv lv wu tu lu
  std::vector<std::vector<mjtNum>> states;
};
Cases g_cases;
int g_nq = 0, g_nv = 0, g_nu = 0;

// the descriptor cost in the oracle's expression order (per entry: the quadratic
// term when its weight is not zero, then the linear term when its weight is not
// zero; qpos, qvel, ctrl; index ascending)
mjtNum desc_terms(mjtNum c, const mjtNum* x, const mjtNum* w, const mjtNum* t, const mjtNum* l, int n) {
  for (int i = 0; i < n; i++) {
    if (w[i] != 0) {
      mjtNum dx = x[i] - t[i];
      c += w[i] * dx * dx;
    }
    if (l[i] != 0) c += l[i] * x[i];
  }
  return c;
}
mjtNum descCost(const mjData* d) {
  const Cases& C = g_cases;
  mjtNum s = 0;
  s = desc_terms(s, d->qpos, C.a[0].data(), C.a[1].data(), C.a[2].data(), g_nq);
  s = desc_terms(s, d->qvel, C.a[3].data(), C.a[4].data(), C.a[5].data(), g_nv);
  s = desc_terms(s, d->ctrl, C.a[6].data(), C.a[7].data(), C.a[8].data(), g_nu);
  return s;
}

bool read_cases(const char* path, const mjModel* m) {
  static const char* tags[9] = {"wq", "tq", "lq", "wv", "tv", "lv", "wu", "tu", "lu"};
  const int len[9] = {m->nq, m->nq, m->nq, m->nv, m->nv, m->nv, m->nu, m->nu, m->nu};
  g_nq = m->nq; g_nv = m->nv; g_nu = m->nu;
  for (int i = 0; i < 9; i++) g_cases.a[i].assign(len[i], 0.0);
  FILE* f = fopen(path, "r");
  if (!f) return false;
  char tag[16];
  const size_t nstate = 1 + (size_t)m->nq + 2 * (size_t)m->nv + m->nu;
  while (fscanf(f, "%15s", tag) == 1) {
    std::vector<mjtNum>* dst = nullptr;
    size_t want = nstate;
    for (int i = 0; i < 9; i++)
      if (!strcmp(tag, tags[i])) { dst = &g_cases.a[i]; want = (size_t)len[i]; }
    if (!dst) {
      if (strcmp(tag, "state")) { fclose(f); return false; }
      g_cases.states.emplace_back();
      dst = &g_cases.states.back();
    }
    dst->assign(want, 0.0);
    for (size_t k = 0; k < want; k++) {
      char tok[64];
      if (fscanf(f, "%63s", tok) != 1) { fclose(f); return false; }
      (*dst)[k] = strtod(tok, nullptr);
    }
  }
  fclose(f);
  return !g_cases.states.empty();
}

void load_state(const mjModel* m, mjData* d, const std::vector<mjtNum>& s) {
  const mjtNum* p = s.data();
  d->time = *p++;
  mju_copy(d->qpos, p, m->nq); p += m->nq;
  mju_copy(d->qvel, p, m->nv); p += m->nv;
  mju_copy(d->qacc_warmstart, p, m->nv); p += m->nv;
  mju_copy(d->ctrl, p, m->nu);
}

int any_model(mjModel* m, const char* mode, const char* path, bool device_cost) {
  if (!read_cases(path, m)) {
    fprintf(stderr, "FAIL: could not read the cases of %s\n", path);
    return 1;
  }
  stepCostFn_t fn = descCost;
  if (device_cost) {
    ilqg_cost c{};
    const Cases& C = g_cases;
    c.wq = C.a[0].data(); c.tq = C.a[1].data(); c.lq = C.a[2].data();
    c.wv = C.a[3].data(); c.tv = C.a[4].data(); c.lv = C.a[5].data();
    c.wu = C.a[6].data(); c.tu = C.a[7].data(); c.lu = C.a[8].data();
    ilqg_legacy::register_cost(fn, &c, m->nq, m->nv, m->nu);
  }
  const int nv = m->nv, nu = m->nu, D = nv * (2 * nv + nu) + 2 * nv + nu;
  std::vector<mjtNum> deriv((size_t)D, 0.0);
  mjData* d = mj_makeData(m);
  for (const auto& s : g_cases.states) {
    load_state(m, d, s);
    if (!strcmp(mode, "costcols")) {
      ilqg_legacy::host_cost_columns(m, d, fn, deriv.data());
      hex("g", deriv.data() + nv * (2 * nv + nu), 2 * nv + nu);
    } else {
      calcMJDerivatives(m, d, deriv.data(), fn);
      hex("deriv", deriv.data(), D);
    }
  }
  mj_deleteData(d);
  return 0;
}
}  // namespace

int main(int argc, const char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: legacy_members model.xml members | initv [iters] | mu value [iters] | mutate |\n"
                    "       costcols cases.txt | fd cases.txt [--device-cost];  legacy_members - quat seed count\n");
    return 2;
  }
  if (!strcmp(argv[2], "quat"))
    return quat_cases(argc > 3 ? strtoull(argv[3], nullptr, 10) : 1, argc > 4 ? atoi(argv[4]) : 3000);
  mj_activate("mjkey.txt");
  char error[1000] = "";
  mjModel* m = mj_loadXML(argv[1], 0, error, 1000);
  if (!m) mju_error_s("Load model error: %s", error);
  if (!strcmp(argv[2], "costcols") || !strcmp(argv[2], "fd")) {
    if (argc < 4) mju_error("legacy_members: the cases file is missing");
    const int rc = any_model(m, argv[2], argv[3], argc > 4 && !strcmp(argv[4], "--device-cost"));
    mj_deleteModel(m);
    return rc;
  }
  if (m->nv != kNv || m->nu != kNu) mju_error("legacy_members drives the inverted pendulum (nv=2, nu=1)");
  mjData* d = mj_makeData(m);
  for (int i = 0; i < 10; i++) mj_step(m, d);  // inverted_pendulum.cpp:12-13
  int rc = !strcmp(argv[2], "members") ? members(m, d)
           : !strcmp(argv[2], "mu")    ? mu(m, d, argc > 3 ? atof(argv[3]) : 1000.0, argc > 4 ? atoi(argv[4]) : 1)
           : !strcmp(argv[2], "mutate") ? mutate(m, d)
                                       : initv(m, d, argc > 3 ? atoi(argv[3]) : 1);
  mj_deleteData(d);
  mj_deleteModel(m);
  return rc;
}
