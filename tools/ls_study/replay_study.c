/* Newton replay study (STUDY TOOL): how many iterations of the oracle's Newton
 * solves repeat the one before them bit for bit?  Hooked into oracle/mjsub.c
 * solver_newton (-DORA_NT_STUDY), called once per iteration after its line
 * search and before its update.
 *
 * The hook sees jar, Jv and alpha, not qacc and Ma.  A call counts as a
 * period-1 replay when its jar, Jv and alpha have the previous call's bits and
 * jar_prev + alpha_prev * Jv_prev == jar: the previous call's update, applied
 * to the previous jar, gives this call's jar, which marks the same solve (and,
 * with jar == jar_prev, an update that changed no word of jar).  Period 2: the
 * same against the call two back, both links of the chain holding, and not a
 * period-1 replay.  A solve is the longest chain of linked calls; one of
 * CAP = 30 calls (the FD sweep's iteration cap, mjderivative.cpp:37) reached
 * the cap, "frozen" when its last call was a replay.
 * This is less than the full (qacc, Ma, jar) comparison the device makes: a
 * step may leave jar alone and still move qacc.  Run on one thread. */
#include <stdio.h>
#include <string.h>
#define MAXNE 256
#define CAP 30
typedef struct {
  int ne, ok;
  double jar[MAXNE], Jv[MAXNE], alpha;
} snap;
static snap p1, p2; /* the previous call, the one before it */
static int chain;    /* calls linked to this one so far (same solve) */
static int last_replay;
static long n_iter, n_p1, n_p2, n_cap, n_cap_frozen, n_big;

static int same_words(const double* a, const double* b, int n) { return memcmp(a, b, sizeof(double) * (size_t)n) == 0; }
/* next's jar is prev's jar after prev's update */
static int linked(const snap* prev, int ne, const double* jar) {
  if (!prev->ok || prev->ne != ne || prev->alpha == 0) return 0; /* alpha == 0 ended prev's solve */
  for (int i = 0; i < ne; i++) {
    double x = prev->jar[i] + prev->alpha * prev->Jv[i];
    if (memcmp(&x, jar + i, sizeof x)) return 0;
  }
  return 1;
}
static int equal(const snap* s, int ne, const double* jar, const double* Jv, double alpha) {
  return s->ok && s->ne == ne && same_words(s->jar, jar, ne) && same_words(s->Jv, Jv, ne) &&
         memcmp(&s->alpha, &alpha, sizeof alpha) == 0;
}
static void end_solve(void) {
  if (chain == CAP) {
    n_cap++;
    n_cap_frozen += last_replay;
  }
}

void ora_nt_study_iter(int ne, const double* jar, const double* Jv, double alpha, const int* state) {
  (void)state;
  n_iter++;
  if (ne > MAXNE) {
    n_big++;
    end_solve();
    chain = 0;
    p1.ok = p2.ok = 0;
    return;
  }
  const int l1 = linked(&p1, ne, jar);
  int replay = 0;
  if (l1 && equal(&p1, ne, jar, Jv, alpha)) {
    n_p1++;
    replay = 1;
  } else if (l1 && p2.ok && p2.ne == ne && linked(&p2, ne, p1.jar) && equal(&p2, ne, jar, Jv, alpha)) {
    n_p2++;
    replay = 1;
  }
  if (l1 && chain < CAP) {
    chain++;
  } else {
    end_solve();
    chain = 1;
  }
  last_replay = replay;
  p2 = p1;
  p1.ne = ne;
  p1.ok = 1;
  p1.alpha = alpha;
  memcpy(p1.jar, jar, sizeof(double) * (size_t)ne);
  memcpy(p1.Jv, Jv, sizeof(double) * (size_t)ne);
}
void ora_nt_study_report(char* out, int cap) {
  end_solve();
  chain = 0;
  snprintf(out, cap,
           "{\"newton_iterations\": %ld, \"period1_replays\": %ld, \"period2_replays\": %ld, "
           "\"capped_solves\": %ld, \"capped_solves_frozen\": %ld, \"iterations_over_%d_rows\": %ld}",
           n_iter, n_p1, n_p2, n_cap, n_cap_frozen, MAXNE, n_big);
}
void ora_nt_study_reset(void) {
  n_iter = n_p1 = n_p2 = n_cap = n_cap_frozen = n_big = 0;
  chain = 0;
  last_replay = 0;
  p1.ok = p2.ok = 0;
}
