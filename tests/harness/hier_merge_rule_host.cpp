// TEST INFRASTRUCTURE (tests/test_hier_merge_rule_on_host.py): the PRODUCT's csrc/hier_merge_rule.h -- copied next to
// this file at test time, never edited -- compiled for the host; its "common.h" is the stand-in of
// tests/harness/host_math.  host_merge_rows walks the children as hp_remerge_kernel does (csrc/hier_prune.hip).  The
// main below runs a few fixed cases through it and checks what needs no reference (unit quaternions, ascending
// eigenvalues, the covariance the row stands for against the moment-matched one), so that this file can also be built
// stand-alone, e.g. with -fsanitize=address,undefined, and run by hand.
#include "hier_merge_rule.h"

#include <cstdio>
#include <vector>

// n nodes; node j owns the next counts[j] child rows (xyz [*,3], shs [*,W], alpha [*], log_scales [*,3], rots [*,4]).
// Outputs per node: the float32 row as the kernel writes it, and the double covariance (xx xy xz yy yz zz) before the
// eigen tail.  weights: NULL (every child is a leaf: alpha s0 s1 s2 of its row) or the carried weight of every child row.
extern "C" void host_merge_rows(const float* xyz, const float* shs, const float* alpha, const float* log_scales,
                                const float* rots, const double* weights, const int64_t* counts, int64_t n, int64_t W, float* out_xyz,
                                float* out_shs, float* out_alpha, float* out_log_scales, float* out_rots, double* out_cov) {
  int64_t sc = 0;
  for (int64_t id = 0; id < n; ++id) {
    const int64_t cc = counts[id];
    std::vector<double> wts((size_t)cc);
    double sum = 0.0;
    for (int64_t c = 0; c < cc; ++c) {
      const int64_t r = sc + c;
      const double ls[3] = {log_scales[r * 3 + 0], log_scales[r * 3 + 1], log_scales[r * 3 + 2]};
      wts[(size_t)c] = weights ? weights[r] : hgs::merge_child_weight((double)alpha[r], ls);
      sum += wts[(size_t)c];
    }
    const double ws = hgs::merge_weight_sum(sum);
    double mu[3] = {0.0, 0.0, 0.0}, al = 0.0;
    for (int64_t c = 0; c < cc; ++c) {
      const int64_t r = sc + c;
      const double f = wts[(size_t)c] / ws;
      wts[(size_t)c] = f;
      const double x[3] = {xyz[r * 3 + 0], xyz[r * 3 + 1], xyz[r * 3 + 2]};
      hgs::merge_add_mean(f, x, mu);
      al += f * (double)alpha[r];
    }
    double cv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t c = 0; c < cc; ++c) {
      const int64_t r = sc + c;
      const double x[3] = {xyz[r * 3 + 0], xyz[r * 3 + 1], xyz[r * 3 + 2]};
      const double ls[3] = {log_scales[r * 3 + 0], log_scales[r * 3 + 1], log_scales[r * 3 + 2]};
      const double q[4] = {rots[r * 4 + 0], rots[r * 4 + 1], rots[r * 4 + 2], rots[r * 4 + 3]};
      double cc6[6];
      hgs::merge_child_cov(q, ls, cc6);
      hgs::merge_add_cov(wts[(size_t)c], x, cc6, mu, cv);
    }
    for (int a = 0; a < 3; ++a) out_xyz[id * 3 + a] = (float)mu[a];
    out_alpha[id] = hgs::merge_alpha(al);
    float ls[3], q[4];
    hgs::merge_cov_to_row(cv, ls, q);
    for (int a = 0; a < 3; ++a) out_log_scales[id * 3 + a] = ls[a];
    for (int a = 0; a < 4; ++a) out_rots[id * 4 + a] = q[a];
    for (int k = 0; k < 6; ++k) out_cov[id * 6 + k] = cv[k];
    for (int64_t j = 0; j < W; ++j) {
      double acc = 0.0;
      for (int64_t c = 0; c < cc; ++c) acc += wts[(size_t)c] * (double)shs[(sc + c) * W + j];
      out_shs[id * W + j] = (float)acc;
    }
    sc += cc;
  }
}

namespace {

// a small deterministic generator (no <random>: the same numbers with every library)
struct Lcg {
  uint64_t s;
  double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
  double sym() { return 2.0 * next() - 1.0; }
};

int check_node(const char* name, const float* ls, const float* q, const double* cv) {
  int bad = 0;
  const double qn = sqrt((double)q[0] * q[0] + (double)q[1] * q[1] + (double)q[2] * q[2] + (double)q[3] * q[3]);
  if (!(fabs(qn - 1.0) <= 1e-6)) { printf("%s: |q| = %.9g\n", name, qn); ++bad; }
  if (!(ls[0] <= ls[1] && ls[1] <= ls[2])) { printf("%s: log-scales do not ascend: %g %g %g\n", name, ls[0], ls[1], ls[2]); ++bad; }
  // the covariance the row stands for
  const double qd[4] = {q[0], q[1], q[2], q[3]}, lsd[3] = {ls[0], ls[1], ls[2]};
  double back[6];
  hgs::merge_child_cov(qd, lsd, back);
  double num = 0.0, den = 0.0;
  const int wgt[6] = {1, 2, 2, 1, 2, 1};
  for (int k = 0; k < 6; ++k) {
    const double floor_k = (k == 0 || k == 3 || k == 5) ? fmax(cv[k], 1e-12) : cv[k];   // (clamped eigenvalues)
    num += wgt[k] * (back[k] - floor_k) * (back[k] - floor_k);
    den += wgt[k] * cv[k] * cv[k];
  }
  if (!(sqrt(num) <= 1e-5 * fmax(sqrt(den), 1e-12) + 3e-12)) { printf("%s: covariance off by %.3g (norm %.3g)\n", name, sqrt(num), sqrt(den)); ++bad; }
  return bad;
}

}  // namespace

int main() {
  const int64_t ks[6] = {1, 2, 3, 7, 2, 3};
  const int64_t W = 48;
  int bad = 0;
  Lcg g{12345};
  for (int t = 0; t < 6; ++t) {
    const int64_t k = ks[t];
    std::vector<float> xyz((size_t)k * 3), shs((size_t)(k * W)), alpha((size_t)k), ls((size_t)k * 3), rots((size_t)k * 4);
    for (int64_t c = 0; c < k; ++c) {
      for (int a = 0; a < 3; ++a) { xyz[(size_t)(c * 3 + a)] = (float)(3.0 * g.sym()); ls[(size_t)(c * 3 + a)] = (float)(g.sym() - 1.5); }
      for (int a = 0; a < 4; ++a) rots[(size_t)(c * 4 + a)] = (float)g.sym();
      alpha[(size_t)c] = (float)g.next();
      for (int64_t j = 0; j < W; ++j) shs[(size_t)(c * W + j)] = (float)g.sym();
    }
    if (t == 4) {           // two children with equal covariance
      for (int a = 0; a < 3; ++a) ls[(size_t)(3 + a)] = ls[(size_t)a];
      for (int a = 0; a < 4; ++a) rots[(size_t)(4 + a)] = rots[(size_t)a];
    }
    if (t == 5) for (int64_t c = 0; c < k; ++c) alpha[(size_t)c] = 0.0f;   // all weights zero: the 1e-30 clamp
    if (t == 2) alpha[1] = 0.0f;                                             // a child of zero weight
    float oxyz[3], oalpha[1], ols[3], oq[4];
    std::vector<float> oshs((size_t)W);
    double ocov[6];
    host_merge_rows(xyz.data(), shs.data(), alpha.data(), ls.data(), rots.data(), nullptr, &k, 1, W, oxyz, oshs.data(), oalpha, ols, oq, ocov);
    char name[32];
    snprintf(name, sizeof(name), "case %d (k = %lld)", t, (long long)k);
    bad += check_node(name, ols, oq, ocov);
    if (!(oalpha[0] >= 0.0f && oalpha[0] <= 1.0f)) { printf("%s: alpha = %g\n", name, oalpha[0]); ++bad; }
    if (t == 5 && !(oxyz[0] == 0.0f && oxyz[1] == 0.0f && oxyz[2] == 0.0f && ols[0] == ols[2])) { printf("%s: zero weights\n", name); ++bad; }
  }
  printf("hier_merge_rule_host: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
