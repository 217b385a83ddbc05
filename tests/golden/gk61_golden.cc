// gk61_golden.cc -- golden-data harness (tests/golden/make_gk61_golden.py builds and runs it; never part of the package).
//
// The REFERENCE's gauss_kronrod_integrate<61> (its gausskronrod.h, included where it lies: -I <reference tree>) on the project's own
// integrands (artis_amd/csrc/bf_heating.h), so that only the integrator differs between the golden data and the project's
// artis_bfh::gk61_integrate. Reads one case per line from stdin (numbers as hex floats):
//   fn <which> <p> <a> <b> <tol>                                   the analytic integrands artis_bfh::Gk61TestFn
//   bfh <npoints> <increment> <nu_edge> <T_R> <W> <xs[npoints]>    artis_bfh::BfhIntegrand over its table, depth 15, 1e-3
// and prints "<result> <error> <evaluations>" per fn case, and for a bfh case that triple twice on one line: with the stage's own
// exp / expm1 (tb_exp, tb_expm1), then with the same formula on std::exp / std::expm1.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gausskronrod.h"

#include "../../artis_amd/csrc/bf_heating.h"

namespace {
struct LibMath {
  static double exp(const double x) { return std::exp(x); }
  static double expm1(const double x) { return std::expm1(x); }
};
template <class Math>
void bfh_case(const artis::DevModel &M, const float *xs, double nu_edge, float T_R, float W) {
  const artis_bfh::BfhIntegrand<Math> f = artis_bfh::bfh_integrand<Math>(M, xs, nu_edge, T_R, W);
  long evals = 0;
  double error = 0.;
  const double r = gauss_kronrod_integrate<61>(
      [&](const double nu) {
        evals++;
        return f(nu);
      },
      nu_edge, nu_edge * M.last_phixs_nuovernuedge, 15, artis_bfh::EPSREL, &error);
  std::printf("%a %a %ld", r, error, evals);
}
}  // namespace

int main() {
  char kind[8];
  while (std::scanf("%7s", kind) == 1) {
    if (std::strcmp(kind, "fn") == 0) {
      int which = 0;
      double p[4];
      if (std::scanf("%d %la %la %la %la", &which, &p[0], &p[1], &p[2], &p[3]) != 5) return 1;
      int64_t evals = 0;
      const artis_bfh::Gk61TestFn f{which, p[0], &evals};
      double error = 0.;
      const double r = gauss_kronrod_integrate<61>(f, p[1], p[2], 15, p[3], &error);
      std::printf("%a %a %ld\n", r, error, (long)evals);
    } else {
      int np = 0;
      double inc, nu_edge, T_R, W;
      if (std::scanf("%d %la %la %la %la", &np, &inc, &nu_edge, &T_R, &W) != 5) return 1;
      std::vector<float> xs((size_t)np);
      for (int i = 0; i < np; i++) {
        double v;
        if (std::scanf("%la", &v) != 1) return 1;
        xs[(size_t)i] = (float)v;
      }
      artis::DevModel M{};
      M.NPHIXSPOINTS = np;
      M.NPHIXSNUINCREMENT = inc;
      M.last_phixs_nuovernuedge = (1.0 + (inc * (np - 1)));
      bfh_case<artis_bfh::TbMath>(M, xs.data(), nu_edge, (float)T_R, (float)W);
      std::printf(" ");
      bfh_case<LibMath>(M, xs.data(), nu_edge, (float)T_R, (float)W);
      std::printf("\n");
    }
  }
  return 0;
}
