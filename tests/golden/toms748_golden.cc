// toms748_golden.cc -- golden-data harness (tests/golden/make_toms748_golden.py builds and runs it; never part of the package).
//
// The REFERENCE's toms748_solve (its toms748.h, included where it lies: -I <reference tree>) on the residuals of the project's
// own x86 calculate_planck_mean_frequency (artis_amd/csrc/radfield_fit.h), so that only the solver differs between the golden
// data and the project's artis_rf::toms748. Reads one case per line from stdin:
//   bin <nu_lower> <nu_upper> <nu_bar> <ax> <bx> <tol> <maxit>
//   fn <which> <ax> <bx> <tol> <maxit>
// (numbers as hex floats) and prints "<lo> <hi> <evaluations>" per case, lo and hi as hex floats.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

#include "toms748.h"

#include "../../artis_amd/csrc/radfield_fit.h"

namespace {
double analytic(int which, double x) {  // the list of tests/radfield_host/radfield_host.cc
  switch (which) {
    case 0: return cos(x) - x;
    case 1: return x * x * x - 2 * x - 5;
    case 2: return exp(x) - 2;
    case 3: return x * x * x * x * x - 1e-3;
    case 4: return tanh(10 * (x - 0.3));
    default: return (x - 1) * (x - 1) * (x - 1);
  }
}
}  // namespace

int main() {
  char kind[8];
  while (std::scanf("%7s", kind) == 1) {
    double p[6];
    int which = 0;
    long maxit = 0;
    std::pair<double, double> r;
    std::uintmax_t it = 0;
    if (std::strcmp(kind, "bin") == 0) {
      if (std::scanf("%la %la %la %la %la %la %ld", &p[0], &p[1], &p[2], &p[3], &p[4], &p[5], &maxit) != 7) return 1;
      const artis_rf::BinResidual f{p[0], p[1], p[2]};
      const double tol = p[5];
      it = (std::uintmax_t)maxit;
      r = toms748_solve(f, p[3], p[4], f(p[3]), f(p[4]),
                        [tol](double a, double b) { return std::abs(a - b) <= (tol * std::min(std::abs(a), std::abs(b))); }, it);
    } else {
      if (std::scanf("%d %la %la %la %ld", &which, &p[0], &p[1], &p[2], &maxit) != 5) return 1;
      auto f = [which](double x) { return analytic(which, x); };
      const double tol = p[2];
      it = (std::uintmax_t)maxit;
      r = toms748_solve(f, p[0], p[1], f(p[0]), f(p[1]),
                        [tol](double a, double b) { return std::abs(a - b) <= (tol * std::min(std::abs(a), std::abs(b))); }, it);
    }
    std::printf("%a %a %ju\n", r.first, r.second, it);
  }
  return 0;
}
