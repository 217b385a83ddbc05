// rows_main.cc -- TEST HARNESS ONLY: deposition_validate, build_dep_rows and vectors_validate of artis_amd/csrc/deposition.h with a main
// of their own, for a run under the address and undefined-behaviour sanitizers (make rows_sanitized). Reads the networks that
// `python tests/deposition_common.py DIR` writes (one text file each, the format of tests/decay_host/rows_main.cc), gives every
// nuclide energies from a fixed rule, validates, builds the rows, forms the power vectors from unit coefficients and prints a checksum
// over every row array; then checks that a few malformed copies are refused.
#define ARTIS_HOST_EMU 1
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../artis_amd/csrc/deposition.h"

namespace {
struct Net {
  int nn = 0, np = 0;
  std::vector<int32_t> anumber, z, a, start, idx, type, top, end;
  std::vector<double> life, branch, mass, gamma, particle, q, prob, vol, radial;
  artis_deposition_model m{};
};

bool read(const char *path, Net &n, int64_t ncell) {
  std::ifstream f(path);
  int ne = 0;
  if (!(f >> n.nn >> n.np >> ne)) return false;
  n.anumber.resize((size_t)ne);
  for (auto &v : n.anumber) f >> v;
  n.z.resize((size_t)n.nn), n.a.resize((size_t)n.nn), n.life.resize((size_t)n.nn);
  for (int i = 0; i < n.nn; i++) f >> n.z[(size_t)i] >> n.a[(size_t)i] >> n.life[(size_t)i];
  n.start.resize((size_t)n.np + 1);
  for (auto &v : n.start) f >> v;
  n.idx.resize((size_t)n.start.back());
  for (auto &v : n.idx) f >> v;
  n.branch.resize((size_t)n.np), n.type.resize((size_t)n.np);
  for (auto &v : n.branch) f >> v;
  for (auto &v : n.type) f >> v;
  if (!f) return false;
  for (int p = 0; p < n.np; p++) {
    n.top.push_back(n.idx[(size_t)n.start[(size_t)p]]);
    n.end.push_back(n.idx[(size_t)n.start[(size_t)p + 1] - 1]);
  }
  const size_t nn = (size_t)n.nn;
  n.gamma.assign(nn, 0.), n.particle.assign(6 * nn, 0.), n.q.assign(6 * nn, 0.), n.prob.assign(6 * nn, 0.);
  for (size_t i = 0; i < nn; i++) {
    n.mass.push_back(n.a[i] * artis::MH);
    if (!(n.life[i] > 0.)) continue;
    n.gamma[i] = 1e-6 * (double)(1 + i % 5);
    for (int p = 0; p < n.np; p++)
      if (n.start[(size_t)p + 1] - n.start[(size_t)p] == 2 && n.top[(size_t)p] == (int32_t)i) {
        const size_t t = (size_t)n.type[(size_t)p];
        n.prob[6 * i + t] = n.branch[(size_t)p];
        n.particle[6 * i + t] = 2e-6 * (double)(1 + t);
        n.q[6 * i + t] = 5e-6 * (double)(1 + t);
      }
  }
  n.vol.assign((size_t)ncell, 1e40), n.radial.assign((size_t)ncell, 1e14);
  n.m.struct_size = sizeof(artis_deposition_model);
  n.m.nnuclides = n.nn;
  n.m.npts_nonempty = (int32_t)ncell;
  n.m.nuc_endecay_gamma = n.gamma.data();
  n.m.nuc_endecay_particle = n.particle.data();
  n.m.nuc_endecay_q = n.q.data();
  n.m.nuc_branchprob = n.prob.data();
  n.m.assocvolume_tmin = n.vol.data();
  n.m.radial_pos_tmin = n.radial.data();
  return true;
}

uint64_t mix(uint64_t h, const std::vector<int32_t> &v) {
  for (int32_t x : v) h = (h ^ (uint64_t)(uint32_t)x) * 1099511628211ull;
  return h;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s NETWORK.txt ...\n", argv[0]);
    return 2;
  }
  const int64_t ncell = 7;
  for (int k = 1; k < argc; k++) {
    Net n;
    if (!read(argv[k], n, ncell)) {
      std::fprintf(stderr, "%s: cannot read\n", argv[k]);
      return 2;
    }
    std::string bad = artis_dep::deposition_validate(n.m, n.nn, ncell);
    if (!bad.empty()) {
      std::fprintf(stderr, "%s: refused: %s\n", argv[k], bad.c_str());
      return 1;
    }
    const artis_dep::Rows r = artis_dep::build_dep_rows(n.m, n.nn, n.np, n.top.data(), n.end.data(), n.life.data(), &bad);
    if (!bad.empty()) {
      std::fprintf(stderr, "%s: rows refused: %s\n", argv[k], bad.c_str());
      return 1;
    }
    const artis_dep::Tables T = artis_dep::host_tables(r, n.nn, n.np, n.life.data(), n.mass.data());
    // every entry of every vector from unit coefficients: walks every row to its end
    const std::vector<double> coeff((size_t)n.np + 1, 1.), surv((size_t)n.nn + 1, 1.);
    std::vector<double> vectors((size_t)artis_dep::NVECTORS * (size_t)n.nn);
    for (int v = 0; v < artis_dep::NVECTORS; v++)
      for (int i = 0; i < n.nn; i++) vectors[(size_t)v * (size_t)n.nn + (size_t)i] = artis_dep::power_entry(T, coeff.data(), surv.data(), v, i);
    if (!artis_dep::vectors_validate(vectors.data(), n.nn, n.life.data()).empty()) {
      std::fprintf(stderr, "%s: the vectors of unit coefficients are refused\n", argv[k]);
      return 1;
    }
    uint64_t h = 14695981039346656037ull;
    for (const auto *v : {&r.top_start, &r.top_path, &r.top_end, &r.rad_nuc}) h = mix(h, *v);
    std::printf("%s: %d nuclides, %d paths, %d radioactive, %zu row entries, checksum %016llx\n", argv[k], n.nn, n.np, T.nrad, r.top_path.size(),
                (unsigned long long)h);
    // malformed copies: each must be refused, none may read out of bounds
    int refused = 0;
    {
      Net m;
      read(argv[k], m, ncell);
      m.gamma[0] = -1.;
      refused += !artis_dep::deposition_validate(m.m, m.nn, ncell).empty();
    }
    {
      Net m;
      read(argv[k], m, ncell);
      m.prob[3] = 1.5;
      refused += !artis_dep::deposition_validate(m.m, m.nn, ncell).empty();
    }
    {
      Net m;
      read(argv[k], m, ncell);
      m.vol[2] = 0.;
      refused += !artis_dep::deposition_validate(m.m, m.nn, ncell).empty();
    }
    {
      Net m;
      read(argv[k], m, ncell);
      refused += !artis_dep::deposition_validate(m.m, m.nn + 1, ncell).empty();
    }
    {
      Net m;
      read(argv[k], m, ncell);
      m.top[0] = m.nn;  // a path whose top is out of range
      std::string why;
      (void)artis_dep::build_dep_rows(m.m, m.nn, m.np, m.top.data(), m.end.data(), m.life.data(), &why);
      refused += !why.empty();
    }
    {
      Net m;
      read(argv[k], m, ncell);
      m.life[(size_t)m.top[0]] = -1.;  // a path whose top is stable
      std::string why;
      (void)artis_dep::build_dep_rows(m.m, m.nn, m.np, m.top.data(), m.end.data(), m.life.data(), &why);
      refused += !why.empty();
    }
    std::printf("%s: %d of 6 malformed copies refused\n", argv[k], refused);
    if (refused != 6) return 1;
  }
  return 0;
}
