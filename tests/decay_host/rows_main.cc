// rows_main.cc -- TEST HARNESS ONLY: decay_validate and build_rows of artis_amd/csrc/decay_update.h with a main of their own, for a run
// under the address and undefined-behaviour sanitizers (make rows_sanitized). Reads the networks that `python tests/decay_common.py DIR`
// writes (one text file each), validates them, builds their rows and prints a checksum over every row array; then checks that a
// few malformed copies are refused.
#define ARTIS_HOST_EMU 1
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../artis_amd/csrc/decay_update.h"

namespace {
struct Net {
  std::vector<int32_t> anumber, z, a, start, idx, type;
  std::vector<double> life, branch;
  artis_decay_model d{};
};

bool read(const char *path, Net &n) {
  std::ifstream f(path);
  int nn = 0, np = 0, ne = 0;
  if (!(f >> nn >> np >> ne)) return false;
  n.anumber.resize((size_t)ne);
  for (auto &v : n.anumber) f >> v;
  n.z.resize((size_t)nn), n.a.resize((size_t)nn), n.life.resize((size_t)nn);
  for (int i = 0; i < nn; i++) f >> n.z[(size_t)i] >> n.a[(size_t)i] >> n.life[(size_t)i];
  n.start.resize((size_t)np + 1);
  for (auto &v : n.start) f >> v;
  n.idx.resize((size_t)n.start.back());
  for (auto &v : n.idx) f >> v;
  n.branch.resize((size_t)np), n.type.resize((size_t)np);
  for (auto &v : n.branch) f >> v;
  for (auto &v : n.type) f >> v;
  n.d.struct_size = sizeof(artis_decay_model);
  n.d.nnuclides = nn;
  n.d.npaths = np;
  n.d.nuc_z = n.z.data();
  n.d.nuc_a = n.a.data();
  n.d.nuc_meanlife = n.life.data();
  n.d.path_start = n.start.data();
  n.d.path_nucindex = n.idx.data();
  n.d.path_branchproduct = n.branch.data();
  n.d.path_last_decaytype = n.type.data();
  n.d.t_model = 86400.;
  return (bool)f;
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
  for (int k = 1; k < argc; k++) {
    Net n;
    if (!read(argv[k], n)) {
      std::fprintf(stderr, "%s: cannot read\n", argv[k]);
      return 2;
    }
    const std::string bad = artis_decay::decay_validate(n.d);
    if (!bad.empty()) {
      std::fprintf(stderr, "%s: refused: %s\n", argv[k], bad.c_str());
      return 1;
    }
    const artis_decay::Rows r = artis_decay::build_rows(n.d, n.anumber.data(), (int)n.anumber.size());
    uint64_t h = 14695981039346656037ull;
    for (const auto *v : {&r.row_start, &r.row_coef, &r.row_top, &r.row_path, &r.row_kind, &r.elem_nuc_start, &r.elem_nuc, &r.nuc_element}) h = mix(h, *v);
    std::printf("%s: %d nuclides, %d paths, %zu row entries, He4 at %d, checksum %016llx\n", argv[k], n.d.nnuclides, n.d.npaths, r.row_coef.size(),
                r.he4_nucindex, (unsigned long long)h);
    // malformed copies: each must be refused, none may read out of bounds
    int refused = 0;
    {
      Net m = n;
      read(argv[k], m);
      m.idx[(size_t)m.start[1]] = m.d.nnuclides;
      refused += !artis_decay::decay_validate(m.d).empty();
    }
    {
      Net m;
      read(argv[k], m);
      m.life[(size_t)m.idx[0]] = 0.;
      refused += !artis_decay::decay_validate(m.d).empty();
    }
    {
      Net m;
      read(argv[k], m);
      m.start[1] = m.start[0] + 1;
      refused += !artis_decay::decay_validate(m.d).empty();
    }
    std::printf("%s: %d of 3 malformed copies refused\n", argv[k], refused);
    if (refused != 3) return 1;
  }
  return 0;
}
