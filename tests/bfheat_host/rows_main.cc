// rows_main.cc -- TEST HARNESS ONLY. The x86 harness of the bound-free heating coefficients (bfheat_host.cc, included as it is) with a
// main of its own, built with -fsanitize=address,undefined (Makefile target rows_sanitized): it reads a model and one call's arrays from
// the file tests/bfheat_common.py dump_call writes (the format of tests/thermal_host/rows_main.cc), gives every array an allocation of
// exactly its size, and runs the threaded update, the integrator on analytic integrands that subdivide down to the depth cap, and the
// integral over a table of its own, as the Python tests do through the shared library.
//   file: int64 sizeof(artis_model), the struct's bytes; int64 npatch, then per array of the model {int64 offset of its pointer in the
//   struct, int64 nbytes, bytes}; int64 nptr, then per pointer of the call {int64 nbytes (-1: null), bytes}; double d[3]; int64 nprocs
#include <cstdio>
#include <cstdlib>
#include <string>

#include "bfheat_host.cc"

namespace {
struct Reader {
  FILE *f;
  void bytes(void *to, size_t n) {
    if (n > 0 && std::fread(to, 1, n, f) != n) {
      std::fprintf(stderr, "short file\n");
      std::exit(2);
    }
  }
  int64_t i64() {
    int64_t v = 0;
    bytes(&v, sizeof v);
    return v;
  }
};
}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: rows_sanitized DUMP...\n");
    return 2;
  }
  for (int a = 1; a < argc; a++) {
    FILE *f = std::fopen(argv[a], "rb");
    if (!f) {
      std::fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    Reader r{f};
    if (r.i64() != (int64_t)sizeof(artis_model)) {
      std::fprintf(stderr, "the dump was written for another artis_model\n");
      return 2;
    }
    artis_model model;
    r.bytes(&model, sizeof model);
    std::vector<void *> owned;
    const int64_t npatch = r.i64();
    for (int64_t k = 0; k < npatch; k++) {
      const int64_t off = r.i64(), nbytes = r.i64();
      void *p = std::malloc((size_t)(nbytes > 0 ? nbytes : 1));
      r.bytes(p, (size_t)nbytes);
      std::memcpy(reinterpret_cast<char *>(&model) + off, &p, sizeof p);
      owned.push_back(p);
    }
    const int64_t nptr = r.i64();
    if (nptr != P_COUNT) {
      std::fprintf(stderr, "the dump holds %lld pointers, the harness takes %d\n", (long long)nptr, (int)P_COUNT);
      return 2;
    }
    std::vector<void *> ptrs((size_t)nptr, nullptr);
    for (int64_t k = 0; k < nptr; k++) {
      const int64_t nbytes = r.i64();
      if (nbytes < 0) continue;
      ptrs[(size_t)k] = std::malloc((size_t)(nbytes > 0 ? nbytes : 1));
      r.bytes(ptrs[(size_t)k], (size_t)nbytes);
      owned.push_back(ptrs[(size_t)k]);
    }
    double d[3];
    r.bytes(d, sizeof d);
    const int32_t iv[1] = {(int32_t)r.i64()};
    std::fclose(f);

    void *h = bfh_host_model_new(&model);
    const HostModel &hm = *static_cast<const HostModel *>(h);
    const int64_t n = hm.M.npts_nonempty;
    bfh_host_update(h, ptrs.data(), d, iv, 4);
    const int64_t *totals = static_cast<const int64_t *>(ptrs[P_OUT_TOTALS]);
    const int32_t *flags = static_cast<const int32_t *>(ptrs[P_OUT_FLAGS]);
    int64_t flagged = 0;
    for (int64_t c = 0; c < n; c++) flagged += flags[c] != 0;
    // the walk, down to the cap: a step at an irrational point with a tolerance it cannot meet, a kink, and the two trivial forms
    const artis_gk61_case cases[4] = {{4, 0, 0.70710678118654752, 0., 1., 1e-12}, {3, 0, 0.3, 0., 1., 1e-10}, {0, 0, 2., 1., 1., 1e-3}, {1, 0, 1., 2., -1., 1e-9}};
    artis_gk61_result res[4];
    bfh_host_gk61(4, cases, res);
    std::vector<float> xs(12, 1e-18f);
    double integral[4];
    bfh_host_integral(12, 0.1, xs.data(), 3e15, 12000.f, 0.3f, integral);
    std::printf("%s: %lld cells, %lld flagged, %lld nodes, %lld integrals subdivided, %lld at the cap; analytic walk %d nodes to depth %d; table integral %g\n",
                argv[a], (long long)n, (long long)flagged, (long long)totals[0], (long long)totals[1], (long long)totals[2], (int)res[0].nodes,
                (int)res[0].maxdepth, integral[0]);
    bfh_host_model_free(h);
    for (void *p : owned) std::free(p);
  }
  return 0;
}
