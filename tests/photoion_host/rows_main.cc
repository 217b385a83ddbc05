// rows_main.cc -- TEST HARNESS ONLY. The x86 harness of the photoionisation coefficients (photoion_host.cc, included as it is) with a
// main of its own, built with -fsanitize=address,undefined (Makefile target rows_sanitized): it reads a model and one call's arrays from
// the file tests/photoion_common.py dump_call writes (the format of tests/thermal_host/rows_main.cc), gives every array an allocation of
// exactly its size, and runs the threaded computation with both Math policies, as the Python tests do through the shared library.
//   file: int64 sizeof(artis_model), the struct's bytes; int64 npatch, then per array of the model {int64 offset of its pointer in the
//   struct, int64 nbytes, bytes}; int64 nptr, then per pointer of the call {int64 nbytes (-1: null), bytes}; double d[3]
//   {use_bf_estimators, nts, unused}; int64 nthreads
#include <cstdio>
#include <cstdlib>
#include <string>

#include "photoion_host.cc"

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
    const int nthreads = (int)r.i64();
    std::fclose(f);

    void *h = pi_host_model_new(&model);
    int64_t sizes[10];
    pi_host_sizes(h, sizes);
    int64_t sum[artis_pi::NTOTALS] = {};
    int64_t flagged = 0;
    double total = 0.;
    for (int math = 0; math < 2; math++) {
      pi_host_compute(h, ptrs.data(), d, math, nthreads);
      const int64_t *totals = static_cast<const int64_t *>(ptrs[P_OUT_TOTALS]);
      for (int k = 0; k < artis_pi::NTOTALS; k++) sum[k] += totals[k];
      const int32_t *flags = static_cast<const int32_t *>(ptrs[P_OUT_FLAGS]);
      for (int64_t c = 0; c < sizes[0]; c++) flagged += flags[c] != 0;
      const double *coeff = static_cast<const double *>(ptrs[P_OUT_COEFF]);
      for (int64_t k = 0; k < sizes[0] * sizes[1]; k++) total += coeff[k];
    }
    std::printf("%s: %lld cells x %lld entries; %lld from estimators, %lld integrals, %lld nodes, %lld at the cap, %lld not finite, %lld cells flagged; sum %g\n",
                argv[a], (long long)sizes[0], (long long)sizes[1], (long long)sum[0], (long long)sum[1], (long long)sum[2], (long long)sum[3],
                (long long)sum[4], (long long)flagged, total);
    pi_host_model_free(h);
    for (void *p : owned) std::free(p);
  }
  return 0;
}
