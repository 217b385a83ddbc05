// rows_main.cc -- TEST HARNESS ONLY. The x86 harness of the rate-coefficient tables (ratecoeff_host.cc, included as it is) with a main of
// its own, built with -fsanitize=address,undefined (Makefile target rows_sanitized): it reads a model from the file
// tests/ratecoeff_common.py dump_call writes (the format of tests/thermal_host/rows_main.cc; the call has no arrays of its own), gives
// every array an allocation of exactly its size, and runs the threaded tables with both Math policies and in both forms, as the Python
// tests do through the shared library.
//   file: int64 sizeof(artis_model), the struct's bytes; int64 npatch, then per array of the model {int64 offset of its pointer in the
//   struct, int64 nbytes, bytes}; int64 nptr (0); double d[3] (unused); int64 nthreads
#include <cstdio>
#include <cstdlib>
#include <string>

#include "ratecoeff_host.cc"

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
    if (r.i64() != 0) {
      std::fprintf(stderr, "the dump holds pointers of a call; this harness takes none\n");
      return 2;
    }
    double d[3];
    r.bytes(d, sizeof d);
    const int nthreads = (int)r.i64();
    std::fclose(f);

    void *h = rc_host_model_new(&model);
    int64_t sizes[5];
    rc_host_sizes(h, sizes);
    const size_t n = (size_t)(sizes[0] * sizes[1]);
    std::vector<int32_t> conts((size_t)sizes[0] * 2 + 1);
    rc_host_conts(h, conts.data());
    int64_t nodes = 0, integrals = 0, flagged = 0;
    double sum = 0.;
    for (int math = 0; math < 2; math++)
      for (int shared = 0; shared < 2; shared++) {
        // allocations of exactly the tables' size: a write past a table is the sanitizer's to find
        double *spont = static_cast<double *>(std::malloc(n * sizeof(double) + (n == 0)));
        double *gamma = sizes[2] == 3 ? static_cast<double *>(std::malloc(n * sizeof(double) + (n == 0))) : nullptr;
        double *cool = static_cast<double *>(std::malloc(n * sizeof(double) + (n == 0)));
        int32_t *flags = static_cast<int32_t *>(std::malloc(n * sizeof(int32_t) + (n == 0)));
        int64_t totals[artis_rc::NTOTALS];
        rc_host_tables(h, math, shared, nthreads, spont, gamma, cool, flags, totals);
        integrals += totals[0];
        nodes += totals[1];
        flagged += totals[3];
        for (size_t i = 0; i < n; i++) sum += spont[i] + cool[i] + (gamma ? gamma[i] : 0.);
        std::free(spont);
        std::free(gamma);
        std::free(cool);
        std::free(flags);
      }
    std::printf("%s: %lld continua (%lld covered) x %lld temperatures, %lld tables; %lld integrals, %lld nodes, %lld flagged; sum %g\n", argv[a],
                (long long)sizes[0], (long long)sizes[3], (long long)sizes[1], (long long)sizes[2], (long long)integrals, (long long)nodes,
                (long long)flagged, sum);
    rc_host_model_free(h);
    for (void *p : owned) std::free(p);
  }
  return 0;
}
