// rows_main.cc -- TEST HARNESS ONLY. The x86 harness of the thermal balance (thermal_host.cc, included as it is) with a main of its own,
// built with -fsanitize=address,undefined (Makefile target rows_sanitized): it reads a model and one call's arrays from the file
// tests/thermal_common.py dump_call writes, gives every array an allocation of exactly its size, and runs the threaded solve, the rates
// with and without the ion balance and the residual scan of a few cells, as the Python tests do through the shared library.
//   file: int64 sizeof(artis_model), the struct's bytes; int64 npatch, then per array of the model {int64 offset of its pointer in the
//   struct, int64 nbytes, bytes}; int64 nptr, then per pointer of the call {int64 nbytes (-1: null), bytes}; double d[3]; int64 nprocs
#include <cstdio>
#include <cstdlib>
#include <string>

#include "thermal_host.cc"

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

    void *h = tb_host_model_new(&model);
    const HostModel &hm = *static_cast<const HostModel *>(h);
    const int64_t n = hm.M.npts_nonempty;
    tb_host_solve(h, ptrs.data(), d, iv, 4);
    const int32_t *flags = static_cast<const int32_t *>(ptrs[P_OUT_FLAGS]);
    const int32_t *evals = static_cast<const int32_t *>(ptrs[P_OUT_EVALS]);
    const int32_t *fit_flags = static_cast<const int32_t *>(ptrs[P_FIT_FLAGS]);
    int64_t bracketed = 0, total_evals = 0, fitted = 0, scanned = 0;
    for (int64_t c = 0; c < n; c++) {
      bracketed += (flags[c] & ARTIS_THERMAL_BRACKETED) != 0;
      total_evals += evals[c];
      fitted += (fit_flags[c] & ARTIS_RADFIELD_FITTED) != 0;
    }
    // the residual of the first fitted cells over the whole range (reads the solve's U and Gamma from the output arrays)
    const double T[4] = {artis_tb::MINTEMP, 2. * artis_tb::MINTEMP, 0.5 * artis_tb::MAXTEMP, artis_tb::MAXTEMP};
    double res[4];
    for (int64_t c = 0; c < n && scanned < 8; c++)
      if (fit_flags[c] & ARTIS_RADFIELD_FITTED) {
        tb_host_residuals(h, ptrs.data(), d, iv, c, 4, T, res);
        scanned++;
      }
    tb_host_rates(h, ptrs.data(), d, iv, 1, 3);  // at the resident T_e with the ion balance (P_RATES_TE is null in the dump)
    tb_host_rates(h, ptrs.data(), d, iv, 0, 3);
    double diff[3];
    tb_host_ratecoeff_diff(h, 6000.f, 1e8f, diff);
    std::printf("%s: %lld cells, %lld fitted, %lld bracketed, %lld evaluations, %lld cells scanned, %.0f rate coefficients compared\n", argv[a],
                (long long)n, (long long)fitted, (long long)bracketed, (long long)total_evals, (long long)scanned, diff[2]);
    tb_host_model_free(h);
    for (void *p : owned) std::free(p);
  }
  return 0;
}
