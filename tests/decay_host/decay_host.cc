// decay_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The bodies of artis_amd/csrc/decay_update.h -- the ones the engine's kernels call -- compiled for x86 with g++ and applied in plain
// loops (cells split over a few std::threads) to host arrays: what artis_amd_decay_update computes on the device. Also exports the
// validator, the row builder and the Bateman sum for tests/test_decay_update_rules.py.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../artis_amd/csrc/decay_update.h"

namespace {
struct HostDecay {
  artis_decay_model d;
  int nelements;
  int64_t ncell;
  artis_decay::Rows rows;
  artis_decay::Tables T;
  std::vector<float> X;  // [nuclide][cell], as the engine keeps it
};
std::string g_error;

template <class F>
void parallel_cells(int64_t ncell, int nthreads, F work) {
  const int nt = nthreads > 1 ? nthreads : 1;
  std::vector<std::thread> pool;
  const int64_t chunk = (ncell + nt - 1) / nt;
  for (int t = 0; t < nt; t++) {
    const int64_t c0 = t * chunk, c1 = c0 + chunk < ncell ? c0 + chunk : ncell;
    if (c0 < c1) pool.emplace_back(work, c0, c1);
  }
  for (auto &th : pool) th.join();
}
}  // namespace

extern "C" {

// calculate_decaychain without the expansion factor; out: {abundance, scale, x_dom}
void decay_host_decaychain(const double *lambdas, int n, double timediff, double *out) {
  const artis_decay::Chain ch = artis_decay::decaychain(lambdas, n, timediff);
  out[0] = ch.abund;
  out[1] = ch.scale;
  out[2] = ch.x_dom;
}

// decay_validate's text ("" for a usable model); ncell = 0: the per-cell arrays are not looked at
const char *decay_host_validate(const artis_decay_model *d, int64_t ncell, int nelements) {
  g_error = artis_decay::decay_validate(*d, ncell, nelements);
  return g_error.c_str();
}

// the rows of a validated model (the model's arrays must outlive the handle); NULL with decay_host_validate's text otherwise
void *decay_host_new(const artis_decay_model *d, const int32_t *elem_anumber, int nelements, int64_t ncell) {
  g_error = artis_decay::decay_validate(*d, ncell, nelements);
  if (!g_error.empty()) return nullptr;
  HostDecay *h = new HostDecay{*d, nelements, ncell, artis_decay::build_rows(*d, elem_anumber, nelements), {}, {}};
  h->T = artis_decay::host_tables(h->d, h->rows, nelements);
  h->X.resize((size_t)(ncell * d->nnuclides));
  for (int64_t c = 0; c < ncell; c++)
    for (int n = 0; n < d->nnuclides; n++) h->X[(size_t)(n * ncell + c)] = d->initnucmassfrac[c * d->nnuclides + n];
  return h;
}
void decay_host_free(void *h) { delete static_cast<HostDecay *>(h); }
const char *decay_host_last_error(void) { return g_error.c_str(); }

int decay_host_he4(const void *h) { return static_cast<const HostDecay *>(h)->rows.he4_nucindex; }
int64_t decay_host_nentries(const void *h) { return (int64_t)static_cast<const HostDecay *>(h)->rows.row_path.size(); }
// row_start [nnuclides + 1], row_path / row_kind [nentries] (kind 0: the path's end coefficient, 1: its He4 coefficient),
// nuc_element [nnuclides], elem_nuc_start [nelements + 1], elem_nuc [elem_nuc_start[nelements]]
void decay_host_rows(const void *hv, int32_t *row_start, int32_t *row_path, int32_t *row_kind, int32_t *nuc_element, int32_t *elem_nuc_start,
                     int32_t *elem_nuc) {
  const artis_decay::Rows &r = static_cast<const HostDecay *>(hv)->rows;
  const auto put = [](int32_t *to, const std::vector<int32_t> &v) {
    if (!v.empty()) std::memcpy(to, v.data(), sizeof(int32_t) * v.size());
  };
  put(row_start, r.row_start);
  put(row_path, r.row_path);
  put(row_kind, r.row_kind);
  put(nuc_element, r.nuc_element);
  put(elem_nuc_start, r.elem_nuc_start);
  put(elem_nuc, r.elem_nuc);
}

// calc_nuc_massfrac_coeffs at t_mid: endnuc_coeff, he4_coeff, scale, x_dom [npaths], survivingfrac [nnuclides]
void decay_host_coeffs(const void *hv, double t_mid, double *endnuc_coeff, double *he4_coeff, double *survivingfrac, double *scale, double *x_dom) {
  const HostDecay &h = *static_cast<const HostDecay *>(hv);
  const double t_afterinit = t_mid - h.d.t_model;
  for (int p = 0; p < h.T.npaths; p++) artis_decay::path_coeffs(h.T, p, t_afterinit, endnuc_coeff, he4_coeff, scale, x_dom);
  for (int n = 0; n < h.T.nnuclides; n++) survivingfrac[n] = artis_decay::nuc_survivingfrac(h.T, n, t_afterinit);
}

// The per-cell work of artis_amd_decay_update with given coefficients: rho [ncell], elem_massfracs, elem_meanweight [ncell][nelements],
// nuc_massfracs [ncell][nnuclides] (or NULL)
void decay_host_cells(const void *hv, double t_mid, double tmin, const double *endnuc_coeff, const double *he4_coeff, const double *survivingfrac,
                      float *rho, float *elem_massfracs, float *elem_meanweight, double *nuc_massfracs, int nthreads) {
  const HostDecay &h = *static_cast<const HostDecay *>(hv);
  const artis_decay::Tables &T = h.T;
  std::vector<double> coef((size_t)(2 * T.npaths) + 1);
  for (int p = 0; p < T.npaths; p++) {
    coef[(size_t)p] = endnuc_coeff[p];
    coef[(size_t)(T.npaths + p)] = he4_coeff[p];
  }
  const artis_decay::Coeffs K{coef.data(), survivingfrac};
  parallel_cells(h.ncell, nthreads, [&](int64_t c0, int64_t c1) {
    for (int64_t c = c0; c < c1; c++) {
      rho[c] = artis_decay::cell_rho(h.d.rho_tmin[c], t_mid, tmin);
      for (int el = 0; el < T.nelements; el++)
        artis_decay::element_entry(T, K, h.X.data(), h.ncell, c, el, h.d.elem_untrackedstable_initmassfrac, elem_massfracs, elem_meanweight);
      if (nuc_massfracs)
        for (int n = 0; n < T.nnuclides; n++) nuc_massfracs[c * T.nnuclides + n] = artis_decay::nuc_massfrac(T, K, h.X.data(), h.ncell, c, n);
    }
  });
}

}  // extern "C"
