// ionbal_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The per-element bodies of artis_amd/csrc/ion_balance.h -- the ones the engine's kernels call -- compiled for x86 with g++ and
// applied in plain loops (cells split over a few std::threads) to host copies of the inputs: what artis_amd_grid_update computes on the device
// once its temperatures, gamma estimators and thickness are resolved. Also exports the pieces (the ion_alpha_sp table, the
// ground-continuum indices, the n_e residual of one cell) for tests/test_ion_balance_rules.py.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../artis_amd/csrc/model_build.h"
#include "../../artis_amd/csrc/ion_balance.h"

using artis::DevModel;

namespace {
struct HostModel {
  artis::ModelOwned own;
  DevModel M;
  explicit HostModel(const artis_model *m) { M = artis::make_host_model_view(*m, own); }
};

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

// the model view every call below works on (make_host_model_view, as the engine makes it before uploading)
void *ib_host_model_new(const artis_model *m) { return new HostModel(m); }
void ib_host_model_free(void *h) { delete static_cast<HostModel *>(h); }

double ib_host_minpop(void) { return ARTIS_OPT_MINPOP; }
int ib_host_force_saha(void) { return ARTIS_OPT_FORCE_SAHA_ION_BALANCE; }
int ib_host_excitation_use_tj(void) { return ARTIS_OPT_LTEPOP_EXCITATION_USE_TJ; }
int ib_host_tablesize(void) { return ARTIS_OPT_TABLESIZE; }
int ib_host_maxions(void) { return artis_ib::MAXIONS; }
// the engine's temperature grid [TABLESIZE + 1]
void ib_host_temperature_grid(const void *h, double *out) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  for (int i = 0; i <= ARTIS_OPT_TABLESIZE; i++) out[i] = hm.M.temperature_grid[i];
}

// the ion_alpha_sp table [nions][TABLESIZE] (float) and each ion's ground-continuum index [nions]
void ib_host_alpha_sp(const void *h, float *alpha_sp, int32_t *gci) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  const DevModel &M = hm.M;
  for (int ui = 0; ui < M.nions; ui++)
    for (int t = 0; t < ARTIS_OPT_TABLESIZE; t++) artis_ib::alpha_sp_entry(M, ui, t, alpha_sp, gci);
}

// get_ion_spontrecombcoeff of an ion at T_e on a given table
double ib_host_ion_spontrecombcoeff(const void *h, const float *alpha_sp, int ui, float T_e) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  return artis_ib::ion_spontrecombcoeff(hm.M, alpha_sp, ui, T_e);
}

// The per-cell work of artis_amd_grid_update on resolved inputs:
//   TJ, Te [ncell]: the cell's final temperatures; forced [ncell]: 1 where the cell is balanced with forced Saha (lte_iteration
//   or THICK); ground_cur [ncell*nions]: the current ground populations; massfrac, meanweight [ncell*nelements] (meanweight NULL:
//   the model's elem_meannucmass); rho, clump [ncell]; gamma [ncell*nbfg]: the normalised gamma estimator.
// Out: nnetot, U, phi, uppermost, ground, nne, nne_root, evals, flags (as artis_grid_update_result).
void ib_host_balance(const void *h, int64_t ncell, const float *TJ, const float *Te, const int32_t *forced, const float *ground_cur,
                     const float *massfrac, const float *meanweight, const float *rho, const float *clump, const double *gamma,
                     float *nnetot, float *U, double *phi, int32_t *uppermost, float *ground, float *nne, float *nne_root, int32_t *evals,
                     int32_t *flags, int nthreads) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  const DevModel &M = hm.M;
  std::vector<float> alpha_sp((size_t)M.nions * ARTIS_OPT_TABLESIZE + 1);
  std::vector<int32_t> gci((size_t)M.nions + 1);
  ib_host_alpha_sp(h, alpha_sp.data(), gci.data());
  std::vector<float> Te_cell((size_t)ncell + 1);  // (cell_setup's copy of Te: no override here)
  const artis_ib::CellArrays a{rho, massfrac, meanweight, M.elem_meannucmass, U, phi, gamma, gci.data(), M.nbfcontinua_ground,
                               uppermost, flags, evals, ground, nne, nne_root};
  parallel_cells(ncell, nthreads, [&](int64_t c0, int64_t c1) {
    for (int64_t c = c0; c < c1; c++) {
      artis_ib::cell_setup(M, c, a, Te, nullptr, nullptr, forced[c] != 0, Te_cell.data(), nnetot);
      for (int ui = 0; ui < M.nions; ui++) artis_ib::partfunct_entry(M, c, ui, TJ, Te_cell.data(), ground_cur, massfrac, U, &flags[c]);
      for (int ui = 0; ui < M.nions; ui++)
        artis_ib::phi_entry(M, c, ui, flags[c], U, Te_cell.data(), clump, alpha_sp.data(), gci.data(), gamma, a.nbfg, phi);
      artis_ib::solve_cell(M, c, a);
    }
  });
}

// the n_e residual (nne_solution_f) of one cell at nne, with that cell's U, phi, gamma, the ground-continuum indices and the
// cell's uppermost ions
double ib_host_residual(const void *h, float rho, const float *massfrac, const float *meanweight, const float *U, const double *phi,
                        const double *gamma, const int32_t *gci_in, const int32_t *uppermost, double nne, int32_t *flags) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  const DevModel &M = hm.M;
  std::vector<int32_t> up(uppermost, uppermost + M.nelements);
  const artis_ib::Cell cell{rho, massfrac, meanweight ? meanweight : M.elem_meannucmass, U, phi, gamma, gci_in, up.data()};
  return artis_ib::nne_residual(M, cell, nne, flags);
}

}  // extern "C"
