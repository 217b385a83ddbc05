// stage_thermal.h -- artis_amd_thermal_*: the thermal balance of the thin (fitted) cells and artis_amd_grid_update_thermal, which hands
// its result to the ion balance (stage_ionbal.h) (rules and bodies: thermal_balance.h).
// Kernels on the caller's stream, every output element with one writer: k_tb_clear (one lane per cell), k_tb_renorm (one lane per
// (cell, ground continuum)), k_tb_gamma (one lane per (cell, ion), after the renormalisation), k_tb_partfunct (one lane per (cell, ion):
// artis_ib::partfunct_entry), k_tb_solve and k_tb_rates (one WAVE per cell, 256-thread workgroups, a persistent grid sized from the CU
// count; the waves take cells from a list through one integer atomic).
//
// k_tb_solve: the wave keeps the cell's per-ion arrays (phi, Gamma, U, ground populations, uppermost ions) in its own slice of LDS and
// the Boltzmann factors e_l of the cell's levels in its own row of a scratch array in HBM (nlevels doubles per wave of the grid; a wave
// re-reads its own row in every evaluation, so the row is expected, not measured, to stay in cache). All 64 lanes run artis_tb::find_Te with the same values: the ion balance of an evaluation is done
// redundantly on every lane (the code and bits of k_ib_solve), a rate is summed with the lanes strided over the cell's list and the
// partial sums exchanged by lane-xor (artis_tb::combine64's order), then taken from lane 0, so that every lane holds identical bits and
// the search's branches stay uniform. No __syncthreads() anywhere; the cross-lane exchanges stand outside every branch that depends on
// a computed value's rounding; the searches are bounded by 100 (T_e) and 50 (n_e) evaluations.
#pragma once

namespace {

#if ARTIS_TB_SUPPORTED

struct TbArgs {
  artis::DevModel M;
  artis_tb::Arrays A;
  const float *fit_Te;      // k_tb_clear
  const float *ground_cur;  // k_tb_partfunct: the resident ground populations
  const int32_t *list;      // k_tb_solve: the fitted cells (null: every cell, k_tb_rates)
  int32_t nlist;
  int32_t *cursor;
  double *e_l_rows;         // [waves of the grid][nlevels]
  const float *rates_Te;    // k_tb_rates
  int32_t rebalance;
  int32_t slice_bytes;      // LDS per wave
};

// the wave's form of artis_tb::SeqLanes
struct WaveLanes {
  int lane;
  template <class F>
  __device__ double sum(const int n, F term) const {
    double s = 0.;
    for (int i = lane; i < n; i += artis_tb::NLANES) s += term(i);
    for (int m = artis_tb::NLANES / 2; m >= 1; m >>= 1) s = s + __shfl_xor(s, m, artis_tb::NLANES);
    return __shfl(s, 0, artis_tb::NLANES);
  }
  template <class F>
  __device__ void each(const int n, F entry) const {
    for (int i = lane; i < n; i += artis_tb::NLANES) entry(i);
    __threadfence_block();  // (the wave's own stores, before its other lanes read them)
  }
};

__global__ void __launch_bounds__(BLOCK) k_tb_clear(TbArgs a) {
  const int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (c < a.A.ncell) artis_tb::cell_clear(a.M, a.A, c, a.fit_Te);
}

__global__ void __launch_bounds__(BLOCK) k_tb_renorm(TbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.A.ncell * a.A.nbfg) return;
  const int64_t c = i / a.A.nbfg;
  const int32_t flag = artis_tb::renorm_cell_entry(a.M, a.A, c, (int)(i - c * a.A.nbfg));
  if (flag) atomicOr(&a.A.flags[c], flag);
}

__global__ void __launch_bounds__(BLOCK) k_tb_gamma(TbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.A.ncell * a.M.nions) return;
  const int64_t c = i / a.M.nions;
  artis_tb::gamma_cell_entry(a.M, a.A, c, (int)(i - c * a.M.nions));
}

__global__ void __launch_bounds__(BLOCK) k_tb_partfunct(TbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.A.ncell * a.M.nions) return;
  const int64_t c = i / a.M.nions;
  int32_t flags = 0;
  artis_ib::partfunct_entry(a.M, c, (int)(i - c * a.M.nions), a.A.fit_TJ, a.A.fit_TJ, a.ground_cur, a.A.massfrac, a.A.U, &flags);
  if (flags) atomicOr(&a.A.flags[c], flags);
}

// the wave's slice of LDS: phi and Gamma (doubles), then U and the ground populations (floats), then the uppermost ions
struct TbSlice {
  double *phi, *gamma;
  float *U, *ground;
  int32_t *uppermost;
};
inline int32_t tb_slice_bytes(const artis::DevModel &M) {
  const int64_t b = 8 * ((int64_t)M.nions + M.nbfcontinua_ground) + 4 * (2 * (int64_t)M.nions + M.nelements);
  return (int32_t)((b + 15) & ~(int64_t)15);
}
__device__ inline TbSlice tb_slice(const TbArgs &a, char *base) {
  TbSlice s;
  s.phi = (double *)base;
  s.gamma = s.phi + a.M.nions;
  s.U = (float *)(s.gamma + a.M.nbfcontinua_ground);
  s.ground = s.U + a.M.nions;
  s.uppermost = (int32_t *)(s.ground + a.M.nions);
  return s;
}

// the next entry of the list for the whole wave (-1: none left)
__device__ inline int64_t tb_next_cell(const TbArgs &a, const int lane) {
  int idx = 0;
  if (lane == 0) idx = atomicAdd(a.cursor, 1);
  idx = __shfl(idx, 0, artis_tb::NLANES);
  if (idx >= a.nlist) return -1;
  return a.list ? a.list[idx] : idx;
}

// SOLVE: artis_tb::find_Te; else the rates at a.rates_Te (a.rebalance: with the ion balance first)
template <bool SOLVE>
__device__ inline void tb_wave_cells(const TbArgs &a) {
  extern __shared__ double tb_lds[];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const TbSlice sl = tb_slice(a, (char *)tb_lds + (int64_t)wave * a.slice_bytes);
  double *e_l = a.e_l_rows + ((int64_t)blockIdx.x * (BLOCK / 64) + wave) * a.M.nlevels;
  const WaveLanes lanes{lane};
  const artis::DevModel &M = a.M;
  for (int64_t c = tb_next_cell(a, lane); c >= 0; c = tb_next_cell(a, lane)) {
    const bool rebalance = SOLVE || a.rebalance;
    // the cell's rows into the slice; e_l at the temperature the populations are excited at
    const float *U_src = (rebalance ? a.A.U : a.A.res_U) + c * M.nions;
    lanes.each(M.nions, [&](const int ui) {
      sl.U[ui] = U_src[ui];
      sl.ground[ui] = a.A.res_ground[c * M.nions + ui];
      sl.phi[ui] = 0.;
    });
    lanes.each(a.A.nbfg, [&](const int g) { sl.gamma[g] = a.A.gamma[c * a.A.nbfg + g]; });
    artis_tb::fill_boltzmann(M, rebalance ? a.A.fit_TJ[c] : a.A.res_TJ[c], e_l, lanes);
    const artis_tb::CellFixed f = artis_tb::cell_fixed(M, a.A, c, sl.U, sl.gamma, e_l);
    artis_tb::CellWork w{};
    w.phi = sl.phi;
    w.ground = sl.ground;
    w.uppermost = sl.uppermost;
    w.nne = a.A.res_nne[c];
    if (SOLVE) {
      const artis_tb::Found r = artis_tb::find_Te(M, f, w, lanes);
      if (lane == 0) artis_tb::cell_store(M, a.A, c, r, w);
    } else {
      const float T_e = a.rates_Te ? a.rates_Te[c] : a.A.res_Te[c];
      artis_tb::rates_cell(M, a.A, c, f, w, T_e, rebalance, lanes);
      if (lane == 0) artis_tb::rates_store(M, a.A, c, T_e, rebalance, w);
    }
    __threadfence_block();  // (lane 0 has read the slice before the next cell's rows overwrite it)
  }
}

__global__ void __launch_bounds__(BLOCK) k_tb_solve(TbArgs a) { tb_wave_cells<true>(a); }
__global__ void __launch_bounds__(BLOCK) k_tb_rates(TbArgs a) { tb_wave_cells<false>(a); }

#endif  // ARTIS_TB_SUPPORTED

// everything of artis_amd_thermal_*: one block, made at the first call
struct TbState {
  StageBlock block;
  int64_t ncell = 0, nions = 0, nelements = 0, nbfg = 0, nlevels = 0, nwaves = 0;
  float *d_rho = nullptr, *d_massfrac = nullptr, *d_meanweight = nullptr, *d_clump = nullptr;  // the matter the last solve used
  double *d_bfheat = nullptr, *d_dep = nullptr;  // [n][nlevels]; ntlepton | alpha | spfission [3][n]
  double *d_renorm = nullptr, *d_gamma = nullptr, *d_Te_solved = nullptr, *d_bracket = nullptr, *d_rates = nullptr, *d_phi = nullptr, *d_e_l = nullptr;
  float *d_U = nullptr, *d_Te = nullptr, *d_nne = nullptr, *d_ground = nullptr, *d_rates_Te = nullptr;
  float *d_Te_solve = nullptr;  // the last solve's T_e (artis_amd_thermal_rates writes d_Te too; the hand-over reads this one)
  int32_t *d_evals = nullptr, *d_flags = nullptr, *d_list = nullptr, *d_cursor = nullptr, *d_target_level = nullptr;
  bool valid = false, solved = false;  // something to download; the last solve stands (its Gamma, U and matter)
  uint64_t fit_serial = 0;             // the fit the last solve was made on
  uint64_t cellstate_serial = 0;       // ... and the resident cell state it read
  int64_t nfitted = 0, total_evals = 0, ncells_flagged[ARTIS_THERMAL_NFLAGS] = {};
  double kernel_ms[ARTIS_THERMAL_NTIMES] = {};
};

void tb_free(TbState *st) { delete st; }

#if ARTIS_TB_SUPPORTED

int tb_init(artis_amd_engine *e) {
  if (e->tb) return ARTIS_OK;
  const DevModel &h = e->Mh;
  TbState *st = new TbState();
  const int64_t n = st->ncell = h.npts_nonempty, ni = st->nions = h.nions, ne = st->nelements = h.nelements, nl = st->nlevels = h.nlevels;
  const int64_t g = st->nbfg = h.nbfcontinua_ground;
  st->nwaves = (int64_t)(e->ncu > 0 ? e->ncu : 256) * 2 * (BLOCK / 64);  // two workgroups per CU at the most
  const int rc = st->block.make(
      {piece(&st->d_rho, n), piece(&st->d_massfrac, n * ne), piece(&st->d_meanweight, n * ne), piece(&st->d_clump, n), piece(&st->d_bfheat, n * nl),
       piece(&st->d_dep, 3 * n), piece(&st->d_renorm, n * g), piece(&st->d_gamma, n * g), piece(&st->d_Te_solved, n), piece(&st->d_bracket, 2 * n),
       piece(&st->d_rates, n * ARTIS_THERMAL_NRATES), piece(&st->d_phi, n * ni), piece(&st->d_e_l, st->nwaves * nl), piece(&st->d_U, n * ni),
       piece(&st->d_Te, n), piece(&st->d_nne, n), piece(&st->d_ground, n * ni), piece(&st->d_rates_Te, n), piece(&st->d_Te_solve, n), piece(&st->d_evals, n), piece(&st->d_flags, n),
       piece(&st->d_list, n), piece(&st->d_cursor, 1), piece(&st->d_target_level, h.nphixstargets_total)},
      "thermal", "the result block");
  if (rc != ARTIS_OK) {
    delete st;
    return rc;
  }
  // the level of every photoionisation target
  std::vector<int32_t> nt((size_t)(nl > 0 ? nl : 1)), start((size_t)(nl > 0 ? nl : 1)), target((size_t)(h.nphixstargets_total > 0 ? h.nphixstargets_total : 1));
  hipError_t err = hipSuccess;
  if (nl > 0) {
    err = hipMemcpy(nt.data(), e->M.level_nphixstargets, sizeof(int32_t) * (size_t)nl, hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(start.data(), e->M.level_phixstargetstart, sizeof(int32_t) * (size_t)nl, hipMemcpyDeviceToHost);
  }
  if (err == hipSuccess) {
    for (int64_t ul = 0; ul < nl; ul++)
      for (int t = 0; t < nt[(size_t)ul]; t++)
        if (start[(size_t)ul] + t < h.nphixstargets_total) target[(size_t)(start[(size_t)ul] + t)] = (int32_t)ul;
    err = stage_copy(st->d_target_level, target.data(), h.nphixstargets_total, hipMemcpyHostToDevice);
  }
  if (err != hipSuccess) {
    delete st;
    return stage_error(ARTIS_ERR_HIP, std::string("thermal: the targets' levels: ") + hipGetErrorString(err));
  }
  e->tb = st;
  return ARTIS_OK;
}

// the ion balance's ion_alpha_sp table and ground-continuum indices (stage_ionbal.h: made once per engine)
int tb_alpha_sp(artis_amd_engine *e, hipStream_t s) {
  int rc = ib_init(e);
  if (rc != ARTIS_OK) return rc;
  IbState *ib = e->ib;
  if (ib->have_alpha_sp || ib->nions <= 0) return ARTIS_OK;
  IbArgs a{};
  a.M = e->M;
  a.alpha_sp = ib->d_alpha_sp;
  a.gci = ib->d_gci;
  hipLaunchKernelGGL(k_ib_alpha_sp, dim3(nblocks(ib->nions * ARTIS_OPT_TABLESIZE)), dim3(BLOCK), 0, s, a);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("thermal: k_ib_alpha_sp: ") + hipGetErrorString(err));
  ib->have_alpha_sp = true;
  return ARTIS_OK;
}

// the arrays both calls hand to the kernels; the matter and clump pointers are set by the caller
TbArgs tb_args(artis_amd_engine *e) {
  TbState *st = e->tb;
  TbArgs a{};
  a.M = e->M;
  artis_tb::Arrays &A = a.A;
  A.ncell = st->ncell;
  A.nbfg = (int32_t)st->nbfg;
  A.res_TJ = e->C.TJ;
  A.res_TR = e->C.TR;
  A.res_W = e->C.W;
  A.res_Te = e->C.Te;
  A.res_nne = e->C.nne;
  A.res_ground = e->C.ion_groundlevelpops;
  A.res_U = e->C.ion_partfuncts;
  A.res_renorm = e->C.corrphotoionrenorm;
  A.fit_TJ = e->rf->d_TJ;
  A.fit_flags = e->rf->d_flags;
  A.meanweight_model = e->M.elem_meannucmass;
  A.gamma_raw = e->E.gammaestimator;
  A.ff_raw = e->E.ffheatingestimator;
  A.col_raw = e->E.colheatingestimator;
  A.gamma_stride = 2;
  A.est_stride = 8;
  A.assocvol = e->rf->d_assocvol;
  A.prev_mid = e->rf->prev_mid;
  A.tmin = e->model_copy.tmin;
  A.deltat = e->rf->deltat;
  A.nprocs = e->rf->nprocs;
  A.bfheatingcoeffs = st->d_bfheat;
  A.ntlepton_dep = st->d_dep;
  A.dep_alpha = st->d_dep ? st->d_dep + st->ncell : nullptr;
  A.dep_spfission = st->d_dep ? st->d_dep + 2 * st->ncell : nullptr;
  A.alpha_sp = e->ib->d_alpha_sp;
  A.gci = e->ib->d_gci;
  A.target_level = st->d_target_level;
  A.renorm = st->d_renorm;
  A.gamma = st->d_gamma;
  A.U = st->d_U;
  A.Te = st->d_Te;
  A.nne = st->d_nne;
  A.Te_solved = st->d_Te_solved;
  A.bracket = st->d_bracket;
  A.evals = st->d_evals;
  A.flags = st->d_flags;
  A.rates = st->d_rates;
  A.ground = st->d_ground;
  A.phi = st->d_phi;
  a.fit_Te = e->rf->d_Te;
  a.ground_cur = e->C.ion_groundlevelpops;
  a.cursor = st->d_cursor;
  a.e_l_rows = st->d_e_l;
  a.slice_bytes = tb_slice_bytes(e->Mh);
  return a;
}

// what both calls check first, and the heating inputs into the block
// dev_bfheat: the coefficients are on the device already (artis_amd_thermal_solve_bfheated), p->bfheatingcoeffs must be NULL then
int tb_begin(artis_amd_engine *e, const artis_thermal_params *p, hipStream_t s, const char *call, const double *dev_bfheat = nullptr) {
  const std::string who = std::string(call) + ": ";
  if (!e->have_cells) return stage_error(ARTIS_ERR_ARG, who + "no cell state (artis_amd_set_cellstate)");
  if (!e->rf || !e->rf->valid || !e->fit_since_step)
    return stage_error(ARTIS_ERR_ARG, who + "needs an artis_amd_radfield_fit since the last propagation call");
  if (dev_bfheat && p->bfheatingcoeffs) return stage_error(ARTIS_ERR_ARG, who + "bfheatingcoeffs must be NULL (the coefficients are the bound-free heating stage's)");
  if (!dev_bfheat && !p->bfheatingcoeffs) return stage_error(ARTIS_ERR_ARG, who + "bfheatingcoeffs is required");
  const bool dep_host = p->ntlepton_dep || p->dep_alpha || p->dep_spfission;
  if (dep_host && !(p->ntlepton_dep && p->dep_alpha && p->dep_spfission))
    return stage_error(ARTIS_ERR_ARG, who + "ntlepton_dep, dep_alpha and dep_spfission come together or not at all");
  if (!dep_host && (!e->dep || !e->dep->valid)) return stage_error(ARTIS_ERR_ARG, who + "no deposition inputs and no deposition update (artis_amd_deposition_update)");
  if (!ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT && !e->M.elem_meannucmass)
    return stage_error(ARTIS_ERR_ARG, who + "the element number densities need artis_model.elem_meannucmass");
  HIP_TRY(hipSetDevice(e->device));
  int rc = tb_alpha_sp(e, s);
  if (rc != ARTIS_OK) return rc;
  if ((rc = tb_init(e)) != ARTIS_OK) return rc;
  TbState *st = e->tb;
  if (tb_slice_bytes(e->Mh) * (BLOCK / 64) > 64 * 1024) return stage_error(ARTIS_ERR_UNSUPPORTED, who + "the per-ion arrays of four cells do not fit 64 KiB of LDS");
  const int64_t n = st->ncell;
  if (!dev_bfheat) HIP_TRY(stage_copy(st->d_bfheat, p->bfheatingcoeffs, n * st->nlevels, hipMemcpyHostToDevice, &s));
  if (dep_host) {
    HIP_TRY(stage_copy(st->d_dep, p->ntlepton_dep, n, hipMemcpyHostToDevice, &s));
    HIP_TRY(stage_copy(st->d_dep ? st->d_dep + n : nullptr, p->dep_alpha, n, hipMemcpyHostToDevice, &s));
    HIP_TRY(stage_copy(st->d_dep ? st->d_dep + 2 * n : nullptr, p->dep_spfission, n, hipMemcpyHostToDevice, &s));
  } else {  // the deposition block: eps_ana [5][n] | dep [5][n] (alpha, spfission: channels 3, 4) | ntlepton [n]
    const double *cell = e->dep->d_cell;
    const int64_t nch = artis_dep::NCHANNELS;
    HIP_TRY(stage_copy(st->d_dep, cell ? cell + 2 * nch * n : nullptr, n, hipMemcpyDeviceToDevice, &s));
    HIP_TRY(stage_copy(st->d_dep ? st->d_dep + n : nullptr, cell ? cell + (nch + 3) * n : nullptr, n, hipMemcpyDeviceToDevice, &s));
    HIP_TRY(stage_copy(st->d_dep ? st->d_dep + 2 * n : nullptr, cell ? cell + (nch + 4) * n : nullptr, n, hipMemcpyDeviceToDevice, &s));
  }
  return ARTIS_OK;
}

// one launch of a wave-per-cell kernel over nlist entries
template <class K>
hipError_t tb_launch_waves(artis_amd_engine *e, K kernel, TbArgs &a, hipStream_t s) {
  TbState *st = e->tb;
  const int64_t per_block = BLOCK / 64;
  int64_t blocks = (a.nlist + per_block - 1) / per_block;
  if (blocks > st->nwaves / per_block) blocks = st->nwaves / per_block;
  const hipError_t err = hipMemsetAsync(st->d_cursor, 0, sizeof(int32_t), s);
  if (err != hipSuccess) return err;  // (a stale cursor would let the waves find the list used up)
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(BLOCK), (size_t)a.slice_bytes * per_block, s, a);
  return hipGetLastError();
}

#endif  // ARTIS_TB_SUPPORTED

int tb_unsupported(const char *call) {
  const char *opt = artis_tb::unsupported_option();
  return stage_error(ARTIS_ERR_UNSUPPORTED, std::string(call) + ": this build has " + (opt ? opt : "an unsupported option") +
                                                ": the thermal balance of the thin cells is the host's");
}

#if ARTIS_TB_SUPPORTED
// artis_amd_thermal_solve; dev_bfheat: artis_amd_thermal_solve_bfheated (stage_bfheat.h), the coefficients read where they lie
int tb_solve(artis_amd_engine *e, const artis_thermal_params *p, void *hip_stream, const double *dev_bfheat) {
  STAGE_STRUCT_SIZE(p, artis_thermal_params, "thermal_solve");
  const bool host_matter = p->rho || p->elem_massfracs || p->elem_meanweight;
  if (host_matter && (!p->rho || !p->elem_massfracs)) return stage_error(ARTIS_ERR_ARG, "thermal_solve: rho and elem_massfracs come together");
  if (host_matter && ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT && !p->elem_meanweight)
    return stage_error(ARTIS_ERR_ARG, "thermal_solve: this build has USE_CALCULATED_MEANATOMICWEIGHT: elem_meanweight is required");
  if (!host_matter && (!e->decay || !e->decay->valid)) return stage_error(ARTIS_ERR_ARG, "thermal_solve: no matter and no decay update (artis_amd_decay_update)");
  hipStream_t s = (hipStream_t)hip_stream;
  int rc = tb_begin(e, p, s, "thermal_solve", dev_bfheat);
  if (rc != ARTIS_OK) return rc;
  TbState *st = e->tb;
  st->valid = st->solved = false;
  const int64_t n = st->ncell, ni = st->nions, ne = st->nelements;
  const hipMemcpyKind from = host_matter ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  HIP_TRY(stage_copy(st->d_rho, host_matter ? p->rho : e->decay->d_rho, n, from, &s));
  HIP_TRY(stage_copy(st->d_massfrac, host_matter ? p->elem_massfracs : e->decay->d_massfrac, n * ne, from, &s));
  if (ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT)
    HIP_TRY(stage_copy(st->d_meanweight, host_matter ? p->elem_meanweight : e->decay->d_meanweight, n * ne, from, &s));
  if (p->clumpfactor)
    HIP_TRY(stage_copy(st->d_clump, p->clumpfactor, n, hipMemcpyHostToDevice, &s));
  else
    HIP_TRY(stage_copy(st->d_clump, e->C.clumpfactor, n, hipMemcpyDeviceToDevice, &s));
  // the fitted cells, in cell order
  std::vector<int32_t> fit_flags((size_t)(n > 0 ? n : 1)), list;
  HIP_TRY(stage_copy(fit_flags.data(), e->rf->d_flags, n, hipMemcpyDeviceToHost, &s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int64_t c = 0; c < n; c++)
    if (fit_flags[(size_t)c] & ARTIS_RADFIELD_FITTED) list.push_back((int32_t)c);
  st->nfitted = (int64_t)list.size();
  HIP_TRY(stage_copy(st->d_list, list.data(), st->nfitted, hipMemcpyHostToDevice, &s));
  TbArgs a = tb_args(e);
  if (dev_bfheat) a.A.bfheatingcoeffs = dev_bfheat;
  a.A.rho = st->d_rho;
  a.A.massfrac = st->d_massfrac;
  a.A.meanweight_cell = ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT ? st->d_meanweight : nullptr;
  a.A.clump = st->d_clump;
  a.list = st->d_list;
  a.nlist = (int32_t)st->nfitted;
  // the kernels follow each other on the stream without a wait of the host's in between, so that the events' spans are the kernels';
  // a launch that fails is named here, a fault while they run by the wait that ends the call
  auto launched = [&](const char *kernel, hipError_t err) -> int {
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("thermal_solve: ") + kernel + ": " + hipGetErrorString(err));
    return ARTIS_OK;
  };
  if (n > 0) {
    hipLaunchKernelGGL(k_tb_clear, dim3(nblocks(n)), dim3(BLOCK), 0, s, a);
    if ((rc = launched("k_tb_clear", hipGetLastError())) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block.ev[0], s));
  if (n > 0 && st->nbfg > 0) {
    hipLaunchKernelGGL(k_tb_renorm, dim3(nblocks(n * st->nbfg)), dim3(BLOCK), 0, s, a);
    if ((rc = launched("k_tb_renorm", hipGetLastError())) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block.ev[1], s));
  if (n > 0 && ni > 0) {
    hipLaunchKernelGGL(k_tb_gamma, dim3(nblocks(n * ni)), dim3(BLOCK), 0, s, a);
    if ((rc = launched("k_tb_gamma", hipGetLastError())) != ARTIS_OK) return rc;
    hipLaunchKernelGGL(k_tb_partfunct, dim3(nblocks(n * ni)), dim3(BLOCK), 0, s, a);
    if ((rc = launched("k_tb_partfunct", hipGetLastError())) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block.ev[2], s));
  if (st->nfitted > 0 && (rc = launched("k_tb_solve", tb_launch_waves(e, k_tb_solve, a, s))) != ARTIS_OK) return rc;
  HIP_TRY(hipEventRecord(st->block.ev[3], s));
  {
    const hipError_t err = hipStreamSynchronize(s);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("thermal_solve: a kernel of the call: ") + hipGetErrorString(err));
  }
  std::vector<int32_t> flags((size_t)(n > 0 ? n : 1)), evals((size_t)(n > 0 ? n : 1));
  HIP_TRY(stage_copy(flags.data(), st->d_flags, n, hipMemcpyDeviceToHost, &s));
  HIP_TRY(stage_copy(evals.data(), st->d_evals, n, hipMemcpyDeviceToHost, &s));
  HIP_TRY(stage_copy(st->d_Te_solve, st->d_Te, n, hipMemcpyDeviceToDevice, &s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 3; k++) HIP_TRY(st->block.elapsed_ms(k, &st->kernel_ms[k]));
  st->kernel_ms[3] = 0.;
  std::fill(std::begin(st->ncells_flagged), std::end(st->ncells_flagged), 0);
  st->total_evals = 0;
  for (int64_t c = 0; c < n; c++) {
    for (int k = 0; k < ARTIS_THERMAL_NFLAGS; k++)
      if (flags[(size_t)c] & (1 << k)) st->ncells_flagged[k]++;
    st->total_evals += evals[(size_t)c];
  }
  st->fit_serial = e->rf->serial;
  st->cellstate_serial = e->cellstate_serial;
  st->valid = st->solved = true;
  return ARTIS_OK;
}
#endif

}  // namespace

extern "C" {

int artis_amd_thermal_solve(artis_amd_engine *e, const artis_thermal_params *p, void *hip_stream) {
  if (!e || !p) return stage_error(ARTIS_ERR_ARG, "thermal_solve: null engine or parameters");
#if !ARTIS_TB_SUPPORTED
  return tb_unsupported("thermal_solve");
#else
  return tb_solve(e, p, hip_stream, nullptr);
#endif
}

int artis_amd_thermal_rates(artis_amd_engine *e, const artis_thermal_params *p, const float *Te, int rebalance, void *hip_stream) {
  if (!e || !p) return stage_error(ARTIS_ERR_ARG, "thermal_rates: null engine or parameters");
#if !ARTIS_TB_SUPPORTED
  return tb_unsupported("thermal_rates");
#else
  STAGE_STRUCT_SIZE(p, artis_thermal_params, "thermal_rates");
  if (rebalance != 0 && rebalance != 1) return stage_error(ARTIS_ERR_ARG, "thermal_rates: rebalance must be 0 or 1");
  if (rebalance && (!e->tb || !e->tb->solved || !e->rf || e->tb->fit_serial != e->rf->serial || e->tb->cellstate_serial != e->cellstate_serial))
    return stage_error(ARTIS_ERR_ARG, "thermal_rates: rebalance = 1 needs an artis_amd_thermal_solve on the last fit and the resident cell state");
  hipStream_t s = (hipStream_t)hip_stream;
  int rc = tb_begin(e, p, s, "thermal_rates");
  if (rc != ARTIS_OK) return rc;
  TbState *st = e->tb;
  const int64_t n = st->ncell;
  if (Te) HIP_TRY(stage_copy(st->d_rates_Te, Te, n, hipMemcpyHostToDevice, &s));
  TbArgs a = tb_args(e);
  if (rebalance) {
    a.A.rho = st->d_rho;
    a.A.massfrac = st->d_massfrac;
    a.A.meanweight_cell = ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT ? st->d_meanweight : nullptr;
    a.A.clump = st->d_clump;
  } else {
    a.A.rho = e->C.rho;
    a.A.massfrac = e->C.elem_massfracs;
    a.A.meanweight_cell = ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT ? e->C.elem_meanweight : nullptr;
    a.A.clump = e->C.clumpfactor;
  }
  if (ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT && !a.A.meanweight_cell) return stage_error(ARTIS_ERR_ARG, "thermal_rates: the cell state has no elem_meanweight");
  a.list = nullptr;
  a.nlist = (int32_t)n;
  a.rates_Te = Te ? st->d_rates_Te : nullptr;
  a.rebalance = rebalance;
  HIP_TRY(hipEventRecord(st->block.ev[0], s));
  if (n > 0) {
    hipError_t err = tb_launch_waves(e, k_tb_rates, a, s);
    if (err == hipSuccess) err = hipEventRecord(st->block.ev[1], s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("thermal_rates: k_tb_rates: ") + hipGetErrorString(err));
  }
  if (n <= 0) HIP_TRY(hipEventRecord(st->block.ev[1], s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(st->block.elapsed_ms(0, &st->kernel_ms[3]));
  st->valid = true;
  return ARTIS_OK;
#endif
}

int artis_amd_thermal_download(artis_amd_engine *e, artis_thermal_result *out) {
  if (!e || !out) return stage_error(ARTIS_ERR_ARG, "thermal_download: null argument");
#if !ARTIS_TB_SUPPORTED
  return tb_unsupported("thermal_download");
#else
  STAGE_STRUCT_SIZE(out, artis_thermal_result, "thermal_download");
  if (!e->tb || !e->tb->valid) return stage_error(ARTIS_ERR_ARG, "thermal_download: nothing solved (artis_amd_thermal_solve)");
  TbState *st = e->tb;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t n = st->ncell, ni = st->nions, g = st->nbfg;
  const hipMemcpyKind down = hipMemcpyDeviceToHost;
  HIP_TRY(stage_copy(out->Te, st->d_Te, n, down));
  HIP_TRY(stage_copy(out->Te_solved, st->d_Te_solved, n, down));
  HIP_TRY(stage_copy(out->bracket, st->d_bracket, 2 * n, down));
  HIP_TRY(stage_copy(out->evals, st->d_evals, n, down));
  HIP_TRY(stage_copy(out->flags, st->d_flags, n, down));
  HIP_TRY(stage_copy(out->nne, st->d_nne, n, down));
  HIP_TRY(stage_copy(out->rates, st->d_rates, n * ARTIS_THERMAL_NRATES, down));
  HIP_TRY(stage_copy(out->ion_groundlevelpops, st->d_ground, n * ni, down));
  HIP_TRY(stage_copy(out->ion_partfuncts, st->d_U, n * ni, down));
  HIP_TRY(stage_copy(out->phi, st->d_phi, n * ni, down));
  HIP_TRY(stage_copy(out->gamma, st->d_gamma, n * g, down));
  HIP_TRY(stage_copy(out->corrphotoionrenorm, st->d_renorm, n * g, down));
  for (int k = 0; k < ARTIS_THERMAL_NFLAGS; k++) out->ncells_flagged[k] = st->ncells_flagged[k];
  out->total_evals = st->total_evals;
  out->nfitted = st->nfitted;
  out->npts_nonempty = (int32_t)n;
  out->nions = (int32_t)ni;
  out->nbfcontinua_ground = (int32_t)g;
  out->nlevels = (int32_t)st->nlevels;
  for (int k = 0; k < ARTIS_THERMAL_NTIMES; k++) out->kernel_ms[k] = st->kernel_ms[k];
  return ARTIS_OK;
#endif
}

int artis_amd_grid_update_thermal(artis_amd_engine *e, const artis_grid_update *u, const artis_timestep *ts_next, void *hip_stream) {
  if (!e || !u || !ts_next) return stage_error(ARTIS_ERR_ARG, "grid_update_thermal: null engine, update or timestep");
#if !ARTIS_TB_SUPPORTED
  return tb_unsupported("grid_update_thermal");
#else
  STAGE_STRUCT_SIZE(u, artis_grid_update, "grid_update_thermal");
  if (u->rho || u->elem_massfracs || u->elem_meanweight)
    return stage_error(ARTIS_ERR_ARG, "grid_update_thermal: rho, elem_massfracs and elem_meanweight must be NULL (the matter is the thermal solve's)");
  if (u->use_fit != 1) return stage_error(ARTIS_ERR_ARG, "grid_update_thermal: use_fit must be 1");
  if (u->Te) return stage_error(ARTIS_ERR_ARG, "grid_update_thermal: Te must be NULL (the fitted cells' T_e is the thermal solve's)");
  if (!e->tb || !e->tb->solved || !e->rf || !e->rf->valid || e->tb->fit_serial != e->rf->serial || e->tb->cellstate_serial != e->cellstate_serial)
    return stage_error(ARTIS_ERR_ARG, "grid_update_thermal: no artis_amd_thermal_solve on the last artis_amd_radfield_fit and the resident cell state");
  if (u->clumpfactor) return stage_error(ARTIS_ERR_ARG, "grid_update_thermal: clumpfactor must be NULL (the balance and the cell state take the thermal solve's)");
  if (!u->thick && (!e->dep || !e->dep->valid)) return stage_error(ARTIS_ERR_ARG, "grid_update_thermal: thick is required (or an artis_amd_deposition_update)");
  const TbState *st = e->tb;
  IbMatter matter{st->d_rho, st->d_massfrac, st->d_meanweight, u->thick ? nullptr : e->dep->d_thick};
  matter.thermal_Te = st->d_Te_solve;
  matter.thermal_gamma = st->d_gamma;
  matter.thermal_renorm = st->d_renorm;
  matter.thermal_clump = st->d_clump;
  const int rc = ib_grid_update(e, u, ts_next, hip_stream, &matter);
  if (rc == ARTIS_OK) e->tb->solved = false;  // the resident state it was made on is gone
  return rc;
#endif
}

}  // extern "C"
