// stage_decay.h -- artis_amd_decay_*: the decay and abundance update of the grid update (rules and bodies: decay_update.h), and
// artis_amd_grid_update_decayed, which hands its result to the ion balance (stage_ionbal.h) without the host.
// Kernels on the caller's stream, every output element with one writer: k_decay_coeffs (one lane per decay path: both coefficients;
// one lane per nuclide: the surviving fraction; skipped when the host hands its coefficients in), k_decay_cells (one lane per (cell,
// element): the element's nuclides and their rows walked in order, mass fraction and mean weight; the lanes of element 0 also write
// rho), k_decay_nuclides (one lane per (cell, nuclide), only when the caller asks for the nuclides). The initial nuclide mass
// fractions are kept transposed, [nuclide][cell]: the 64 lanes of a wave are 64 neighbouring cells and read one 256-byte line per row
// entry; the entry's coefficient, top nuclide and row bounds are wave-uniform (indexed from blockIdx and kernel arguments only).
#pragma once

namespace {

struct DecayArgs {
  artis_decay::Tables T;
  int64_t ncell;
  double t_afterinit, t_mid, tmin;
  const float *X;          // [nuclide][cell]
  const float *untracked;  // [cell][element]
  const float *rho_tmin;
  double *coef, *surv, *scale, *x_dom;  // coef: [2 * npaths] {endnuc_coeff, he4_coeff}
  float *rho, *massfrac, *meanweight;
  double *nucmf;  // [nuclide][cell]
};

__global__ void __launch_bounds__(BLOCK) k_decay_coeffs(DecayArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i < a.T.npaths)
    artis_decay::path_coeffs(a.T, (int)i, a.t_afterinit, a.coef, a.coef + a.T.npaths, a.scale, a.x_dom);
  else if (i < (int64_t)a.T.npaths + a.T.nnuclides)
    a.surv[i - a.T.npaths] = artis_decay::nuc_survivingfrac(a.T, (int)(i - a.T.npaths), a.t_afterinit);
}

// workgroup b: the cells [BLOCK * (b / nel), + BLOCK) of element b % nel (nel = max(nelements, 1)): consecutive workgroups are the
// elements of one block of cells, whose X lines stay in L2 from one element to the next
__global__ void __launch_bounds__(BLOCK) k_decay_cells(DecayArgs a) {
  const int nel = a.T.nelements > 0 ? a.T.nelements : 1;
  const int el = (int)(blockIdx.x % (unsigned)nel);
  const int64_t c = (int64_t)(blockIdx.x / (unsigned)nel) * BLOCK + threadIdx.x;
  if (c >= a.ncell) return;
  if (el < a.T.nelements) artis_decay::element_entry(a.T, {a.coef, a.surv}, a.X, a.ncell, c, el, a.untracked, a.massfrac, a.meanweight);
  if (el == 0) a.rho[c] = artis_decay::cell_rho(a.rho_tmin[c], a.t_mid, a.tmin);  // (stores last: the table loads above stay scalar)
}

__global__ void __launch_bounds__(BLOCK) k_decay_nuclides(DecayArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.ncell * a.T.nnuclides) return;
  const int nuc = (int)(i / a.ncell);
  a.nucmf[i] = artis_decay::nuc_massfrac(a.T, {a.coef, a.surv}, a.X, a.ncell, i - (int64_t)nuc * a.ncell, nuc);
}

// out[nuclide][cell] = in[cell][nuclide] (set-up, once)
__global__ void __launch_bounds__(BLOCK) k_decay_transpose(const float *in, float *out, int64_t ncell, int32_t nnuc) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= ncell * nnuc) return;
  const int64_t nuc = i / ncell, c = i - nuc * ncell;
  out[i] = in[c * nnuc + nuc];
}

// everything of artis_amd_decay_*: one block made by the set-up (the nuclides' mass fractions, which few callers want, in a second
// one at the first update that asks for them)
struct DecayState {
  StageBlock block, nuc_block;
  int64_t ncell = 0;
  artis_decay::Tables T{};  // device pointers
  double *d_nuc_lambda = nullptr, *d_nuc_mass = nullptr, *d_path_lambda = nullptr, *d_path_branch = nullptr;
  int32_t *d_path_start = nullptr, *d_path_nuc = nullptr, *d_path_type = nullptr, *d_row_start = nullptr, *d_row_coef = nullptr, *d_row_top = nullptr;
  int32_t *d_elem_nuc_start = nullptr, *d_elem_nuc = nullptr;
  float *d_initstable = nullptr, *d_X = nullptr, *d_untracked = nullptr, *d_rho_tmin = nullptr;
  double *d_coef = nullptr, *d_surv = nullptr, *d_scale = nullptr, *d_x_dom = nullptr, *d_nucmf = nullptr;
  float *d_rho = nullptr, *d_massfrac = nullptr, *d_meanweight = nullptr;
  double t_model = 0., t_mid = 0.;
  bool valid = false, have_nuclides = false;
  double kernel_ms[3] = {};
  uint64_t serial = 0;  // counts the updates (stage_deposition.h: which one a deposition update was made on)
  std::vector<int32_t> h_path_top, h_path_end;  // [npaths] every path's first and last nuclide, and the mean lives: what
  std::vector<double> h_meanlife;               // artis_amd_deposition_setup builds its rows from
};

void decay_free(DecayState *st) { delete st; }

}  // namespace

extern "C" {

int artis_amd_decay_setup(artis_amd_engine *e, const artis_decay_model *d) {
  if (!e || !d) return stage_error(ARTIS_ERR_ARG, "decay: null engine or model");
  STAGE_STRUCT_SIZE(d, artis_decay_model, "decay");
  const int64_t n = e->Mh.npts_nonempty;
  const int ne = e->Mh.nelements;
  const std::string bad = artis_decay::decay_validate(*d, n, ne);
  if (!bad.empty()) return stage_error(ARTIS_ERR_ARG, "decay: " + bad);
  HIP_TRY(hipSetDevice(e->device));
  std::vector<int32_t> anumber((size_t)(ne > 0 ? ne : 1));
  if (ne > 0) HIP_TRY(hipMemcpy(anumber.data(), e->M.elem_anumber, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToHost));
  const artis_decay::Rows r = artis_decay::build_rows(*d, anumber.data(), ne);
  decay_free(e->decay);  // a second set-up replaces the first
  e->decay = nullptr;
  dep_free(e->dep);  // ... and the deposition set-up that was made on it goes with it
  e->dep = nullptr;
  pinit_free(e->pinit);  // ... and the pellet set-up made on both
  e->pinit = nullptr;
  init_invalidate(e->init);  // ... and an initial state made on all three is no longer one of this network
  DecayState *st = new DecayState();
  st->ncell = n;
  const int64_t nn = d->nnuclides, np = d->npaths, nflat = (int64_t)r.path_lambda.size(), nrow = (int64_t)r.row_coef.size();
  const int rc = st->block.make(
      {piece(&st->d_nuc_lambda, nn), piece(&st->d_nuc_mass, nn), piece(&st->d_path_lambda, nflat), piece(&st->d_path_branch, np),
       piece(&st->d_path_start, np + 1), piece(&st->d_path_nuc, nflat), piece(&st->d_path_type, np), piece(&st->d_row_start, nn + 1),
       piece(&st->d_row_coef, nrow), piece(&st->d_row_top, nrow), piece(&st->d_elem_nuc_start, (int64_t)ne + 1),
       piece(&st->d_elem_nuc, (int64_t)r.elem_nuc.size()), piece(&st->d_initstable, ne), piece(&st->d_X, nn * n), piece(&st->d_untracked, n * ne),
       piece(&st->d_rho_tmin, n), piece(&st->d_coef, 2 * np), piece(&st->d_surv, nn), piece(&st->d_scale, np), piece(&st->d_x_dom, np),
       piece(&st->d_rho, n), piece(&st->d_massfrac, n * ne), piece(&st->d_meanweight, n * ne)},
      "decay", "the tables and the result block");
  if (rc != ARTIS_OK) {
    delete st;
    return rc;
  }
  e->decay = st;
  const hipMemcpyKind up = hipMemcpyHostToDevice;
  HIP_TRY(stage_copy(st->d_nuc_lambda, r.nuc_lambda.data(), nn, up));
  HIP_TRY(stage_copy(st->d_nuc_mass, r.nuc_mass.data(), nn, up));
  HIP_TRY(stage_copy(st->d_path_lambda, r.path_lambda.data(), nflat, up));
  HIP_TRY(stage_copy(st->d_path_branch, d->path_branchproduct, np, up));
  HIP_TRY(stage_copy(st->d_path_start, d->path_start, np + 1, up));
  HIP_TRY(stage_copy(st->d_path_nuc, d->path_nucindex, nflat, up));
  HIP_TRY(stage_copy(st->d_path_type, d->path_last_decaytype, np, up));
  HIP_TRY(stage_copy(st->d_row_start, r.row_start.data(), nn + 1, up));
  HIP_TRY(stage_copy(st->d_row_coef, r.row_coef.data(), nrow, up));
  HIP_TRY(stage_copy(st->d_row_top, r.row_top.data(), nrow, up));
  HIP_TRY(stage_copy(st->d_elem_nuc_start, r.elem_nuc_start.data(), (int64_t)ne + 1, up));
  HIP_TRY(stage_copy(st->d_elem_nuc, r.elem_nuc.data(), (int64_t)r.elem_nuc.size(), up));
  HIP_TRY(stage_copy(st->d_initstable, d->elem_initstablemeannucmass, ne, up));
  HIP_TRY(stage_copy(st->d_untracked, d->elem_untrackedstable_initmassfrac, n * ne, up));
  HIP_TRY(stage_copy(st->d_rho_tmin, d->rho_tmin, n, up));
  if (nn * n > 0) {  // X arrives [cell][nuclide] and is kept [nuclide][cell]
    float *tmp = nullptr;
    HIP_TRY(hipMalloc((void **)&tmp, sizeof(float) * (size_t)(nn * n)));
    hipError_t err = hipMemcpy(tmp, d->initnucmassfrac, sizeof(float) * (size_t)(nn * n), up);
    if (err == hipSuccess) {
      hipLaunchKernelGGL(k_decay_transpose, dim3(nblocks(nn * n)), dim3(BLOCK), 0, nullptr, tmp, st->d_X, n, (int32_t)nn);
      err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    (void)hipFree(tmp);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("decay: k_decay_transpose: ") + hipGetErrorString(err));
  }
  artis_decay::Tables &T = st->T;
  T.nnuclides = (int32_t)nn;
  T.npaths = (int32_t)np;
  T.nelements = ne;
  T.he4_nucindex = r.he4_nucindex;
  T.nuc_lambda = st->d_nuc_lambda;
  T.nuc_mass = st->d_nuc_mass;
  T.path_start = st->d_path_start;
  T.path_nucindex = st->d_path_nuc;
  T.path_lambda = st->d_path_lambda;
  T.path_branchproduct = st->d_path_branch;
  T.path_last_decaytype = st->d_path_type;
  T.row_start = st->d_row_start;
  T.row_coef = st->d_row_coef;
  T.row_top = st->d_row_top;
  T.elem_nuc_start = st->d_elem_nuc_start;
  T.elem_nuc = st->d_elem_nuc;
  T.elem_initstablemeannucmass = st->d_initstable;
  st->t_model = d->t_model;
  st->h_meanlife.assign(d->nuc_meanlife, d->nuc_meanlife + nn);
  for (int64_t p = 0; p < np; p++) {
    st->h_path_top.push_back(d->path_nucindex[d->path_start[p]]);
    st->h_path_end.push_back(d->path_nucindex[d->path_start[p + 1] - 1]);
  }
  return ARTIS_OK;
}

int artis_amd_decay_update(artis_amd_engine *e, double t_mid, const artis_decay_coeffs *coeffs, int want_nuclides, void *hip_stream) {
  if (!e) return stage_error(ARTIS_ERR_ARG, "decay: null engine");
  if (!e->decay) return stage_error(ARTIS_ERR_ARG, "decay: no network (artis_amd_decay_setup)");
  DecayState *st = e->decay;
  if (!(t_mid >= st->t_model) || !std::isfinite(t_mid)) return stage_error(ARTIS_ERR_ARG, "decay: t_mid is before t_model or non-finite");
  if (coeffs) {
    STAGE_STRUCT_SIZE(coeffs, artis_decay_coeffs, "decay");
    if ((st->T.npaths > 0 && (!coeffs->endnuc_coeff || !coeffs->he4_coeff)) || (st->T.nnuclides > 0 && !coeffs->survivingfrac))
      return stage_error(ARTIS_ERR_ARG, "decay: coefficients without endnuc_coeff, he4_coeff or survivingfrac");
  }
  HIP_TRY(hipSetDevice(e->device));
  const int64_t n = st->ncell, nn = st->T.nnuclides, np = st->T.npaths;
  if (want_nuclides && !st->d_nucmf && nn * n > 0) {
    const int rc = st->nuc_block.make({piece(&st->d_nucmf, nn * n)}, "decay", "the nuclides' mass fractions");
    if (rc != ARTIS_OK) return rc;
  }
  st->valid = false;
  hipStream_t s = (hipStream_t)hip_stream;
  DecayArgs a{};
  a.T = st->T;
  a.ncell = n;
  a.t_afterinit = t_mid - st->t_model;
  a.t_mid = t_mid;
  a.tmin = e->model_copy.tmin;
  a.X = st->d_X;
  a.untracked = st->d_untracked;
  a.rho_tmin = st->d_rho_tmin;
  a.coef = st->d_coef;
  a.surv = st->d_surv;
  a.scale = st->d_scale;
  a.x_dom = st->d_x_dom;
  a.rho = st->d_rho;
  a.massfrac = st->d_massfrac;
  a.meanweight = st->d_meanweight;
  a.nucmf = st->d_nucmf;
  auto done = [&](const char *kernel) -> int {
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("decay: ") + kernel + ": " + hipGetErrorString(err));
    return ARTIS_OK;
  };
  int rc;
  HIP_TRY(hipEventRecord(st->block.ev[0], s));
  if (coeffs) {
    HIP_TRY(stage_copy(st->d_coef, coeffs->endnuc_coeff, np, hipMemcpyHostToDevice, &s));
    HIP_TRY(stage_copy(st->d_coef ? st->d_coef + np : nullptr, coeffs->he4_coeff, np, hipMemcpyHostToDevice, &s));
    HIP_TRY(stage_copy(st->d_surv, coeffs->survivingfrac, nn, hipMemcpyHostToDevice, &s));
    if (np > 0) {
      HIP_TRY(hipMemsetAsync(st->d_scale, 0, sizeof(double) * (size_t)np, s));
      HIP_TRY(hipMemsetAsync(st->d_x_dom, 0, sizeof(double) * (size_t)np, s));
    }
    HIP_TRY(hipStreamSynchronize(s));  // (the caller's arrays are free again)
  } else if (np + nn > 0) {
    hipLaunchKernelGGL(k_decay_coeffs, dim3(nblocks(np + nn)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_decay_coeffs")) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block.ev[1], s));
  if (n > 0) {
    const int64_t nel = a.T.nelements > 0 ? a.T.nelements : 1;
    hipLaunchKernelGGL(k_decay_cells, dim3((unsigned)(nblocks(n) * nel)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_decay_cells")) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block.ev[2], s));
  if (want_nuclides && nn * n > 0) {
    hipLaunchKernelGGL(k_decay_nuclides, dim3(nblocks(nn * n)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_decay_nuclides")) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block.ev[3], s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 3; k++) HIP_TRY(st->block.elapsed_ms(k, &st->kernel_ms[k]));
  st->t_mid = t_mid;
  st->have_nuclides = want_nuclides != 0;
  st->serial++;
  st->valid = true;
  return ARTIS_OK;
}

int artis_amd_decay_download(artis_amd_engine *e, artis_decay_result *out) {
  if (!e || !out) return stage_error(ARTIS_ERR_ARG, "decay: null argument");
  STAGE_STRUCT_SIZE(out, artis_decay_result, "decay");
  if (!e->decay || !e->decay->valid) return stage_error(ARTIS_ERR_ARG, "decay: nothing updated (artis_amd_decay_update)");
  DecayState *st = e->decay;
  if (out->nuc_massfracs && !st->have_nuclides) return stage_error(ARTIS_ERR_ARG, "decay: the last update was not asked for the nuclides' mass fractions");
  HIP_TRY(hipSetDevice(e->device));
  const int64_t n = st->ncell, ne = st->T.nelements, nn = st->T.nnuclides, np = st->T.npaths;
  const hipMemcpyKind down = hipMemcpyDeviceToHost;
  HIP_TRY(stage_copy(out->rho, st->d_rho, n, down));
  HIP_TRY(stage_copy(out->elem_massfracs, st->d_massfrac, n * ne, down));
  HIP_TRY(stage_copy(out->elem_meanweight, st->d_meanweight, n * ne, down));
  HIP_TRY(stage_copy(out->endnuc_coeff, st->d_coef, np, down));
  HIP_TRY(stage_copy(out->he4_coeff, st->d_coef ? st->d_coef + np : nullptr, np, down));
  HIP_TRY(stage_copy(out->survivingfrac, st->d_surv, nn, down));
  HIP_TRY(stage_copy(out->path_scale, st->d_scale, np, down));
  HIP_TRY(stage_copy(out->path_x_dom, st->d_x_dom, np, down));
  if (out->nuc_massfracs && nn * n > 0) {  // kept [nuclide][cell], handed out [cell][nuclide]
    std::vector<double> t((size_t)(nn * n));
    HIP_TRY(stage_copy(t.data(), st->d_nucmf, nn * n, down));
    for (int64_t nuc = 0; nuc < nn; nuc++)
      for (int64_t c = 0; c < n; c++) out->nuc_massfracs[c * nn + nuc] = t[(size_t)(nuc * n + c)];
  }
  out->npts_nonempty = (int32_t)n;
  out->nelements = (int32_t)ne;
  out->nnuclides = (int32_t)nn;
  out->npaths = (int32_t)np;
  out->he4_nucindex = st->T.he4_nucindex;
  out->have_nuclides = st->have_nuclides ? 1 : 0;
  for (int k = 0; k < 3; k++) out->kernel_ms[k] = st->kernel_ms[k];
  out->t_mid = st->t_mid;
  return ARTIS_OK;
}

int artis_amd_grid_update_decayed(artis_amd_engine *e, const artis_grid_update *u, const artis_timestep *ts_next, void *hip_stream) {
  if (!e || !u || !ts_next) return stage_error(ARTIS_ERR_ARG, "grid_update_decayed: null engine, update or timestep");
#ifdef ARTIS_PRESET_NLTENEBULAR
  return stage_error(ARTIS_ERR_UNSUPPORTED, "grid_update_decayed: this build has NLTE populations (the nebular family): the ion balance is the host's");
#endif
  STAGE_STRUCT_SIZE(u, artis_grid_update, "grid_update_decayed");
  if (!e->decay || !e->decay->valid) return stage_error(ARTIS_ERR_ARG, "grid_update_decayed: no decay update (artis_amd_decay_update)");
  if (e->decay->t_mid != ts_next->mid) return stage_error(ARTIS_ERR_ARG, "grid_update_decayed: the decay update was made for another t_mid than ts_next->mid");
  if (u->rho || u->elem_massfracs || u->elem_meanweight)
    return stage_error(ARTIS_ERR_ARG, "grid_update_decayed: rho, elem_massfracs and elem_meanweight must be NULL (the matter is the decay update's)");
  const IbMatter matter{e->decay->d_rho, e->decay->d_massfrac, e->decay->d_meanweight};
  return ib_grid_update(e, u, ts_next, hip_stream, &matter);
}

}  // extern "C"
