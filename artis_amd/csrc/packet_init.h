// packet_init.h -- the initial pellet population, per decay path, per cell, per propagation cell and per packet.
//
// What the reference's packet_init() does before the first timestep (packet.cc:91-161): the decay energy every path releases per mass of
// its top nuclide during the simulation (calc_energy_per_massoftopnuc_decaypath decay.cc:1067), per model cell the decay energy per mass
// (get_modelcell_endecay_per_mass decay.cc:1052), the cumulative energy over ALL propagation cells in index order (packet.cc:116-131),
// and per packet (place_pellet packet.cc:54) the cell, a random position in it (grid.cc:1603), the decay channel, the decay time, the
// decaying nuclide and what it emits (setup_radioactive_pellet decay.cc:1347, sample_decaytime decay.cc:482, choose_gamma_ray
// gammapkt.cc:869), direction and rest-frame energy; at the end the normalisation of the packet energies (packet.cc:149-159). The
// engine's kernels (stage_packet_init.h) and the loops of tests/packet_init_host (x86) call the same bodies.
//
// Every sum here is a chain of dependent additions in the reference's order. The one that costs packets x paths in the reference -- the
// running sum of X[top[p]] * E[p] a packet's channel is drawn from -- is walked ONCE per cell (cell_checkpoints), which keeps the running
// value before every CKPT_STRIDE-th path; a packet searches its cell's checkpoints and re-adds at most CKPT_STRIDE terms from the stored
// double (choose_channel): the same additions from the same value, so the same bits as the reference's whole walk.
//
// A packet draws from its own generator (seeded seed_base + n, input.cc:1912) in the reference's order. The decay time is a rejection
// loop without a bound in the reference; here a call makes at most `budget` trials and says whether one was accepted, the generator's
// state between two whole trials is all that has to be kept to go on.
//
// Floating-point discipline as decay_update.h: -ffp-contract=off, the reference's order of operations and float / double mixing.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "deposition.h"

namespace artis_pinit {

constexpr int CKPT_STRIDE = 64;  // paths between two checkpoints of a cell's running sum
constexpr int CKPT_DEPTH = 32;   // X lines a lane has in flight before it adds the first of them (k_pinit_checkpoints)
constexpr int NDECAYTYPES = 6;
constexpr int DEFAULT_TRIALS_PER_LAUNCH = 4096;
constexpr int MAX_CONTINUATION_LAUNCHES = 4096;
constexpr int CHANNEL_UNSET = -2;  // a packet whose channel has not been drawn yet

// ---- tables: views of host or device arrays

// the propagation grid (the engine's model)
struct Grid {
  int32_t gridtype, ngrid;
  int32_t ncoordgrid[3], coordstride[3];
  const double *coord_pos_min_tmin[3];
  const int32_t *propcell_nonemptymgi;  // [ngrid] -1: empty
  double rmax, tmin;
};

struct Tables {
  int32_t nnuclides, npaths;
  // per path: its nuclides [path_start[p], path_start[p + 1]) top ... end (the daughter of the last decay), their lambdas beside them
  const int32_t *path_start, *path_nucindex, *path_last_decaytype, *path_top;
  const double *path_lambda, *path_branchproduct;
  // per nuclide
  const double *nuc_meanlife, *nuc_mass;
  const double *endecay_gamma, *endecay_particle, *probsum;  // [nn], [nn][NDECAYTYPES], [nn]
  const int32_t *gamma_start;                                // [nn + 1]
  const double *gamma_energy, *gamma_probability;
  const double *initenergyq;  // [ncell]; null: no initial-energy channel
  double t_model, tmin, tmax;
  int32_t initial_packets_on;
};

AHD int ncheckpoints(const int npaths) { return (npaths + CKPT_STRIDE - 1) / CKPT_STRIDE; }

// ---- the grid (grid.cc:215-225, :1559, :1577)

AHD int coordidx(const Grid &G, const int cellindex, const int axis) { return (cellindex / G.coordstride[axis]) % G.ncoordgrid[axis]; }
AHD double coordmin(const Grid &G, const int cellindex, const int axis) { return G.coord_pos_min_tmin[axis][coordidx(G, cellindex, axis)]; }
AHD double coordmax(const Grid &G, const int cellindex, const int axis) {
  const int idx = coordidx(G, cellindex, axis);
  return idx < G.ncoordgrid[axis] - 1 ? G.coord_pos_min_tmin[axis][idx + 1] : G.rmax;
}

// get_propcell_volume_tmin grid.cc:1577
AHD double propcell_volume_tmin(const Grid &G, const int cellindex) {
  if (G.gridtype == ARTIS_GRID_CARTESIAN3D) {
    const double deltax = coordmax(G, 0, 0) - coordmin(G, 0, 0);
    return artis::pow3(deltax);
  }
  if (G.gridtype == ARTIS_GRID_CYLINDRICAL2D) {
    const double delta_z = coordmax(G, 0, 1) - coordmin(G, 0, 1);
    const double delta_rcylsquared = artis::pow2(coordmax(G, cellindex, 0)) - artis::pow2(coordmin(G, cellindex, 0));
    return delta_z * artis::PI * delta_rcylsquared;
  }
  return 4. / 3. * artis::PI * (artis::pow3(coordmax(G, cellindex, 0)) - artis::pow3(coordmin(G, cellindex, 0)));
}

// std::lerp(a, b, t) as libstdc++ evaluates it (the form of P0811R3): the two-product form when a and b do not have the same sign,
// b itself at t == 1, else a + t (b - a) clamped at b so that it stays monotonic near t = 1. NOT a + t (b - a) for all inputs.
AHD double lerp_std(const double a, const double b, const double t) {
  if ((a <= 0 && b >= 0) || (a >= 0 && b <= 0)) return t * b + (1 - t) * a;
  if (t == 1) return b;
  const double x = a + t * (b - a);
  return (t > 1) == (b > a) ? (b < x ? x : b) : (b > x ? x : b);
}

// get_propcell_random_xyz_position_tmin grid.cc:1603
AHD void random_position(const Grid &G, const int cellindex, artis::Pkt &rng, double pos[3]) {
  if (G.gridtype == ARTIS_GRID_SPHERICAL1D) {
    const double r_inner = coordmin(G, cellindex, 0);
    const double r_outer = coordmax(G, cellindex, 0);
    const double radius = cbrt(lerp_std(artis::pow3(r_outer), artis::pow3(r_inner), artis::rng_uniform_pos(rng)));
    double iso[3];
    artis::rand_isotropic(rng, iso);
    for (int i = 0; i < 3; i++) pos[i] = iso[i] * radius;
  } else if (G.gridtype == ARTIS_GRID_CYLINDRICAL2D) {
    const double rcyl_inner = coordmin(G, cellindex, 0);
    const double rcyl_outer = coordmax(G, cellindex, 0);
    const double rcyl_rand = sqrt(lerp_std(artis::pow2(rcyl_outer), artis::pow2(rcyl_inner), artis::rng_uniform_pos(rng)));
    const double theta_rand = artis::rng_uniform(rng) * 2 * artis::PI;
    const double z_rand = lerp_std(coordmin(G, cellindex, 1), coordmax(G, cellindex, 1), artis::rng_uniform_pos(rng));
    double s, c;
    artis::sin_cos(theta_rand, &s, &c);
    pos[0] = c * rcyl_rand;
    pos[1] = s * rcyl_rand;
    pos[2] = z_rand;
  } else {
    for (int axis = 0; axis < 3; axis++) {
      const double cmin = coordmin(G, cellindex, axis);
      pos[axis] = cmin + (artis::rng_uniform_pos(rng) * (coordmax(G, cellindex, axis) - cmin));
    }
  }
}

// ---- per path

// calc_energy_per_massoftopnuc_decaypath decay.cc:1067 for one path
AHD double path_energy(const Tables &T, const int p) {
  const int i0 = T.path_start[p], n = T.path_start[p + 1] - i0;
  const int top = T.path_nucindex[i0], last = T.path_nucindex[i0 + n - 2];
  const double time_min_decay = T.initial_packets_on ? T.t_model : T.tmin;
  const double f1 = artis_decay::decaychain(T.path_lambda + i0, n, T.tmax - T.t_model, true).abund;  // calc_decaypath_unitfactor decay.cc:500
  const double f0 = artis_decay::decaychain(T.path_lambda + i0, n, time_min_decay - T.t_model, true).abund;
  const double d = f1 - f0;
  const double fdecayed = d > 0. ? d : 0.;
  // get_decaypath_lastdecayenergy decay.cc:238
  const double endecay = T.endecay_gamma[last] + T.endecay_particle[(int64_t)last * NDECAYTYPES + T.path_last_decaytype[p]];
  const double lastdecayenergy = endecay / T.probsum[last];
  return T.path_branchproduct[p] * fdecayed * lastdecayenergy / T.nuc_mass[top];
}

// ---- per cell. X is [nuclide][cell] (stride cells per nuclide), float; ckpt is [ncheckpoints + 1][cell]

// The running sum of X[top[p]] * E[p] over the paths in order (decay.cc:1057, :1360): its value before path j * CKPT_STRIDE goes to
// ckpt[j] (store: this lane has a cell of its own), the total to ckpt[ncheckpoints] and to the caller. The loads of CKPT_DEPTH paths
// are issued before their additions; top and E are indexed by the loop counters only.
AHD double cell_checkpoints(const int npaths, const int32_t *__restrict__ top, const double *__restrict__ E, const float *__restrict__ X, const int64_t stride,
                            const int64_t c, double *__restrict__ ckpt, const bool store) {
  static_assert(CKPT_STRIDE % CKPT_DEPTH == 0, "a checkpoint falls between two batches of loads");
  double sum = 0.;
  int k = 0;
  for (; k + CKPT_DEPTH <= npaths; k += CKPT_DEPTH) {
    if (k % CKPT_STRIDE == 0 && store) ckpt[(int64_t)(k / CKPT_STRIDE) * stride + c] = sum;
    float x[CKPT_DEPTH];
#pragma unroll
    for (int j = 0; j < CKPT_DEPTH; j++) x[j] = X[(int64_t)top[k + j] * stride + c];
#pragma unroll
    for (int j = 0; j < CKPT_DEPTH; j++) sum += x[j] * E[k + j];
  }
  for (; k < npaths; k++) {
    if (k % CKPT_STRIDE == 0 && store) ckpt[(int64_t)(k / CKPT_STRIDE) * stride + c] = sum;
    sum += X[(int64_t)top[k] * stride + c] * E[k];
  }
  if (store) ckpt[(int64_t)ncheckpoints(npaths) * stride + c] = sum;
  return sum;
}

// term `cellindex` of en_cumulative (packet.cc:119-131); an empty cell adds nothing (+0.0 to a non-negative sum: the same value)
AHD double cumulative_term(const Grid &G, const Tables &T, const float *rho_tmin, const double *endecay_per_mass, const int cellindex) {
  const int c = G.propcell_nonemptymgi[cellindex];
  if (c < 0) return 0.;
  const double initial_en_per_mass = T.initenergyq ? T.initenergyq[c] : 0.;
  return propcell_volume_tmin(G, cellindex) * rho_tmin[c] * (endecay_per_mass[c] + initial_en_per_mass);
}

// ---- per packet

// what the per-packet bodies work with besides the tables
struct Work {
  Tables T;
  Grid G;
  const double *E;  // [npaths] the energy vector
  const float *X;
  int64_t ncell;
  const double *ckpt;
  const double *en_cumulative;  // [ngrid]
  double e_cmf_per_packet;
};

// Xoshiro128PP::seed random.h:117 through SplitMix32 (random.h:36-40, :78-89)
AHD void seed_rng(artis::Pkt &rng, const uint32_t seed) {
  uint64_t state = (uint64_t)seed + 0x9E3779B97F4A7C15ull;
  state = (state ^ (state >> 30U)) * 0xBF58476D1CE4E5B9ull;
  state = (state ^ (state >> 27U)) * 0x94D049BB133111EBull;
  uint32_t s = (uint32_t)(state ^ (state >> 31U));
  uint32_t out[4];
  for (int i = 0; i < 4; i++) {
    uint32_t r = (s += 0x9e3779b9U);
    r = (r ^ (r >> 16U)) * 0x21f0aaadU;
    r = (r ^ (r >> 15U)) * 0x735a2d97U;
    out[i] = r ^ (r >> 15U);
  }
  rng.s0 = out[0], rng.s1 = out[1], rng.s2 = out[2], rng.s3 = out[3];
}
AHD void load_rng(artis::Pkt &rng, const artis_packet &q) { rng.s0 = q.rngstate[0], rng.s1 = q.rngstate[1], rng.s2 = q.rngstate[2], rng.s3 = q.rngstate[3]; }
AHD void store_rng(const artis::Pkt &rng, artis_packet &q) { q.rngstate[0] = rng.s0, q.rngstate[1] = rng.s1, q.rngstate[2] = rng.s2, q.rngstate[3] = rng.s3; }

// the defaults of packet.h:115-153
AHD void packet_defaults(artis_packet &q) {
  const double nan = NAN;
  q.prop_time = -1.;
  for (int i = 0; i < 3; i++) {
    q.pos[i] = 0., q.dir[i] = 0.;
    q.em_pos[i] = nan, q.trueem_pos[i] = nan;
  }
  q.nu_cmf = 0., q.e_cmf = 0., q.nu_rf = 0., q.e_rf = 0.;
  q.next_trans = -1, q.nscatterings = 0;
  q.emissiontype = ARTIS_EMTYPE_NOTSET;
  q.em_time = -1.f;
  q.absorptiontype = 0;
  q.absorptionfreq = 0., q.stokes_q = 0., q.stokes_u = 0.;
  q.trueemissiontype = ARTIS_EMTYPE_NOTSET;
  q.trueem_time = -1.f;
  q.type = 0, q.cellindex = -1, q.escape_type = 0;
  q.escape_time = -1.f;
  q.tdecay = -1.;
  q.number = -1;
  q.originated_from_particlenotgamma = 0;
  q.pellet_decaytype = -1, q.pellet_nucindex = -1;
}

// the channel of a draw by a cell's checkpoints (decay.cc:1356-1378): the first entry of the cell's running sum -- with the initial-energy
// entry behind the paths when that channel is on -- that is greater than u * the last entry. npaths: the initial-energy channel.
AHD int choose_channel(const Work &W, const int64_t c, const float u) {
  const Tables &T = W.T;
  const int nck = ncheckpoints(T.npaths);
  const double paths_total = W.ckpt[(int64_t)nck * W.ncell + c];
  const double last = T.initenergyq ? paths_total + T.initenergyq[c] : paths_total;
  const double zrand_en = u * last;
  // the first block whose last entry (the next block's checkpoint) is greater than the target
  int lo = 0, len = nck;
  while (len > 0) {
    const int half = len / 2;
    if (!(zrand_en < W.ckpt[(int64_t)(lo + half + 1) * W.ncell + c])) {
      lo += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  if (lo >= nck) return T.npaths;
  double sum = W.ckpt[(int64_t)lo * W.ncell + c];
  const int p1 = (lo + 1) * CKPT_STRIDE < T.npaths ? (lo + 1) * CKPT_STRIDE : T.npaths;
  for (int p = lo * CKPT_STRIDE; p < p1; p++) {
    sum += W.X[(int64_t)T.path_top[p] * W.ncell + c] * W.E[p];
    if (zrand_en < sum) return p;
  }
  return p1 - 1;  // (not reached: the block's last entry is this sum)
}

// the same channel from the whole running sum, as the reference builds it for every packet (the restatement the tests hold the
// checkpoints against); cum: scratch of npaths + 1 doubles
AHD int choose_channel_full(const Work &W, const int64_t c, const float u, double *cum) {
  const Tables &T = W.T;
  double energysum = 0.;
  int n = 0;
  for (int p = 0; p < T.npaths; p++) {
    energysum += W.X[(int64_t)T.path_top[p] * W.ncell + c] * W.E[p];
    cum[n++] = energysum;
  }
  if (T.initenergyq) {
    energysum += T.initenergyq[c];
    cum[n++] = energysum;
  }
  return artis::upper_bound_d(cum, n, u * cum[n - 1]);
}

// place_pellet packet.cc:54-68: draw 1 (the cell) and the position. The generator's state is left in q.
AHD void pellet_place(const Work &W, const int64_t n, const uint32_t seed, artis_packet &q) {
  artis::Pkt rng;
  seed_rng(rng, seed);
  packet_defaults(q);
  const double etot_simtime = W.en_cumulative[W.G.ngrid - 1];
  const double targetval = artis::rng_uniform(rng) * etot_simtime;
  int cellindex = artis::upper_bound_d(W.en_cumulative, W.G.ngrid, targetval);
  if (cellindex > W.G.ngrid - 1) cellindex = W.G.ngrid - 1;  // (not reached: u < 1 and the sum's last entry is positive)
  q.cellindex = cellindex;
  q.number = (int32_t)n;
  q.prop_time = W.G.tmin;
  random_position(W.G, cellindex, rng, q.pos);
  store_rng(rng, q);
}

// sample_decaytime decay.cc:482 with a bound: at most `budget` whole trials; true: one was accepted (*tdecay). *trials counts them.
AHD bool sample_decaytime(const Tables &T, const int p, artis::Pkt &rng, const int budget, int32_t *trials, double *tdecay) {
  const double tdecaymin = !T.initial_packets_on ? T.tmin : T.t_model;
  const int i0 = T.path_start[p], maxlength = T.path_start[p + 1] - i0 - 1;
  for (int trial = 0; trial < budget; trial++) {
    double t = T.t_model;
    for (int i = 0; i < maxlength; i++) t -= T.nuc_meanlife[T.path_nucindex[i0 + i]] * log((double)artis::rng_uniform_pos(rng));
    if (*trials < 0x7fffffff) (*trials)++;
    if (!(t <= tdecaymin || t >= T.tmax)) {
      *tdecay = t;
      return true;
    }
  }
  return false;
}

// choose_gamma_ray gammapkt.cc:869: nu_cmf of the line drawn; -1 without a draw for a nuclide with no lines
AHD double choose_gamma_ray(const Tables &T, const int nuc, artis::Pkt &rng) {
  const int g0 = T.gamma_start[nuc], g1 = T.gamma_start[nuc + 1];
  if (g0 >= g1) return -1;
  const double E_gamma = T.endecay_gamma[nuc];
  const double zrand = artis::rng_uniform(rng);
  double runtot = 0.;
  for (int g = g0; g < g1; g++) {
    runtot += T.gamma_probability[g] * T.gamma_energy[g] / E_gamma;
    if (zrand < runtot) return T.gamma_energy[g] / artis::HPLANCK;
  }
  return T.gamma_energy[g1 - 1] / artis::HPLANCK;
}

// packet.cc:83-85
AHD void pellet_restframe(const Grid &G, artis_packet &q) {
  artis::vnorm(q.pos, q.dir);
  const double dopplerfactor = artis::doppler_at(q.pos[0], q.pos[1], q.pos[2], q.dir[0], q.dir[1], q.dir[2], q.prop_time);
  q.e_rf = q.e_cmf / dopplerfactor;
}

// setup_radioactive_pellet decay.cc:1347 of a placed packet, from the generator state in q. *channel: CHANNEL_UNSET before the first
// call, then the channel drawn. At most `budget` decay-time trials: false when none was accepted -- the packet is left as it was but
// for its generator state and *trials, and a further call goes on from there.
AHD bool pellet_decay(const Work &W, artis_packet &q, int32_t *channel, int32_t *trials, const int budget) {
  const Tables &T = W.T;
  artis::Pkt rng;
  load_rng(rng, q);
  if (*channel == CHANNEL_UNSET) {
    const int64_t c = W.G.propcell_nonemptymgi[q.cellindex];
    *channel = choose_channel(W, c, artis::rng_uniform(rng));
    if (*channel >= T.npaths) {  // the cell's initial energy
      q.tdecay = T.tmin;
      q.type = ARTIS_TYPE_RADIOACTIVE_PELLET;
      q.e_cmf = W.e_cmf_per_packet;
      q.nu_cmf = W.e_cmf_per_packet / artis::HPLANCK;
      q.pellet_nucindex = -1;
      q.pellet_decaytype = -1;
      pellet_restframe(W.G, q);
      store_rng(rng, q);
      return true;
    }
  }
  const int p = *channel;
  double tdecay;
  const bool accepted = sample_decaytime(T, p, rng, budget, trials, &tdecay);
  store_rng(rng, q);
  if (!accepted) return false;
  q.tdecay = tdecay;
  q.e_cmf = W.e_cmf_per_packet;
  q.type = ARTIS_TYPE_RADIOACTIVE_PELLET;
  const int nuc = T.path_nucindex[T.path_start[p + 1] - 2];
  const int decaytype = T.path_last_decaytype[p];
  q.pellet_nucindex = nuc;
  q.pellet_decaytype = decaytype;
  const double engamma = T.endecay_gamma[nuc];
  const double enparticle = T.endecay_particle[(int64_t)nuc * NDECAYTYPES + decaytype];
  const bool particle = (artis::rng_uniform(rng) >= engamma / (engamma + enparticle));
  q.originated_from_particlenotgamma = particle ? 1 : 0;
  q.nu_cmf = particle ? enparticle / artis::HPLANCK : choose_gamma_ray(T, nuc, rng);
  pellet_restframe(W.G, q);
  store_rng(rng, q);
  return true;
}

// packet.cc:156-159
AHD void pellet_normalise(artis_packet &q, const double e_ratio) {
  q.e_cmf *= e_ratio;
  q.e_rf *= e_ratio;
}

// ---- host: validation (plain C++)

// empty: the model is usable on a decay set-up of nnuclides nuclides (nuc_meanlife) and ncell cells; else what is wrong with it, naming
// the nuclide. *unsupported: the refusal is of an option this stage does not have, not of a value
inline std::string packet_init_validate(const artis_packet_init_model &m, const int nnuclides, const int64_t ncell, const double *nuc_meanlife, const double tmin,
                                        const double t_model, bool *unsupported) {
  const auto finite_nonneg = [](double v) { return std::isfinite(v) && v >= 0.; };
  *unsupported = false;
  if (!m.uniform_pellet_energies) {
    *unsupported = true;
    return "UNIFORM_PELLET_ENERGIES off (a Bateman sum per packet, decay.cc:1407-1425) is not built";
  }
  if (m.max_trials_per_launch < 0) return "max_trials_per_launch is negative (0: the default)";
  if (!std::isfinite(m.tmax) || !(m.tmax > tmin)) return "tmax <= tmin, or non-finite";
  if (t_model > tmin) return "t_model > tmin";
  if (nnuclides > 0 && (!m.nuc_decay_daughters_probsum || !m.gamma_start)) return "nuc_decay_daughters_probsum and gamma_start are required";
  const bool channel = m.initial_packets_on && m.use_model_initial_energy;
  if (channel && ncell > 0 && !m.initenergyq) return "INITIAL_PACKETS_ON with USE_MODEL_INITIAL_ENERGY needs initenergyq";
  if (!channel && m.initenergyq) return "initenergyq without INITIAL_PACKETS_ON and USE_MODEL_INITIAL_ENERGY";
  if (nnuclides > 0 && m.gamma_start[0] != 0) return "gamma_start[0] is not 0";
  for (int n = 0; n < nnuclides; n++) {
    const std::string name = "nuclide " + std::to_string(n) + ": ";
    const double ps = m.nuc_decay_daughters_probsum[n];
    if (!finite_nonneg(ps)) return name + "a negative or non-finite decay_daughters_probsum";
    if (nuc_meanlife[n] > 0. && !(ps > 0.)) return name + "it decays and its decay_daughters_probsum is not positive";
    if (m.gamma_start[n + 1] < m.gamma_start[n]) return name + "gamma_start is not monotone";
    if (m.gamma_start[n + 1] > m.gamma_start[n] && (!m.gamma_energy || !m.gamma_probability)) return name + "lines without gamma_energy and gamma_probability";
    for (int g = m.gamma_start[n]; g < m.gamma_start[n + 1]; g++)
      if (!finite_nonneg(m.gamma_energy[g]) || !finite_nonneg(m.gamma_probability[g])) return name + "a negative or non-finite line energy or probability";
  }
  if (channel)
    for (int64_t c = 0; c < ncell; c++)
      if (!finite_nonneg(m.initenergyq[c])) return "cell " + std::to_string(c) + ": a negative or non-finite initenergyq";
  return "";
}

// a handed-in energy vector is usable as it is: finite and non-negative
inline std::string energy_vector_validate(const double *E, const int npaths) {
  for (int p = 0; p < npaths; p++)
    if (!std::isfinite(E[p]) || E[p] < 0.) return "path " + std::to_string(p) + ": a negative or non-finite energy";
  return "";
}

}  // namespace artis_pinit
