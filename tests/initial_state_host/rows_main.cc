// rows_main.cc -- TEST HARNESS ONLY: the harness of initial_state_host.cc with a main of its own, for a build under the address and
// undefined-behaviour sanitizers (Makefile: rows_sanitized). Reads the networks that `python tests/initial_common.py DIR` writes (one
// text file each, the format of tests/decay_host/rows_main.cc), gives every nuclide energies from a fixed rule and 70 cells (more than
// one wave's worth, not a multiple of anything) mass fractions from another, forms the energy vector with the expansion factor and runs
// every cell with each of the three grey types and with the initial-energy channel on and off; prints a checksum; then checks that a
// few malformed parameter sets are refused.
#include <cstdio>
#include <fstream>

#include "initial_state_host.cc"

namespace {
struct Net {
  int nn = 0, np = 0;
  std::vector<int32_t> anumber, z, a, start, idx, type, gstart;
  std::vector<double> life, branch, gamma, particle, q, prob, vol, radial, probsum, initq;
  std::vector<float> X, rho_tmin, untracked, stablemass;
  artis_decay_model d{};
  artis_deposition_model em{};
  artis_packet_init_model m{};
};

bool read(const char *path, Net &n, int64_t ncell, bool channel) {
  std::ifstream f(path);
  int ne = 0;
  if (!(f >> n.nn >> n.np >> ne)) return false;
  n.anumber.resize((size_t)ne);
  for (auto &v : n.anumber) f >> v;
  n.z.resize((size_t)n.nn), n.a.resize((size_t)n.nn), n.life.resize((size_t)n.nn);
  for (int i = 0; i < n.nn; i++) f >> n.z[(size_t)i] >> n.a[(size_t)i] >> n.life[(size_t)i];
  n.start.resize((size_t)n.np + 1);
  for (auto &v : n.start) f >> v;
  n.idx.resize((size_t)n.start.back());
  for (auto &v : n.idx) f >> v;
  n.branch.resize((size_t)n.np), n.type.resize((size_t)n.np);
  for (auto &v : n.branch) f >> v;
  for (auto &v : n.type) f >> v;
  if (!f) return false;
  const size_t nn = (size_t)n.nn;
  n.gamma.assign(nn, 0.), n.particle.assign(6 * nn, 0.), n.q.assign(6 * nn, 0.), n.prob.assign(6 * nn, 0.), n.probsum.assign(nn, 0.);
  for (size_t i = 0; i < nn; i++) {
    if (!(n.life[i] > 0.)) continue;
    n.gamma[i] = 1e-6 * (double)(1 + i % 5);
    n.probsum[i] = 1.;
    for (int t = 0; t < 6; t++) n.particle[6 * i + (size_t)t] = 2e-7 * (double)(1 + t);
  }
  n.gstart.assign(nn + 1, 0);
  n.vol.assign((size_t)ncell, 1e40), n.radial.assign((size_t)ncell, 1e14), n.initq.assign((size_t)ncell, 3e15);
  n.X.resize((size_t)ncell * nn), n.rho_tmin.resize((size_t)ncell), n.untracked.assign(1, 0.f), n.stablemass.assign(1, 0.f);
  for (int64_t c = 0; c < ncell; c++) {
    n.rho_tmin[(size_t)c] = 1e-12f * (float)(1 + c % 7);
    for (size_t i = 0; i < nn; i++) n.X[(size_t)c * nn + i] = (c == 1) ? 0.f : 0.5f / (float)nn / (float)(1 + ((size_t)c + i) % 4);
  }
  n.d.struct_size = sizeof(n.d);
  n.d.nnuclides = n.nn, n.d.npaths = n.np;
  n.d.nuc_z = n.z.data(), n.d.nuc_a = n.a.data(), n.d.nuc_meanlife = n.life.data();
  n.d.path_start = n.start.data(), n.d.path_nucindex = n.idx.data(), n.d.path_branchproduct = n.branch.data(), n.d.path_last_decaytype = n.type.data();
  n.d.t_model = 86400.;
  n.d.initnucmassfrac = n.X.data(), n.d.elem_untrackedstable_initmassfrac = n.untracked.data(), n.d.elem_initstablemeannucmass = n.stablemass.data();
  n.d.rho_tmin = n.rho_tmin.data();
  n.em.struct_size = sizeof(n.em);
  n.em.nnuclides = n.nn, n.em.npts_nonempty = (int32_t)ncell;
  n.em.nuc_endecay_gamma = n.gamma.data(), n.em.nuc_endecay_particle = n.particle.data(), n.em.nuc_endecay_q = n.q.data(), n.em.nuc_branchprob = n.prob.data();
  n.em.assocvolume_tmin = n.vol.data(), n.em.radial_pos_tmin = n.radial.data();
  n.m.struct_size = sizeof(n.m);
  n.m.nuc_decay_daughters_probsum = n.probsum.data(), n.m.gamma_start = n.gstart.data();
  n.m.initenergyq = channel ? n.initq.data() : nullptr;
  n.m.tmax = 80. * 86400.;
  n.m.initial_packets_on = n.m.use_model_initial_energy = channel ? 1 : 0;
  n.m.uniform_pellet_energies = 1;
  return true;
}

uint64_t mix(uint64_t h, const void *p, size_t bytes) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < bytes; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s NETWORK.txt ...\n", argv[0]);
    return 2;
  }
  const int64_t ncell = 70;
  const double tmin = 2. * 86400., tstart = 2.05 * 86400., rmax = 4e14;
  for (int k = 1; k < argc; k++)
    for (const bool channel : {false, true}) {
      Net n;
      if (!read(argv[k], n, ncell, channel)) {
        std::fprintf(stderr, "%s: cannot read\n", argv[k]);
        return 2;
      }
      void *h = init_host_new(&n.d, &n.em, &n.m, ncell, tmin);
      if (!h) {
        std::fprintf(stderr, "%s: refused: %s\n", argv[k], init_host_last_error());
        return 1;
      }
      const size_t np = (size_t)n.np, nc = (size_t)ncell;
      std::vector<double> E(np + 1), scale(np + 1), x_dom(np + 1), endecay(nc);
      init_host_energy(h, tstart, E.data(), scale.data(), x_dom.data());
      // two elements, the second a lanthanide whose mass fraction runs over the branches of JUST2022
      const int32_t anumber[2] = {26, 60};
      std::vector<float> rho(nc), massfrac(2 * nc), ffegrp(nc), ye(nc), T(nc), kappa(nc), depth(nc);
      std::vector<int32_t> thick(nc), flags(nc);
      for (size_t c = 0; c < nc; c++) {
        rho[c] = n.rho_tmin[c] * 0.9f;
        massfrac[2 * c] = 0.5f;
        massfrac[2 * c + 1] = std::pow(10.f, -9.f + (float)(c % 10));
        ffegrp[c] = (float)(c % 11) / 10.f;
        ye[c] = 0.05f * (float)(1 + c % 9);
      }
      uint64_t sum = 14695981039346656037ull;
      int64_t counts[5];
      int32_t first;
      for (const int type : {ARTIS_GREY_FEGROUP_APPROX, ARTIS_GREY_TANAKA2020, ARTIS_GREY_JUST2022}) {
        artis_initial_params p{};
        p.struct_size = sizeof(p);
        p.tstart = tstart;
        p.nts_first = 0, p.num_grey_timesteps = 2;
        p.optical_depth_is_thick = 10., p.optical_depth_is_thick_vpkt = 5.;
        p.rpkt_grey_type = type;
        p.mfegroup = 1e33, p.mtot_input = 2.8e33;
        p.ffegrp = ffegrp.data(), p.initelectronfrac = ye.data();
        if (*init_host_validate(&p, ncell, n.d.t_model)) {
          std::fprintf(stderr, "%s: parameters refused: %s\n", argv[k], init_host_last_error());
          return 1;
        }
        init_host_cells(h, &p, E.data(), rmax, rho.data(), massfrac.data(), anumber, 2, T.data(), endecay.data(), kappa.data(), depth.data(), thick.data(),
                        flags.data(), counts, &first, 3);
        init_host_grey(h, &p, rmax, rho.data(), massfrac.data(), anumber, 2, T.data(), kappa.data(), depth.data(), thick.data());
        sum = mix(mix(mix(mix(sum, T.data(), 4 * nc), kappa.data(), 4 * nc), thick.data(), 4 * nc), endecay.data(), 8 * nc);
        if (counts[0] + counts[1] + counts[2] + counts[3] != ncell || counts[4] != 0) {
          std::fprintf(stderr, "%s: the branch counts do not add up\n", argv[k]);
          return 1;
        }
      }
      std::printf("%s channel %d: %d nuclides, %d paths, checksum %016llx\n", argv[k], (int)channel, n.nn, n.np, (unsigned long long)sum);
      // malformed parameter sets: each must be refused, none may read out of bounds
      int refused = 0;
      artis_initial_params p{};
      p.struct_size = sizeof(p);
      p.tstart = tstart;
      p.rpkt_grey_type = ARTIS_GREY_JUST2022;
      refused += *init_host_validate(&p, ncell, n.d.t_model) == 0 ? 0 : 100;  // (this one is usable)
      p.tstart = 0.5 * n.d.t_model;
      refused += *init_host_validate(&p, ncell, n.d.t_model) != 0;
      p.tstart = tstart;
      p.rpkt_grey_type = 3;
      refused += *init_host_validate(&p, ncell, n.d.t_model) != 0;
      p.rpkt_grey_type = ARTIS_GREY_TANAKA2020;
      refused += *init_host_validate(&p, ncell, n.d.t_model) != 0;  // no initelectronfrac
      ye[5] = 0.f;
      p.initelectronfrac = ye.data();
      refused += *init_host_validate(&p, ncell, n.d.t_model) != 0;
      p.rpkt_grey_type = ARTIS_GREY_FEGROUP_APPROX;
      p.ffegrp = ffegrp.data();
      refused += *init_host_validate(&p, ncell, n.d.t_model) != 0;  // mtot_input 0
      std::printf("%s channel %d: %d of 5 malformed parameter sets refused\n", argv[k], (int)channel, refused);
      init_host_free(h);
      if (refused != 5) return 1;
    }
  return 0;
}
