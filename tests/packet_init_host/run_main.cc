// run_main.cc -- TEST HARNESS ONLY: the harness of packet_init_host.cc with a main of its own, for a build under the address and
// undefined-behaviour sanitizers (Makefile: run_sanitized). A three-nuclide network (A -> B -> C, C stable: the paths A-B, A-B-C, B-C)
// on a 1D, a 2D and a 3D grid with empty cells, with more paths than one checkpoint stride by repeating the network, the initial-energy
// channel on and off, and a trial budget of 1 so that every packet is parked and continued.
#include <cstdio>

#include "packet_init_host.cc"

namespace {
int run_grid(int gridtype, int copies, bool channel) {
  const int nc = 4;
  artis_model model{};
  model.gridtype = gridtype;
  const int ndim = gridtype == ARTIS_GRID_SPHERICAL1D ? 1 : gridtype == ARTIS_GRID_CYLINDRICAL2D ? 2 : 3;
  model.rmax = 4e14;
  model.tmin = 2. * 86400.;
  std::vector<double> coord[3];
  int ngrid = 1;
  for (int a = 0; a < 3; a++) {
    model.ncoordgrid[a] = a < ndim ? nc : 1;
    ngrid *= model.ncoordgrid[a];
    const bool from_zero = gridtype == ARTIS_GRID_SPHERICAL1D || (gridtype == ARTIS_GRID_CYLINDRICAL2D && a == 0);
    for (int i = 0; i < model.ncoordgrid[a]; i++) coord[a].push_back(from_zero ? model.rmax * i / nc : -model.rmax + 2 * model.rmax * i / nc);
    model.coord_pos_min_tmin[a] = coord[a].data();
  }
  model.ngrid = ngrid;
  std::vector<int32_t> prop((size_t)ngrid);
  int ncell = 0;
  for (int i = 0; i < ngrid; i++) prop[(size_t)i] = (i % 5 == 3) ? -1 : ncell++;
  model.npts_nonempty = ncell;
  model.propcell_nonemptymgi = prop.data();

  const int nn = 3 * copies, np = 3 * copies;
  std::vector<int32_t> z, a_, start{0}, nuc, type;
  std::vector<double> life, branch, gamma, particle((size_t)nn * 6, 0.), qval((size_t)nn * 6, 0.), bprob((size_t)nn * 6, 0.), probsum, genergy, gprob;
  std::vector<int32_t> gstart{0};
  for (int k = 0; k < copies; k++) {
    const int b = 3 * k;
    z.insert(z.end(), {28, 27, 26});
    a_.insert(a_.end(), {56 + k, 56 + k, 56 + k});
    life.insert(life.end(), {8.8 * 86400. * (1 + k), 111. * 86400. * (1 + 0.5 * k), -1.});
    gamma.insert(gamma.end(), {2.7e-6, 5.7e-6, 0.});
    probsum.insert(probsum.end(), {1., 1., 0.});
    particle[(size_t)(b + 1) * 6 + ARTIS_DECAYTYPE_BETAPLUS] = 1e-6;
    bprob[(size_t)b * 6 + ARTIS_DECAYTYPE_ELECTRONCAPTURE] = 1.;
    bprob[(size_t)(b + 1) * 6 + ARTIS_DECAYTYPE_BETAPLUS] = 1.;
    genergy.insert(genergy.end(), {1e-6, 1.7e-6});
    gprob.insert(gprob.end(), {0., 2.7 / 1.7});
    gstart.push_back((int32_t)genergy.size());  // A: two lines, the first of zero probability
    gstart.push_back((int32_t)genergy.size());  // B: none
    gstart.push_back((int32_t)genergy.size());
    const int paths[3][3] = {{b, b + 1, -1}, {b, b + 1, b + 2}, {b + 1, b + 2, -1}};
    for (const auto &p : paths) {
      for (int i = 0; i < 3; i++)
        if (p[i] >= 0) nuc.push_back(p[i]);
      start.push_back((int32_t)nuc.size());
      branch.push_back(1.);
      type.push_back(nuc.back() % 3 == 1 ? ARTIS_DECAYTYPE_ELECTRONCAPTURE : ARTIS_DECAYTYPE_BETAPLUS);
    }
  }
  std::vector<float> X((size_t)ncell * nn), rho((size_t)ncell), untracked(1), stablemass(1);
  for (int c = 0; c < ncell; c++) {
    rho[(size_t)c] = 1e-12f * (1 + c % 7);
    for (int n = 0; n < nn; n++) X[(size_t)c * nn + n] = (c == 1 || n % 3 == 2) ? 0.f : 0.3f / (float)copies / (float)(1 + (c + n) % 4);
  }
  artis_decay_model d{};
  d.struct_size = sizeof(d);
  d.nnuclides = nn, d.npaths = np;
  d.nuc_z = z.data(), d.nuc_a = a_.data(), d.nuc_meanlife = life.data();
  d.path_start = start.data(), d.path_nucindex = nuc.data(), d.path_branchproduct = branch.data(), d.path_last_decaytype = type.data();
  d.t_model = 86400.;
  d.initnucmassfrac = X.data(), d.elem_untrackedstable_initmassfrac = untracked.data(), d.elem_initstablemeannucmass = stablemass.data(), d.rho_tmin = rho.data();
  std::vector<double> vol((size_t)ncell, 1e40), radial((size_t)ncell, 1e14), initq((size_t)ncell, 3e15);
  initq[1] = 0.;
  artis_deposition_model em{};
  em.struct_size = sizeof(em);
  em.nnuclides = nn, em.npts_nonempty = ncell;
  em.nuc_endecay_gamma = gamma.data(), em.nuc_endecay_particle = particle.data(), em.nuc_endecay_q = qval.data(), em.nuc_branchprob = bprob.data();
  em.assocvolume_tmin = vol.data(), em.radial_pos_tmin = radial.data();
  artis_packet_init_model m{};
  m.struct_size = sizeof(m);
  m.nuc_decay_daughters_probsum = probsum.data(), m.gamma_start = gstart.data(), m.gamma_energy = genergy.data(), m.gamma_probability = gprob.data();
  m.initenergyq = channel ? initq.data() : nullptr;
  m.tmax = 80. * 86400.;
  m.initial_packets_on = m.use_model_initial_energy = channel ? 1 : 0;
  m.uniform_pellet_energies = 1;
  void *h = pinit_host_new(&model, &d, &em, &m);
  if (!h) {
    std::printf("refused: %s\n", pinit_host_last_error());
    return 1;
  }
  std::vector<double> E((size_t)np), endecay((size_t)ncell), encum((size_t)ngrid);
  pinit_host_energy(h, E.data());
  const double etot = pinit_host_cells(h, E.data(), endecay.data(), encum.data(), 3);
  const int64_t npackets = 3000;
  std::vector<artis_packet> pk((size_t)npackets), pk1((size_t)npackets);
  std::memset((void *)pk.data(), 0, sizeof(artis_packet) * pk.size());
  std::memset((void *)pk1.data(), 0, sizeof(artis_packet) * pk1.size());
  std::vector<int32_t> ch((size_t)npackets), tr((size_t)npackets), ch1((size_t)npackets), tr1((size_t)npackets);
  std::vector<double> unit((size_t)npackets), margin((size_t)npackets);
  double scal[4], scal1[4];
  const int calls = pinit_host_run(h, npackets, 77u, pk.data(), ch.data(), tr.data(), scal, 4096, 1 << 20, unit.data(), margin.data(), 3);
  const int calls1 = pinit_host_run(h, npackets, 77u, pk1.data(), ch1.data(), tr1.data(), scal1, 1, 1 << 20, nullptr, nullptr, 2);
  int bad = calls != 1 || calls1 < 1 || std::memcmp((const void *)pk.data(), (const void *)pk1.data(), sizeof(artis_packet) * pk.size()) != 0;
  for (int64_t n = 0; n < npackets; n++) {
    bad |= prop[(size_t)pk[(size_t)n].cellindex] < 0 || prop[(size_t)pk[(size_t)n].cellindex] == 1;
    bad |= pinit_host_channel(h, prop[(size_t)pk[(size_t)n].cellindex], 0.37f, 0) != pinit_host_channel(h, prop[(size_t)pk[(size_t)n].cellindex], 0.37f, 1);
  }
  std::printf("grid %d copies %d channel %d: etot %.6e e_ratio %.17g calls %d / %d %s\n", gridtype, copies, (int)channel, etot, scal[3], calls, calls1, bad ? "BAD" : "ok");
  pinit_host_free(h);
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  for (int gridtype : {ARTIS_GRID_SPHERICAL1D, ARTIS_GRID_CYLINDRICAL2D, ARTIS_GRID_CARTESIAN3D})
    for (int copies : {1, 30})
      for (bool channel : {false, true}) bad |= run_grid(gridtype, copies, channel);
  return bad;
}
