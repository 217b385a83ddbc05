/*
 * artis_amd.h -- C-ABI of the MI355X packet-propagation engine for ARTIS.
 *
 * Drop-in boundary: the per-timestep packet update of the reference,
 *   update_packets(nts, packets)                     update_packets.cc:530
 *     -> update_packet_cellcache_group()             update_packets.cc:468
 *        -> do_packet() for TYPE_RPKT / TYPE_KPKT / TYPE_PRE_KPKT
 *                                                    update_packets.cc:257
 *           -> do_rpkt() / do_rpkt_step()            rpkt.cc:983 / rpkt.cc:542
 *           -> kpkt::do_kpkt(), do_kpkt_blackbody()  kpkt.cc:425 / kpkt.cc:399
 *           -> do_macroatom()                        macroatom.cc:360
 *     preceded by cellcacheslot_populate()           update_packets.cc:397
 * and the estimator reduction radfield::reduce_estimators() radfield.cc:988.
 *
 * Every struct below is a flat view (plain pointers and sizes) of arrays the
 * reference already owns; field names follow the reference's globals.
 * Nothing here depends on torch, HIP types or C++.
 */
#ifndef ARTIS_AMD_H
#define ARTIS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- enums: values are the reference's, they are written to packets*.out -- */
/* packet.h:38 enum packet_type */
enum {
  ARTIS_TYPE_NONE = 0,
  ARTIS_TYPE_GAMMA = 10,
  ARTIS_TYPE_RPKT = 11,
  ARTIS_TYPE_KPKT = 12,
  ARTIS_TYPE_MA = 13,
  ARTIS_TYPE_NTLEPTON_DEPOSITED = 20,
  ARTIS_TYPE_NONTHERMAL_PREDEPOSIT_BETAMINUS = 21,
  ARTIS_TYPE_NONTHERMAL_PREDEPOSIT_BETAPLUS = 22,
  ARTIS_TYPE_NONTHERMAL_PREDEPOSIT_ALPHA = 23,
  ARTIS_TYPE_NTALPHA_FISPROD_DEPOSITED = 24,
  ARTIS_TYPE_ESCAPE = 32,
  ARTIS_TYPE_RADIOACTIVE_PELLET = 100,
  ARTIS_TYPE_PRE_KPKT = 120
};

/* packet.h:85 */
#define ARTIS_EMTYPE_NOTSET (-9999000)
#define ARTIS_EMTYPE_FREEFREE (-9999999)
/* packet.h:89 enum absorption_type */
#define ARTIS_ABSTYPE_FREEFREE (-1)
#define ARTIS_ABSTYPE_BOUNDFREE (-2)
#define ARTIS_ABSTYPE_GAMMA_COMPTON (-3)
#define ARTIS_ABSTYPE_GAMMA_PHOTOELECTRIC (-4)
#define ARTIS_ABSTYPE_GAMMA_PAIRPRODUCTION (-5)
#define ARTIS_ABSTYPE_PELLET_NOGAMMASPEC (-6)
#define ARTIS_ABSTYPE_PELLET_BEFORESIMSTART (-7)
#define ARTIS_ABSTYPE_PELLET_PARTICLEDECAY (-10)

/* globals.h:21 enum ma_action */
enum {
  ARTIS_MA_ACTION_RADDEEXC = 0,
  ARTIS_MA_ACTION_COLDEEXC = 1,
  ARTIS_MA_ACTION_RADRECOMB = 2,
  ARTIS_MA_ACTION_COLRECOMB = 3,
  ARTIS_MA_ACTION_INTERNALDOWNSAME = 4,
  ARTIS_MA_ACTION_INTERNALDOWNLOWER = 5,
  ARTIS_MA_ACTION_INTERNALUPSAME = 6,
  ARTIS_MA_ACTION_INTERNALUPHIGHER = 7,
  ARTIS_MA_ACTION_INTERNALUPHIGHERNT = 8,
  ARTIS_MA_ACTION_COUNT = 9
};

/* stats.h:13 enum class Counter (same numbering) */
enum {
  ARTIS_STAT_MA_ACTIVATION_COLLEXC = 0,
  ARTIS_STAT_MA_ACTIVATION_COLLION = 1,
  ARTIS_STAT_MA_ACTIVATION_NTCOLLEXC = 2,
  ARTIS_STAT_MA_ACTIVATION_NTCOLLION = 3,
  ARTIS_STAT_MA_ACTIVATION_BB = 4,
  ARTIS_STAT_MA_ACTIVATION_BF = 5,
  ARTIS_STAT_MA_ACTIVATION_FB = 6,
  ARTIS_STAT_MA_DEACTIVATION_COLLDEEXC = 7,
  ARTIS_STAT_MA_DEACTIVATION_COLLRECOMB = 8,
  ARTIS_STAT_MA_DEACTIVATION_BB = 9,
  ARTIS_STAT_MA_DEACTIVATION_FB = 10,
  ARTIS_STAT_MA_INTERNALUPHIGHER = 11,
  ARTIS_STAT_MA_INTERNALUPHIGHERNT = 12,
  ARTIS_STAT_MA_INTERNALDOWNLOWER = 13,
  ARTIS_STAT_K_TO_MA_COLLEXC = 14,
  ARTIS_STAT_K_TO_MA_COLLION = 15,
  ARTIS_STAT_K_TO_R_FF = 16,
  ARTIS_STAT_K_TO_R_FB = 17,
  ARTIS_STAT_K_TO_R_BB = 18,
  ARTIS_STAT_K_FROM_FF = 19,
  ARTIS_STAT_K_FROM_BF = 20,
  ARTIS_STAT_NT_FROM_GAMMA = 21,
  ARTIS_STAT_NT_TO_IONISATION = 22,
  ARTIS_STAT_NT_TO_EXCITATION = 23,
  ARTIS_STAT_NT_TO_KPKT = 24,
  ARTIS_STAT_K_FROM_EARLIERDECAY = 25,
  ARTIS_STAT_INTERACTIONS = 26,
  ARTIS_STAT_ELECTRON_SCATTERINGS = 27,
  ARTIS_STAT_RESONANCESCATTERINGS = 28,
  ARTIS_STAT_CELLCROSSINGS = 29,
  ARTIS_STAT_UPSCATTER = 30,
  ARTIS_STAT_DOWNSCATTER = 31,
  ARTIS_STAT_UPDATECELL = 32,
  ARTIS_STAT_PKTESCAPES = 33,
  ARTIS_STAT_COUNT = 34,
  /* extra slots, not in the reference: the unit of the headline metric */
  ARTIS_STAT_X_RPKT_STEPS = 34, /* calls of do_rpkt_step() rpkt.cc:542 */
  ARTIS_STAT_X_KPKT_STEPS = 35, /* calls of do_kpkt()/do_kpkt_blackbody() */
  ARTIS_STAT_X_LINES_VISITED = 36, /* lines walked in get_possible_event() rpkt.cc:121 */
  ARTIS_STAT_X_MA_JUMPS = 37, /* iterations of the do_macroatom() loop macroatom.cc:385 */
  ARTIS_STAT_X_CHI_EVALS = 38, /* continuum opacity evaluations that missed the packet's cache, rpkt.cc:1029 */
  ARTIS_STAT_X_CONT_VISITED = 39, /* bound-free continua summed in calculate_chi_bf_gammacontr() rpkt.cc:808 */
  ARTIS_STAT_X_GAMMA_STEPS = 40, /* calls of gammapkt::do_gamma() gammapkt.cc:911 */
  /* virtual packets (vpkt.h:34-37): nvpkt_created, nvpkt_esc_from_rpkt / _kpkt / _macroatom */
  ARTIS_STAT_X_VPKT_CREATED = 48, ARTIS_STAT_X_VPKT_ESC_RPKT = 49, ARTIS_STAT_X_VPKT_ESC_KPKT = 50, ARTIS_STAT_X_VPKT_ESC_MA = 51,
  /* 41 (do_kpkt's third phase clock), 42..47 and 52..63: free for profiling builds (-DARTIS_PROFILE / -DARTIS_PROFILE_MA: wave-cycle accounting; the
   * do_rpkt_step() phase clocks also take 48..52, so a profiling build of a VPKT_ON preset is refused at compile time) */
  ARTIS_NSTATS = 64
};

/* constants.h:73 GridType */
enum { ARTIS_GRID_SPHERICAL1D = 0, ARTIS_GRID_CYLINDRICAL2D = 1, ARTIS_GRID_CARTESIAN3D = 2 };
/* grid.h:29 CellThickness */
enum { ARTIS_CELL_THIN = 0, ARTIS_CELL_THICK = 1, ARTIS_CELL_THICK_VPKT_ONLY = 2 };
/* kpkt.cc:42 CoolingType */
enum { ARTIS_COOLING_FREEFREE = 0, ARTIS_COOLING_FREEBOUND = 1, ARTIS_COOLING_COLLEXC = 2, ARTIS_COOLING_COLLION = 3 };

/* ---- packet: layout of the reference's struct Packet in its GPU_ON form --- */
/* packet.h:117-169 (rngstate first: packet.h:118-122). Field order and types
 * are the reference's so a reference-side Packet* can be passed unchanged. */
typedef struct artis_packet {
  uint32_t rngstate[4]; /* Xoshiro128PP state, random.h:101 */
  double prop_time;
  double pos[3];
  double dir[3];
  double nu_cmf;
  double e_cmf;
  double nu_rf;
  double e_rf;
  int32_t next_trans;
  int32_t nscatterings;
  int32_t emissiontype;
  double em_pos[3];
  float em_time;
  int32_t absorptiontype;
  double absorptionfreq;
  double stokes_q;
  double stokes_u;
  int32_t trueemissiontype;
  double trueem_pos[3];
  float trueem_time;
  int32_t type;
  int32_t cellindex;
  int32_t escape_type;
  float escape_time;
  double tdecay;
  int32_t number;
  uint8_t originated_from_particlenotgamma;
  int32_t pellet_decaytype;
  int32_t pellet_nucindex;
} artis_packet;

/* ---- static model: atomic data + propagation grid (set once per run) ------ */
typedef struct artis_model {
  /* sizes */
  int32_t nelements;
  int32_t nions;      /* get_includedions() atomic.h:391 */
  int32_t nlevels;    /* get_includedlevels() atomic.h:37 */
  int32_t nlines;     /* globals::nlines */
  int32_t nalltrans;  /* size of globals::alltrans arrays */
  int32_t nphixstargets_total; /* size of globals::allphixstargets_* */
  int32_t nphixslevels;        /* number of levels with a phixs table */
  int32_t nbfcontinua;         /* globals::nbfcontinua */
  int32_t nbfcontinua_ground;  /* globals::nbfcontinua_ground */
  int32_t ncoolingterms;       /* kpkt ncoolingterms kpkt.cc:233 */
  int32_t nmatransblock;       /* sum over levels of 2*ndowntrans+nuptrans input.cc:1542 */
  int32_t NPHIXSPOINTS;        /* globals::NPHIXSPOINTS */
  double NPHIXSNUINCREMENT;    /* globals::NPHIXSNUINCREMENT */

  /* per element (globals::elements, globals.h:60) */
  const int32_t *elem_nions;
  const int32_t *elem_uniqueionindexstart;
  const int32_t *elem_anumber;
  const int32_t *elem_lowest_ionstage;

  /* per ion, indexed by uniqueionindex (struct Ion, globals.h:45) */
  const int32_t *ion_element;
  const int32_t *ion_nlevels;
  const int32_t *ion_nlevels_ionising;
  const int32_t *ion_maxrecombininglevel;
  const int32_t *ion_uniquelevelindexstart;
  const int32_t *ion_coolingoffset;
  const int32_t *ion_ncoolingterms;

  /* per level, indexed by uniquelevelindex (struct AllLevels, globals.h:181) */
  const double *level_epsilon;
  const float *level_statweight;
  const int32_t *level_alltrans_startdown;
  const int32_t *level_ndowntrans;
  const int32_t *level_nuptrans;
  const int32_t *level_closestgroundlevelcont;
  const int32_t *level_phixsstart;
  const int32_t *level_nphixstargets;
  const int32_t *level_phixstargetstart;
  const int32_t *level_bflist_start;
  const int32_t *level_matransblock_start;

  /* globals::alltrans (struct AllTransitions, globals.h:151) */
  const int32_t *alltrans_lineindex;
  const int32_t *alltrans_targetlevelindex;
  const float *alltrans_einstein_A;
  const float *alltrans_coll_str;
  const float *alltrans_osc_strength;
  const uint8_t *alltrans_forbidden;

  /* globals::linelist (struct TransitionLines, globals.h:229), descending nu */
  const double *line_nu;
  const int32_t *line_elementindex;
  const int32_t *line_ionindex;
  const int32_t *line_uniquelevelindex_lower;
  const int32_t *line_uniquelevelindex_upper;
  const float *line_B_ul;
  const float *line_B_lu;

  /* photoionisation */
  const float *allphixs;                       /* [nphixslevels*NPHIXSPOINTS] globals.h:149 */
  const int32_t *allphixstargets_levelindex;   /* globals.h:173 */
  const double *allphixstargets_probability;   /* globals.h:174 */

  /* globals::allcont (struct AllCont, globals.h:253), ascending nu_edge */
  const double *allcont_nu_edge;
  const int32_t *allcont_element;
  const int32_t *allcont_ion;
  const int32_t *allcont_level;
  const int32_t *allcont_phixstargetindex;
  const int32_t *allcont_upperlevel;
  const int32_t *allcont_uniquelevelindex;
  const double *allcont_probability;
  const int32_t *allcont_groundcontestimindex;

  /* ground-level continua, ascending nu_edge (globals.h:272-274) */
  const double *groundcont_nu_edge;

  /* temperature LUTs, [nbfcontinua*TABLESIZE], index get_bflutindex() ratecoeff.cc:123 */
  const double *spontrecombcoeffs;
  const double *corrphotoioncoeffs;
  const double *bfcooling_coeffs;

  /* cooling list (kpkt.cc:44-46) */
  /* (the entries of an ion after its collisional excitations must be in the order calculate_cooling_rates_ion() writes them -- kpkt.cc:122-190,
   * i.e. as setup_coolinglist() lays them out: artis_amd_engine_create() checks it and refuses a list that is not, ARTIS_ERR_ARG) */
  const uint8_t *coolinglist_type;
  const int32_t *coolinglist_level;
  const int32_t *coolinglist_phixstargetindex;

  /* propagation grid (grid.cc) */
  int32_t gridtype;       /* ARTIS_GRID_* */
  int32_t ncoordgrid[3];  /* grid.cc ncoordgrid */
  int32_t ngrid;          /* grid::ngrid */
  int32_t npts_nonempty;  /* grid::get_nonempty_npts_model() */
  double tmin;            /* globals::tmin */
  double vmax;            /* globals::vmax */
  double rmax;            /* globals::rmax */
  const double *coord_pos_min_tmin[3]; /* grid.cc coord_pos_min_tmin */
  const int32_t *propcell_nonemptymgi; /* [ngrid] grid::get_propcell_nonemptymgi(), -1 = empty */

  /* static inputs of the non-thermal channels, required by builds with ARTIS_OPT_NT_ON (else may be NULL):
   * [nelements] globals::elements[].initstablemeannucmass (grid.cc:1515, USE_CALCULATED_MEANATOMICWEIGHT off) and
   * [nions] nonthermal get_sum_q_over_binding_energy(element, ion) (nonthermal.cc:553; from the host's binding-energy data) */
  const float *elem_meannucmass;
  const double *ion_nt_sum_q_over_binding;

  /* whole-ejecta scalars of the Barnes thermalisation efficiency (update_packets.cc:69-77): grid::get_ejecta_kinetic_energy()
   * (grid.h:139) and grid::mtot_input (grid.h:40). Read only by builds with that scheme; 0 elsewhere. */
  double ejecta_kinetic_energy;
  double mtot_input;

  /* [nbfcontinua] globals::allcont.bfestimindex (input.cc:932-947): index of the continuum's detailed bound-free estimator,
   * -1 where LEVEL_HAS_BFEST() is false; nbfestim = number of estimators (globals::bfestim_nu_edge.size()). NULL / 0: every
   * continuum has one (artisoptions_nltenebular.h:82), the estimator index is the continuum index. */
  const int32_t *allcont_bfestimindex;
  int32_t nbfestim;

  /* [npts_nonempty] grid::get_rho_tmin(mgi): the density at tmin, read by the Wollaeger and Guttman gamma-ray
   * thermalisation schemes (gammapkt.cc:819, :853) for the column density along a ray; NULL elsewhere */
  const float *rho_tmin;

  /* XCOM photoionisation cross sections (gammapkt.cc:244-261 photoion_data, read from xcom_photoion_data.txt), per element
   * of the model: element e has the points [xcom_elem_start[e], xcom_elem_start[e+1]) of xcom_energy [MeV, rising] and
   * xcom_sigma [cm^2]; an element beyond the table or without data has none. Builds with USE_XCOM_GAMMAPHOTOION (which also
   * read elem_meannucmass for the element number densities); NULL elsewhere. */
  const int32_t *xcom_elem_start; /* [nelements + 1] */
  const double *xcom_energy;
  const double *xcom_sigma;

  /* [detailed_linecount] radfield.cc detailed_lineindices: the lines with their own intensity estimator, rising line index
   * (builds with DETAILED_LINE_ESTIMATORS_ON; NULL / 0 elsewhere) */
  const int32_t *detailed_lineindices;
  int32_t detailed_linecount;

  /* ---- virtual packets (builds with VPKT_ON): what read_vpktparameterfile() (vpkt.cc:673) leaves of vpkt.txt; 0 / NULL
   * elsewhere (ABI 5). Observer directions (costheta, phi); the opacity choices of every spectrum (vpkt.cc:79: 0 full, -1 no
   * lines, -2 no bound-free, -3 no free-free, -4 no electron scattering, Z > 0 without that element's lines); the arrival
   * time window and the frequency ranges in which a virtual packet is traced at all; the optical depth at which it is
   * dropped; the optional velocity-grid map (time window, frequency ranges); globals::nprocs (vpkt.cc:130). */
  int32_t vpkt_nobsdirections;
  const double *vpkt_obsdirs_costheta; /* [vpkt_nobsdirections] */
  const double *vpkt_obsdirs_phi;
  int32_t vpkt_nspectraperobsdir;
  const int32_t *vpkt_opacityexclusions; /* [vpkt_nspectraperobsdir] */
  double vpkt_timemin_input, vpkt_timemax_input;
  int32_t vpkt_nwavelengthranges;
  const double *vpkt_numin_input; /* [vpkt_nwavelengthranges] */
  const double *vpkt_numax_input;
  double vpkt_tau_max;
  int32_t vpkt_vgrid_on;
  double vpkt_tmin_grid, vpkt_tmax_grid;
  int32_t vpkt_grid_nwavelengthranges;
  const double *vpkt_nu_grid_min; /* [vpkt_grid_nwavelengthranges] */
  const double *vpkt_nu_grid_max;
  int32_t vpkt_nprocs;
} artis_model;
/* the fixed grids of the virtual-packet spectra, vpkt.h:21-32 */
#define ARTIS_VGRID_NY 50
#define ARTIS_VGRID_NZ 50
#define ARTIS_VSPEC_NUBINS 2500
#define ARTIS_VSPEC_TIMEBINS 5
#define ARTIS_VSPEC_NUMIN (2.99792458e+10 / 10000 * 1e8)
#define ARTIS_VSPEC_NUMAX (2.99792458e+10 / 3500 * 1e8)
#define ARTIS_VSPEC_TIMEMIN (3 * 86400.)
#define ARTIS_VSPEC_TIMEMAX (8 * 86400.)

/* ---- per-timestep cell state written by the reference's update_grid() ----- */
typedef struct artis_cellstate {
  /* [npts_nonempty], grid.h:19-37 */
  const float *rho;
  const float *Te;
  const float *TJ;
  const float *TR;
  const float *W;
  const float *nne;
  const float *nnetot;
  const float *kappagrey;
  const int32_t *thick;
  const float *clumpfactor;
  /* [npts_nonempty*nions] grid.h:44-45 */
  const float *ion_groundlevelpops;
  const float *ion_partfuncts;
  /* [npts_nonempty*nelements] grid.h:42 */
  const float *elem_massfracs;
  /* [npts_nonempty*nbfcontinua_ground] globals.h:126 */
  const double *corrphotoionrenorm;
  /* [npts_nonempty] grid::get_ffegrp(mgi): iron-group mass fraction, read by the gamma-ray opacities
   * (gammapkt.cc:416, :516). May be NULL when no TYPE_GAMMA packet is handed over (treated as 0). */
  const float *ffegrp;
  /* [npts_nonempty*nlevels] level populations from the host's NLTE / LTE solution (ltepop.cc:169-180 get_levelpop); NULL:
   * the engine evaluates the LTE populations itself (calculate_levelpop_lte ltepop.cc:395) */
  const double *levelpops;
  /* [npts_nonempty*nphixstargets_total] corrected photoionisation coefficient of every bound-free pair, what
   * get_corrphotoioncoeff() (ratecoeff.cc:840) returns when USE_LUT_PHOTOION is off (the normalised bound-free estimators of
   * the previous timestep, or the radiation-field integral): required by builds with ARTIS_OPT_USE_LUT_PHOTOION == 0 */
  const double *corrphotoioncoeff;
  /* [npts_nonempty*RADFIELDBINCOUNT] W and T_R of the multibin radiation field (radfield.cc:208-214; W < 0: bin without a
   * solution): required by builds with ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON */
  const float *radfieldbin_W;
  const float *radfieldbin_T_R;
  /* Solution of the host's Spencer-Fano solver, read by the non-thermal channels of do_ntlepton_deposit() and of the
   * macro-atom (nonthermal.cc:215-250): required by builds with ARTIS_OPT_NT_ON.
   *   nt_frac_ionisation / nt_frac_excitation [npts_nonempty]  NonThermalCellSolution::frac_ionisation / frac_excitation
   *   nt_deposition_rate_density [npts_nonempty]               ntlepton_deposition_rate_density_all_cells
   *   nt_eff_ionpot [npts_nonempty*nions]                      NonThermalSolutionIon::eff_ionpot
   *   nt_prob_num_auger, nt_ionenfrac_num_auger [npts_nonempty*nions*(NT_MAX_AUGER_ELECTRONS+1)]
   *   nt_exc_count [npts_nonempty]                             NonThermalCellSolution::frac_excitations_list_size
   *   nt_exc_* [npts_nonempty*nt_excitations_stored]           the cell's NonThermalExcitation list, ascending alltransindex */
  const float *nt_frac_ionisation;
  const float *nt_frac_excitation;
  const double *nt_deposition_rate_density;
  const float *nt_eff_ionpot;
  const float *nt_prob_num_auger;
  const float *nt_ionenfrac_num_auger;
  const int32_t *nt_exc_count;
  const double *nt_exc_frac_deposition;
  const double *nt_exc_ratecoeffperdeposition;
  const int32_t *nt_exc_alltransindex;
  int32_t nt_excitations_stored; /* nonthermal.cc nt_excitations_stored: stride of the nt_exc_* lists */
  /* [npts_nonempty*ARTIS_EXPOPAC_NBINS] what calculate_expansion_opacities() (rpkt.cc:1071, called from update_grid.cc:655)
   * leaves per cell: the binned line opacity kappa [cm^2/g] (read by builds with RPKT_USE_EXPANSION_OPACITIES) and the
   * running integral of kappa * B_nu(T_e) over the bins (read with RPKT_BOUNDBOUND_THERMALISATION_PROBABILITY).
   * Both NULL: the engine calculates them itself when it populates the cell cache. */
  const float *expansionopacities;
  const double *expansionopacity_planck_cumulative;
  /* [npts_nonempty*detailed_linecount] radfield.cc prev_Jb_lu_normed[].value: the normalised line intensities of the previous
   * timestep, what get_Jb_lu() returns (builds with DETAILED_LINE_ESTIMATORS_ON) */
  const double *Jb_lu_normed;
  /* [npts_nonempty*nelements] grid::elem_meanweight_allcells (grid.cc:1509): the mean atomic weight [g] of each element in
   * each cell; read for the element number densities (XCOM photoelectric opacities, non-thermal channels) by builds with
   * USE_CALCULATED_MEANATOMICWEIGHT (kilonova_lte and its variants); NULL elsewhere (ABI 4) */
  const float *elem_meanweight;
} artis_cellstate;

typedef struct artis_timestep {
  int32_t nts;          /* timestep number */
  double start;         /* globals::timesteps[nts].start */
  double width;         /* globals::timesteps[nts].width */
  double mid;           /* globals::timesteps[nts].mid */
  double max_path_step; /* globals::max_path_step update_grid.cc:753 */
} artis_timestep;

/* ---- estimators: accumulated into, never zeroed, by update_packets -------- */
typedef struct artis_estimators {
  double *J;                   /* [npts_nonempty] radfield.cc J */
  double *nuJ;                 /* [npts_nonempty] radfield.cc nuJ */
  double *ffheatingestimator;  /* [npts_nonempty] globals.h:133 */
  double *colheatingestimator; /* [npts_nonempty] globals.h:134 */
  double *gammaestimator;      /* [npts_nonempty*nbfcontinua_ground] globals.h:128 */
  double *bfheatingestimator;  /* [npts_nonempty*nbfcontinua_ground] globals.h:131 */
  int64_t *stats;              /* [ARTIS_NSTATS] stats.cc event counters */
  double *dep_estimator_gamma; /* [npts_nonempty] globals::dep_estimator_gamma (gammapkt.cc:568); may be NULL */
  double *scalars;             /* [ARTIS_NSCALARS] per-timestep sums, see ARTIS_SCALAR_*; may be NULL */
  /* [npts_nonempty] globals::dep_estimator_electron / _positron / _alpha (update_packets.cc:160-173); may be NULL */
  double *dep_estimator_electron;
  double *dep_estimator_positron;
  double *dep_estimator_alpha;
  /* multibin radiation field estimators radfieldbins.J_raw / nuJ_raw [npts_nonempty*RADFIELDBINCOUNT] (radfield.cc:745-790)
   * and detailed bound-free estimators bfrate_raw [npts_nonempty*nbfestim] (radfield.cc:215; nbfestim = nbfcontinua unless
   * artis_model.allcont_bfestimindex selects a subset). Written by builds with the corresponding options; may be NULL. */
  double *radfieldbin_J;
  double *radfieldbin_nuJ;
  double *bfrate_raw;
  /* detailed line estimators Jb_lu_raw[][].value and .contribcount [npts_nonempty*detailed_linecount] (radfield.cc:773
   * update_lineestimator). Builds with DETAILED_LINE_ESTIMATORS_ON; may be NULL. */
  double *Jb_lu_raw;
  int64_t *Jb_lu_contribcount;
  /* virtual-packet spectra vspecpol[timebin][obsdir * nspectraperobsdir + opacity choice].flux[nubin].{I, Q, U}
   * (vpkt.cc:56, add_to_vspecpol :116): [ARTIS_VSPEC_TIMEBINS][nobsdirections*nspectraperobsdir][ARTIS_VSPEC_NUBINS][3], and the
   * velocity-grid map vgrid[ny][nz].flux[wlbin][obsdir].{I, Q, U} (:138): [ARTIS_VGRID_NY][ARTIS_VGRID_NZ][grid_nwavelengthranges]
   * [nobsdirections][3]. Builds with VPKT_ON; may be NULL (ABI 5). The counters nvpkt_created / nvpkt_esc_from_* are
   * stats[ARTIS_STAT_X_VPKT_*]. */
  double *vspecpol;
  double *vgrid_flux;
} artis_estimators;
enum {
  ARTIS_SCALAR_GAMMA_DEP_DISCRETE = 0,   /* globals::timesteps[nts].gamma_dep_discrete gammapkt.cc:926 */
  ARTIS_SCALAR_NT_ENERGY_DEPOSITED = 1,  /* nonthermal.cc nt_energy_deposited (:2524, :2530) */
  /* globals::timesteps[nts].* written by update_pellet() (update_packets.cc:199-231) ... */
  ARTIS_SCALAR_PELLET_DECAYS = 2,
  ARTIS_SCALAR_GAMMA_EMISSION = 3,
  ARTIS_SCALAR_POSITRON_EMISSION = 4,
  ARTIS_SCALAR_ELECTRON_EMISSION = 5,
  ARTIS_SCALAR_ALPHA_EMISSION = 6,
  ARTIS_SCALAR_SPFISSION_DEP_DISCRETE = 7,
  /* ... and by do_nonthermal_predeposit() (update_packets.cc:162-172) */
  ARTIS_SCALAR_ELECTRON_DEP_DISCRETE = 8,
  ARTIS_SCALAR_POSITRON_DEP_DISCRETE = 9,
  ARTIS_SCALAR_ALPHA_DEP_DISCRETE = 10,
  ARTIS_NSCALARS = 11
};
/* decay::DecayType values read from Packet::pellet_decaytype (decay.h:21-26) */
enum { ARTIS_DECAYTYPE_ALPHA = 0, ARTIS_DECAYTYPE_ELECTRONCAPTURE = 1, ARTIS_DECAYTYPE_BETAPLUS = 2, ARTIS_DECAYTYPE_BETAMINUS = 3,
       ARTIS_DECAYTYPE_NONE = 4, ARTIS_DECAYTYPE_SPONTFISSION = 5 };

/* ---- engine ---------------------------------------------------------------- */
typedef struct artis_amd_engine artis_amd_engine;

/* All functions return 0 on success, a negative ARTIS_ERR_* otherwise;
 * artis_amd_last_error() gives the message. No function falls back to a CPU
 * path: without a usable HIP device artis_amd_engine_create() fails. */
#define ARTIS_OK 0
#define ARTIS_ERR_NODEVICE (-1)
#define ARTIS_ERR_HIP (-2)
#define ARTIS_ERR_ARG (-3)
#define ARTIS_ERR_UNSUPPORTED (-4)
#define ARTIS_ERR_NOTCONVERGED (-5)
#define ARTIS_ERR_RCCL (-6)

const char *artis_amd_last_error(void);
/* 6 -- and it stays 6 with the photoionisation coefficients (artis_photoion_params, artis_photoion_result, artis_amd_set_cellstate_photoion and
 * artis_amd_photoion_download): additive; artis_amd_set_cellstate is unchanged.
 * It stayed 6 with the deposition rates and thickness flags (artis_deposition_model, artis_deposition_params, artis_deposition_result and
 * the five functions artis_amd_deposition_setup / _update / _download / _devptr and artis_amd_grid_update_deposited): additive again.
 * It stayed 6 with the decay and abundance update (artis_decay_model, artis_decay_coeffs, artis_decay_result and the four functions
 * artis_amd_decay_setup / _update / _download and artis_amd_grid_update_decayed): new functions and new structs only, no existing one changed.
 * It stayed 6 with the engine configuration (artis_amd_config, artis_amd_plan and their four functions below): functions were added,
 * no existing struct or function changed, so a caller built against the earlier header of version 6 runs unchanged.
 * 6: artis_amd_record_tiers() added (no struct changed); 5: virtual-packet configuration and spectra appended;
 * 4: artis_cellstate.elem_meanweight appended (3: cell state and estimators of the nltenebular options) */
int artis_amd_abi_version(void);
/* Name of the options preset the library was compiled with (include/artis_options.h): "classic" or "kilonova_lte".
 * Like the reference, one binary per artisoptions.h. */
const char *artis_amd_options_preset(void);
size_t artis_amd_sizeof_packet(void);

/* Create an engine on HIP device `device` and upload the static model.
 * Replaces the table set-up the reference's GPU build leaves in unified memory
 * (MPI_shared_array, mpi_logging.h). The same as artis_amd_engine_create_ex() with a default configuration. */
int artis_amd_engine_create(const artis_model *model, int device, artis_amd_engine **out);

/* ---- engine configuration ----------------------------------------------------
 * How an engine uses its device: what input.txt and artisoptions.h are to the reference (input.cc:1862, constants.h:105-107), stated by the host
 * per engine instead of per process. PRECEDENCE, for every field: a value set here wins; a field left at its "automatic / default" value takes
 * the ARTIS_AMD_* variable named with it if that is set; otherwise the built-in default. None of it changes a packet history: the fields
 * place work and memory, never physics.
 * The kernel forms, sorts and chunkings that the other ARTIS_AMD_* variables select are experiment switches and stay variables. */
typedef struct artis_amd_config {
  size_t  struct_size;          /* sizeof(artis_amd_config) of the caller. Larger than the library's: refused. Smaller (an older caller): accepted,
                                   the fields beyond it take their defaults */
  int64_t cache_budget_bytes;   /* bytes the cell-cache rows may take; 0 = automatic: 80 % of the free device memory at creation less the
                                   population scratch and the head-room (ARTIS_AMD_CACHE_BUDGET_MB). Set: the layout no longer depends on what
                                   else is on the device. It must hold one row */
  int64_t cache_headroom_bytes; /* taken off the free memory before the automatic rule: what is allocated later (packets, a second engine);
                                   -1 = default, 0 (ARTIS_AMD_CACHE_HEADROOM_MB) */
  int64_t pop_scratch_bytes;    /* scratch of the cell-cache population; -1 = default, 2 GB (ARTIS_AMD_POP_SCRATCH_MB) */
  double  ma_hot_fraction;      /* share of every ion's levels (the lowest ones) with a static macro-atom record in every row, in (0, 1];
                                   < 0 = automatic: 1 when the cache fits, else the share that needs the fewest tiles (ARTIS_AMD_MA_HOTFRAC) */
  double  ma_pool_fraction;     /* the shared pool of on-demand records as a share of what all cold levels' records would take, >= 0 (above 1
                                   counts as 1); -1 = default, 0.15 (ARTIS_AMD_MA_POOLFRAC) */
  int64_t tail_threshold;       /* packets left at which the tail kernel takes over; 0 = never; -1 = default, 4096 (16384 in builds with
                                   detailed bound-free estimators) (ARTIS_AMD_TAIL). VPKT_ON builds never use the tail kernel: always 0 */
  int64_t tile_park_at;         /* tiled cache: packets left of a larger visit at which the visit parks them for the tile's next visit;
                                   -1 = default, 3145728 (ARTIS_AMD_TILE_PARK_AT) */
  int32_t keep_line_dpop;       /* the rows' per-line population factors: -1 = automatic (dropped when the cache does not fit one tile with them
                                   and needs fewer without), 0 = drop them, 1 = keep them, or fail if the budget cannot hold a row that has
                                   them (ARTIS_AMD_DPOP) */
  int32_t reserved;             /* must be 0 */
} artis_amd_config;
size_t artis_amd_sizeof_config(void);
/* Every field "automatic / default", struct_size filled in. */
void artis_amd_config_default(artis_amd_config *cfg);
/* artis_amd_engine_create() with a configuration (NULL: the default one). The configuration is checked before the device is touched:
 * ARTIS_ERR_ARG for a struct_size larger than the library's, reserved != 0, a hot fraction of 0 or above 1, a negative pool fraction other
 * than -1, any other negative value that is not the field's default, a cache_budget_bytes that cannot hold one row, keep_line_dpop == 1
 * with a budget that cannot hold a row with line_dpop; ARTIS_ERR_UNSUPPORTED for a VPKT_ON build whose cache would be tiled. On any
 * failure *out is NULL and nothing stays allocated. */
int artis_amd_engine_create_ex(const artis_model *model, int device, const artis_amd_config *cfg, artis_amd_engine **out);
/* The values the engine runs with, every "automatic" resolved: the budget the rows were sized by, the hot and pool shares of
 * artis_amd_record_tiers(), keep_line_dpop 0 or 1, ... effective->struct_size is the caller's (artis_amd_config_default() fills it in). */
int artis_amd_engine_config(artis_amd_engine *eng, artis_amd_config *effective);

/* The layout artis_amd_engine_create_ex() would choose for this model and configuration, without building it: the same sizing code, no
 * cache, pool or scratch allocated, nothing uploaded. free_bytes = 0 asks the device (hipMemGetInfo) and is what creation would see at
 * this moment; free_bytes > 0 is taken instead and the device is not touched. With cache_budget_bytes set and free_bytes given the plan is a
 * pure function of the model and the configuration: a layout that can be reproduced on a shared device. An engine created from the same
 * configuration right afterwards reports the same numbers through artis_amd_cache_tiles(), artis_amd_record_tiers() and
 * artis_amd_engine_config(). (Under the automatic budget the plan takes the model's arrays off the free memory as the sum of their sizes;
 * creation measures again after uploading them, allocation granularity included.) Errors as artis_amd_engine_create_ex(). */
typedef struct artis_amd_plan {
  size_t  struct_size;         /* sizeof(artis_amd_plan) of the caller, set before the call (rule as artis_amd_config.struct_size) */
  int64_t bytes_per_cell;      /* cache row */
  int64_t cells_resident;      /* rows per tile */
  int32_t ntiles;
  int32_t ncold_levels;
  double  hot_fraction;
  int64_t pool_slots;          /* 16-byte slots of the shared pool per resident cell */
  int64_t cache_bytes, pool_bytes, pop_scratch_bytes, model_bytes; /* what creation would allocate: all rows (the pool's part of them),
                                                                      the population scratch, the model's tables */
  int64_t free_bytes_assumed;  /* the free memory the automatic rules used: hipMemGetInfo, or the caller's */
  int32_t line_dpop_kept;
  int32_t reserved;
} artis_amd_plan;
size_t artis_amd_sizeof_plan(void);
int artis_amd_engine_plan(const artis_model *model, int device, const artis_amd_config *cfg, int64_t free_bytes, artis_amd_plan *plan);

void artis_amd_engine_destroy(artis_amd_engine *eng);

/* Upload the cell state of the coming timestep and fill every cell's cache:
 * cellcacheslot_populate() for all non-empty cells (update_packets.cc:397,
 * multi-slot form update_packets.cc:551-560) and the per-ion cumulative
 * cooling of kpkt::calculate_cooling_rates() (kpkt.cc:281). */
int artis_amd_set_cellstate(artis_amd_engine *eng, const artis_cellstate *cells, const artis_timestep *ts);

/* Re-run the cell-cache population for the cell state already uploaded (what update_packets() of the
 * reference does at its start, update_packets.cc:551-560). hip_stream is a hipStream_t (NULL = default). */
int artis_amd_populate_cellcache(artis_amd_engine *eng, void *hip_stream);

/* Cell-cache tiling. The cache of every non-empty cell is resident when it fits the budget (artis_amd_config.cache_budget_bytes, or
 * 80 % of the free HBM at engine creation less scratch and head-room); otherwise there are rows for `*cells_per_tile` cells at a time
 * (`*ntiles` = how many such sets cover the model) and artis_amd_update_packets*() visits sets of cells (make the cells in
 * which most packets wait resident -- cells that are resident already keep their rows --, advance the packets that sit in
 * them until they leave the set or are done, next set, ... until no packet is left): the reference's single-slot cell cache
 * (update_packets.cc:397-460, :551-621) with a set of cells instead of one cell. With a cache that does not fit the engine also
 * chooses macro-atom record tiers that need few tiles (artis_amd_record_tiers). Packet histories do not depend on any of it. */
int artis_amd_cache_tiles(artis_amd_engine *eng, int32_t *ntiles, int64_t *cells_per_tile, int64_t *bytes_per_cell);

/* Host-buffer form of update_packets() (update_packets.cc:530): every packet
 * whose type is in do_packet()'s switch (update_packets.cc:257: pellets, gamma
 * packets, non-thermal pre-deposits and deposits, r-, k- and pre-k-packets) is
 * advanced to the end of the timestep with the physics of the classic preset
 * (include/artis_options.h); packets of any other type are returned untouched.
 * Estimators are ADDED to est (host arrays; NULL members are skipped). */
int artis_amd_update_packets(artis_amd_engine *eng, artis_packet *packets, int64_t npackets,
                             artis_estimators *est);

/* Device-resident form, for callers that keep packets in HBM across timesteps:
 * upload once, step many times, download when needed. */
int artis_amd_packets_upload(artis_amd_engine *eng, const artis_packet *packets, int64_t npackets);
int artis_amd_packets_download(artis_amd_engine *eng, artis_packet *packets, int64_t npackets);
int artis_amd_packets_snapshot(artis_amd_engine *eng); /* save current device packets */
int artis_amd_packets_restore(artis_amd_engine *eng);  /* restore the snapshot */
/* Propagate the resident packets through the timestep set by
 * artis_amd_set_cellstate(). hip_stream is a hipStream_t (NULL = default). */
int artis_amd_update_packets_device(artis_amd_engine *eng, void *hip_stream);
int artis_amd_estimators_zero(artis_amd_engine *eng, void *hip_stream);
int artis_amd_estimators_download(artis_amd_engine *eng, artis_estimators *est_add_into);

/* Device pointers of the estimator block for an in-place RCCL all-reduce
 * (the reference's radfield::reduce_estimators(), radfield.cc:988, and the
 * MPI_Allreduce of the heating/gamma estimators in sn3d.cc). The block is one
 * contiguous array of `*ndoubles` doubles. */
int artis_amd_estimators_devptr(artis_amd_engine *eng, void **dptr, int64_t *ndoubles);

/* The estimator reduction at the end of a timestep in the host layer: ONE in-place RCCL all-reduce (sum, f64) of the
 * whole estimator block over the ranks' GPUs, enqueued on hip_stream. Replaces radfield::reduce_estimators()
 * (radfield.cc:988) and the MPI_Allreduce calls on the heating / photoionisation estimators in the timestep loop
 * (sn3d.cc:565-590). nccl_comm is the caller's ncclComm_t, or NULL to use the communicator made by
 * artis_amd_comm_init(). RCCL is bound at run time (the librccl already in the process, else ROCm's). */
#define ARTIS_AMD_COMM_ID_BYTES 128 /* sizeof(ncclUniqueId) */
int artis_amd_allreduce_estimators(artis_amd_engine *eng, void *nccl_comm, void *hip_stream);
/* Communicator set-up for hosts that do not hold an ncclComm_t yet: rank 0 draws an id (ncclGetUniqueId) and hands its
 * 128 bytes to the other ranks by whatever the host already has (MPI_Bcast in the reference, globals::my_rank /
 * nprocs); every rank then calls artis_amd_comm_init (ncclCommInitRank on the engine's device; collective). The
 * engine owns the communicator and destroys it with itself. */
int artis_amd_comm_unique_id(void *id_out /* ARTIS_AMD_COMM_ID_BYTES */);
int artis_amd_comm_init(artis_amd_engine *eng, int nranks, int rank, const void *id_bytes);
/* Number of ranks RCCL itself reports for the communicator (ncclCommCount): what the reduce really spans. */
int artis_amd_comm_count(artis_amd_engine *eng, void *nccl_comm, int *nranks);

/* Timing of the dominant kernel inside the last artis_amd_update_packets_device
 * call, measured with HIP events on the launch stream. */
int artis_amd_last_kernel_ms(artis_amd_engine *eng, double *propagate_ms, int64_t *nlaunches);
/* Tiled cell cache (artis_amd_cache_tiles): sweeps over the tiles made by the last artis_amd_update_packets_device call, tile
 * fills inside it with their summed duration [ms], and the packets listed over all (sweep, tile) visits. */
int artis_amd_last_tiling(artis_amd_engine *eng, int64_t *sweeps, int64_t *tile_fills, double *fill_ms, int64_t *listed);
/* ... of which sparse fills (only the cells of the tile in which packets waited), and the cells populated over all fills */
int artis_amd_last_tiling_fills(artis_amd_engine *eng, int64_t *sparse_fills, int64_t *cells_filled);
/* ... and the packets that a visit of a tile left waiting in it for the tile's next visit instead of running them to their end in a
 * launch of their own (round 4: the last <= ARTIS_AMD_TAIL packets of a visit that began larger; ARTIS_AMD_TILE_PARK=0 switches it off) */
int artis_amd_last_tiling_parked(artis_amd_engine *eng, int64_t *parked);
/* On-demand macro-atom records (rows that hold static records for the lowest levels of every ion only: DESIGN.md section 2): how often the last
 * artis_amd_update_packets_device call found the shared pool of the other levels' records used up and emptied it (the records are filled again
 * when next needed: it costs fills, never an answer; the reference, which fills a level's rates on first use too, keeps them all: macroatom.cc:398-417) */
int artis_amd_last_pool_resets(artis_amd_engine *eng, int64_t *resets);
/* Which record tiers the engine keeps for this model (chosen at creation from the cache budget -- artis_amd_config.cache_budget_bytes or the free device
 * memory at that moment -- unless artis_amd_config.ma_hot_fraction gives them): the share of every ion's levels with a static record in every
 * cell's row (1 = all of them: no on-demand records), the number of cold levels, and the 16-byte slots of the shared pool per resident cell.
 * Two runs are comparable in time and in artis_amd_last_pool_resets() only if these agree. Any pointer may be NULL. (ABI 6) */
int artis_amd_record_tiers(artis_amd_engine *eng, double *hot_fraction, int32_t *ncold_levels, int64_t *pool_slots);
/* ... and how much of that pool the last artis_amd_update_packets_device call left in use (since the pool was last emptied), in units of 128
 * bytes, beside the pool's size: a pool that runs near its size thrashes (artis_amd_last_pool_resets), one far below it could give its memory
 * to static records (a larger hot fraction). (ABI 6) */
int artis_amd_last_pool_usage(artis_amd_engine *eng, int64_t *units_used, int64_t *units_cap);
/* Absent ions: the population of the cell cache leaves out the static macro-atom records of the ions whose population in
 * the cell is at most ARTIS_AMD_MA_ABSENT_EPS times their element's (negative: none are left out), and a packet that reaches such a record has it
 * filled by the slow-path kernel -- the same bits the population would have written. *skipped: the records the last population (of the whole cache,
 * or of the cells a tiled run made resident last) left out; *filled: the records the last artis_amd_update_packets_device call filled on demand.
 * Either pointer may be NULL. (ABI 6: an added entry point; nothing that existed changes) */
int artis_amd_last_absent_records(artis_amd_engine *eng, int64_t *skipped, int64_t *filled);
/* Which forms of the thermal kernel (macro-atom walks + k-packet steps) the last artis_amd_update_packets_device call
 * launched, as a mask: the form is chosen per launch from the atomic data's size and the list's length, and a parity test has to know that the
 * form it means to check is the one that ran. (ABI 6) */
#define ARTIS_AMD_THERMAL_PLAIN 1         /* k_thermal<256, 0>: target tables in HBM (any size; lists below 4096 entries) */
#define ARTIS_AMD_THERMAL_LDS_TABLES 2    /* k_thermal<1024, 1>: target levels + LevelPack in LDS (<= 2048 levels, <= 32768 transitions) */
#define ARTIS_AMD_THERMAL_LDS_LEVELPACK 4 /* k_thermal<1024, 2>: LevelPack alone in LDS (<= 9856 levels; not used while the per-cell LDS estimator arrays are active) */
#define ARTIS_AMD_THERMAL_REFILL 8        /* k_thermal_q (ARTIS_AMD_REFILL=1) */
#define ARTIS_AMD_THERMAL_COLD 16         /* ... instantiated with the on-demand records' look-ups (the model has cold levels) */
#define ARTIS_AMD_THERMAL_TAIL 32         /* k_tail took the population's last packets */
#define ARTIS_AMD_THERMAL_LATE 64         /* k_late carried the end of the population: r-packets, thermal packets and slow-path actions in one persistent launch */
int artis_amd_last_thermal_variants(artis_amd_engine *eng, int32_t *mask);
/* How the kernels of the last artis_amd_update_packets_device call added to the per-cell estimators, as a mask: the form follows from the
 * number of non-empty cells (few-cells caps: k_rpkt 512 with the continuum table in LDS, 3072 without it; k_thermal 4096; k_gamma 2048),
 * the kernel form and the ARTIS_AMD_* switches, and a parity test has to know that the path it means to check is the one that ran.
 * (k_slow and k_tail always add with device-wide atomics and are not reported.) (ABI 6) */
#define ARTIS_AMD_EST_RPKT_LDS_CONT 1          /* k_rpkt<true>: the workgroup's LDS array of per-cell sums, continuum table in LDS */
#define ARTIS_AMD_EST_RPKT_LDS_NOCONT 2        /* k_rpkt<false>: the workgroup's LDS array (up to 3072 cells) without the table */
#define ARTIS_AMD_EST_RPKT_LDS_LINE 32768      /* k_rpkt<false, .., true> (ARTIS_AMD_LINELDS=1): the LDS array, up to 512 cells */
#define ARTIS_AMD_EST_RPKT_WAVECACHE 4         /* k_rpkt: every wave's direct-mapped cache of per-cell sums (physics.h est_cache_add) */
#define ARTIS_AMD_EST_RPKT_GLOBAL 8            /* k_rpkt: device-wide atomics (the LINE_LDS form has no room for the caches) */
#define ARTIS_AMD_EST_THERMAL_LDS 16           /* k_thermal: the workgroup's LDS array of colheatingestimator sums */
#define ARTIS_AMD_EST_THERMAL_WAVECACHE 32     /* k_thermal: every wave's cache (est_cache_add_one) */
#define ARTIS_AMD_EST_THERMAL_GLOBAL 64        /* k_thermal<1024, 2> / k_thermal_q / switched off: device-wide atomics */
#define ARTIS_AMD_EST_GAMMA_LDS 128            /* k_gamma: the workgroup's LDS array of dep_estimator_gamma sums */
#define ARTIS_AMD_EST_GAMMA_GLOBAL 256         /* k_gamma: device-wide atomics */
#define ARTIS_AMD_EST_BF_INPLACE 512           /* detailed bound-free estimators added inside k_rpkt (ARTIS_AMD_BFDEFER=0) */
#define ARTIS_AMD_EST_BF_DENSE_CONTLDS 1024    /* ... deferred to k_bfest_dense<true>: continuum table in LDS */
#define ARTIS_AMD_EST_BF_DENSE_HBM 2048        /* ... deferred to k_bfest_dense<false>: continuum table in HBM */
#define ARTIS_AMD_EST_BF_LPR16 4096            /* k_bfest_dense with 16, 32 or 64 lanes per record (ARTIS_AMD_DENSE_LPR) */
#define ARTIS_AMD_EST_BF_LPR32 8192
#define ARTIS_AMD_EST_BF_LPR64 16384
int artis_amd_last_estimator_forms(artis_amd_engine *eng, int32_t *mask);

/* Per-kernel split of the last artis_amd_update_packets_device call: summed launch durations [ms] and summed
 * packet counts of the r-packet kernel (k_rpkt) and of the thermal kernels (k_ma + k_kpkt). */
int artis_amd_last_kernel_breakdown(artis_amd_engine *eng, double *rpkt_ms, int64_t *rpkt_threads, double *thermal_ms,
                                    int64_t *thermal_threads);

int artis_amd_last_kernel_launches(artis_amd_engine *eng, int64_t *rpkt_launches, int64_t *thermal_launches);
/* The same for each kernel: index 0 k_rpkt, 1 k_ma, 2 k_kpkt, 3 k_slow. */
int artis_amd_last_kernel_table(artis_amd_engine *eng, double ms[4], int64_t launches[4], int64_t packets[4]);

/* Diagnostics: the cell cache of one non-empty cell in the reference's layout (globals::cellcache[nonemptymgi] spans,
 * globals.h:283-311). Any pointer may be NULL. The engine's rows hold the macro-atom's cumulative sums as 15-bit filters only
 * (DESIGN.md section 2): `matrans` (allmacroatomictransitions, globals.h:287) is re-added on the device from the transitions'
 * rate coefficients -- the values a draw gets that the filters cannot decide -- and the call fails with
 * ARTIS_ERR_NOTCONVERGED if a filter entry of the cell's records differs from the sequential form's. An engine that keeps
 * on-demand records (atomic data whose static records do not fit; ARTIS_AMD_MA_HOTFRAC) shows the records
 * that exist: a cold level that no packet has reached in this cell since the cache was filled reads as zeros. */
int artis_amd_debug_cellcache(artis_amd_engine *eng, int nonemptymgi, double *levelpops, double *maprocessrates,
                              double *matrans, double *allcont_nnlevel, double *allcont_departure,
                              double *allcont_edgepart, uint64_t *allcont_keepbits, double *corrphotoioncoeff,
                              double *cooling_contrib, double *ion_cooling_contribs, double *chi_ff_nnionpart);
/* Diagnostics: ONE array of a cell's row AS STORED -- the arrays the view above does not show: what the population keeps for the
 * packet kernels beside the reference's spans, the engine's own expansion-opacity tables and the derived non-thermal arrays. The cell is made
 * resident or the cache filled exactly as by artis_amd_debug_cellcache(), and the row is found through the row table (a tiled cache: the row
 * of a cell is not its index). `dst` receives the row's bytes, *written_bytes (may be NULL) their number.
 *   element types: double, but ALLCONT_PAIR / _KEPTPAIR {double, double}; ALLCONT_KEEPBITS uint64 (the padded row, nkeepwords words);
 *   ALLCONT_KEPTLIST / _KEEPPREFIX int32; COOL_GUIDE uint16; EXPANSIONOPACITIES float.
 *   ALLCONT_KEPTLIST and _KEPTPAIR have a place for every continuum; the population writes the first (number of set keep bits) places.
 * ARTIS_ERR_ARG: the array does not exist in this build or model (LINE_DPOP of an engine that forms the factors on the fly; COOL_GUIDE without
 * guides; the expansion tables of another build or handed over by the host, the Planck integral without RPKT_BB_THERMALISATION; the non-thermal
 * arrays without NT_ON), an unknown enumerator, or dst_bytes smaller than the row (nothing is copied then, and *written_bytes receives the
 * row's size; in the other two cases it receives 0). */
enum artis_amd_cc_array {
  ARTIS_AMD_CC_LINE_DPOP = 0,           /* [ndpop] */
  ARTIS_AMD_CC_BF_RADRECOMB = 1,        /* [nphixstargets_total] */
  ARTIS_AMD_CC_BF_COLRECOMB = 2,
  ARTIS_AMD_CC_BF_COLION = 3,
  ARTIS_AMD_CC_BF_COOLING = 4,
  ARTIS_AMD_CC_ALLCONT_PAIR = 5,        /* [nbfcontinua][2] */
  ARTIS_AMD_CC_ALLCONT_KEPTLIST = 6,    /* [nbfcontinua] */
  ARTIS_AMD_CC_ALLCONT_KEEPPREFIX = 7,  /* [nkeepwords] */
  ARTIS_AMD_CC_ALLCONT_KEPTPAIR = 8,    /* [nbfcontinua][2] */
  ARTIS_AMD_CC_COOL_GUIDE = 9,          /* [nguide] */
  ARTIS_AMD_CC_ION_COOLING_C = 10,      /* [nions] the ions' cooling totals before the prefix sum */
  ARTIS_AMD_CC_EXPANSIONOPACITIES = 11,              /* [ARTIS_EXPOPAC_NBINS] float */
  ARTIS_AMD_CC_EXPANSIONOPACITY_PLANCK_CUMULATIVE = 12, /* [ARTIS_EXPOPAC_NBINS] */
  ARTIS_AMD_CC_NT_IONRATECOEFF = 13,    /* [nions] */
  ARTIS_AMD_CC_NT_IONENRATE_CUM = 14,   /* [nions] */
  ARTIS_AMD_CC_ALLCONT_KEEPBITS = 15,   /* [nkeepwords] the whole padded row of the bitmap */
  ARTIS_AMD_CC_COUNT = 16
};
int artis_amd_debug_cellcache_array(artis_amd_engine *eng, int nonemptymgi, int which, void *dst, int64_t dst_bytes, int64_t *written_bytes);
/* Test / debug: the many-keys work-list sort (more than 8192 keys) on host arrays. keys[i] in [0, nkeys) is the key of list[i]; out[0..n)
 * receives list's entries ordered by non-decreasing key (any order among equal keys). A list shorter than 512 entries is copied as it is, as
 * the propagation leaves it. The engine's lists are not touched (its sort scratch is used, and grown for a longer list). ARTIS_ERR_UNSUPPORTED for more keys than the sort
 * takes (2^25), ARTIS_ERR_ARG for 8192 keys or fewer or a key outside the range. */
int artis_amd_debug_sort_list(artis_amd_engine *eng, const int32_t *keys, const int32_t *list, int32_t n, int64_t nkeys, int32_t *out);

/* Summed launch durations (HIP events on the launch stream) of the last artis_amd_update_packets_device() call by kind of kernel:
 * 0 k_rpkt (+ k_bfest_dense), 1 k_thermal, 2 k_slow, 3 k_gamma, 4 k_blackbody, 5 k_tail, 6 tile fills inside the call; 7 k_late.
 * launches may be NULL (it counts the launches of every kind but the tile fills). */
int artis_amd_last_kernel_ms_by_kind(artis_amd_engine *eng, double ms[8], int64_t launches[8]);

/* Measurement builds only (-DARTIS_VISIT_COUNTS, tools/visit_sparsity.py): how many macro-atom transitions the last
 * propagation call drew in the record of every (non-empty cell, level), counts[nonemptymgi * nlevels + level]; the reference fills a
 * level's rates when a packet first reaches it (macroatom.cc:398-417 calc_rates_if_needed). Any other build returns ARTIS_ERR_ARG. */
int artis_amd_debug_visit_counts(artis_amd_engine *eng, uint32_t *counts, int64_t n);

/* ---- emergent spectra and light curves ---------------------------------------
 * The reference's binning of the escaped packets (add_to_spec_res / add_to_lc_res, spectrum_lightcurve.cc:544-713; exspec.cc:30-130)
 * over the resident population, on the device. Every output element is the sequential sum of its contributions in the caller's
 * packet order (the order artis_amd_packets_download returns): the same bits whatever slots the engine gave the packets.
 * Layouts are the reference's (Spectra, spectrum_lightcurve.h), T = ntimesteps, B = ARTIS_SPEC_MNUBINS,
 * P = proccount = 2 * nelements * max_nions + 1, A = nelements * max_nions:
 *   lum, lumcmf [T]; flux(_q, _u) [nnu * T + nts]; emission(_q, _u), trueemission [(nnu * T + nts) * P + column];
 *   absorption(_q, _u) [(nnu * T + nts) * A + element * max_nions + ion]; gamma_lum, gamma_lumcmf [T]; gamma_flux [nnu * T + nts].
 * With dirbin == ARTIS_SPEC_ALL_DIRBINS every r-packet array has a leading axis of 1 + ARTIS_SPEC_MABINS slots: slot 0 the angle
 * average, slot s direction bin s - 1. The gamma arrays are always the angle average. */
#define ARTIS_SPEC_MNUBINS 1000 /* exspec.h:8 */
#define ARTIS_SPEC_MABINS 100   /* exspec.h:12 */
#define ARTIS_SPEC_ALL_DIRBINS (-2)
typedef struct artis_spectra_config {
  int64_t struct_size;       /* sizeof(artis_spectra_config) */
  int32_t ntimesteps;        /* >= 1 */
  int32_t dirbin;            /* -1: angle average; 0..MABINS-1: that direction bin (x MABINS); ARTIS_SPEC_ALL_DIRBINS */
  const double *ts_start;    /* [ntimesteps] strictly increasing (globals::timesteps[].start) */
  const double *ts_width;    /* [ntimesteps] */
  double tmin, tmax;         /* globals::tmin / tmax */
  int32_t emission_absorption;  /* emission, trueemission and absorption decompositions */
  int32_t stokes;               /* Q and U of flux (and of emission / absorption) */
  int32_t gamma;                /* gamma light curve and spectrum (0.05 .. 4 MeV, exspec.cc:61-64) */
  int32_t reserved;
} artis_spectra_config;
typedef struct artis_spectra {
  int64_t struct_size;  /* sizeof(artis_spectra) */
  /* host arrays to fill (layouts above); NULL: skip. An array the last compute did not produce is an ARTIS_ERR_ARG. */
  double *lum, *lumcmf, *flux, *flux_q, *flux_u, *emission, *emission_q, *emission_u, *trueemission, *absorption, *absorption_q,
      *absorption_u, *gamma_lum, *gamma_lumcmf, *gamma_flux;
  float *lower_freq, *delta_freq, *gamma_lower_freq, *gamma_delta_freq; /* [ARTIS_SPEC_MNUBINS] float32 bin edges; NULL: skip */
  /* reported */
  int64_t nescaped_rpkt, nescaped_gamma;
  int32_t ntimesteps, ndirslots, nelements, max_nions, proccount, reserved;
} artis_spectra;
/* Bin the resident population (after artis_amd_packets_upload, artis_amd_update_packets_device or artis_amd_update_packets).
 * Reads packets only. Scratch is allocated at the first call and reused. Synchronous. */
int artis_amd_spectra_compute(artis_amd_engine *eng, const artis_spectra_config *cfg, void *hip_stream);
/* The outputs of the last compute as one device block of *ndoubles doubles (for an all-reduce over ranks): the produced arrays
 * of artis_spectra in the order of its fields. */
int artis_amd_spectra_devptr(artis_amd_engine *eng, void **dptr, int64_t *ndoubles);
int artis_amd_spectra_download(artis_amd_engine *eng, artis_spectra *out);

/* ---- radiation-field fit ---------------------------------------------------------
 * The radiation-field part of the reference's grid update (update_grid_cell, update_grid.cc:462-573), on the device, from the
 * engine's estimator block (after the all-reduce: the summed estimators) and its current cell state (artis_amd_set_cellstate):
 *   every non-empty cell: estimator_normfactor = 1 / (assocvolume_tmin * (prev_mid / tmin)^3) / deltat / nprocs,
 *     J_normfactor = estimator_normfactor / 4 pi, J = J_raw * J_normfactor (normalise_J radfield.cc:893);
 *   LTE iteration or THICK cell: T_J from J (get_T_J_from_J radfield.cc:956; non-finite: the previous T_J), clamped to
 *     [MINTEMP, MAXTEMP]; T_R = T_e = T_J, W = 1; nuJ stays raw and the bins keep their current values;
 *   other cells: nuJ normalised, the full-spectrum fit (set_params_fullspec radfield.cc:400; nubar non-finite or 0: T_J, T_R,
 *     W stay) and, in multibin builds, (W, T_R) of every bin (fit_parameters radfield.cc:806: TOMS 748 root of the Planck mean
 *     frequency in [500, 250000] K; the last bin takes T_e); T_e stays (its thermal-balance solve is the host's);
 *   detailed bound-free estimators (builds with them): bfrate_normed = float(bfrate_raw * estimator_normfactor / H) for every
 *     cell that is not THICK, unless lte_iteration (normalise_bf_estimators radfield.cc:902-925); THICK cells keep what the
 *     engine's block held (zero when first made, or bfrate_normed_seed);
 *   detailed line estimators (builds with them): Jb_lu_normed = Jb_lu_raw * J_normfactor and the contribution counts.
 * The reference's log lines become flag bits per cell and counts per cell and per call. The call changes no estimator, packet,
 * counter or cell state; two calls on the same state give identical results. */
#define ARTIS_RADFIELD_FITTED 1      /* the cell went through the fit (not THICK, not lte_iteration) */
#define ARTIS_RADFIELD_NUBAR_KEPT 2  /* nuJ / J non-finite or 0: T_J, T_R and W of the cell state kept */
#define ARTIS_RADFIELD_TJ_KEPT 4     /* LTE / THICK: T_J from J non-finite, the previous T_J kept */
#define ARTIS_RADFIELD_TJ_LOW 8      /* T_J clamped to MINTEMP */
#define ARTIS_RADFIELD_TJ_HIGH 16    /* ... to MAXTEMP */
#define ARTIS_RADFIELD_TR_LOW 32     /* full-spectrum T_R clamped to MINTEMP */
#define ARTIS_RADFIELD_TR_HIGH 64    /* ... to MAXTEMP */
/* per-cell and per-call counts of bins: [0] T_R at or below 500 K, [1] at or above 250000 K (both from the root search: a bin
 * retried or zeroed afterwards is still counted here), [2] W > 1e4 or non-finite, retried at 250000 K, [3] of those, W still
 * > 1e4: T_R = -99, W = 0, [4] root search stopped at 100 evaluations */
#define ARTIS_RADFIELD_COUNT_TRMIN 0
#define ARTIS_RADFIELD_COUNT_TRMAX 1
#define ARTIS_RADFIELD_COUNT_RETRIED 2
#define ARTIS_RADFIELD_COUNT_ZEROED 3
#define ARTIS_RADFIELD_COUNT_NOTCONVERGED 4
#define ARTIS_RADFIELD_NCOUNTS 5
typedef struct artis_radfield_config {
  int64_t struct_size;                /* sizeof(artis_radfield_config) */
  double prev_mid;                    /* globals::timesteps[nts_prev].mid */
  double deltat;                      /* globals::timesteps[nts_prev].width, > 0 */
  int32_t nprocs;                     /* globals::nprocs, >= 1 */
  int32_t lte_iteration;              /* globals::lte_iteration */
  const double *assocvolume_tmin;     /* [npts_nonempty] grid::get_modelcell_assocvolume_tmin(mgi), > 0 */
  const float *bfrate_normed_seed;    /* [npts_nonempty*nbfestim] or NULL: copied into the engine's block first */
} artis_radfield_config;
typedef struct artis_radfield {
  int64_t struct_size; /* sizeof(artis_radfield) */
  /* host arrays to fill; NULL: skip. An array this build does not make (bins, bf or line estimators) is an ARTIS_ERR_ARG. */
  double *J, *nuJ, *J_normfactor;     /* [npts_nonempty] */
  float *TJ, *TR, *Te, *W;            /* [npts_nonempty] */
  int32_t *flags;                     /* [npts_nonempty] ARTIS_RADFIELD_* bits */
  int32_t *cell_counts;               /* [npts_nonempty][ARTIS_RADFIELD_NCOUNTS] */
  float *radfieldbin_T_R, *radfieldbin_W; /* [npts_nonempty*nbins] */
  float *bfrate_normed;               /* [npts_nonempty*nbfestim] */
  double *Jb_lu_normed;               /* [npts_nonempty*detailed_linecount] */
  int64_t *Jb_lu_contribcount;
  /* reported */
  int64_t totals[ARTIS_RADFIELD_NCOUNTS];
  int32_t npts_nonempty, nbins, nbfestim, detailed_linecount; /* 0 where the build has none */
  double kernel_ms[2]; /* HIP-event time of the last fit: [0] the per-cell kernel, [1] the per-bin kernel */
} artis_radfield;
/* Fit into the engine's result block (allocated at the first call, all of it at once). Synchronous on hip_stream. */
int artis_amd_radfield_fit(artis_amd_engine *eng, const artis_radfield_config *cfg, void *hip_stream);
/* Copy the results of the last fit to the host (sizes in the reported fields even when every pointer is NULL). */
int artis_amd_radfield_download(artis_amd_engine *eng, artis_radfield *out);

/* ---- ionisation balance and hand-over of the grid update ------------------------------
 * The rest of the reference's grid update of an LTE timestep or a THICK cell (update_grid_cell, update_grid.cc:504-510 and
 * :530-549), and calculate_ion_balance_nne (ltepop.cc:475) after the host's T_e solve, on the device, in builds without NLTE
 * populations. In order:
 *   1. the new timestep's rho and composition; nnetot (grid.cc:1719)
 *   2. the temperatures: T_J, T_R, W, T_e of the last artis_amd_radfield_fit (use_fit = 1; Te[] overrides the cells it fitted,
 *      whose T_e the fit leaves), or the host's (use_fit = 0: forced Saha in every cell, the initial timestep)
 *   3. the normalised gamma estimator: the engine's raw block (after the all-reduce) x estimator_normfactor / H with the
 *      normfactor of the last fit (update_grid.cc:358); use_fit = 0: not formed (zero)
 *   4. per non-empty cell: partition functions (ltepop.cc:204, T_exc = T_J with LTEPOP_EXCITATION_USE_TJ, else T_e) and the ion
 *      balance: forced Saha where lte_iteration holds or the cell is THICK, otherwise Saha or rate balance as
 *      FORCE_SAHA_ION_BALANCE says; n_e from a TOMS 748 root in [0, rho / MH] (RelTol 1e-3, 50 evaluations), the ground
 *      populations, then n_e again from the stored floats (set_calculated_nne ltepop.cc:242)
 *   5. corrphotoionrenorm = 1 in LTE and THICK cells (USE_LUT_PHOTOION builds, update_grid.cc:539-543)
 *   6. the result becomes the engine's cell state and the cell cache is filled, as artis_amd_set_cellstate followed by
 *      artis_amd_populate_cellcache would (a tiled cache forgets its rows)
 * A cell flagged NOT_BRACKETED, NONFINITE or INVALID_U refuses the whole state: ARTIS_ERR_NOTCONVERGED, the previous state stays
 * resident. Builds with NLTE populations (the nebular family): ARTIS_ERR_UNSUPPORTED. The result is bitwise reproducible (one
 * writer per output element, no float atomics). Scratch is allocated at the first call, all of it at once. */
#define ARTIS_IONBAL_NEUTRAL 1        /* every element at its lowest stage: set_groundlevelpops_neutral (ltepop.cc:254) */
#define ARTIS_IONBAL_MAXIT 2          /* the n_e root search stopped at 50 evaluations */
#define ARTIS_IONBAL_PHI_OVERFLOW 4   /* an uppermost ion limited by the overflow of nne_max x phi (ltepop.cc:336) */
#define ARTIS_IONBAL_FRAC_ZEROED 8    /* a non-finite ion fraction set to 0 (ltepop.cc:377) */
#define ARTIS_IONBAL_NOT_BRACKETED 16 /* the residual has one sign at 0 and at rho / MH (refused) */
#define ARTIS_IONBAL_INVALID_U 32     /* a partition function <= 0 or non-finite (refused) */
#define ARTIS_IONBAL_NONFINITE 64     /* a non-finite n_e (refused) */
#define ARTIS_IONBAL_FORCED_SAHA 128  /* the cell was balanced with forced Saha (lte_iteration or THICK) */
#define ARTIS_IONBAL_NTIMES 4
typedef struct artis_grid_update {
  int64_t struct_size;      /* sizeof(artis_grid_update) */
  int32_t use_fit;          /* 1: T_J, T_R, W, T_e and lte_iteration of the last artis_amd_radfield_fit (ARTIS_ERR_ARG if none
                               since the last step); 0: the host's TJ/TR/W/Te below and forced Saha in every cell (the initial
                               timestep, update_grid.cc:504-510, which is always an LTE iteration: update_grid.cc:684) */
  const float *TJ, *TR, *W; /* [npts_nonempty], required when use_fit == 0 */
  const float *Te;          /* [npts_nonempty] or NULL: T_e of cells the fit did not set (its fitted cells: the host's T_e
                               solve); NULL keeps the cell's current T_e. use_fit == 0: required */
  /* the new timestep's matter: the host's decay / abundance update (update_grid.cc:714-720), or -- all three NULL, through
   * artis_amd_grid_update_decayed -- the engine's own (artis_amd_decay_update) */
  const float *rho;               /* [npts_nonempty] */
  const float *elem_massfracs;    /* [npts_nonempty*nelements] */
  const float *elem_meanweight;   /* [npts_nonempty*nelements]: USE_CALCULATED_MEANATOMICWEIGHT builds only (elsewhere the
                                     element number densities use artis_model.elem_meannucmass, then required) */
  const int32_t *thick;     /* [npts_nonempty] flags for the NEXT step's packets (update_grid.cc:618-627); the balance uses the
                               current ones */
  const float *kappagrey, *clumpfactor, *ffegrp; /* [npts_nonempty] or NULL: keep the engine's */
} artis_grid_update;
typedef struct artis_grid_update_result {
  int64_t struct_size; /* sizeof(artis_grid_update_result) */
  /* host arrays to fill; NULL: skip */
  float *Te, *TJ, *TR, *W, *nne, *nnetot, *rho; /* [npts_nonempty] the cell state written */
  float *ion_partfuncts, *ion_groundlevelpops;  /* [npts_nonempty*nions] */
  int32_t *uppermost_ion;                       /* [npts_nonempty*nelements] (ltepop.cc:308) */
  double *gamma_normed;                         /* [npts_nonempty*nbfcontinua_ground] the normalised gamma estimator */
  double *phi;                                  /* [npts_nonempty*nions] phi of every ion below its element's top ion (0 there) */
  float *nne_root;                              /* [npts_nonempty] the root search's n_e (0: neutral fallback) */
  int32_t *flags;                               /* [npts_nonempty] ARTIS_IONBAL_* bits */
  int32_t *evals;                               /* [npts_nonempty] evaluations of the n_e residual */
  /* reported */
  int64_t ncells_flagged[8];                    /* cells with bit k of ARTIS_IONBAL_* set */
  int64_t total_evals;
  int32_t npts_nonempty, nions, nelements, nbfcontinua_ground;
  double kernel_ms[ARTIS_IONBAL_NTIMES];        /* HIP-event time: [0] gamma + partition functions, [1] phi, [2] per-cell solve,
                                                   [3] the cell-cache fill */
} artis_grid_update_result;
int artis_amd_grid_update(artis_amd_engine *eng, const artis_grid_update *u, const artis_timestep *ts_next, void *hip_stream);
/* Copy the result of the last artis_amd_grid_update to the host (also after a refused call: its flags and counts). */
int artis_amd_grid_update_download(artis_amd_engine *eng, artis_grid_update_result *out);

/* ---- decay and abundance update ---------------------------------------------------------
 * The composition part of the reference's grid update (update_grid.cc:710-720) on the device: decay::calc_nuc_massfrac_coeffs
 * (decay.cc:1284: per decay path the Bateman sum at t_mid - t_model, decay.h:56 without the expansion factor; per nuclide the
 * surviving fraction), decay::update_abundances (decay.cc:1230: per cell the nuclides' mass fractions as the sparse product of those
 * coefficients with the cell's initial nuclide mass fractions, summed to element mass fractions and mean weights) and set_rho
 * (update_grid.cc:718). Every output element has one writer and is the sequential sum of its contributions in decay-path order: the
 * result is bitwise reproducible, and with the host's coefficients handed in it is the host's bit for bit. Works in every build. */
typedef struct artis_decay_model {
  int64_t struct_size;                /* sizeof(artis_decay_model) */
  int32_t nnuclides;
  int32_t npaths;
  const int32_t *nuc_z, *nuc_a;       /* [nnuclides] */
  const double *nuc_meanlife;         /* [nnuclides] seconds; <= 0: stable */
  const int32_t *path_start;          /* [npaths + 1] into path_nucindex */
  const int32_t *path_nucindex;       /* flat: every path's nuclides, top ... end (decay.cc DecayPath::nucindex) */
  const double *path_branchproduct;   /* [npaths] */
  const int32_t *path_last_decaytype; /* [npaths] ARTIS_DECAYTYPE_* of the step into the end nuclide */
  double t_model;                     /* grid::get_t_model() */
  const float *initnucmassfrac;                   /* [npts_nonempty][nnuclides] grid::get_modelinitnucmassfrac, in non-empty order */
  const float *elem_untrackedstable_initmassfrac; /* [npts_nonempty][nelements] */
  const float *elem_initstablemeannucmass;        /* [nelements] */
  const float *rho_tmin;                          /* [npts_nonempty] */
} artis_decay_model;
typedef struct artis_decay_coeffs {
  int64_t struct_size;          /* sizeof(artis_decay_coeffs) */
  const double *endnuc_coeff;   /* [npaths] NucMassFracCoeffs::decaypath_endnuc_coeff */
  const double *he4_coeff;      /* [npaths] */
  const double *survivingfrac;  /* [nnuclides] */
} artis_decay_coeffs;
typedef struct artis_decay_result {
  int64_t struct_size; /* sizeof(artis_decay_result) */
  /* host arrays to fill; NULL: skip */
  float *rho;                                         /* [npts_nonempty] */
  float *elem_massfracs, *elem_meanweight;            /* [npts_nonempty*nelements] */
  double *endnuc_coeff, *he4_coeff, *survivingfrac;   /* the coefficients the device used */
  double *path_scale, *path_x_dom;                    /* [npaths] of the end nuclide's Bateman sum: lambdaproduct * largest |term|, and lambda * (t_mid - t_model)
                                                         of that term (zero when the coefficients were handed in) */
  double *nuc_massfracs;                              /* [npts_nonempty][nnuclides]; ARTIS_ERR_ARG unless the update was asked for them */
  /* reported */
  int32_t npts_nonempty, nelements, nnuclides, npaths;
  int32_t he4_nucindex, have_nuclides;
  double kernel_ms[3]; /* HIP-event time: [0] k_decay_coeffs, [1] k_decay_cells, [2] k_decay_nuclides */
  double t_mid;
} artis_decay_result;
/* Validate the network (ARTIS_ERR_ARG with a text naming the path: a path shorter than 2, a nuclide index out of range, a nuclide before
 * a path's end with meanlife <= 0, two equal decay constants in a path, a non-finite or negative input), build the product's rows,
 * upload everything. A second call replaces the first. */
int artis_amd_decay_setup(artis_amd_engine *eng, const artis_decay_model *model);
/* The update at t_mid on hip_stream (synchronous). coeffs_or_null: the host's coefficients, used as they are; NULL: the device forms
 * them. want_nuclides: also every nuclide's mass fraction. ARTIS_ERR_ARG without a set-up or for t_mid < t_model. */
int artis_amd_decay_update(artis_amd_engine *eng, double t_mid, const artis_decay_coeffs *coeffs_or_null, int want_nuclides, void *hip_stream);
/* Copy the results of the last update to the host (sizes in the reported fields even when every pointer is NULL). */
int artis_amd_decay_download(artis_amd_engine *eng, artis_decay_result *out);
/* artis_amd_grid_update with the matter of the last artis_amd_decay_update: u->rho, u->elem_massfracs and u->elem_meanweight must be NULL;
 * ARTIS_ERR_ARG unless a decay update is valid and its t_mid == ts_next->mid. */
int artis_amd_grid_update_decayed(artis_amd_engine *eng, const artis_grid_update *u, const artis_timestep *ts_next, void *hip_stream);

/* ---- deposition rates and thickness --------------------------------------------------------
 * What the reference's grid update computes from the decay coefficients and the deposition estimators, on the device: the analytic
 * emission power of every source nuclide in five channels and the six qdot vectors (decay.cc:1105-1168), per cell the analytic emission
 * rates, the normalised deposition estimators and the non-thermal leptons' deposition rate density (nonthermal.cc:2340, sn3d.cc:532-563),
 * the grey depth and the thickness flag of the next step's packets (update_grid.cc:606-627), and the timestep totals of deposition.out
 * (sn3d.cc:240-286). Every sum is the sequential sum of the reference, in its order: the result is bitwise reproducible. Works in every
 * build. The vectors' order everywhere: gamma, positron, electron, alpha, spfission, then qdot of ARTIS_DECAYTYPE_* 0..5. */
#define ARTIS_DEP_NCHANNELS 5
#define ARTIS_DEP_NVECTORS 11
#define ARTIS_DEP_NTOTALS 15
typedef struct artis_deposition_model {
  int64_t struct_size;                /* sizeof(artis_deposition_model) */
  int32_t nnuclides, npts_nonempty;   /* the decay set-up's (checked) */
  const double *nuc_endecay_gamma;    /* [nnuclides] erg per decay (decay.cc nucdecayenergygamma) */
  const double *nuc_endecay_particle; /* [nnuclides][6] in ARTIS_DECAYTYPE_* order (nucdecayenergyparticle) */
  const double *nuc_endecay_q;        /* [nnuclides][6] (nucdecayenergyqval) */
  const double *nuc_branchprob;       /* [nnuclides][6] (get_nuc_decaybranchprob) */
  const double *assocvolume_tmin;     /* [npts_nonempty] grid::get_modelcell_assocvolume_tmin */
  const double *radial_pos_tmin;      /* [npts_nonempty] grid::get_modelcell_mean_radial_pos_tmin (grid.cc:1675) */
} artis_deposition_model;
typedef struct artis_deposition_params {
  int64_t struct_size;     /* sizeof(artis_deposition_params) */
  double mid, width;       /* of the step just propagated: what its estimators are normalised with */
  int32_t nts, nprocs;     /* ... its number; globals::nprocs */
  int32_t nts_next;        /* the step the flags are for: THICK needs nts_next < num_grey_timesteps */
  int32_t num_grey_timesteps;
  double optical_depth_is_thick;
  double optical_depth_is_thick_vpkt; /* read in builds with VPKT_ON */
  const double *power_vectors;        /* NULL: the device forms them; else [ARTIS_DEP_NVECTORS][nnuclides], used as they are */
} artis_deposition_params;
typedef struct artis_deposition_result {
  int64_t struct_size; /* sizeof(artis_deposition_result) */
  /* host arrays to fill; NULL: skip */
  double *eps_ana;                           /* [5][npts_nonempty] erg/s/cm^3: eps_{gamma, positron, electron, alpha, spfission}_ana */
  double *dep;                               /* [5][npts_nonempty] dep_* in the same order */
  double *ntlepton_deposition_rate_density;  /* [npts_nonempty] */
  float *grey_depth;                         /* [npts_nonempty] */
  int32_t *thick;                            /* [npts_nonempty] ARTIS_CELL_* for the next step's packets */
  double *power_vectors;                     /* [ARTIS_DEP_NVECTORS][nnuclides] erg/s per gram of the source nuclide */
  double *totmassnuclide;                    /* [nnuclides] g */
  /* reported */
  double totals[ARTIS_DEP_NTOTALS]; /* gamma_dep, positron_dep, electron_dep, alpha_dep [erg]; then the vectors' products with totmassnuclide
                                       [erg/s]: eps_{gamma, positron, electron, alpha, spfission}_ana_power, qdot of the six decay types */
  double mtot;
  int32_t npts_nonempty, nnuclides, nradioactive, nts_next;
  double t_mid;
  double kernel_ms[3]; /* HIP-event time: [0] k_dep_powers (and the packing), [1] k_dep_cells, [2] k_dep_totals */
} artis_deposition_result;
/* Needs artis_amd_decay_setup (a new one invalidates this set-up). Validates (ARTIS_ERR_ARG with a text naming the nuclide: a negative or
 * non-finite energy, a branch probability outside [0, 1]; a non-positive assocvolume_tmin, a negative or non-finite radial_pos_tmin, sizes
 * that are not the decay set-up's), builds the rows of the paths by top nuclide and the list of radioactive nuclides, forms
 * totmassnuclide and mtot. A second call replaces the first. */
int artis_amd_deposition_setup(artis_amd_engine *eng, const artis_deposition_model *model);
/* The update on hip_stream (synchronous), from the last artis_amd_decay_update (its t_mid, rho and coefficients), the estimator block as it
 * stands (as after artis_amd_allreduce_estimators) and the cell state's kappagrey. ARTIS_ERR_ARG without either set-up or a valid decay update. */
int artis_amd_deposition_update(artis_amd_engine *eng, const artis_deposition_params *params, void *hip_stream);
/* Copy the results of the last update to the host (sizes in the reported fields even when every pointer is NULL). */
int artis_amd_deposition_download(artis_amd_engine *eng, artis_deposition_result *out);
/* The result block on the device, for the stages that read it: eps_ana [5][n], dep [5][n], ntlepton [n] (doubles, contiguous from *eps_ana),
 * grey_depth (float [n]) and thick (int32 [n]). Any pointer may be NULL. */
int artis_amd_deposition_devptr(artis_amd_engine *eng, const double **eps_ana, const float **grey_depth, const int32_t **thick, int64_t *npts_nonempty);
/* artis_amd_grid_update_decayed with the flags of the last artis_amd_deposition_update, device to device: u->thick must be NULL too.
 * ARTIS_ERR_ARG unless a deposition update is valid, was made for nts_next == ts_next->nts and on the decay update of ts_next->mid. */
int artis_amd_grid_update_deposited(artis_amd_engine *eng, const artis_grid_update *u, const artis_timestep *ts_next, void *hip_stream);

/* ---- pellet initialisation -----------------------------------------------------------------
 * The reference's packet_init() (packet.cc:91) on the device: the energy every decay path releases per mass of its top nuclide between
 * t0 (t_model with initial packets on, else tmin) and tmax (decay.cc:1067), per cell the decay energy per mass (decay.cc:1052), the
 * cumulative energy over ALL propagation cells in index order (packet.cc:116-131), and per packet n -- generator seeded seed_base + n
 * (input.cc:1912) -- the cell, the position (grid.cc:1603), the decay channel (decay.cc:1347), the decay time (decay.cc:482), the decaying
 * nuclide with its particle / gamma choice and gamma line (gammapkt.cc:869), direction and rest-frame energy (packet.cc:83-85); then the
 * normalisation of packet.cc:149-159. Every sum is the sequential sum of the reference, in its order; every packet draws from its own
 * generator in the reference's order, and the state left in the packet is the one propagation continues from. With the host's energy
 * vector handed in, every discrete field, the generator state, the energies and the 3D positions are the host's bit for bit; decay times,
 * 1D / 2D positions, directions and e_rf differ by the device's log / cbrt / sin / cos against the host's. Works in every build. */
#define ARTIS_PINIT_NKERNELS 7
typedef struct artis_packet_init_model {
  int64_t struct_size;                        /* sizeof(artis_packet_init_model) */
  const double *nuc_decay_daughters_probsum;  /* [nnuclides] Nuclide::decay_daughters_probsum (decay.cc:238) */
  const int32_t *gamma_start;                 /* [nnuclides + 1] nuclide n's lines are [gamma_start[n], gamma_start[n + 1]); none: it emits no gamma packets */
  const double *gamma_energy;                 /* [gamma_start[nnuclides]] erg */
  const double *gamma_probability;            /* ... per decay */
  const double *initenergyq;                  /* [npts_nonempty] grid::get_initenergyq [erg/g]; NULL unless initial_packets_on && use_model_initial_energy */
  double tmax;                                /* globals::tmax (tmin is the model's) */
  int32_t initial_packets_on;                 /* INITIAL_PACKETS_ON */
  int32_t use_model_initial_energy;           /* USE_MODEL_INITIAL_ENERGY */
  int32_t uniform_pellet_energies;            /* UNIFORM_PELLET_ENERGIES: 0 is ARTIS_ERR_UNSUPPORTED */
  int32_t max_trials_per_launch;              /* decay-time trials of one packet per launch before it is parked; 0: 4096 */
} artis_packet_init_model;
typedef struct artis_packet_init_result {
  int64_t struct_size; /* sizeof(artis_packet_init_result) */
  /* host arrays to fill; NULL: skip */
  double *en_cumulative;      /* [ngrid] */
  double *energy_vector;      /* [npaths] energy_per_massoftopnuc_decaypath as the device used it */
  double *endecay_per_mass;   /* [npts_nonempty] */
  int32_t *channel;           /* [npackets] the decay channel of every packet in caller order: its path, npaths for the initial-energy channel */
  int32_t *trials;            /* [npackets] its decay-time trials */
  /* reported */
  int64_t npackets;
  int32_t ngrid, npts_nonempty, npaths, ncheckpoints;
  double etot_simtime, e_cmf_per_packet, e_cmf_total, e_ratio;
  int32_t continuation_launches; /* launches that continued parked packets */
  int32_t max_trials;            /* the largest trial count of one packet */
  double kernel_ms[ARTIS_PINIT_NKERNELS]; /* HIP-event time: [0] k_pinit_energy, [1] k_pinit_checkpoints, [2] k_pinit_cumulative, [3] k_pinit_place,
                                             [4] k_pinit_decay (all launches), [5] k_pinit_gather, k_pinit_total and k_pinit_scale, [6] the installation */
} artis_packet_init_result;
/* Needs artis_amd_decay_setup and artis_amd_deposition_setup (a new one of either invalidates this set-up). Validates (ARTIS_ERR_ARG with a
 * text naming the nuclide: a non-finite or negative value, a probsum <= 0 for a decaying nuclide, gamma_start not monotone; tmax <= tmin,
 * t_model > tmin, the initial-energy channel without initenergyq), refuses uniform_pellet_energies == 0 (ARTIS_ERR_UNSUPPORTED), uploads.
 * A second call replaces the first. */
int artis_amd_packet_init_setup(artis_amd_engine *eng, const artis_packet_init_model *model);
/* Make npackets pellets on hip_stream (synchronous) and install them as the resident population, exactly as artis_amd_packets_upload
 * would with the same structs: artis_amd_packets_download returns them in caller order. energy_vector_or_null: [npaths] the host's
 * energy_per_massoftopnuc_decaypath, used as it is; NULL: the device forms it. A packet whose decay time is not accepted within
 * max_trials_per_launch trials is parked with its generator state and continued by a further launch (the result does not depend on where
 * it was cut); after 4096 such launches ARTIS_ERR_NOTCONVERGED names the path. On any error the previous population stays resident. */
int artis_amd_packet_init(artis_amd_engine *eng, int64_t npackets, uint32_t seed_base, const double *energy_vector_or_null, void *hip_stream);
/* Copy the results of the last artis_amd_packet_init to the host (sizes in the reported fields even when every pointer is NULL). */
int artis_amd_packet_init_download(artis_amd_engine *eng, artis_packet_init_result *out);

/* ---- initial temperatures and the first cell state ------------------------------------------
 * What the reference does to the cells before the first timestep, on the device: assign_initial_temperatures() (grid.cc:1077-1135) --
 * the energy every decay path has released per mass of its top nuclide between t_model and tstart, weighted for the adiabatic loss
 * since (calc_energy_per_massoftopnuc_decaypath_withexpansion decay.cc:1086, the useexpansionfactor branch of calculate_decaychain
 * decay.h:56), per cell the sequential sum over the paths (decay.cc:1052) plus initenergyq when the pellet set-up has both
 * initial_packets_on and use_model_initial_energy, T_initial with its three clamps, T_e = T_J = T_R = T_initial, W = 1 --, kappagrey
 * (calculate_cell_kappagrey grid.cc:1864-1926, the type a RUNTIME field) and the first step's grey depth and thickness flags
 * (update_grid.cc:606-627). artis_amd_grid_update_initial then balances every cell with forced Saha from these arrays and the decay
 * update's matter and makes the result the engine's FIRST cell state: no artis_amd_set_cellstate is needed before it. Builds without
 * NLTE populations; the nebular family: ARTIS_ERR_UNSUPPORTED. Every output element has one writer, no float atomics: bitwise
 * reproducible. The result block is allocated at the first artis_amd_initial_state. */
#define ARTIS_GREY_FEGROUP_APPROX 0 /* RpktGreyType of constants.h:91, in its order */
#define ARTIS_GREY_TANAKA2020 1
#define ARTIS_GREY_JUST2022 2
#define ARTIS_INITIAL_INSIDE 0         /* a cell's flags: which branch of grid.cc:1113-1128 it took ... */
#define ARTIS_INITIAL_BELOW_MINTEMP 1
#define ARTIS_INITIAL_ABOVE_MAXTEMP 2
#define ARTIS_INITIAL_NONFINITE 3
#define ARTIS_INITIAL_BRANCH_MASK 3
#define ARTIS_INITIAL_KAPPA_INVALID 4  /* ... and this bit: its kappagrey is negative or not finite (the asserts of grid.cc:1923-1924) */
typedef struct artis_initial_params {
  int64_t struct_size;                    /* sizeof(artis_initial_params) */
  double tstart;                          /* globals::timesteps[0].mid */
  int32_t nts_first, num_grey_timesteps;  /* the step the flags are for */
  double optical_depth_is_thick, optical_depth_is_thick_vpkt;
  int32_t rpkt_grey_type;                 /* ARTIS_GREY_FEGROUP_APPROX / _TANAKA2020 / _JUST2022: RPKT_GREY_TYPE of artisoptions.h */
  double mfegroup, mtot_input;            /* FEGROUP_APPROX */
  const float *ffegrp;                    /* [npts_nonempty] FEGROUP_APPROX */
  const float *initelectronfrac;          /* [npts_nonempty] TANAKA2020 */
  const double *energy_vector;            /* NULL: the device forms it; else the host's [npaths], used as it is */
} artis_initial_params;
typedef struct artis_initial_result {
  int64_t struct_size; /* sizeof(artis_initial_result) */
  /* host arrays to fill; NULL: skip */
  float *T_initial;          /* [npts_nonempty] */
  double *endecay_per_mass;  /* [npts_nonempty] decayedenergy_per_mass of grid.cc:1107 (with initenergyq when the channel is on) */
  float *kappagrey;          /* [npts_nonempty] */
  float *grey_depth;         /* [npts_nonempty] */
  int32_t *thick;            /* [npts_nonempty] ARTIS_CELL_* for the packets of step nts_first */
  int32_t *flags;            /* [npts_nonempty] ARTIS_INITIAL_* */
  double *energy_vector;     /* [npaths] as the device used it */
  double *path_scale;        /* [npaths] what the rounding of a path's expansion sum is measured in (0 with a handed-in vector) */
  double *path_x_dom;        /* [npaths] lambda x timediff of the term that sets it */
  /* reported */
  int64_t ncells_branch[4];  /* cells per ARTIS_INITIAL_INSIDE / _BELOW_MINTEMP / _ABOVE_MAXTEMP / _NONFINITE */
  int64_t ncells_kappa_invalid;
  int32_t first_nonfinite_cell; /* the lowest non-empty cell index with a non-finite temperature; -1: none */
  int32_t npts_nonempty, npaths, rpkt_grey_type, nts_first, reserved;
  double first_nonfinite_rho_tmin, first_nonfinite_endecay; /* of that cell (0 without one) */
  double tstart;
  double kernel_ms[2];       /* HIP-event time: [0] k_init_energy (or the vector's upload), [1] k_init_cells */
} artis_initial_result;
/* Needs artis_amd_decay_setup, artis_amd_deposition_setup, artis_amd_packet_init_setup and a valid artis_amd_decay_update at
 * t_mid == tstart (its rho and elem_massfracs), else ARTIS_ERR_ARG with a text naming what is missing; also for tstart < t_model, an
 * unknown grey type, TANAKA2020 with an initelectronfrac <= 0, FEGROUP_APPROX without ffegrp or with mtot_input <= 0. Synchronous. */
int artis_amd_initial_state(artis_amd_engine *eng, const artis_initial_params *params, void *hip_stream);
/* Copy the results of the last artis_amd_initial_state to the host (sizes in the reported fields even when every pointer is NULL). */
int artis_amd_initial_state_download(artis_amd_engine *eng, artis_initial_result *out);
/* artis_amd_grid_update for the first timestep: matter from the last artis_amd_decay_update (as artis_amd_grid_update_decayed),
 * T_J = T_R = T_e = T_initial, W = 1, kappagrey and the flags of step ts_first->nts from the last artis_amd_initial_state, device to
 * device. u->use_fit must be 0 and u->TJ / TR / W / Te / rho / elem_massfracs / elem_meanweight / thick / kappagrey NULL.
 * u->clumpfactor is required while no cell state is resident; u->ffegrp NULL: zeros, as artis_amd_set_cellstate. The balance's
 * "current" state is the reference's before its first update_grid: ground populations 0 (grid.cc:427) and every cell THICK
 * (update_grid.cc:495-501: W == 1), whatever is resident. Works without a resident cell state; a refused balance leaves the engine
 * as it was (without a previous state: without one). ARTIS_ERR_ARG unless the initial state and the decay update were made for
 * ts_first->mid and ts_first->nts. */
int artis_amd_grid_update_initial(artis_amd_engine *eng, const artis_grid_update *u, const artis_timestep *ts_first, void *hip_stream);

/* ---- thermal balance of the thin cells -----------------------------------------------------
 * What the reference's grid update does for a cell the radiation-field fit has fitted, outside an LTE iteration, on the device: the
 * renormalisation of the photoionisation estimator (update_grid.cc:344-387), Gamma per ground population of every ion with a ground
 * continuum (calculate_iongamma_per_gspop ratecoeff.cc:926), the partition functions at the fit's T_J and the T_e of the thermal
 * balance (call_T_e_finder thermalbalance.cc:258: a TOMS 748 root of heating - cooling in [MINTEMP, MAXTEMP], every evaluation with
 * its own ion balance; damped to [0.5, 2] x the resident T_e). The bound-free heating coefficients (calculate_bfheatingcoeffs, with
 * their renormalisation applied) come from the host, or from artis_amd_bfheating_update below without leaving the device
 * (artis_amd_thermal_solve_bfheated). Builds with LTEPOP_EXCITATION_USE_TJ, USE_LUT_PHOTOION, without NT_ON,
 * DIRECT_COL_HEAT and NLTE populations (classic and its variants); every other build: ARTIS_ERR_UNSUPPORTED, the text names the option.
 * A rate is summed by the 64 lanes of a wave in a fixed order (artis_amd/csrc/thermal_balance.h): bitwise reproducible. */
#define ARTIS_THERMAL_BRACKETED 256     /* a sign change over [MINTEMP, MAXTEMP]: the root search ran */
#define ARTIS_THERMAL_PINNED_LOW 512    /* cooling wins everywhere (or non-finite ends): MINTEMP */
#define ARTIS_THERMAL_PINNED_HIGH 1024  /* heating wins everywhere: MAXTEMP */
#define ARTIS_THERMAL_NONFINITE 2048    /* the residual at MINTEMP or MAXTEMP is not finite */
#define ARTIS_THERMAL_DAMPED_UP 4096    /* the solution was above 2 x the resident T_e */
#define ARTIS_THERMAL_DAMPED_DOWN 8192  /* ... below 0.5 x */
#define ARTIS_THERMAL_MAXIT 16384       /* the root search stopped at 100 evaluations */
#define ARTIS_THERMAL_RENORM_ONE 32768  /* a ground continuum of the cell could not be renormalised: corrphotoionrenorm = 1 there */
#define ARTIS_THERMAL_NFLAGS 16         /* bits 0-7: ARTIS_IONBAL_* of the last evaluation's ion balance */
#define ARTIS_THERMAL_NRATES 10
#define ARTIS_THERMAL_NTIMES 4
typedef struct artis_thermal_params {
  int64_t struct_size; /* sizeof(artis_thermal_params) */
  /* the new timestep's matter, as artis_grid_update's; all three NULL: the device arrays of the last artis_amd_decay_update */
  const float *rho;             /* [npts_nonempty] */
  const float *elem_massfracs;  /* [npts_nonempty*nelements] */
  const float *elem_meanweight; /* [npts_nonempty*nelements]: USE_CALCULATED_MEANATOMICWEIGHT builds only */
  const double *bfheatingcoeffs; /* [npts_nonempty*nlevels] calculate_bfheatingcoeffs' result (thermalbalance.cc:217) with its
                                    renormalisation applied; required */
  /* [npts_nonempty] each; all three NULL: the block of the last artis_amd_deposition_update */
  const double *ntlepton_dep, *dep_alpha, *dep_spfission;
  const float *clumpfactor; /* [npts_nonempty] or NULL: the resident one */
} artis_thermal_params;
typedef struct artis_thermal_result {
  int64_t struct_size; /* sizeof(artis_thermal_result) */
  /* host arrays to fill; NULL: skip */
  float *Te;           /* [npts_nonempty] the T_e stored (an unfitted cell: the fit's, T_J) */
  double *Te_solved;   /* [npts_nonempty] before the damping */
  double *bracket;     /* [npts_nonempty][2] the final bracket (both Te_solved without a root search) */
  int32_t *evals;      /* [npts_nonempty] evaluations of the residual */
  int32_t *flags;      /* [npts_nonempty] ARTIS_THERMAL_* | ARTIS_IONBAL_* */
  float *nne;          /* [npts_nonempty] */
  double *rates;       /* [npts_nonempty][ARTIS_THERMAL_NRATES]: cooling_ff, cooling_collisional, cooling_fb, cooling_adiabatic,
                          heating_ff, heating_bf, heating_collisional, heating_dep, heating - cooling, dep_frac_heating */
  float *ion_groundlevelpops; /* [npts_nonempty*nions] */
  float *ion_partfuncts;      /* [npts_nonempty*nions] at the fit's T_J */
  double *phi;                /* [npts_nonempty*nions] of the last evaluation */
  double *gamma;              /* [npts_nonempty*nbfcontinua_ground] Gamma per ground population */
  double *corrphotoionrenorm; /* [npts_nonempty*nbfcontinua_ground] */
  /* reported */
  int64_t ncells_flagged[ARTIS_THERMAL_NFLAGS]; /* cells with bit k set */
  int64_t total_evals, nfitted;
  int32_t npts_nonempty, nions, nbfcontinua_ground, nlevels;
  double kernel_ms[ARTIS_THERMAL_NTIMES]; /* HIP-event time: [0] k_tb_renorm, [1] k_tb_gamma and k_tb_partfunct, [2] k_tb_solve,
                                             [3] k_tb_rates of the last artis_amd_thermal_rates */
} artis_thermal_result;
/* The solve on hip_stream (synchronous). Needs a cell state and an artis_amd_radfield_fit since the last propagation call. Leaves
 * estimators, packets and the resident cell state untouched; keeps device copies of the matter it used. */
int artis_amd_thermal_solve(artis_amd_engine *eng, const artis_thermal_params *params, void *hip_stream);
/* The rates of every non-empty cell at Te[] (NULL: the resident T_e) into the same result block. Like the solve it needs
 * params->bfheatingcoeffs, the deposition inputs (or a deposition update) and a fit since the last propagation call (the estimators'
 * normalisation is the fit's), with either value of rebalance. rebalance = 0: with the resident n_e,
 * ground populations, partition functions, T_J and matter (params' matter is not read); rebalance = 1: the ion balance of a solve's
 * evaluation at Te[] first, with Gamma, partition functions and matter of the last artis_amd_thermal_solve (ARTIS_ERR_ARG without one). */
int artis_amd_thermal_rates(artis_amd_engine *eng, const artis_thermal_params *params, const float *Te, int rebalance, void *hip_stream);
/* Copy the results to the host (sizes in the reported fields even when every pointer is NULL). */
int artis_amd_thermal_download(artis_amd_engine *eng, artis_thermal_result *out);
/* artis_amd_grid_update with the matter the last artis_amd_thermal_solve used (u->rho, u->elem_massfracs and u->elem_meanweight must be
 * NULL), u->use_fit = 1, and in the cells the fit fitted the solve's T_e, Gamma per ground population (the balance's gamma) and
 * corrphotoionrenorm (written to the cell state). u->thick NULL: the flags of the last artis_amd_deposition_update. Unfitted cells go
 * as in artis_amd_grid_update. u->clumpfactor must be NULL: the balance uses the clumping factors the solve used, and they become the
 * cell state's. ARTIS_ERR_ARG unless a thermal solve is valid, was made on the last fit and on the cell state that is still resident
 * (an artis_amd_set_cellstate or a hand-over since the solve makes it stale; so it does for artis_amd_thermal_rates with rebalance = 1). */
int artis_amd_grid_update_thermal(artis_amd_engine *eng, const artis_grid_update *u, const artis_timestep *ts_next, void *hip_stream);

/* ---- bound-free heating coefficients of the thin cells ---------------------------------------
 * calculate_bfheatingcoeffs (thermalbalance.cc:217) with the bfheatingestimator renormalisation in front of it (update_grid.cc:412-443)
 * on the device, for the cells the last radiation-field fit has fitted: one adaptive 61-point Gauss-Kronrod integral
 * (gauss_kronrod_integrate<61>, depth 15, 1e-3) per (cell, photoionisation target) and one per (cell, ground continuum). The ground
 * integrals read the RESIDENT T_R and W (the reference renormalises before fit_parameters), the levels' integrals the fit's. Rules:
 * artis_amd/csrc/bf_heating.h; the same builds as the thermal balance, every other: ARTIS_ERR_UNSUPPORTED. Bitwise reproducible. */
#define ARTIS_BFHEAT_RENORM_ONE 1 /* a ground continuum of the cell could not be renormalised (integral not > 0, ratio not finite): 1 */
#define ARTIS_BFHEAT_NONFINITE 2  /* a coefficient of the cell is not finite (the call refuses the block) */
#define ARTIS_BFHEAT_NTOTALS 3
#define ARTIS_BFHEAT_NTIMES 2
typedef struct artis_bfheating_params {
  int64_t struct_size; /* sizeof(artis_bfheating_params) */
  /* [npts_nonempty] each, together or not at all. NULL: the last fit's T_R and W. Given: those instead, in the levels' integrals
   * (a host with its own fit) */
  const float *TR, *W;
} artis_bfheating_params;
typedef struct artis_bfheating_result {
  int64_t struct_size; /* sizeof(artis_bfheating_result) */
  /* host arrays to fill; NULL: skip */
  double *coeffs;  /* [npts_nonempty*nlevels] bfheatingcoeffs, renormalised; +0 in unfitted cells and for levels without targets */
  double *renorm;  /* [npts_nonempty*nbfcontinua_ground] the renormalisation factors; +0 in unfitted cells and places no ion has */
  int32_t *flags;  /* [npts_nonempty] ARTIS_BFHEAT_* */
  /* reported */
  int64_t totals[ARTIS_BFHEAT_NTOTALS]; /* 61-point nodes evaluated, integrals that subdivided, integrals that reached depth 15 */
  int64_t nfitted, nintegrals;
  int32_t npts_nonempty, nlevels, nbfcontinua_ground, nlevels_with_targets;
  double kernel_ms[ARTIS_BFHEAT_NTIMES]; /* HIP-event time: [0] k_bfh_ground, [1] k_bfh_levels (all its launches) */
} artis_bfheating_result;
/* The update on hip_stream (synchronous). Needs a cell state and an artis_amd_radfield_fit since the last propagation call (its flags,
 * and the estimators' normalisation). Leaves estimators, packets, counters and the resident cell state untouched; remembers the fit and
 * the cell state it was made on. A coefficient that is not finite: ARTIS_ERR_NOTCONVERGED with the count in the text, nothing valid. */
int artis_amd_bfheating_update(artis_amd_engine *eng, const artis_bfheating_params *params, void *hip_stream);
/* Copy the results to the host (sizes in the reported fields even when every pointer is NULL). */
int artis_amd_bfheating_download(artis_amd_engine *eng, artis_bfheating_result *out);
/* artis_amd_thermal_solve with the coefficients of the last artis_amd_bfheating_update, read where they lie on the device:
 * params->bfheatingcoeffs must be NULL. ARTIS_ERR_ARG unless that update was made on the last fit and on the cell state that is still
 * resident (as artis_amd_grid_update_thermal asks of the solve). */
int artis_amd_thermal_solve_bfheated(artis_amd_engine *eng, const artis_thermal_params *params, void *hip_stream);
/* Test hook: gauss_kronrod_integrate<61>(f, a, b, 15, tol, &error) of the analytic integrands of tests/golden/gk61_reference.json
 * (artis_amd/csrc/bf_heating.h Gk61TestFn) on the current device, one lane per case, so that the subdividing walk runs there. */
typedef struct artis_gk61_case {
  int32_t which, reserved;
  double p, a, b, tol;
} artis_gk61_case;
typedef struct artis_gk61_result {
  double result, error;
  int64_t evals;
  int32_t nodes, maxdepth;
} artis_gk61_result;
int artis_amd_debug_gk61(int32_t ncases, const artis_gk61_case *cases, artis_gk61_result *out);

/* ---- rate-coefficient tables -----------------------------------------------------------------
 * precalculate_rate_coefficient_integrals (ratecoeff.cc:143-233) on the device: spontrecombcoeffs, bfcooling_coeffs and, in builds with
 * USE_LUT_PHOTOION, corrphotoioncoeffs, [nbfcontinua][TABLESIZE] each, from the model's cross-section tables; one adaptive 61-point
 * Gauss-Kronrod integral (depth 15, 1e-3) per table and entry. Covered: ions 0 .. nions-2 of every element, levels below
 * nlevels_ionising, every target, at (level_bflist_start[level] + target) * TABLESIZE + temperature index; every other element is +0.
 * Rules: artis_amd/csrc/ratecoeff_tables.h; every build. Bitwise reproducible. Not built: the calibration to a recombination-rate file
 * (read_recombrate_file / scale_level_phixs multiply the finished tables): a host that calibrates keeps handing its tables in. */
#define ARTIS_RATECOEFF_BAD_ALPHA_SP 1  /* the entry's alpha_sp is negative or not finite (the reference asserts) */
#define ARTIS_RATECOEFF_BAD_GAMMACORR 2 /* ... its gammacorr is not >= 0 */
#define ARTIS_RATECOEFF_BAD_BFCOOLING 4 /* ... its bfcooling coefficient is negative or not finite */
#define ARTIS_RATECOEFF_BAD_SAHAFACT 8  /* ... its modified_sahafact is negative or not finite */
typedef struct artis_ratecoeff_request {
  int64_t struct_size; /* sizeof(artis_ratecoeff_request) */
  int32_t install;     /* 1: copy the tables over the model's on the device (set-up phase only, see below); 0: compute only */
  int32_t reserved;
  int64_t items_per_launch; /* entries (continuum x temperature) per kernel launch; 0: the default */
} artis_ratecoeff_request;
typedef struct artis_ratecoeff_stats {
  int64_t struct_size; /* sizeof(artis_ratecoeff_stats) */
  int64_t integrals, nodes, at_depth_cap; /* integrals taken, 61-point nodes evaluated, integrals that reached depth 15 */
  int64_t flagged, first_flagged;         /* entries with a flag; the first one's index (-1: none) */
  int64_t nbfcontinua, ncovered;          /* rows of a table; rows the reference's loops write */
  int32_t tablesize, ntables;             /* TABLESIZE; 3 with USE_LUT_PHOTOION, else 2 */
  double kernel_ms;                       /* HIP-event time of all launches of k_rc_tables */
} artis_ratecoeff_stats;
/* Compute the tables (synchronous, on the null stream); the block is allocated at the first call. An entry the reference would
 * assert on is flagged: with any, ARTIS_ERR_NOTCONVERGED naming the first and the count, and nothing is installed (the download still
 * shows tables and flags). install = 1 is allowed only while the engine is being set up -- no artis_amd_set_cellstate or hand-over yet,
 * and the ion balance's ion_alpha_sp table not made: the pairs' coefficients of the cell cache, the cooling lists and ion_alpha_sp are
 * all derived from the tables after that; otherwise ARTIS_ERR_ARG saying which. Creation reads only the tables' addresses, so a host
 * that installs may hand in placeholders (zeros). Without install the engine's model, cell state, packets and estimators are untouched. */
int artis_amd_ratecoeff_compute(artis_amd_engine *eng, const artis_ratecoeff_request *request);
/* Copy the last computed tables ([nbfcontinua*TABLESIZE] doubles each), the per-entry flags ([nbfcontinua*TABLESIZE], ARTIS_RATECOEFF_*)
 * and the counts to the host; any pointer may be NULL. A non-NULL corrphotoion in a build without USE_LUT_PHOTOION: ARTIS_ERR_ARG. */
int artis_amd_ratecoeff_download(artis_amd_engine *eng, double *spont, double *corrphotoion, double *bfcooling, int32_t *flags,
                                 artis_ratecoeff_stats *stats);

/* ---- photoionisation coefficients of builds without USE_LUT_PHOTOION -------------------------
 * get_corrphotoioncoeff (ratecoeff.cc:840) for every bound-free pair of every cell on the device, in place of the host array
 * artis_cellstate.corrphotoioncoeff: the normalised bound-free estimator of the last timestep where the build keeps one and it is >= 0
 * (DETAILED_BF_ESTIMATORS_ON, from DETAILED_BF_ESTIMATORS_USEFROMTIMESTEP on), else one adaptive 61-point Gauss-Kronrod integral
 * (depth 15, 1e-3) over the cell's radiation field (calculate_corrphotoioncoeff_integral, ratecoeff.cc:480-521), read from the state that
 * is being set: level populations, T_e, n_e, W, T_R and the multibin W, T_R. Continuum i of the model's allcont_* arrays writes entry
 * level_phixstargetstart[level] + target of the cell's row; an entry no continuum writes is +0. Rules: artis_amd/csrc/photoion.h.
 * Bitwise reproducible. Builds with USE_LUT_PHOTOION: ARTIS_ERR_UNSUPPORTED. */
#define ARTIS_PHOTOION_NONFINITE 1 /* per-cell flag: a coefficient of the cell is not finite (the reference asserts) */
#define ARTIS_PHOTOION_SRC_ESTIMATOR 1 /* per-entry source: the bound-free estimator */
#define ARTIS_PHOTOION_SRC_INTEGRAL 2  /* ... the integral (0: no continuum writes the entry) */
#define ARTIS_PHOTOION_NTOTALS 5
typedef struct artis_photoion_params {
  size_t struct_size;          /* sizeof(artis_photoion_params) */
  int32_t use_bf_estimators;   /* globals::timestep >= DETAILED_BF_ESTIMATORS_USEFROMTIMESTEP (artisoptions.h; 13 in every shipped file);
                                * must be 0 in a build without DETAILED_BF_ESTIMATORS_ON */
  const float *bfrate_normed;  /* [npts_nonempty][nbfestim] prev_bfrate_normed, or NULL: the last artis_amd_radfield_fit's block, device
                                * to device */
  int32_t cells_per_launch;    /* 0 = default; for tests */
} artis_photoion_params;
typedef struct artis_photoion_result {
  int64_t struct_size; /* sizeof(artis_photoion_result) */
  /* host arrays to fill; NULL: skip */
  double *coeff;   /* [npts_nonempty*nphixstargets_total] */
  uint8_t *source; /* [npts_nonempty*nphixstargets_total] ARTIS_PHOTOION_SRC_* */
  int32_t *flags;  /* [npts_nonempty] ARTIS_PHOTOION_* */
  /* reported */
  int64_t totals[ARTIS_PHOTOION_NTOTALS]; /* entries from estimators, integrals, 61-point nodes, integrals that reached depth 15,
                                           * non-finite coefficients */
  int32_t npts_nonempty, nphixstargets_total, nbfcontinua, nbfestim;
  double kernel_ms; /* HIP-event time of all launches of k_photoion */
} artis_photoion_result;
/* artis_amd_set_cellstate for a host that does not make corrphotoioncoeff: cells->corrphotoioncoeff must be NULL (else ARTIS_ERR_ARG).
 * Uploads the state, computes the coefficients on hip_stream from the state just uploaded (the radiation-field timestep test uses
 * ts->nts), makes them the cell state's and populates the cell cache as artis_amd_set_cellstate does (synchronous). ARTIS_ERR_ARG:
 * cells->levelpops missing; a multibin build without the bins; use_bf_estimators in a build without DETAILED_BF_ESTIMATORS_ON, or with
 * bfrate_normed NULL and no valid artis_amd_radfield_fit; every refusal of artis_amd_set_cellstate. Any coefficient that is not finite:
 * ARTIS_ERR_NOTCONVERGED with the count in the text, and no cell state is resident (as after any refused artis_amd_set_cellstate);
 * artis_amd_photoion_download still shows the block until the next cell state is set. */
int artis_amd_set_cellstate_photoion(artis_amd_engine *eng, const artis_cellstate *cells, const artis_timestep *ts,
                                     const artis_photoion_params *params, void *hip_stream);
/* Copy the coefficients of the last artis_amd_set_cellstate_photoion, the per-entry sources, the per-cell flags and the counts to the
 * host (sizes in the reported fields even when every pointer is NULL). ARTIS_ERR_ARG once another cell state has been set. */
int artis_amd_photoion_download(artis_amd_engine *eng, artis_photoion_result *out);

#ifdef __cplusplus
}
#endif
#endif /* ARTIS_AMD_H */
