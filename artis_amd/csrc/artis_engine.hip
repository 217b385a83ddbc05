// artis_engine.hip -- the MI355X packet-propagation engine behind include/artis_amd.h.
//
// Layout of the work on the GPU (gfx950, wave64):
//   * model tables, cell state and the per-cell cache live in HBM for the whole timestep;
//   * packets are three arrays of cache-line records (tables.h PktStore: hot / flight / cold), one lane per packet;
//   * one timestep = populate kernels (cell cache) + repeated k_propagate launches over a compacted
//     list of packets that still need updating. Each thread advances its packet by at most `budget`
//     do_packet() calls, then survivors are appended to the next list with a wave ballot;
//   * estimators are accumulated with hardware f64 atomics, event counters in LDS and flushed per block.
// There is no CPU path in this library: every entry point needs a HIP device.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is bound at run time (rccl_api below)

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include <cmath>

#include "model_build.h"
#include "engine_config.h"
#include "cache_residency.h"
#include "physics.h"
#include "radfield_fit.h"
#include "ion_balance.h"
#include "decay_update.h"
#include "deposition.h"
#include "packet_init.h"
#include "initial_state.h"
#include "thermal_balance.h"
#include "bf_heating.h"
#include "ratecoeff_tables.h"
#include "photoion.h"
#include "spectra.h"

#include <rocprim/device/device_radix_sort.hpp>

using namespace artis;

namespace {

thread_local std::string g_last_error;

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      g_last_error = std::string(#expr) + ": " + hipGetErrorString(_e);                            \
      return ARTIS_ERR_HIP;                                                                        \
    }                                                                                              \
  } while (0)

constexpr int BLOCK = 256;

// ------------------------------------------------------------------ the kernels, inside this anonymous namespace, in the order they build on each other
#include "cellcache_kernels.h"      // populate kernels
#include "list_kernels.h"           // packet layout, work lists, k_classify
#include "sort_kernels.h"           // the work lists' sorts
#include "rpkt_kernels.h"           // work pulling, k_rpkt, the dense bound-free estimator rows
#include "gamma_kernel.h"           // k_gamma
#include "thermal_kernels.h"        // k_thermal
#include "thermal_refill_kernel.h"  // k_thermal_q
#include "late_kernel.h"            // k_late
#include "tail_slow_kernels.h"      // k_tail, k_slow, k_blackbody
#include "vpkt_kernel.h"            // k_vpkt

inline int nblocks(int64_t n) { return (int)((n + BLOCK - 1) / BLOCK); }

// the timestep-end stages (stage_*.h, included at the end of this file); the engine holds each one's state from its first call on
struct SpecState;
void spec_free(SpecState *st);
struct RfState;
void rf_free(RfState *st);
struct IbState;
void ib_free(IbState *st);
struct DecayState;
void decay_free(DecayState *st);
struct DepState;
void dep_free(DepState *st);
struct PinitState;
void pinit_free(PinitState *st);
struct InitState;
void init_free(InitState *st);
void init_invalidate(InitState *st);  // a new decay set-up: what the initial state was made on is gone
struct TbState;
void tb_free(TbState *st);
struct BfhState;
void bfh_free(BfhState *st);
struct RcState;
void rc_free(RcState *st);
struct PiState;
void pi_free(PiState *st);

}  // namespace

// ------------------------------------------------------------------ engine object
// What one artis_amd_update_packets_device call did: zeroed when the call begins, read by the artis_amd_last_* accessors.
struct LastCall {
  double propagate_ms = 0., kms[NEXT_NKINDS] = {}, kms_tail = 0., fill_ms = 0.;  // summed launch durations: all, per kind, the tail kernel's; tile fills'
  double kms_late = 0.;          // ... k_late's
  int64_t late_launches = 0, tail_launches = 0;
  int64_t late_bailouts = 0;     // waves of k_late that gave up waiting for work (ARTIS_AMD_TRACE prints them)
  int64_t klaunches[NEXT_NKINDS] = {}, kthreads[NEXT_NKINDS] = {}, nlaunches = 0;
  // tiled runs: sweeps over the tiles, tile fills (sparse ones, cells filled), packets listed per (sweep, tile), packets parked
  int64_t sweeps = 0, tile_fills = 0, sparse_fills = 0, cells_filled = 0, listed = 0, parked = 0;
  int64_t pool_resets = 0;       // times the pool of on-demand records was emptied because it was used up
  int32_t thermal_variants = 0, est_forms = 0;  // thermal-kernel instantiations launched; how the kernels added to the per-cell estimators (include/artis_amd.h)
};
// what the many-keys sort of a list of up to `capacity` entries needs besides its input and output: one allocation
struct SortScratch {
  void *base = nullptr;
  int64_t capacity = 0;
  int2 *pairs = nullptr;          // [capacity] pass 1's output: (key, entry), bucket by bucket
  int32_t *mat = nullptr;         // [SORT_HI_MAX][tiles of the list] the tiles' bucket counts, scanned in place
  int32_t *tiles = nullptr;       // the scan's tile totals
  int32_t *seg = nullptr;         // [SORT_HI_MAX + 1] where every bucket begins
  int32_t *chunk_base = nullptr;  // [SORT_HI_MAX + 1] pass 2's chunks before every bucket
};
// The cell cache's host state: which cells hold rows (cache_residency.h), the device copies of that, and what a fill works on and with (stage_cellcache.h).
struct CellCache {
  // Cell-cache tiling: the cache rows of `res.tile_cells` non-empty cells are resident at a time (all of them when they fit
  // the budget: ntiles == 1). With more tiles, update_packets sweeps over them -- populate a tile, advance every packet
  // that sits in one of its cells until it leaves the tile or is done -- until no packet is left (what the reference's
  // single-slot cell cache does cell by cell, update_packets.cc:397-460, 551-621).
  int ntiles = 1;
  int tile_lo = 0, tile_hi = 0;   // one tile: all cells (the range a whole-cache fill works on)
  int tile_valid_lo = -1;         // one tile: 0 once the cache is populated for the current cell state (-1: not)
  // several tiles: which cell's cache each row holds, populated for the current cell state (physics.h Env::krow_tab; make_resident())
  artis_residency::Residency res;
  int32_t *d_krow = nullptr;         // the device's copy of res.krow
  std::vector<int32_t> h_cell_grid;  // [npts_nonempty] the grid cell of a non-empty cell (the inverse of propcell_nonemptymgi)
  size_t cache_bytes_per_cell = 0;
  // the cells a fill of a tiled cache works on (make_resident()). Sparse fills: a visit for which few packets wait makes the cells in which they
  // wait (and the cells around those) resident instead of a whole window. ARTIS_AMD_SPARSE_FILL=0: whole windows.
  int32_t *d_fill_cells = nullptr;
  bool sparse_fill = true;
  int64_t sparse_max_listed = 16384;  // ... for visits that list at most this many packets (ARTIS_AMD_SPARSE_MAX; 512 in round 3:
                                      // 4 tiles 3327 / 3205 / 3188 ms at 512 / 4096 / 16384, with parked tails 3222 / 3123 / 2982)
  // Adaptive tiles (round 6; ARTIS_AMD_TILE_ADAPT=0: the fixed ranges of rounds 2-5). WHICH cells are resident is chosen before every visit from
  // the number of packets that wait in every cell (k_count_waiting): the window of tile_cells consecutive cells in which most packets wait
  // (ARTIS_AMD_TILE_BLOCK=0), or the blocks of tile_block consecutive cells in which most wait, wherever they lie (a tile = a SET of cells: rows are
  // addressed through Env::krow_tab). A cell that is resident and still wanted keeps its row -- only the cells that are new to the set are filled.
  // The first visits take the densest parts of the ejecta; afterwards the waiting packets sit on both sides of the earlier sets' edges, and a set laid
  // across such an edge lets them cross it freely instead of waiting once per crossing and fixed tile.
  bool tile_adapt = true;
  int64_t tile_block = 0;
  bool pool_keep = true;
  int32_t *d_waiting = nullptr;  // [npts_nonempty + 1] packets waiting per cell; the last entry: packets that need no row
  std::vector<int32_t> h_waiting;
  // the population's scratch: the collisional-excitation cooling terms of `pop_batch` cells at a time (k_matrans writes them,
  // k_cooling_chain turns them into running sums, k_collexc_filter into the records' cooling filters; nothing of it is kept)
  double *d_collexc_terms = nullptr;
  int64_t pop_batch = 0;
};
struct artis_amd_engine {
  int device = 0;
  EngineConfig cfg;           // the resolved configuration (engine_config.h resolve_config: struct field, else ARTIS_AMD_* variable, else default)
  double cache_budget = 0.;   // [B] the budget the rows were sized by (given, or the automatic rule on the free memory at creation)
  SpecState *spec = nullptr;  // artis_amd_spectra_*: nothing until the first call
  RfState *rf = nullptr;      // artis_amd_radfield_*: nothing until the first call
  IbState *ib = nullptr;      // artis_amd_grid_update*: nothing until the first call
  DecayState *decay = nullptr;  // artis_amd_decay_*: nothing until artis_amd_decay_setup
  DepState *dep = nullptr;      // artis_amd_deposition_*: nothing until artis_amd_deposition_setup
  PinitState *pinit = nullptr;  // artis_amd_packet_init*: nothing until artis_amd_packet_init_setup
  InitState *init = nullptr;    // artis_amd_initial_state*: nothing until the first call
  TbState *tb = nullptr;        // artis_amd_thermal_*: nothing until the first call
  BfhState *bfh = nullptr;      // artis_amd_bfheating_*: nothing until the first call
  RcState *rc = nullptr;        // artis_amd_ratecoeff_*: nothing until the first call
  PiState *pi = nullptr;        // artis_amd_set_cellstate_photoion: nothing until the first call
  double *pi_coeff = nullptr;   // ... its coefficients [cell][nphixstargets_total] among cell_allocs (null: the cell state is not of that call)
  uint64_t cellstate_serial = 0;  // counts the changes of the resident cell state (artis_amd_set_cellstate, the hand-over of artis_amd_grid_update*)
  bool fit_since_step = false;  // an artis_amd_radfield_fit since the last propagation call (artis_amd_grid_update use_fit)
  ModelOwned own;
  std::vector<void *> model_allocs;
  std::vector<void *> cell_allocs;
  std::vector<void *> cache_allocs;
  DevModel M{};  // device pointers
  DevModel Mh{};  // host view (counts)
  artis_model model_copy{};                        // sizes + level_matransblock_start kept for diagnostics
  std::vector<int32_t> own_matransblock_start;
  DevCells C{};
  DevCache K{};
  DevStep S{};
  DevEst E{};
  bool have_cells = false;
  bool expopac_own = false;  // the expansion-opacity tables are the engine's (calculated at cell-cache population)
  BfEvent *d_bfev = nullptr;     // deferred bound-free estimator updates of one k_rpkt launch (DETAILED_BF builds)
  int32_t *d_bfev_count = nullptr;
  // the sums of the deferred updates, [cell][place in the cell's list of kept continua]: the additions of a record go to
  // neighbouring doubles instead of ~30 separate 64-byte sectors of bfrate_raw; k_bfrate_expand moves them when a call ends
  double *d_bfrate_kept = nullptr;
  bool bfrate_kept_dirty = false;  // a call ended in an error before its sums were moved
  int32_t bfev_cap = 0;
  bool bf_defer = true;          // ARTIS_AMD_BFDEFER=0: add in place inside k_rpkt
  // virtual packets (VPKT_ON builds): the configuration block, and the events one launch records for k_vpkt (at most
  // budget_r per packet on the launch's list: an electron scattering per do_rpkt_step(), one emission per thermal visit)
  VpktConfig *d_vpkt_config = nullptr;
  VpktSeed *d_vpkt_queue = nullptr;
  int32_t *d_vpkt_count = nullptr;
  int32_t vpkt_cap = 0;
  CellCache cc;  // the cell cache: which cells hold rows, what a fill works on (stage_cellcache.h)
  int32_t *d_target_level = nullptr;
  double *d_est = nullptr;
  int64_t est_ndoubles = 0;
  int64_t nvspec = 0, nvgrid = 0;  // doubles of the virtual-packet spectra / velocity-grid map at the end of the block
  unsigned long long *d_stats = nullptr;
  int32_t *d_err = nullptr;      // (the slot after the list counters: one copy brings both to the host)
  int32_t *h_counts = nullptr;   // pinned: the host's copy of the list counters and the error flag after every launch
  // packets
  int64_t npackets = -1;           // -1: no resident population
  void *d_pkt = nullptr;           // the three record arrays of the resident population (tables.h PktStore)
  void *d_pkt_snapshot = nullptr;
  size_t pkt_bytes = 0;
  PktStore P{};
  artis_packet *d_aos = nullptr;
  int64_t aos_capacity = 0;
  bool aos_valid = false;  // d_aos still holds the caller's structs of the resident population (set by the upload)
  int32_t *d_lists[NEXT_NKINDS][2] = {};      // per kind: current and alternate work list
  int32_t *d_keys[NEXT_NKINDS][2] = {};       // ... and the sort keys of their entries
  int32_t *d_sorted = nullptr;                // counting-sort output
  int32_t *d_perm = nullptr;                  // record slot -> index in the caller's packet array (k_aos_to_rec)
  bool use_perm = false;                      // d_perm describes the resident population
  bool slot_order_by_cell = true;             // ARTIS_AMD_SLOTSORT=0: slots in the caller's order
  int32_t *d_hist = nullptr;                  // [SORT_LDS_KEYS + 1] key histogram of the few-keys sort
  int32_t *d_tiles = nullptr;                 // ... and its scan's tile totals
  SortScratch sort_scratch;                   // the many-keys sort's buffers, allocated with the lists
  bool sort_attr_set = false;                 // k_sort_segments may use its 128 KB of LDS on this engine's device
  int32_t *d_count = nullptr;                 // [NEXT_NKINDS] current-list counts, [NEXT_NKINDS] alternate-list count
  int32_t *d_cursors = nullptr;               // [PULL_SLOTS] chunk cursors of the running pull kernel (work_pull.h)
  int ncu = 256;
  double *d_gamma_ws = nullptr;   // per-packet groundcont_gamma_contr lists (physics.h Env)
  int32_t *d_gamma_gi = nullptr;
  int32_t *d_gamma_n = nullptr;
  int64_t ws_capacity = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  LastCall last;  // what the last artis_amd_update_packets_device call did (artis_amd_last_*)
  // (builds with the detailed bound-free estimators -- the nltenebular family -- alternate twice as often between the
  // kernels and their r-packet steps are ~3x as heavy: measured optimum 16384 / 4 / 1024 instead of 4096 / 8 / 2048,
  // nltenebular step 1801 -> 1690 ms, profiles/r03/neb_sweep*.txt)
  int tail_max = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? 16384 : 4096;  // r-packets + thermal packets left at which k_tail takes over (artis_amd_config.tail_threshold; 0 = never)
  bool tail_always = false;           // ... also for a population that starts below it (ARTIS_AMD_TAIL_ALWAYS=1)
  // k_late: r-packets + thermal packets left at which one persistent launch takes over from the split kernels (ARTIS_AMD_LATE; 0 = never;
  // chosen by a sweep on the headline, profiles/r08/late_kernel.md), for a population that began larger -- or any (ARTIS_AMD_LATE_ALWAYS=1)
  int64_t late_max = 200000;
  bool late_always = false;
  bool late_strict = false;           // ARTIS_AMD_LATE_STRICT=1: a wave of k_late that gave up waiting fails the call (tests)
  bool late_attr_set = false;         // k_late's dynamic-LDS attribute has been set on this engine's device
  int32_t *d_late_ring[LATE_NQ] = {nullptr, nullptr, nullptr};  // the workgroups' queues (allocated with the lists)
  int32_t *d_late_bail = nullptr;     // the slot after the error flag
#ifdef ARTIS_PROFILE_LATE
  int32_t *d_late_stamp = nullptr;    // (k_late's profile: LateArgs::stamp; lives as long as the process)
#endif
  bool park_tails = true;     // ARTIS_AMD_TILE_PARK=0: every visit of a tile runs its packets to their end (rounds 2-3)
  // artis_amd_config.tile_park_at: packets left of a larger visit at which it parks them (0 / <= tail_max: round 4's rule, at the tail kernel's
  // threshold). Measured on the headline at a quarter of its cache (4 tiles, adaptive windows; profiles/r06/tiling.md): 4096 / 32768 / 131072 /
  // 524288 / 2097152 -> 2395 / 2147 / 1971 / 1899 / 1868 ms per step (untiled 760); with this round's rows for sets of cells and record tiers (two tiles
  // of rows with a quarter of the levels hot): 131072 / 524288 / 2097152 / 3145728 / 4194304 -> 1550 / 1532 / 1504 (1485 on the box of the last two) / 1448 / 1452 ms;
  // three tiles at 11600 MB: 2097152 / 3145728 / 4194304 -> 1590 / 1573 / 1670 ms
  int64_t park_at = 3145728;
  int64_t last_pool_used = 0, last_pool_cap = 0;  // units (128 B) of the pool in use at the end of the last call that had cold levels / its size (no call resets them)
  double ma_hotfrac = 1.;        // the share of every ion's levels that has a static record (given, or chosen by engine_fill from the cache budget)
  bool vpkt_cont_lds = true;  // ARTIS_AMD_VPKT_CONTLDS=0: k_vpkt reads the continuum table from memory (four workgroups of 256 per CU)
  bool tile_zigzag = false;  // ARTIS_AMD_TILE_ZIGZAG=1: sweeps alternate their direction (measured slower: profiles/r03/tiling.md)
  int64_t last_visits = 0;  // visits of the last call that had packets (the driver's own count: adaptive tiles, trace)
  // do_rpkt_step() calls per packet per launch. 8 in rounds 2-3; with the r-packet kernel's reads requested ahead (round 4) the list's order
  // -- sorted by cell and frequency before every launch -- is worth more than the launches saved: 857 / 855 / 851 / 846 / 860 / 881 ms per step
  // at 8 / 6 / 5 / 4 / 3 / 2 (classic; kilonova_lte 859 / 844 / 858 at 8 / 4 / 3; nltenebular, 4 since round 3: 1199 / 1204 / 1235 at 4 / 3 / 2)
  // (8 stays where a step is cheap and launches are not: the expansion-opacity build with thermalising bound-bound events, 520 vs 567 ms,
  // and the virtual-packet builds, whose every launch is followed by k_vpkt: 1250 vs 1268 ms)
  int budget_r = (ARTIS_OPT_RPKT_BB_THERMALISATION || ARTIS_OPT_VPKT_ON) ? 8 : 4;
  int budget_g = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? 32 : 64;      // ... of a gamma packet (k_gamma)
  int budget_t = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? 1024 : 2048;  // macro-atom transitions / k-packet steps per packet per launch
  // A launch lasts as long as its slowest packet, and a list that does not fill the GPU any more (the last tenth of a
  // timestep's rounds) is bound by that alone. Smaller budgets for such lists (ARTIS_AMD_SMALL_LIST, ARTIS_AMD_BUDGET_T_SMALL /
  // _R_SMALL; 0 = off, the default) were measured: classic 1160 -> 1182..1258 ms per step (the extra rounds cost more than
  // the shorter launches save), nltenebular 1500 -> 1481 (profiles/r03/small_list_budgets.txt).
  int small_list = 300000;
  int budget_t_small = 0;
  int budget_r_small = 0;
  // k_thermal's unit budget while its list still has entries, in launches with the hand-over at list exhaustion below (EngineConfig::budget_t_bulk,
  // ARTIS_AMD_BUDGET_T_BULK; 0 = none). None: the wave's other lanes keep pulling beside a long history and the hand-over ends the launch anyway, so
  // budget_t there only stored, listed, sorted and loaded such a packet again every round. Launches without hand-over keep budget_t.
  int budget_t_bulk = 0;
  // ... and after the launch's list is used up (ARTIS_AMD_DRAIN_T; 0 = off), in launches of at least drain_min_list packets
  int drain_t = 48;
  int drain_r = 1;       // ... do_rpkt_step() calls after the r-packet list is used up (ARTIS_AMD_DRAIN_R; 0 = off)
  int64_t drain_min_list = 1000000;
  bool sort_lists = true;
  bool sort_nu = true;
  // The r-packet list sorted by (frequency bin, cell) instead of (cell, frequency bin) (round 5; ARTIS_AMD_SORT_NUMAJOR=0: rounds 2-4): the
  // 64 packets a wave holds then lie in one of 32 frequency bins (four per octave) -- their opacity sums run over windows of similar length
  // and their line walks through the same stretch of the line list -- and in ~7 neighbouring cells of it. k_rpkt 263 -> 251 ms with 16 bins,
  // 244 with 32, 245 with 64, 250 with 128 (MI355X, headline workload; profiles/r05/sort_numajor.txt).
  bool sort_numajor = true;
  int sort_cellshift = 0;  // ARTIS_AMD_SORT_CELLSHIFT (with the frequency bin as the major part only)
  bool sort_ma = true;
  // lists with more entries per cell of the tile than this are not sorted (sort_by_key) unless the kernel accumulates its
  // per-cell estimators in LDS; measured crossover of the thermal lists with 1e7 packets: between 20^3 and 30^3 cells
  // (1 250 / 370 per cell). ARTIS_AMD_SORT_MAXPC_R / _T.
  // 512 < cells <= 3072: k_rpkt keeps J / nuJ / ffheating in LDS instead of the continuum table (12^3 grid, 912 cells:
  // k_rpkt 292 -> 215 ms; 14^3, 1472 cells: 249 -> 225 ms). ARTIS_AMD_RPKT_EST_OVER_CONT=0: the table wins the LDS.
  bool rpkt_est_over_cont = true;
  int ma_bins = SORT_MABINS;    // the thermal list sorted by (cell, a hash of the macro-atom's ion) instead of by cell alone: the lanes of a wave
                                // start in the records of one or two ions (ARTIS_AMD_MABINS=1: by cell; step 1060 -> ~1050 ms)
  bool ma_filters = true;       // macro-atom transitions decided on the records' 15-bit filters (ARTIS_AMD_MAFILTERS=0: on the f64 values)
  int dense_lpr = 32;           // k_bfest_dense: lanes per record (64 = a wave per record; ARTIS_AMD_DENSE_LPR)
  bool dense_cont_lds = true;   // k_bfest_dense reads the continuum table from LDS (nltenebular step 1917 -> 1882 ms); ARTIS_AMD_DENSE_CONTLDS=0
  bool cellest_in_lds = true;  // ARTIS_AMD_CELLEST_LDS=0: every estimator add is a global atomic
  bool estcache = true;        // ARTIS_AMD_ESTCACHE=0: k_rpkt without its waves' caches of per-cell accumulators (physics.h Env::estcache)
  int sort_maxpc_r = 20000;
  int sort_maxpc_t = 600;
  // one list chunk per wave instead of one per XCD (work_pull.h pull): measured on MI355X, 1e7 packets: k_rpkt -4 %
  // (a wave's lanes share continuum windows and line ranges), k_thermal +30 % (every wave then has its own cells in
  // flight and the L2 working set of macro-atom records triples)
  bool wave_chunks_r = true, wave_chunks_t = false;
  bool cu_chunks_t = false;  // ARTIS_AMD_CUCHUNKS_T=1: k_thermal takes one list chunk per compute unit (HW_REG_HW_ID);
                             // measured +7 %: like every finer chunking it puts more cells in flight per XCD
  bool cont_lds = true;      // k_rpkt keeps the static continuum table (ContPack) in LDS when it fits (ARTIS_AMD_CONTLDS=0: HBM)
  bool line_lds = false;     // ARTIS_AMD_LINELDS=1: the line list's frequencies in LDS instead (k_rpkt<false, .., true>; measured slower)
  int thermal_blocks_per_cu = ARTIS_THERMAL_WAVES;  // tuning: resident k_thermal blocks per CU
  bool thermal_refill = false;  // ARTIS_AMD_REFILL=1: k_thermal_q (walk contexts in per-wave LDS slots, lanes refilled inside the transition loop)
  int tq_low = 48;              // ... its low-water mark of walking lanes (ARTIS_AMD_TQ_LOW)
  bool tq_attr_set = false;     // ... its dynamic-LDS attribute has been set on this engine's device
  bool ma_tables_lds = true;  // k_thermal<1024, true>: the static target tables in LDS when they fit (ARTIS_AMD_MATABLES_LDS=0: in HBM)
  bool trace = false;
  uint32_t *d_visit_counts = nullptr;  // -DARTIS_VISIT_COUNTS builds: [cell][level] transitions drawn per record in the last call
  // ABSENT IONS (tables.h; EngineConfig::ma_absent_eps >= 0): [resident row][nions] the ions whose static records the last population of the row left
  // out, and the two counters behind artis_amd_last_absent_records(): records left out by the last population | filled on demand in the last call
  uint8_t *d_ion_absent = nullptr;
  double *d_ion_popsum = nullptr;  // k_ion_absent's scratch, [resident row][nions]
  unsigned long long *d_absent_counts = nullptr;
  int64_t last_absent_skipped = 0, last_absent_filled = 0;
  ncclComm_t comm = nullptr;  // created by artis_amd_comm_init(), owned by the engine
};

// The configuration of an engine, resolved once (engine_config.h resolve_config: struct field, else ARTIS_AMD_* variable, else default) into e->cfg, which
// the sizing code reads, and into the driver's fields. Called by artis_amd_engine_create_ex before anything is sized; no other place reads these variables.
static void apply_config(artis_amd_engine *e, const artis_amd_config &checked) {
  e->cfg = resolve_config(checked);
  if (e->cfg.tail_given) e->tail_max = e->cfg.tail_threshold;
  if (ARTIS_OPT_VPKT_ON) e->tail_max = 0;  // (see the estimator block: the event queue is sized per split launch)
  if (e->cfg.park_given) e->park_at = e->cfg.tile_park_at;
  if (e->cfg.bulk_given) e->budget_t_bulk = e->cfg.budget_t_bulk;
  // ABSENT IONS: off by default in the builds with non-thermal ionisation (the nebular family) -- their macro-atoms reach sparsely populated ions
  // through the non-thermal channels, 3.1e5 fills per headline step at eps = 1e-12, and the step is 27 ms longer (profiles/r12/absent_ions.md);
  // ARTIS_AMD_MA_ABSENT_EPS turns it on
  if (ARTIS_OPT_NT_ON && e->cfg.src_absent == CONFIG_DEFAULT) e->cfg.ma_absent_eps = -1.;
}
static void trace_config(const artis_amd_engine *e) {
  const EngineConfig &c = e->cfg;
  fprintf(stderr,
          "[artis_amd] configuration: cache_budget_bytes %.0f (%s), cache_headroom_bytes %.0f (%s), pop_scratch_bytes %.0f (%s), ma_hot_fraction %.3f (%s), "
          "ma_pool_fraction %.3f (%s), tail_threshold %d (%s), tile_park_at %lld (%s), keep_line_dpop %d (%s)\n",
          e->cache_budget, c.budget_given ? config_source_name(c.src_budget) : "default: automatic", c.cache_headroom, config_source_name(c.src_headroom),
          c.pop_scratch, config_source_name(c.src_scratch), e->ma_hotfrac, c.hot_given ? config_source_name(c.src_hot) : "default: automatic", c.ma_pool,
          config_source_name(c.src_pool), e->tail_max, config_source_name(c.src_tail), (long long)e->park_at, config_source_name(c.src_park),
          e->Mh.ndpop > 0 ? 1 : 0, c.keep_line_dpop >= 0 ? config_source_name(c.src_dpop) : "default: automatic");
  fprintf(stderr, "[artis_amd] absent ions: ARTIS_AMD_MA_ABSENT_EPS %g (%s)%s\n", c.ma_absent_eps, config_source_name(c.src_absent),
          e->d_ion_absent != nullptr ? "" : ": every static record is populated");
}

// The experiment switches (ARTIS_AMD_*: kernel forms, sorts, chunking) of the fields above (engine_fill). Order: BUDGET before _R / _T, SORT_CELLSHIFT after SORT_NUMAJOR.
static void read_switches(artis_amd_engine *e) {
  if (const char *b = std::getenv("ARTIS_AMD_BUDGET")) {  // tuning / tests: launch budgets never change results
    e->budget_r = std::max(1, std::atoi(b));
    e->budget_t = std::max(1, std::atoi(b));
    e->budget_g = e->budget_r * 8;
  }
  if (const char *b = std::getenv("ARTIS_AMD_BUDGET_R")) e->budget_r = std::max(1, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_BUDGET_T")) e->budget_t = std::max(1, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_SMALL_LIST")) e->small_list = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_BUDGET_T_SMALL")) e->budget_t_small = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_BUDGET_R_SMALL")) e->budget_r_small = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_DRAIN_T")) e->drain_t = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_DRAIN_R")) e->drain_r = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_DRAIN_MIN")) e->drain_min_list = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_SLOTSORT")) e->slot_order_by_cell = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_BFDEFER")) e->bf_defer = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT")) e->sort_lists = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT_NU")) e->sort_nu = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT_MA")) e->sort_ma = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_TAIL_ALWAYS")) e->tail_always = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_LATE")) e->late_max = std::max<int64_t>(0, std::atoll(b));
  if (const char *b = std::getenv("ARTIS_AMD_LATE_ALWAYS")) e->late_always = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_LATE_STRICT")) e->late_strict = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_RPKT_EST_OVER_CONT")) e->rpkt_est_over_cont = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_DENSE_CONTLDS")) e->dense_cont_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_MABINS")) e->ma_bins = (std::atoi(b) > 1) ? SORT_MABINS : 1;
  if (const char *b = std::getenv("ARTIS_AMD_MAFILTERS")) e->ma_filters = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_DENSE_LPR")) e->dense_lpr = (std::atoi(b) == 64) ? 64 : (std::atoi(b) == 16 ? 16 : 32);
  if (const char *b = std::getenv("ARTIS_AMD_CELLEST_LDS")) e->cellest_in_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_ESTCACHE")) e->estcache = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT_MAXPC_R")) e->sort_maxpc_r = std::max(1, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_SORT_MAXPC_T")) e->sort_maxpc_t = std::max(1, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_WAVECHUNKS_R")) e->wave_chunks_r = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_WAVECHUNKS_T")) e->wave_chunks_t = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_CUCHUNKS_T")) e->cu_chunks_t = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_CONTLDS")) e->cont_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_LINELDS")) e->line_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_TILE_ZIGZAG")) e->tile_zigzag = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_TILE_ADAPT")) e->cc.tile_adapt = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_TILE_BLOCK")) e->cc.tile_block = std::max<int64_t>(0, std::atoll(b));
  if (const char *b = std::getenv("ARTIS_AMD_POOL_KEEP")) e->cc.pool_keep = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_MATABLES_LDS")) e->ma_tables_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_REFILL")) e->thermal_refill = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT_NUMAJOR")) e->sort_numajor = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT_CELLSHIFT")) e->sort_cellshift = e->sort_numajor ? std::max(0, std::min(20, std::atoi(b))) : 0;
  if (const char *b = std::getenv("ARTIS_AMD_TQ_LOW")) e->tq_low = std::max(1, std::min(64, std::atoi(b)));
  if (const char *b = std::getenv("ARTIS_AMD_SPARSE_FILL")) e->cc.sparse_fill = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SPARSE_MAX")) e->cc.sparse_max_listed = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_THERMAL_BLOCKS")) e->thermal_blocks_per_cu = std::max(1, std::min(ARTIS_THERMAL_WAVES, std::atoi(b)));
  e->trace = std::getenv("ARTIS_AMD_TRACE") != nullptr;
  if (const char *b = std::getenv("ARTIS_AMD_VPKT_CONTLDS")) e->vpkt_cont_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_TILE_PARK")) e->park_tails = std::atoi(b) != 0;
}

namespace {

template <typename T>
int upload_array(std::vector<void *> &allocs, const T *host, int64_t count, const T **dev_out) {
  T *d = nullptr;
  const size_t bytes = sizeof(T) * (size_t)(count > 0 ? count : 1);
  HIP_TRY(hipMalloc((void **)&d, bytes));
  allocs.push_back(d);
  if (count > 0) HIP_TRY(hipMemcpy(d, host, sizeof(T) * (size_t)count, hipMemcpyHostToDevice));
  *dev_out = d;
  return ARTIS_OK;
}

int free_all(std::vector<void *> &v) {
  for (void *p : v) (void)hipFree(p);
  v.clear();
  return ARTIS_OK;
}

Env make_env(const artis_amd_engine *e) {
  Env env;
  std::memset(&env, 0, sizeof(env));
  env.M = e->M;
  env.C = e->C;
  env.K = e->K;
  {
    const DevModel &h = e->Mh;
    if (h.ndpop == 0) env.K.line_dpop = nullptr;  // formed on the fly (physics.h line_dpop_at)
    // the pool of on-demand records is one for all resident cells (tables.h "ON-DEMAND RECORDS"): not indexed by cell
    env.ma_pool_cap = (uint32_t)std::min<int64_t>(((int64_t)e->cc.res.tile_cells * h.ma_pool_slots) / MAPOOL_UNIT, 0x7FFFFFF0LL);
    env.ma_pool_full = e->d_count + (2 * NEXT_NKINDS - 1);  // (a spare slot of the counts the host reads after every launch)
  }
  // rows: one per cell (row = cell), or -- a cache that does not fit -- the rows of the cells that are resident now (make_resident())
  env.krow_tab = e->cc.ntiles > 1 ? e->cc.d_krow : nullptr;
  env.tile_all = e->cc.ntiles > 1 ? 0 : 1;
  env.tile_lo = 0;
  env.tile_hi = e->Mh.npts_nonempty;
  env.fill_cells = nullptr;  // (set by populate_tile() of a tiled cache for its own launches)
  env.nfill = 0;
  env.collexc_terms = e->cc.d_collexc_terms;
  {  // few cells: per-cell estimators accumulate in LDS (physics.h Env::cellest_lds)
    const int nc = e->Mh.npts_nonempty;
    env.cellest_n_t = (e->cellest_in_lds && nc <= THERMAL_CELLEST_CAP) ? nc : 0;
    // between the two caps k_rpkt runs without the continuum table in LDS and keeps the estimators there instead
    env.cellest_n_r = (e->cellest_in_lds && nc <= (e->rpkt_est_over_cont ? RPKT_CELLEST_CAP_NOCONT : RPKT_CELLEST_CAP)) ? nc : 0;
    env.cellest_n_g = (e->cellest_in_lds && nc <= GAMMA_CELLEST_CAP) ? nc : 0;
    env.scalars_in_lds = e->cellest_in_lds ? 1 : 0;
    env.estcache_on = e->estcache ? 1 : 0;
    env.ma_filters_off = e->ma_filters ? 0 : 1;
  }
  env.S = e->S;
  env.E = e->E;
  env.est_stride = 8;
  env.pair_stride = 2;
  env.P = e->P;
  env.stats = nullptr;
  env.gamma_ws = e->d_gamma_ws;
  env.bfev = e->bf_defer ? e->d_bfev : nullptr;
  env.bfev_count = e->d_bfev_count;
  env.bfev_cap = e->bfev_cap;
  env.bfrate_kept = (e->bf_defer && e->cc.ntiles == 1) ? e->d_bfrate_kept : nullptr;
  env.gamma_gi = e->d_gamma_gi;
  env.gamma_n = e->d_gamma_n;
  env.errflag = e->d_err;
  env.vpkt_queue = e->d_vpkt_queue;
  env.vpkt_count = e->d_vpkt_count;
  env.vpkt_cap = e->vpkt_cap;
#ifdef ARTIS_VISIT_COUNTS
  env.visit_counts = e->d_visit_counts;
#endif
  env.ion_absent = e->d_ion_absent;
  env.ion_popsum = e->d_ion_popsum;
  env.ma_absent_counts = e->d_absent_counts;
  env.ma_absent_eps = e->cfg.ma_absent_eps;
  return env;
}

void sort_scratch_free(SortScratch &S) {
  if (S.base) (void)hipFree(S.base);
  S = SortScratch{};
}
int sort_scratch_alloc(SortScratch &S, int64_t n) {
  sort_scratch_free(S);
  const size_t cap = (size_t)(n > 0 ? n : 1);
  const size_t matlen = (size_t)SORT_HI_MAX * ((cap + SORT_TILE - 1) / SORT_TILE);
  auto padded = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
  const size_t b_pairs = padded(sizeof(int2) * cap), b_mat = padded(sizeof(int32_t) * matlen), b_tiles = padded(sizeof(int32_t) * (matlen / SCAN_TILE + 2)),
               b_seg = padded(sizeof(int32_t) * (SORT_HI_MAX + 1));
  HIP_TRY(hipMalloc(&S.base, b_pairs + b_mat + b_tiles + 2 * b_seg));
  char *q = (char *)S.base;
  S.pairs = (int2 *)q;
  S.mat = (int32_t *)(q += b_pairs);
  S.tiles = (int32_t *)(q += b_mat);
  S.seg = (int32_t *)(q += b_tiles);
  S.chunk_base = (int32_t *)(q += b_seg);
  S.capacity = (int64_t)cap;
  return ARTIS_OK;
}
std::string sort_too_many_keys_text(int64_t nkeys) {
  return "the work-list sort takes at most " + std::to_string(SORT_MAX_KEYS) + " keys (cells x bins), this list has " + std::to_string(nkeys) +
         ": run without sorted lists (ARTIS_AMD_SORT=0)";
}
// the many-keys sort (the kernels' comment): list[0..n) by keys[] (each in [0, nkeys)) into out[0..n); n <= S.capacity
int sort_many_keys(artis_amd_engine *e, const SortScratch &S, hipStream_t s, const int32_t *list, const int32_t *keys, int32_t n, int64_t nkeys,
                   int32_t *out) {
  if (nkeys > SORT_MAX_KEYS) {
    g_last_error = sort_too_many_keys_text(nkeys);
    return ARTIS_ERR_UNSUPPORTED;
  }
  if (n <= 0 || n > S.capacity) {
    g_last_error = "sort: the list does not fit the sort's buffers";
    return ARTIS_ERR_ARG;
  }
  int keybits = 0;
  while (((int64_t)1 << keybits) < nkeys) keybits++;
  const int lobits = std::max(0, keybits - SORT_HI_BITS);
  const int nb = (int)((nkeys - 1) >> lobits) + 1;
  const int32_t ntiles = (int32_t)(((int64_t)n + SORT_TILE - 1) / SORT_TILE);
  const int32_t matlen = nb * ntiles;
  const int nscan = (matlen + SCAN_TILE - 1) / SCAN_TILE;
  const size_t lds = sizeof(int32_t) * 2 * ((size_t)1 << lobits);
  if (lds > 32 * 1024 && !e->sort_attr_set) {
    HIP_TRY(hipFuncSetAttribute((const void *)k_sort_segments, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(int32_t) * 2 << SORT_LO_BITS_MAX)));
    e->sort_attr_set = true;
  }
  hipLaunchKernelGGL(k_sort_tilehist, dim3(ntiles), dim3(SORT_TB), 0, s, keys, n, lobits, nb, ntiles, S.mat);
  hipLaunchKernelGGL(k_scan_tiles, dim3(nscan), dim3(1024), 0, s, S.mat, matlen, S.tiles);
  if (nscan > 1) {
    hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(1024), 0, s, S.tiles, nscan);
    hipLaunchKernelGGL(k_scan_add, dim3(nscan), dim3(1024), 0, s, S.mat, matlen, S.tiles);
  }
  hipLaunchKernelGGL(k_sort_tilescatter, dim3(ntiles), dim3(SORT_TB), 0, s, list, keys, n, lobits, nb, ntiles, S.mat, S.pairs);
  hipLaunchKernelGGL(k_sort_plan, dim3(1), dim3(1024), 0, s, S.mat, ntiles, nb, n, S.seg, S.chunk_base);
  hipLaunchKernelGGL(k_sort_segments, dim3(n / SORT_SEG_CAP + nb), dim3(BLOCK), lds, s, S.pairs, lobits, nb, S.seg, S.chunk_base, out);
  return ARTIS_OK;
}
// counting sort of list[0..n) by keys[] into out[0..n): in LDS-sized histograms for few keys, the two-pass sort for many
int sort_list(artis_amd_engine *e, hipStream_t s, const int32_t *list, const int32_t *keys, int32_t n, int64_t nkeys, int32_t *out) {
  if (nkeys > SORT_LDS_KEYS) return sort_many_keys(e, e->sort_scratch, s, list, keys, n, nkeys, out);
  const int32_t nk = (int32_t)nkeys;
  HIP_TRY(hipMemsetAsync(e->d_hist, 0, sizeof(int32_t) * (size_t)(nk + 1), s));
  hipLaunchKernelGGL(k_sort_hist_lds, dim3(sort_lds_grid(n)), dim3(BLOCK), 0, s, keys, n, e->d_hist, nk);
  const int ntiles = (nk + SCAN_TILE - 1) / SCAN_TILE;
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(1024), 0, s, e->d_hist, nk, e->d_tiles);
  hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(1024), 0, s, e->d_tiles, ntiles);
  hipLaunchKernelGGL(k_scan_add, dim3(ntiles), dim3(1024), 0, s, e->d_hist, nk, e->d_tiles);
  hipLaunchKernelGGL(k_sort_scatter_lds, dim3(sort_lds_grid(n)), dim3(BLOCK), 0, s, list, keys, n, e->d_hist, out, nk);
  return ARTIS_OK;
}

void free_packet_buffers(artis_amd_engine *e) {
  void **singles[] = {&e->d_pkt, &e->d_pkt_snapshot, (void **)&e->d_sorted, (void **)&e->d_perm, (void **)&e->d_gamma_ws,
                      (void **)&e->d_late_ring[0], (void **)&e->d_late_ring[1], (void **)&e->d_late_ring[2],
                      (void **)&e->d_gamma_gi, (void **)&e->d_gamma_n, (void **)&e->d_bfev, (void **)&e->d_bfev_count,
                      (void **)&e->d_vpkt_queue, (void **)&e->d_vpkt_count};
  e->bfev_cap = 0;
  e->vpkt_cap = 0;
  sort_scratch_free(e->sort_scratch);
  for (void **q : singles) {
    if (*q) (void)hipFree(*q);
    *q = nullptr;
  }
  for (int kind = 0; kind < NEXT_NKINDS; kind++)
    for (int k = 0; k < 2; k++) {
      if (e->d_lists[kind][k]) (void)hipFree(e->d_lists[kind][k]);
      if (e->d_keys[kind][k]) (void)hipFree(e->d_keys[kind][k]);
      e->d_lists[kind][k] = nullptr;
      e->d_keys[kind][k] = nullptr;
    }
  e->npackets = -1;  // nothing resident
  e->use_perm = false;
}

// k_late may take the end of this engine's populations: a build with the kernel, k_tail allowed (no virtual packets, no deferred bound-free
// events), the whole cache resident, no cold levels, and tables that fit the LDS
bool late_possible(const artis_amd_engine *e) {
  return ARTIS_LATE_KERNEL && e->late_max > 0 && e->tail_max > 0 && e->cc.ntiles == 1 && e->Mh.ncold == 0 && e->Mh.nlevels > 0 && e->Mh.nlevels < 32768 &&
         e->Mh.nalltrans > 0 && e->Mh.nbfcontinua > 0 && late_lds_bytes(e->Mh.nlevels, e->Mh.nalltrans, e->Mh.nbfcontinua) <= 160 * 1024 - 1024;
}
int ensure_packet_buffers(artis_amd_engine *e, int64_t n) {
  if (n == e->npackets && e->d_pkt) return ARTIS_OK;
  free_packet_buffers(e);
  e->pkt_bytes = pkt_store_bytes(n);
  HIP_TRY(hipMalloc(&e->d_pkt, e->pkt_bytes));
  e->P = carve_pkt_store(e->d_pkt, n);
  const size_t listbytes = sizeof(int32_t) * (size_t)(n > 0 ? n : 1);
  for (int kind = 1; kind < NEXT_NKINDS; kind++)
    for (int k = 0; k < 2; k++) {
      HIP_TRY(hipMalloc((void **)&e->d_lists[kind][k], listbytes));
      HIP_TRY(hipMalloc((void **)&e->d_keys[kind][k], listbytes));
    }
  HIP_TRY(hipMalloc((void **)&e->d_sorted, listbytes));
  HIP_TRY(hipMalloc((void **)&e->d_perm, listbytes));
  if (late_possible(e)) {  // (120 MB at 1e7 packets: only for an engine that can launch k_late)
    for (int k = 0; k < LATE_NQ; k++) HIP_TRY(hipMalloc((void **)&e->d_late_ring[k], listbytes));
  }
  if (const int rc = sort_scratch_alloc(e->sort_scratch, n)) return rc;
  e->ws_capacity = n > 0 ? n : 1;
  const size_t wsbytes = sizeof(double) * (size_t)(e->Mh.nbfcontinua_ground + 1) * (size_t)e->ws_capacity;
  HIP_TRY(hipMalloc((void **)&e->d_gamma_ws, wsbytes));
  HIP_TRY(hipMalloc((void **)&e->d_gamma_gi, wsbytes / 2));
  HIP_TRY(hipMalloc((void **)&e->d_gamma_n, sizeof(int32_t) * (size_t)e->ws_capacity));
  HIP_TRY(hipMemset(e->d_gamma_n, 0, sizeof(int32_t) * (size_t)e->ws_capacity));
#if ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON
  if (e->Mh.nbfcontinua > 0) {  // one k_rpkt launch records at most budget_r updates per packet on its list
    const int64_t cap = std::min<int64_t>((int64_t)(n > 0 ? n : 1) * e->budget_r, 0x7FFFFFF0LL);
    HIP_TRY(hipMalloc((void **)&e->d_bfev, sizeof(BfEvent) * (size_t)cap));
    HIP_TRY(hipMalloc((void **)&e->d_bfev_count, sizeof(int32_t)));
    HIP_TRY(hipMemset(e->d_bfev_count, 0, sizeof(int32_t)));
    e->bfev_cap = (int32_t)cap;
  }
#endif
#if ARTIS_OPT_VPKT_ON
  {
    const int64_t cap = std::min<int64_t>((int64_t)(n > 0 ? n : 1) * std::max(e->budget_r, 1), 0x7FFFFFF0LL);
    HIP_TRY(hipMalloc((void **)&e->d_vpkt_queue, sizeof(VpktSeed) * (size_t)cap));
    HIP_TRY(hipMalloc((void **)&e->d_vpkt_count, sizeof(int32_t)));
    HIP_TRY(hipMemset(e->d_vpkt_count, 0, sizeof(int32_t)));
    e->vpkt_cap = (int32_t)cap;
  }
#endif
  e->npackets = n;  // committed only now: a failed allocation above leaves "nothing resident" (npackets == -1)
  return ARTIS_OK;
}

int ensure_aos(artis_amd_engine *e, int64_t n) {
  if (n <= e->aos_capacity && e->d_aos) return ARTIS_OK;
  if (e->d_aos) (void)hipFree(e->d_aos);
  e->d_aos = nullptr;
  e->aos_valid = false;
  HIP_TRY(hipMalloc((void **)&e->d_aos, sizeof(artis_packet) * (size_t)(n > 0 ? n : 1)));
  e->aos_capacity = n;
  return ARTIS_OK;
}

// The npackets structs in d_aos become the resident population (buffers made by ensure_packet_buffers / ensure_aos): slots in the order of
// the packets' cells, records from the structs. What artis_amd_packets_upload does after its copy, and artis_amd_packet_init after its kernels.
int install_resident_aos(artis_amd_engine *e, int64_t npackets) {
  // a snapshot belongs to the population (and slot permutation) it was taken of
  if (e->d_pkt_snapshot) (void)hipFree(e->d_pkt_snapshot);
  e->d_pkt_snapshot = nullptr;
  if (npackets > 0) {
    e->aos_valid = true;
    e->use_perm = false;
    if (e->slot_order_by_cell && e->sort_lists && npackets >= 2 * BLOCK) {
      // counting sort of the packet indices by propagation cell (the work-list sort kernels; the lists are free now)
      int32_t *ident = e->d_lists[NEXT_RPKT][0], *keys = e->d_lists[NEXT_RPKT][1];
      const int32_t n32 = (int32_t)npackets;
      const int32_t nkeys = e->Mh.ngrid;
      hipStream_t s = nullptr;
      hipLaunchKernelGGL(k_aos_cellkeys, dim3(nblocks(npackets)), dim3(BLOCK), 0, s, e->d_aos, npackets, nkeys, ident, keys);
      if (const int rc2 = sort_list(e, s, ident, keys, n32, nkeys, e->d_perm)) return rc2;
      e->use_perm = true;
    }
    hipLaunchKernelGGL(k_aos_to_rec, dim3(nblocks(npackets)), dim3(BLOCK), 0, nullptr, e->d_aos, e->P, e->use_perm ? e->d_perm : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  return ARTIS_OK;
}

}  // namespace

namespace {
int engine_fill(artis_amd_engine *e, const artis_model *model);

// ---- sizing: the layout decisions of an engine, as pure functions of the model, the resolved configuration (engine_config.h) and the free device
// memory. engine_fill() builds what they say; artis_amd_engine_plan() reports it without building anything.

// bytes of one cell's cache row
size_t cache_row_bytes(const DevModel &h) {
  size_t per_cell = 0;
#define SZ(f, T, per) per_cell += sizeof(T) * (size_t)(per);
  ARTIS_CACHE_ARRAYS(SZ, h)
#undef SZ
  return per_cell;
}

// Macro-atom record tiers (tables.h "ON-DEMAND RECORDS"): every level a static record while the whole cell cache fits one tile; when it
// does not (even without line_dpop), static records for the lowest share of every ion's levels and a pool of ma_pool_fraction (0.15) of the rest for
// the cold levels packets reach. A given hot share (artis_amd_config.ma_hot_fraction, ARTIS_AMD_MA_HOTFRAC) is taken as it is; free_b is read only without one.
// (pool share: 0.25 in round 5. Measured on the 4e5-line set, 50^3 / 1e7, round 6 -- artis_amd_last_pool_usage(): a step leaves 48 % of a quarter-share
// pool in use; with 0.15 the tier search affords hot 0.25 instead of 0.15 and the step takes 15.9 s instead of 16.6 (pool 64 % used); with 0.10 hot 0.30,
// 15.7 s, 87 % used -- too close to a pool that is used up and emptied. profiles/r06/pool_share.txt)
void choose_record_tiers(const artis_model &model, ModelOwned &own, const EngineConfig &cfg, double free_b, DevModel *Mh, double *hotfrac) {
  const double hot = cfg.hot_given ? cfg.ma_hot : 1., pool = cfg.ma_pool;
  *Mh = make_host_model_view(model, own, hot, pool);
  *hotfrac = hot;
  if (cfg.hot_given) return;
  auto tiles_needed = [&]() -> int64_t {
    size_t per_cell = cache_row_bytes(*Mh);
    per_cell -= sizeof(double) * (size_t)Mh->ndpop;  // (dropped first when the cache does not fit: plan_cache_rows)
    const int64_t fit = std::max<int64_t>(1, (int64_t)(cache_budget_bytes(cfg, free_b) / (double)(per_cell > 0 ? per_cell : 1)));
    return (model.npts_nonempty + fit - 1) / fit;
  };
  // The largest hot share that lets the whole cache be resident (the fewer cold levels, the fewer first visits pay a fill). If none does, the
  // cache is tiled, and the share is the largest one that needs the FEWEST tiles: smaller rows, more cells resident at a time (round 6; the headline
  // forced to a quarter of its cache: 1875 ms with four tiles of static rows, 1532 ms with two tiles of rows with a quarter of the levels hot --
  // profiles/r06/tiling.md. Round 5 kept the rows static in that case: every refill of a tile emptied the pool then, and a tiled run on on-demand
  // records paid its fills again and again, 3.7 s against 3.0 s; now a fill leaves the pool and the rows of the cells that stay alone.)
  // (round 6: in steps of 0.05 below one half -- with the round-5 steps 0.5 / 0.3 / 0.2 / 0.1 a record that grew by a quarter, the fine bytes, sent
  // the 4e5-line set from 0.2 to 0.1 and doubled its fills)
  // (the fewest tiles among the shares >= 0.2: a tile saved by going lower costs more in cold levels filled on demand than the tile did -- at 11600 MB
  // two tiles at hot 0.10 take 1750 ms, three at 0.5 1620; a cache that fits ONE tile at a lower share takes that: one tile beats any tiling)
  int64_t best_nt = tiles_needed(), tiled_nt = best_nt;
  double best_h = 1., cur_h = 1., tiled_h = 1.;
  for (const double h : {0.9, 0.8, 0.7, 0.6, 0.5, 0.45, 0.4, 0.35, 0.3, 0.25, 0.2, 0.15, 0.1, 0.05}) {
    if (best_nt <= 1) break;
    *Mh = make_host_model_view(model, own, h, pool);
    cur_h = h;
    const int64_t nt = tiles_needed();
    if (nt < best_nt) {
      best_nt = nt;
      best_h = h;
    }
    if (h > 0.199 && nt < tiled_nt) {
      tiled_nt = nt;
      tiled_h = h;
    }
  }
  if (best_nt > 1) best_h = tiled_h;
  if (cur_h != best_h) *Mh = make_host_model_view(model, own, best_h, pool);
  *hotfrac = best_h;
}

// The rows of the cell cache: all cells if that fits the budget, else one tile of cells at a time. free_b: the free device memory once the model's
// tables are resident (read by the automatic budget only).
struct CacheLayout {
  double budget = 0.;      // [B] what the rows may take
  size_t per_cell = 0;     // [B] one row
  int64_t tile_cells = 1;  // rows
  int ntiles = 1;
  bool drop_dpop = false;  // the rows are without line_dpop (the caller sets ndpop = 0)
};
int plan_cache_rows(const DevModel &h, const EngineConfig &cfg, double free_b, CacheLayout *L) {
  const int64_t ncell_all = h.npts_nonempty;
  size_t per_cell = cache_row_bytes(h);
  const double budget = cache_budget_bytes(cfg, free_b);
  {
    // The rows of line_dpop (8 bytes per line and cell: 0.9 of the 3.2 MB of a row with 110 860 lines) are dropped when the cell
    // cache does not fit one tile with them and needs fewer tiles without: the line walk then forms a line's population factor from
    // its record and the two level populations (physics.h line_dpop_at: the same expression, the same bits; two more reads per
    // line visited). artis_amd_config.keep_line_dpop (ARTIS_AMD_DPOP) = 0 / 1 forces either.
    const size_t per_without = per_cell - (sizeof(double) * (size_t)h.ndpop);
    auto tiles_of = [&](size_t per) {
      const int64_t fit = std::max<int64_t>(1, (int64_t)(budget / (double)(per > 0 ? per : 1)));
      return (ncell_all + fit - 1) / fit;
    };
    bool drop = tiles_of(per_cell) > 1 && tiles_of(per_without) < tiles_of(per_cell);
    if (cfg.keep_line_dpop >= 0) drop = cfg.keep_line_dpop == 0;
    if (cfg.dpop_strict && h.ndpop > 0 && (double)per_cell > budget) {
      g_last_error = "artis_amd_config.keep_line_dpop = 1, and the cache budget (" + std::to_string((long long)budget) + " B) cannot hold a row with line_dpop (" +
                     std::to_string(per_cell) + " B; " + std::to_string(per_without) + " B without)";
      return ARTIS_ERR_ARG;
    }
    L->drop_dpop = drop && h.ndpop > 0;
    if (L->drop_dpop) per_cell = per_without;
  }
  L->budget = budget;
  L->per_cell = per_cell;
  const int64_t fit = (int64_t)(budget / (double)(per_cell > 0 ? per_cell : 1));
  if (fit < 1 && cfg.budget_given && cfg.src_budget == CONFIG_STRUCT) {  // (a budget from the variable or from the automatic rule gets one row at a time, as ever)
    g_last_error = "artis_amd_config.cache_budget_bytes (" + std::to_string((long long)budget) + ") cannot hold one row of the cell cache (" + std::to_string(per_cell) + " B)";
    return ARTIS_ERR_ARG;
  }
  L->tile_cells = std::max<int64_t>(1, std::min<int64_t>(ncell_all > 0 ? ncell_all : 1, fit));
  L->ntiles = (int)((ncell_all + L->tile_cells - 1) / L->tile_cells);
  if (L->ntiles < 1) L->ntiles = 1;
  if (ARTIS_OPT_VPKT_ON && L->ntiles > 1) {
    // a virtual packet's ray reads the cache rows of every cell up to the grid's edge (vpkt.cc:183): all of them have to be resident
    g_last_error = "this build has VPKT_ON and the cell cache does not fit one tile (" + std::to_string(per_cell) + " B per cell x " +
                   std::to_string((long long)ncell_all) + " cells): virtual packets need every cell's row resident";
    return ARTIS_ERR_UNSUPPORTED;
  }
  return ARTIS_OK;
}

// the population works through the cells in batches whose cooling terms fit its scratch (artis_amd_config.pop_scratch_bytes: ~2 GB), allocated after the
// cache rows: cells per batch, and the bytes of the scratch
int64_t pop_batch_cells(const DevModel &h, int64_t tile_cells, const EngineConfig &cfg) {
  const int64_t per = std::max<int64_t>(1, (int64_t)h.nupcum) * (int64_t)sizeof(double);
  return std::max<int64_t>(1, std::min<int64_t>(tile_cells, (int64_t)cfg.pop_scratch / per));
}
size_t pop_scratch_alloc_bytes(const DevModel &h, int64_t batch) {
  return (size_t)(batch * std::max<int64_t>(1, (int64_t)h.nupcum) * (int64_t)sizeof(double)) + 64;
}

// bytes of the model's tables on the device (what engine_fill uploads before it sizes the cache: upload_array's sizes)
int64_t model_table_bytes(const DevModel &h) {
  int64_t bytes = 0;
#define SZ(f, T, count) bytes += (int64_t)sizeof(T) * std::max<int64_t>(1, (int64_t)(count));
  ARTIS_MODEL_ARRAYS(SZ, h)
#undef SZ
#define SZO(f, T, count) \
  if (h.f) bytes += (int64_t)sizeof(T) * std::max<int64_t>(1, (int64_t)(count));
  ARTIS_MODEL_OPTIONAL_ARRAYS(SZO, h)
#undef SZO
  const int ndim = (h.gridtype == ARTIS_GRID_SPHERICAL1D) ? 1 : ((h.gridtype == ARTIS_GRID_CYLINDRICAL2D) ? 2 : 3);
  for (int a = 0; a < 3; a++) bytes += (int64_t)sizeof(double) * std::max<int64_t>(1, (a >= ndim) ? 1 : h.ncoordgrid[a]);
  bytes += (int64_t)sizeof(int32_t) * std::max<int64_t>(1, h.nphixstargets_total);  // the target -> level table
  return bytes;
}

// RCCL entry points, resolved at run time from the librccl the process already has (a host that links RCCL itself, or
// torch's own copy in bench.py) or else from the ROCm installation: the engine library itself carries no link-time
// dependency on a particular librccl, and a communicator handed in by the caller is used with the library it came from.
struct RcclApi {
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;  // optional: artis_amd_comm_count()
  bool ok = false;
};
const RcclApi &rccl_api() {
  static RcclApi api = [] {
    RcclApi a;
    void *h = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so"}) {
      h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
      if (h) break;
    }
    if (!h)
      for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
      }
    if (!h) return a;
    a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    a.CommInitRank = (decltype(a.CommInitRank))dlsym(h, "ncclCommInitRank");
    a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
    a.AllReduce = (decltype(a.AllReduce))dlsym(h, "ncclAllReduce");
    a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
    a.CommCount = (decltype(a.CommCount))dlsym(h, "ncclCommCount");
    a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllReduce && a.GetErrorString;
    return a;
  }();
  return api;
}
#define RCCL_TRY(expr)                                                                             \
  do {                                                                                             \
    ncclResult_t _r = (expr);                                                                      \
    if (_r != ncclSuccess) {                                                                       \
      g_last_error = std::string(#expr) + ": " + rccl_api().GetErrorString(_r);                    \
      return ARTIS_ERR_RCCL;                                                                       \
    }                                                                                              \
  } while (0)
}  // namespace

extern "C" {

const char *artis_amd_last_error(void) { return g_last_error.c_str(); }
int artis_amd_abi_version(void) { return 6; }
const char *artis_amd_options_preset(void) {
#if defined(ARTIS_PRESET_NAME)  // given by the build (artis_amd/build.py): the presets of the reference's CI option sets
  return ARTIS_PRESET_NAME;
#elif defined(ARTIS_PRESET_NLTENEBULAR_LINEEST)
  return "nltenebular_lineest";
#elif defined(ARTIS_PRESET_CHRISTINENONTHERMAL)
  return "christinenonthermal";
#elif defined(ARTIS_PRESET_NLTEPHOTOSPHERIC)
  return "nltephotospheric";
#elif defined(ARTIS_PRESET_NLTEWITHOUTNONTHERMAL)
  return "nltewithoutnonthermal";
#elif defined(ARTIS_PRESET_NLTENEBULAR)
  return "nltenebular";
#elif defined(ARTIS_PRESET_KILONOVA_EXPOPAC)
  return "kilonova_expopac";
#elif defined(ARTIS_PRESET_CLASSIC_EXPOPAC_THERM)
  return "classic_expopac_therm";
#elif defined(ARTIS_PRESET_KILONOVA_GAMMA_GREY)
  return "kilonova_gamma_grey";
#elif defined(ARTIS_PRESET_CLASSIC_GAMMA_XCOM)
  return "classic_gamma_xcom";
#elif defined(ARTIS_PRESET_KILONOVA_GAMMA_BARNES)
  return "kilonova_gamma_barnes";
#elif defined(ARTIS_PRESET_KILONOVA_GAMMA_WOLLAEGER)
  return "kilonova_gamma_wollaeger";
#elif defined(ARTIS_PRESET_KILONOVA_GAMMA_GUTTMAN)
  return "kilonova_gamma_guttman";
#elif defined(ARTIS_PRESET_KILONOVA_GAMMAPRODUCTS)
  return "kilonova_gammaproducts";
#elif defined(ARTIS_PRESET_KILONOVA_BARNES)
  return "kilonova_barnes";
#elif defined(ARTIS_PRESET_KILONOVA_WOLLAEGER)
  return "kilonova_wollaeger";
#elif defined(ARTIS_PRESET_KILONOVA_LTE)
  return "kilonova_lte";
#else
  return "classic";
#endif
}
size_t artis_amd_sizeof_packet(void) { return sizeof(artis_packet); }

}  // extern "C"

namespace {
// what the engine requires of a model before anything is sized or uploaded (artis_amd_engine_create_ex, artis_amd_engine_plan)
int validate_model(const artis_model *model) {
  if (model->gridtype != ARTIS_GRID_CARTESIAN3D && model->gridtype != ARTIS_GRID_SPHERICAL1D &&
      model->gridtype != ARTIS_GRID_CYLINDRICAL2D) {
    g_last_error = "unknown grid type";
    return ARTIS_ERR_UNSUPPORTED;
  }
  // the per-packet list of ground-continuum contributions (physics.h chi_bf_gammacontr) relies on the order the
  // reference builds these tables in: groundcont_nu_edge rising (input.cc:802) and, with allcont sorted by nu_edge
  // (input.cc:892), a non-decreasing nearest-edge index (input.cc:703)
  for (int i = 1; i < model->nbfcontinua_ground; i++) {
    if (model->groundcont_nu_edge[i] < model->groundcont_nu_edge[i - 1]) {
      g_last_error = "groundcont_nu_edge is not in ascending order";
      return ARTIS_ERR_ARG;
    }
  }
  for (int i = 0, last = -1; i < model->nbfcontinua; i++) {
    const int gi = model->allcont_groundcontestimindex[i];
    if (gi < 0) continue;
    if (gi < last || gi >= model->nbfcontinua_ground) {
      g_last_error = "allcont_groundcontestimindex does not rise with nu_edge";
      return ARTIS_ERR_ARG;
    }
    last = gi;
  }
  for (int i = 0; i < model->nlevels; i++) {  // what a packed macro-atom transition target can hold (tables.h MaTarget)
    if (model->level_ndowntrans[i] >= MATGT_MAX_NTRANS || model->level_nuptrans[i] >= MATGT_MAX_NTRANS) {
      g_last_error = "a level has more transitions than a packed transition target can describe";
      return ARTIS_ERR_UNSUPPORTED;
    }
  }
  // k_cooling_tail reads what the entries of an ion's cooling list after the collisional excitations are from the list itself
  // (coolinglist_type / _level / _phixstargetindex): they must be in the order calculate_cooling_rates_ion() writes them
  // (kpkt.cc:122-190: the collisional ionisations level by level and target by target, then the bound-free terms likewise)
  for (int el = 0; el < model->nelements && model->ncoolingterms > 0; el++)
    for (int ion = 0; ion < model->elem_nions[el]; ion++) {
      const int ui = model->elem_uniqueionindexstart[el] + ion;
      int k = ((model->elem_lowest_ionstage[el] + ion - 1) > 0) ? 1 : 0;
      const int start = model->ion_uniquelevelindexstart[ui];
      for (int l = 0; l < model->ion_nlevels[ui]; l++) k += (model->level_nuptrans[start + l] > 0) ? 1 : 0;
      bool ok = true;
      if (ion < model->elem_nions[el] - 1 && model->nbfcontinua > 0) {
        const int off = model->ion_coolingoffset[ui];
        for (int pass = 0; pass < 2 && ok; pass++)
          for (int l = 0; l < model->ion_nlevels_ionising[ui] && ok; l++)
            for (int t = 0; t < model->level_nphixstargets[start + l] && ok; t++, k++)
              ok = k < model->ion_ncoolingterms[ui] && model->coolinglist_type[off + k] == (pass == 0 ? ARTIS_COOLING_COLLION : ARTIS_COOLING_FREEBOUND) &&
                   model->coolinglist_level[off + k] == l && model->coolinglist_phixstargetindex[off + k] == t;
      }
      if (!ok || k != model->ion_ncoolingterms[ui]) {
        g_last_error = "the cooling list of an ion is not in the order of calculate_cooling_rates_ion()";
        return ARTIS_ERR_ARG;
      }
    }
  {
    // alltrans is laid out level by level, downward then upward transitions, without gaps (input.cc:565): k_matrans takes a block's
    // extent from its first and last segment, ma_entry_pos() an entry's place from its offset, and the records' filter lines are
    // counted from a level's first entry
    int64_t next = 0;
    for (int ul = 0; ul < model->nlevels; ul++) {
      if (model->level_alltrans_startdown[ul] != next || model->level_ndowntrans[ul] < 0 || model->level_nuptrans[ul] < 0) {
        g_last_error = "alltrans is not contiguous in level order (level_alltrans_startdown[i+1] == startdown[i] + ndown[i] + nup[i])";
        return ARTIS_ERR_ARG;
      }
      next += (int64_t)model->level_ndowntrans[ul] + model->level_nuptrans[ul];
    }
    if (next != model->nalltrans) {
      g_last_error = "the last level's transitions do not end at nalltrans";
      return ARTIS_ERR_ARG;
    }
  }
  for (int i = 0; i < model->nions; i++) {  // DevModel::alltrans_tlevel16: a target level within its ion in 16 bits
    if (model->ion_nlevels[i] > 65535) {
      g_last_error = "an ion has more levels than a 16-bit target level can describe";
      return ARTIS_ERR_UNSUPPORTED;
    }
  }
  {  // the r-packet list's keys (cells x frequency bins) have to fit the work-list sort, unless the lists stay unsorted
    const char *b = std::getenv("ARTIS_AMD_SORT");
    const int64_t nkeys = (int64_t)model->ngrid * SORT_NUBINS;
    if (nkeys > SORT_MAX_KEYS && !(b && std::atoi(b) == 0)) {
      g_last_error = sort_too_many_keys_text(nkeys);
      return ARTIS_ERR_UNSUPPORTED;
    }
  }
  return ARTIS_OK;
}
}  // namespace

extern "C" {

size_t artis_amd_sizeof_config(void) { return sizeof(artis_amd_config); }
size_t artis_amd_sizeof_plan(void) { return sizeof(artis_amd_plan); }
void artis_amd_config_default(artis_amd_config *cfg) {
  if (cfg) config_set_default(cfg);
}

int artis_amd_engine_create(const artis_model *model, int device, artis_amd_engine **out) {
  return artis_amd_engine_create_ex(model, device, nullptr, out);
}

int artis_amd_engine_create_ex(const artis_model *model, int device, const artis_amd_config *cfg, artis_amd_engine **out) {
  if (out) *out = nullptr;
  if (!model || !out) {
    g_last_error = "null argument";
    return ARTIS_ERR_ARG;
  }
  artis_amd_config checked;  // the configuration first: a caller's mistake is reported before the device is touched
  if (const int rc = config_copy_checked(cfg, &checked, &g_last_error)) return rc;
  if (const int rc = validate_model(model)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_last_error = "no HIP device: the artis_amd engine has no CPU path";
    return ARTIS_ERR_NODEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  artis_amd_engine *e = new artis_amd_engine();
  e->device = device;
  apply_config(e, checked);
  const int rc = engine_fill(e, model);
  if (rc != ARTIS_OK) {  // release whatever was allocated before the failing call (g_last_error is already set)
    artis_amd_engine_destroy(e);
    return rc;
  }
  *out = e;
  return ARTIS_OK;
}

}  // extern "C"

namespace {
int engine_fill(artis_amd_engine *e, const artis_model *model) {
  const int device = e->device;
  {  // macro-atom record tiers (choose_record_tiers): given, or chosen from the cache budget -- then from what is free on the device now
    double free_b = 0.;
    if (!e->cfg.hot_given) {
      size_t f = 0, total_b = 0;
      HIP_TRY(hipMemGetInfo(&f, &total_b));
      free_b = (double)f;
    }
    choose_record_tiers(*model, e->own, e->cfg, free_b, &e->Mh, &e->ma_hotfrac);
  }
  e->model_copy = *model;
  e->own_matransblock_start.assign(model->level_matransblock_start, model->level_matransblock_start + model->nlevels);
  e->model_copy.level_matransblock_start = e->own_matransblock_start.data();
  e->M = e->Mh;
  const DevModel &h = e->Mh;
#define UP(f, T, count)                                                                     \
  {                                                                                         \
    int rc = upload_array<T>(e->model_allocs, h.f, (int64_t)(count), (const T **)&e->M.f);  \
    if (rc != ARTIS_OK) return rc;                                                          \
  }
  ARTIS_MODEL_ARRAYS(UP, h)
#undef UP
#define UPMO(f, T, count)                                                                     \
  {                                                                                           \
    e->M.f = nullptr;                                                                         \
    if (h.f) {                                                                                \
      int rc = upload_array<T>(e->model_allocs, h.f, (int64_t)(count), (const T **)&e->M.f);  \
      if (rc != ARTIS_OK) return rc;                                                          \
    }                                                                                         \
  }
  ARTIS_MODEL_OPTIONAL_ARRAYS(UPMO, h)
#undef UPMO
  if ((ARTIS_OPT_GAMMA_THERMALISATION_SCHEME == ARTIS_GAMMA_WOLLAEGER || ARTIS_OPT_GAMMA_THERMALISATION_SCHEME == ARTIS_GAMMA_GUTTMAN) &&
      !e->M.rho_tmin) {
    g_last_error = "this build integrates gamma-ray column densities: artis_model.rho_tmin is required";
    return ARTIS_ERR_ARG;
  }
  if ((ARTIS_OPT_GAMMA_THERMALISATION_SCHEME == ARTIS_GAMMA_BARNES || ARTIS_OPT_PARTICLE_THERMALISATION_SCHEME == ARTIS_PARTICLE_BARNES) &&
      !(h.mtot_input > 0. && h.ejecta_kinetic_energy > 0.)) {
    g_last_error = "this build uses a Barnes thermalisation efficiency: artis_model.mtot_input and ejecta_kinetic_energy are required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_USE_XCOM_GAMMAPHOTOION && (!e->M.xcom_elem_start || !e->M.xcom_energy || !e->M.xcom_sigma || !e->M.elem_meannucmass)) {
    g_last_error = "this build has USE_XCOM_GAMMAPHOTOION: artis_model.xcom_elem_start / xcom_energy / xcom_sigma and elem_meannucmass are required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_DETAILED_LINE_ESTIMATORS_ON && (!e->M.detailed_lineindices || h.detailed_linecount <= 0)) {
    g_last_error = "this build has DETAILED_LINE_ESTIMATORS_ON: artis_model.detailed_lineindices / detailed_linecount are required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_BFEST_SUBSET && !e->M.allcont_bfestimindex) {
    g_last_error = "this build keeps bound-free estimators for a subset of the continua: artis_model.allcont_bfestimindex / nbfestim are required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_NT_ON && (!e->M.elem_meannucmass || !e->M.ion_nt_sum_q_over_binding)) {
    g_last_error = "this build has NT_ON: artis_model.elem_meannucmass and ion_nt_sum_q_over_binding are required";
    return ARTIS_ERR_ARG;
  }
  for (int a = 0; a < 3; a++) {
    const int ndim = (h.gridtype == ARTIS_GRID_SPHERICAL1D) ? 1 : ((h.gridtype == ARTIS_GRID_CYLINDRICAL2D) ? 2 : 3);  // get_ndim grid.cc:120
    const int64_t cnt = (a >= ndim) ? 1 : h.ncoordgrid[a];
    int rc = upload_array<double>(e->model_allocs, h.coord_pos_min_tmin[a], cnt, &e->M.coord_pos_min_tmin[a]);
    if (rc != ARTIS_OK) return rc;
  }
  // allphixstarget index -> level
  {
    std::vector<int32_t> tl((size_t)(h.nphixstargets_total > 0 ? h.nphixstargets_total : 1), 0);
    for (int ul = 0; ul < h.nlevels; ul++)
      for (int t = 0; t < h.level_nphixstargets[ul]; t++) tl[h.level_phixstargetstart[ul] + t] = ul;
    const int32_t *d = nullptr;
    int rc = upload_array<int32_t>(e->model_allocs, tl.data(), h.nphixstargets_total, &d);
    if (rc != ARTIS_OK) return rc;
    e->d_target_level = (int32_t *)d;
  }
  // per-cell cache: all cells if that fits the budget, else one tile of cells at a time (plan_cache_rows)
  const int64_t ncell_all = h.npts_nonempty;
  {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    CacheLayout L;
    if (const int rc = plan_cache_rows(h, e->cfg, (double)free_b, &L)) return rc;
    if (L.drop_dpop) {
      e->Mh.ndpop = 0;
      e->M.ndpop = 0;
    }
    e->cache_budget = L.budget;
    e->cc.cache_bytes_per_cell = L.per_cell;
    e->cc.res.tile_cells = L.tile_cells;
    e->cc.ntiles = L.ntiles;
    e->cc.tile_lo = 0;
    e->cc.tile_hi = (int)std::min<int64_t>(ncell_all, e->cc.res.tile_cells);
  }
  const int64_t nrows = e->cc.res.tile_cells;  // rows allocated
#define CA(f, T, per)                                                                       \
  {                                                                                         \
    T *d = nullptr;                                                                         \
    HIP_TRY(hipMalloc((void **)&d, sizeof(T) * (size_t)(nrows * (int64_t)(per) + MAREC_SLACK)));    \
    e->cache_allocs.push_back(d);                                                           \
    e->K.f = d;                                                                             \
  }
  ARTIS_CACHE_ARRAYS(CA, h)
#undef CA
  // estimators: one contiguous block [cell][8]{J, nuJ, ff, col, dep_gamma, dep_electron, dep_positron, dep_alpha} | [cell][ground continuum][2]{gamma, bfheat} | scalars
  const int64_t ncell = ncell_all;  // estimators cover every cell
  const int64_t g = h.nbfcontinua_ground > 0 ? h.nbfcontinua_ground : 1;
  // ... | scalars | ([cell][bin][2]{radfieldbin_J, radfieldbin_nuJ}) | (bfrate_raw)]
  const int64_t nbinest = ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON ? ncell * ARTIS_OPT_RADFIELDBINCOUNT : 0;
  const int64_t nbfest = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? ncell * (int64_t)h.nbfestim : 0;
  const int64_t nlineest = ARTIS_OPT_DETAILED_LINE_ESTIMATORS_ON ? ncell * (int64_t)h.detailed_linecount : 0;
  // ... | (vspecpol | vgrid_flux)]: the observers' spectra of a VPKT_ON build, inside the block the all-reduce covers
  int64_t nvspec = 0, nvgrid = 0;
#if ARTIS_OPT_VPKT_ON
  {
    VpktConfig V;
    if (!make_vpkt_config(*model, V)) {
      g_last_error = "this build has VPKT_ON: artis_model.vpkt_* (the configuration read from vpkt.txt) is required";
      return ARTIS_ERR_ARG;
    }
    HIP_TRY(hipMalloc((void **)&e->d_vpkt_config, sizeof(VpktConfig)));
    e->model_allocs.push_back(e->d_vpkt_config);
    HIP_TRY(hipMemcpy(e->d_vpkt_config, &V, sizeof(V), hipMemcpyHostToDevice));
    e->M.vpkt = e->d_vpkt_config;
    nvspec = (int64_t)ARTIS_VSPEC_TIMEBINS * V.nobsdirections * V.nspectraperobsdir * ARTIS_VSPEC_NUBINS * 3;
    nvgrid = V.vgrid_on ? (int64_t)ARTIS_VGRID_NY * ARTIS_VGRID_NZ * V.grid_nwavelengthranges * V.nobsdirections * 3 : 0;
    e->tail_max = 0;  // k_tail takes a packet through any number of steps in one launch: more events than the queue is sized for
  }
#endif
  e->nvspec = nvspec;
  e->nvgrid = nvgrid;
  e->est_ndoubles = ncell * 8 + 2 * ncell * g + ARTIS_NSCALARS + 2 * nbinest + nbfest + 2 * nlineest + nvspec + nvgrid;
  HIP_TRY(hipMalloc((void **)&e->d_est, sizeof(double) * (size_t)e->est_ndoubles));
  HIP_TRY(hipMemset(e->d_est, 0, sizeof(double) * (size_t)e->est_ndoubles));
  // [cell][8] {J, nuJ, ffheating, colheating, dep_gamma, dep_electron, dep_positron, dep_alpha}: one 64-byte record per cell
  // (physics.h Env::est_stride), then [cell][ground continuum][2] {gamma, bfheating}
  e->E.J = e->d_est;
  e->E.nuJ = e->d_est + 1;
  e->E.ffheatingestimator = e->d_est + 2;
  e->E.colheatingestimator = e->d_est + 3;
  e->E.dep_estimator_gamma = e->d_est + 4;
  e->E.dep_estimator_electron = e->d_est + 5;
  e->E.dep_estimator_positron = e->d_est + 6;
  e->E.dep_estimator_alpha = e->d_est + 7;
  e->E.gammaestimator = e->d_est + 8 * ncell;
  e->E.bfheatingestimator = e->d_est + 8 * ncell + 1;
  e->E.scalars = e->d_est + 8 * ncell + 2 * ncell * g;
  e->E.radfieldbin_J = nbinest ? e->E.scalars + ARTIS_NSCALARS : nullptr;
  e->E.radfieldbin_nuJ = nbinest ? e->E.radfieldbin_J + 1 : nullptr;  // [cell][bin][2] {J, nuJ}
  e->E.bfrate_raw = nbfest ? e->E.scalars + ARTIS_NSCALARS + 2 * nbinest : nullptr;
  e->E.Jb_lu_raw = nlineest ? e->E.scalars + ARTIS_NSCALARS + 2 * nbinest + nbfest : nullptr;
  e->E.Jb_lu_contribcount = nlineest ? e->E.Jb_lu_raw + nlineest : nullptr;
  e->E.vspecpol = nvspec ? e->E.scalars + ARTIS_NSCALARS + 2 * nbinest + nbfest + 2 * nlineest : nullptr;
  e->E.vgrid_flux = nvgrid ? e->E.vspecpol + nvspec : nullptr;
#if ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON
  if (nbfest > 0 && h.nbfcontinua > 0 && e->cc.ntiles == 1) {
    const size_t bytes = sizeof(double) * (size_t)ncell * (size_t)h.nbfcontinua;
    HIP_TRY(hipMalloc((void **)&e->d_bfrate_kept, bytes));
    HIP_TRY(hipMemset(e->d_bfrate_kept, 0, bytes));
  }
#endif
  HIP_TRY(hipMalloc((void **)&e->d_stats, sizeof(unsigned long long) * ARTIS_NSTATS));
  HIP_TRY(hipMemset(e->d_stats, 0, sizeof(unsigned long long) * ARTIS_NSTATS));
  HIP_TRY(hipMalloc((void **)&e->d_count, sizeof(int32_t) * (2 * NEXT_NKINDS + 2)));
  HIP_TRY(hipMemset(e->d_count, 0, sizeof(int32_t) * (2 * NEXT_NKINDS + 2)));
  e->d_err = e->d_count + (2 * NEXT_NKINDS);
  e->d_late_bail = e->d_err + 1;  // (k_late's count of waves that gave up waiting: travels with the counters)
  HIP_TRY(hipHostMalloc((void **)&e->h_counts, sizeof(int32_t) * (2 * NEXT_NKINDS + 2), hipHostMallocDefault));
  HIP_TRY(hipMalloc((void **)&e->d_cursors, sizeof(int32_t) * PULL_SLOTS));  // (work_pull.h: the chunk cursors + the launch's "list used up" flag)
  HIP_TRY(hipMalloc((void **)&e->cc.d_fill_cells, sizeof(int32_t) * (size_t)(ncell_all > 0 ? ncell_all : 1)));
  if (e->cc.ntiles > 1) {  // rows for a set of cells at a time: the table of rows, no cell resident yet
    HIP_TRY(hipMalloc((void **)&e->cc.d_krow, sizeof(int32_t) * (size_t)ncell_all));
    e->cc.res.init(ncell_all);
    HIP_TRY(hipMemset(e->cc.d_krow, 0xFF, sizeof(int32_t) * (size_t)ncell_all));
    e->cc.h_cell_grid.assign((size_t)ncell_all, 0);
    for (int g = 0; g < h.ngrid; g++)
      if (h.propcell_nonemptymgi[g] >= 0) e->cc.h_cell_grid[(size_t)h.propcell_nonemptymgi[g]] = g;
  }
  {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    e->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  HIP_TRY(hipMalloc((void **)&e->d_hist, sizeof(int32_t) * (SORT_LDS_KEYS + 1)));
  HIP_TRY(hipMalloc((void **)&e->d_tiles, sizeof(int32_t) * (SORT_LDS_KEYS / SCAN_TILE + 2)));
  HIP_TRY(hipEventCreate(&e->ev0));
  HIP_TRY(hipEventCreate(&e->ev1));
  HIP_TRY(hipEventCreate(&e->ev2));
  HIP_TRY(hipEventCreate(&e->ev3));
  read_switches(e);
  {
    // the static part of every macro-atom record (tables.h: filter entries that are never counted) is written once
    const int64_t nrows_ = e->cc.res.tile_cells;  // every resident row; the static parts do not depend on the cell
    Env env0 = make_env(e);
    env0.K = e->K;
    hipLaunchKernelGGL(k_mainit, dim3(nblocks(nrows_ * e->Mh.nlevels)), dim3(BLOCK), 0, nullptr, env0, nrows_);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  {
    // the population works through the cells in batches whose cooling terms fit its scratch (pop_batch_cells)
    e->cc.pop_batch = pop_batch_cells(e->Mh, e->cc.res.tile_cells, e->cfg);
    HIP_TRY(hipMalloc((void **)&e->cc.d_collexc_terms, pop_scratch_alloc_bytes(e->Mh, e->cc.pop_batch)));
  }
  // (a build whose slow path fills records by the lane has no fill into a static slot: everything is populated)
  // (... and a model with cold levels keeps the full population of its static records unless ARTIS_AMD_MA_ABSENT_EPS asks: its step was measured
  // slower with the skip, profiles/r12/absent_ions.md)
  if (e->Mh.ncold > 0 && e->cfg.src_absent == CONFIG_DEFAULT) e->cfg.ma_absent_eps = -1.;
  if (e->cfg.ma_absent_eps >= 0. && ARTIS_MA_WAVE_FILL && e->Mh.nions > 0 && e->Mh.nalltrans > 0) {
    const size_t nb = (size_t)e->cc.res.tile_cells * (size_t)e->Mh.nions;
    HIP_TRY(hipMalloc((void **)&e->d_ion_absent, nb));
    HIP_TRY(hipMemset(e->d_ion_absent, 0, nb));
    HIP_TRY(hipMalloc((void **)&e->d_ion_popsum, nb * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&e->d_absent_counts, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(e->d_absent_counts, 0, 2 * sizeof(unsigned long long)));
  }
  if (e->trace) trace_config(e);
  if (e->trace)
    fprintf(stderr, "[artis_amd] record tiers: static records for %.2f of every ion's levels, %d cold levels, pool of %d slots per resident cell; %d tile(s) of %lld cells, %zu B per cell\n",
            e->ma_hotfrac, e->Mh.ncold, e->Mh.ma_pool_slots, e->cc.ntiles, (long long)e->cc.res.tile_cells, e->cc.cache_bytes_per_cell);
  return ARTIS_OK;
}
}  // namespace

extern "C" {

void artis_amd_engine_destroy(artis_amd_engine *e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->comm && rccl_api().ok) (void)rccl_api().CommDestroy(e->comm);
  free_all(e->model_allocs);
  free_all(e->cell_allocs);
  free_all(e->cache_allocs);
  free_packet_buffers(e);
  spec_free(e->spec);
  rf_free(e->rf);
  ib_free(e->ib);
  decay_free(e->decay);
  dep_free(e->dep);
  pinit_free(e->pinit);
  init_free(e->init);
  tb_free(e->tb);
  bfh_free(e->bfh);
  rc_free(e->rc);
  pi_free(e->pi);
  if (e->h_counts) (void)hipHostFree(e->h_counts);
  void *ptrs[] = {e->d_est, e->d_stats, e->d_aos, e->d_hist, e->d_tiles, e->d_count, e->d_cursors, e->cc.d_krow, e->cc.d_fill_cells, e->cc.d_waiting,
                  e->d_bfrate_kept, e->cc.d_collexc_terms, e->d_visit_counts, e->d_ion_absent, e->d_ion_popsum, e->d_absent_counts};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  for (hipEvent_t ev : {e->ev0, e->ev1, e->ev2, e->ev3})
    if (ev) (void)hipEventDestroy(ev);
  delete e;
}

}  // extern "C"

namespace {

// The arrays every cell state has (ARTIS_CELL_ARRAYS), allocated in place of the previous state's; the optional ones absent. Shared by
// cellstate_upload, which copies the host's arrays into them, and by the hand-over of artis_amd_grid_update_initial (stage_ionbal.h),
// which asks for them zeroed and fills them on the device. No cell state is resident afterwards until the caller says so.
int cellstate_alloc(artis_amd_engine *e, const bool zeroed) {
  e->have_cells = false;  // until every array of the new state is resident
  free_all(e->cell_allocs);
  e->pi_coeff = nullptr;
  const DevModel &h = e->Mh;
#define ALC(f, T, count)                                                \
  {                                                                     \
    T *d = nullptr;                                                     \
    const int64_t cnt = (int64_t)(count);                               \
    const size_t bytes = sizeof(T) * (size_t)(cnt > 0 ? cnt : 1);       \
    HIP_TRY(hipMalloc((void **)&d, bytes));                             \
    e->cell_allocs.push_back(d);                                        \
    if (zeroed) HIP_TRY(hipMemset(d, 0, bytes));                        \
    e->C.f = d;                                                         \
  }
  ARTIS_CELL_ARRAYS(ALC, h)
#undef ALC
#define NUL(f, T, count) e->C.f = nullptr;
  ARTIS_CELL_OPTIONAL_ARRAYS(NUL, h)
#undef NUL
  e->C.nt_excitations_stored = 0;
  e->C.nt_ionratecoeff = nullptr;
  e->C.nt_ionenrate_cum = nullptr;
  return ARTIS_OK;
}

int cellstate_options(artis_amd_engine *e, const bool corrphotoioncoeff_follows);

// artis_amd_set_cellstate in two halves, shared with artis_amd_set_cellstate_photoion (stage_photoion.h), which computes
// corrphotoioncoeff between them. The first: the uploads and what the build's options need from the host; corrphotoioncoeff_follows:
// the caller makes that array on the device before cellstate_finish.
int cellstate_upload(artis_amd_engine *e, const artis_cellstate *cells, const artis_timestep *ts, const bool corrphotoioncoeff_follows) {
  HIP_TRY(hipSetDevice(e->device));
  const DevModel &h = e->Mh;
  DevCells hc = make_host_cells_view(*cells);
  std::vector<float> zero_ffegrp;
  if (!hc.ffegrp) {  // no gamma packets will be handed over: the opacities of gammapkt.cc are never evaluated
    zero_ffegrp.assign((size_t)(h.npts_nonempty > 0 ? h.npts_nonempty : 1), 0.f);
    hc.ffegrp = zero_ffegrp.data();
  }
  int rc = cellstate_alloc(e, false);
  if (rc != ARTIS_OK) return rc;
#define UPC(f, T, count) \
  if ((int64_t)(count) > 0) HIP_TRY(hipMemcpy(const_cast<T *>(e->C.f), hc.f, sizeof(T) * (size_t)(count), hipMemcpyHostToDevice));
  ARTIS_CELL_ARRAYS(UPC, h)
#undef UPC
#define UPO(f, T, count)                                                                     \
  {                                                                                          \
    e->C.f = nullptr;                                                                        \
    if (hc.f) {                                                                              \
      int rc = upload_array<T>(e->cell_allocs, hc.f, (int64_t)(count), (const T **)&e->C.f); \
      if (rc != ARTIS_OK) return rc;                                                         \
    }                                                                                        \
  }
  const int64_t nt_stored = (hc.nt_exc_count && hc.nt_excitations_stored > 0) ? hc.nt_excitations_stored : 0;
  ARTIS_CELL_OPTIONAL_ARRAYS(UPO, h)
#undef UPO
  e->C.nt_excitations_stored = (int32_t)nt_stored;
  rc = cellstate_options(e, corrphotoioncoeff_follows);
  if (rc != ARTIS_OK) return rc;
  e->S = make_step(*ts);
  return ARTIS_OK;
}

// what the options this library was built with need of a cell state whose arrays are in place (absent optional ones null): the
// refusals, and the expansion-opacity tables the engine makes itself
int cellstate_options(artis_amd_engine *e, const bool corrphotoioncoeff_follows) {
  const DevModel &h = e->Mh;
  if (!ARTIS_OPT_USE_LUT_PHOTOION && h.nphixstargets_total > 0 && !e->C.corrphotoioncoeff && !corrphotoioncoeff_follows) {
    g_last_error = "this build has USE_LUT_PHOTOION off: artis_cellstate.corrphotoioncoeff is required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON && (!e->C.radfieldbin_W || !e->C.radfieldbin_T_R)) {
    g_last_error = "this build has the multibin radiation field on: artis_cellstate.radfieldbin_W / _T_R are required";
    return ARTIS_ERR_ARG;
  }
  e->expopac_own = false;
  if (ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT && (ARTIS_OPT_USE_XCOM_GAMMAPHOTOION || ARTIS_OPT_NT_ON) && !e->C.elem_meanweight) {
    g_last_error = "this build has USE_CALCULATED_MEANATOMICWEIGHT and reads element number densities: artis_cellstate.elem_meanweight is required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_DETAILED_LINE_ESTIMATORS_ON && !e->C.Jb_lu_normed) {
    g_last_error = "this build has DETAILED_LINE_ESTIMATORS_ON: artis_cellstate.Jb_lu_normed is required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_EXPOPAC_TABLES) {
    // the tables of calculate_expansion_opacities(): the host's, or (both NULL) made by the engine at cell-cache population
    const bool need_planck = ARTIS_OPT_RPKT_BB_THERMALISATION;
    if (!e->C.expansionopacities && !e->C.expansionopacity_planck_cumulative) {
      const size_t cnt = (size_t)(h.npts_nonempty > 0 ? h.npts_nonempty : 1) * ARTIS_EXPOPAC_NBINS;
      float *dk = nullptr;
      double *dp = nullptr;
      HIP_TRY(hipMalloc((void **)&dk, sizeof(float) * cnt));
      e->cell_allocs.push_back(dk);
      HIP_TRY(hipMemset(dk, 0, sizeof(float) * cnt));
      HIP_TRY(hipMalloc((void **)&dp, sizeof(double) * cnt));
      e->cell_allocs.push_back(dp);
      HIP_TRY(hipMemset(dp, 0, sizeof(double) * cnt));
      e->C.expansionopacities = dk;
      e->C.expansionopacity_planck_cumulative = dp;
      e->expopac_own = true;
    } else if (!e->C.expansionopacities || (need_planck && !e->C.expansionopacity_planck_cumulative)) {
      g_last_error = "expansion-opacity build: hand over both artis_cellstate.expansionopacities and (with a thermalisation "
                     "probability) .expansionopacity_planck_cumulative, or neither (the engine then calculates them)";
      return ARTIS_ERR_ARG;
    }
  }
  return ARTIS_OK;
}

// the second half: what is derived once per cell state, then the cell cache
int cellstate_finish(artis_amd_engine *e) {
  const DevModel &h = e->Mh;
#if ARTIS_OPT_NT_ON
  const int64_t nt_stored = e->C.nt_excitations_stored;
  if (!e->C.nt_frac_ionisation || !e->C.nt_frac_excitation || !e->C.nt_deposition_rate_density || !e->C.nt_eff_ionpot ||
      !e->C.nt_prob_num_auger || !e->C.nt_ionenfrac_num_auger || !e->C.nt_exc_count ||
      (nt_stored > 0 && (!e->C.nt_exc_frac_deposition || !e->C.nt_exc_ratecoeffperdeposition || !e->C.nt_exc_alltransindex))) {
    g_last_error = "this build has NT_ON: the Spencer-Fano solution (artis_cellstate.nt_*) is required";
    return ARTIS_ERR_ARG;
  }
  {
    const size_t bytes = sizeof(double) * (size_t)(h.npts_nonempty > 0 ? h.npts_nonempty : 1) * (size_t)h.nions;
    HIP_TRY(hipMalloc((void **)&e->C.nt_ionratecoeff, bytes));
    e->cell_allocs.push_back(e->C.nt_ionratecoeff);
    HIP_TRY(hipMalloc((void **)&e->C.nt_ionenrate_cum, bytes));
    e->cell_allocs.push_back(e->C.nt_ionenrate_cum);
    if (h.npts_nonempty > 0) {
      const Env env = make_env(e);
      hipLaunchKernelGGL(k_nt_cells, dim3((h.npts_nonempty + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr, env, h.npts_nonempty);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
      int32_t err = 0;
      HIP_TRY(hipMemcpy(&err, e->d_err, sizeof(err), hipMemcpyDeviceToHost));
      if (err != 0) {
        (void)hipMemset(e->d_err, 0, sizeof(int32_t));
        g_last_error = "the Spencer-Fano solution is inconsistent (Auger probabilities do not sum to one): error flag " + std::to_string(err);
        return ARTIS_ERR_ARG;
      }
    }
  }
#endif
  e->have_cells = true;
  e->cellstate_serial++;
  return artis_amd_populate_cellcache(e, nullptr);
}

}  // namespace

extern "C" {

int artis_amd_set_cellstate(artis_amd_engine *e, const artis_cellstate *cells, const artis_timestep *ts) {
  if (!e || !cells || !ts) {
    g_last_error = "null argument";
    return ARTIS_ERR_ARG;
  }
  const int rc = cellstate_upload(e, cells, ts, false);
  if (rc != ARTIS_OK) return rc;
  return cellstate_finish(e);
}

}  // extern "C"

extern "C" {

int artis_amd_engine_config(artis_amd_engine *e, artis_amd_config *effective) {
  if (!e || !effective) {
    g_last_error = "null argument";
    return ARTIS_ERR_ARG;
  }
  const size_t n = effective->struct_size;
  if (n > sizeof(artis_amd_config) || n < sizeof(size_t)) {
    g_last_error = "artis_amd_config.struct_size is not one this library knows: artis_amd_config_default() fills it in";
    return ARTIS_ERR_ARG;
  }
  artis_amd_config c;
  config_set_default(&c);
  c.struct_size = n;
  c.cache_budget_bytes = (int64_t)e->cache_budget;
  c.cache_headroom_bytes = (int64_t)e->cfg.cache_headroom;
  c.pop_scratch_bytes = (int64_t)e->cfg.pop_scratch;
  c.ma_hot_fraction = e->ma_hotfrac;
  c.ma_pool_fraction = e->cfg.ma_pool;
  c.tail_threshold = e->tail_max;
  c.tile_park_at = e->park_at;
  c.keep_line_dpop = e->Mh.ndpop > 0 ? 1 : 0;
  std::memcpy(effective, &c, n);
  return ARTIS_OK;
}

int artis_amd_engine_plan(const artis_model *model, int device, const artis_amd_config *cfg, int64_t free_bytes, artis_amd_plan *plan) {
  if (!model || !plan || free_bytes < 0) {
    g_last_error = !model || !plan ? "null argument" : "free_bytes is negative (0: ask the device)";
    return ARTIS_ERR_ARG;
  }
  const size_t n = plan->struct_size;
  if (n > sizeof(artis_amd_plan) || n < sizeof(size_t)) {
    g_last_error = "artis_amd_plan.struct_size is not one this library knows: set it to sizeof(artis_amd_plan)";
    return ARTIS_ERR_ARG;
  }
  artis_amd_config checked;
  if (const int rc = config_copy_checked(cfg, &checked, &g_last_error)) return rc;
  if (const int rc = validate_model(model)) return rc;
  const EngineConfig rcfg = resolve_config(checked);
  double free_b = (double)free_bytes;
  if (free_bytes == 0) {  // what a creation would find free at this moment
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
      g_last_error = "no HIP device: artis_amd_engine_plan() needs one to ask for the free memory (free_bytes = 0)";
      return ARTIS_ERR_NODEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    size_t f = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&f, &total_b));
    free_b = (double)f;
  }
  ModelOwned own;
  DevModel h;
  double hot = 1.;
  choose_record_tiers(*model, own, rcfg, free_b, &h, &hot);
  const int64_t model_bytes = model_table_bytes(h);
  CacheLayout L;
  if (const int rc = plan_cache_rows(h, rcfg, std::max(0., free_b - (double)model_bytes), &L)) return rc;
  if (L.drop_dpop) h.ndpop = 0;
  artis_amd_plan p;
  std::memset(&p, 0, sizeof(p));
  p.struct_size = n;
  p.bytes_per_cell = (int64_t)L.per_cell;
  p.cells_resident = L.tile_cells;
  p.ntiles = L.ntiles;
  p.ncold_levels = h.ncold;
  p.hot_fraction = hot;
  p.pool_slots = h.ma_pool_slots;
#define SZ(f, T, per) p.cache_bytes += (int64_t)sizeof(T) * (L.tile_cells * (int64_t)(per) + MAREC_SLACK);
  ARTIS_CACHE_ARRAYS(SZ, h)
#undef SZ
  p.pool_bytes = (int64_t)sizeof(U4) * (L.tile_cells * (int64_t)h.ma_pool_slots + MAREC_SLACK);
  p.pop_scratch_bytes = (int64_t)pop_scratch_alloc_bytes(h, pop_batch_cells(h, L.tile_cells, rcfg));
  p.model_bytes = model_bytes;
  p.free_bytes_assumed = (int64_t)free_b;
  p.line_dpop_kept = h.ndpop > 0 ? 1 : 0;
  std::memcpy(plan, &p, n);
  return ARTIS_OK;
}

int artis_amd_packets_upload(artis_amd_engine *e, const artis_packet *packets, int64_t npackets) {
  if (!e || (!packets && npackets > 0) || npackets < 0 || npackets > 2147483000LL) {
    g_last_error = "bad packet buffer";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  int rc = ensure_packet_buffers(e, npackets);
  if (rc != ARTIS_OK) return rc;
  rc = ensure_aos(e, npackets);
  if (rc != ARTIS_OK) return rc;
  if (npackets > 0) HIP_TRY(hipMemcpy(e->d_aos, packets, sizeof(artis_packet) * (size_t)npackets, hipMemcpyHostToDevice));
  return install_resident_aos(e, npackets);
}

int artis_amd_packets_download(artis_amd_engine *e, artis_packet *packets, int64_t npackets) {
  if (!e || npackets != e->npackets || (!packets && npackets > 0)) {
    g_last_error = "packet count does not match the resident population";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (npackets == 0) return ARTIS_OK;
  int rc = ensure_aos(e, npackets);
  if (rc != ARTIS_OK) return rc;
  // the fields this path never touches keep the values the caller uploaded: the structs are still on the device from
  // artis_amd_packets_upload() (no second trip over PCIe: 256 B per packet); copied again only if that buffer was replaced
  if (!e->aos_valid) HIP_TRY(hipMemcpy(e->d_aos, packets, sizeof(artis_packet) * (size_t)npackets, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_rec_to_aos, dim3(nblocks(npackets)), dim3(BLOCK), 0, nullptr, e->P, e->d_aos, e->use_perm ? e->d_perm : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(packets, e->d_aos, sizeof(artis_packet) * (size_t)npackets, hipMemcpyDeviceToHost));
  return ARTIS_OK;
}

int artis_amd_packets_snapshot(artis_amd_engine *e) {
  if (!e || !e->d_pkt) {
    g_last_error = "no resident packets";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (!e->d_pkt_snapshot) HIP_TRY(hipMalloc(&e->d_pkt_snapshot, e->pkt_bytes));
  HIP_TRY(hipMemcpy(e->d_pkt_snapshot, e->d_pkt, e->pkt_bytes, hipMemcpyDeviceToDevice));
  return ARTIS_OK;
}

int artis_amd_packets_restore(artis_amd_engine *e) {
  if (!e || !e->d_pkt || !e->d_pkt_snapshot) {
    g_last_error = "no snapshot";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpy(e->d_pkt, e->d_pkt_snapshot, e->pkt_bytes, hipMemcpyDeviceToDevice));
  return ARTIS_OK;
}

int artis_amd_estimators_zero(artis_amd_engine *e, void *hip_stream) {
  if (!e) return ARTIS_ERR_ARG;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemsetAsync(e->d_est, 0, sizeof(double) * (size_t)e->est_ndoubles, (hipStream_t)hip_stream));
  HIP_TRY(hipMemsetAsync(e->d_stats, 0, sizeof(unsigned long long) * ARTIS_NSTATS, (hipStream_t)hip_stream));
  // (d_bfrate_kept is zero between calls: k_bfrate_expand leaves it so)
  return ARTIS_OK;
}

int artis_amd_estimators_download(artis_amd_engine *e, artis_estimators *est) {
  if (!e || !est) return ARTIS_ERR_ARG;
  HIP_TRY(hipSetDevice(e->device));
  std::vector<double> h((size_t)e->est_ndoubles);
  HIP_TRY(hipMemcpy(h.data(), e->d_est, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  const int64_t ncell = e->Mh.npts_nonempty;
  const int64_t g = e->Mh.nbfcontinua_ground > 0 ? e->Mh.nbfcontinua_ground : 1;
  const double *src = h.data();
  auto add = [](double *dst, const double *s, int64_t cnt) {
    if (!dst) return;
    for (int64_t i = 0; i < cnt; i++) dst[i] += s[i];
  };
  auto add_strided = [](double *dst, const double *s, int64_t cnt, int64_t stride) {
    if (!dst) return;
    for (int64_t i = 0; i < cnt; i++) dst[i] += s[i * stride];
  };
  add_strided(est->J, src, ncell, 8);
  add_strided(est->nuJ, src + 1, ncell, 8);
  add_strided(est->ffheatingestimator, src + 2, ncell, 8);
  add_strided(est->colheatingestimator, src + 3, ncell, 8);
  add_strided(est->dep_estimator_gamma, src + 4, ncell, 8);
  add_strided(est->dep_estimator_electron, src + 5, ncell, 8);
  add_strided(est->dep_estimator_positron, src + 6, ncell, 8);
  add_strided(est->dep_estimator_alpha, src + 7, ncell, 8);
  add_strided(est->gammaestimator, src + 8 * ncell, ncell * g, 2);
  add_strided(est->bfheatingestimator, src + 8 * ncell + 1, ncell * g, 2);
  add(est->scalars, src + 8 * ncell + 2 * ncell * g, ARTIS_NSCALARS);
  {
    const int64_t nbinest = ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON ? ncell * ARTIS_OPT_RADFIELDBINCOUNT : 0;
    const int64_t nbfest = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? ncell * (int64_t)e->Mh.nbfestim : 0;
    const double *ext = src + 8 * ncell + 2 * ncell * g + ARTIS_NSCALARS;
    if (nbinest) {
      add_strided(est->radfieldbin_J, ext, nbinest, 2);
      add_strided(est->radfieldbin_nuJ, ext + 1, nbinest, 2);
    }
    if (nbfest) add(est->bfrate_raw, ext + 2 * nbinest, nbfest);
    const int64_t nlineest = ARTIS_OPT_DETAILED_LINE_ESTIMATORS_ON ? ncell * (int64_t)e->Mh.detailed_linecount : 0;
    if (nlineest) {
      add(est->Jb_lu_raw, ext + 2 * nbinest + nbfest, nlineest);
      if (est->Jb_lu_contribcount)
        for (int64_t i = 0; i < nlineest; i++) est->Jb_lu_contribcount[i] += (int64_t)ext[2 * nbinest + nbfest + nlineest + i];
    }
    if (e->nvspec) add(est->vspecpol, ext + 2 * nbinest + nbfest + 2 * nlineest, e->nvspec);
    if (e->nvgrid) add(est->vgrid_flux, ext + 2 * nbinest + nbfest + 2 * nlineest + e->nvspec, e->nvgrid);
  }
  if (est->stats) {
    unsigned long long st[ARTIS_NSTATS];
    HIP_TRY(hipMemcpy(st, e->d_stats, sizeof(st), hipMemcpyDeviceToHost));
    for (int i = 0; i < ARTIS_NSTATS; i++) est->stats[i] += (int64_t)st[i];
  }
  return ARTIS_OK;
}

int artis_amd_estimators_devptr(artis_amd_engine *e, void **dptr, int64_t *ndoubles) {
  if (!e || !dptr || !ndoubles) return ARTIS_ERR_ARG;
  *dptr = e->d_est;
  *ndoubles = e->est_ndoubles;
  return ARTIS_OK;
}

int artis_amd_comm_unique_id(void *id_out) {
  if (!id_out) return ARTIS_ERR_ARG;
  if (!rccl_api().ok) {
    g_last_error = "librccl could not be loaded";
    return ARTIS_ERR_RCCL;
  }
  ncclUniqueId id;
  RCCL_TRY(rccl_api().GetUniqueId(&id));
  std::memcpy(id_out, id.internal, ARTIS_AMD_COMM_ID_BYTES);
  return ARTIS_OK;
}

int artis_amd_comm_init(artis_amd_engine *e, int nranks, int rank, const void *id_bytes) {
  if (!e || !id_bytes || nranks < 1 || rank < 0 || rank >= nranks) {
    g_last_error = "bad communicator arguments";
    return ARTIS_ERR_ARG;
  }
  if (!rccl_api().ok) {
    g_last_error = "librccl could not be loaded";
    return ARTIS_ERR_RCCL;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (e->comm) {
    (void)rccl_api().CommDestroy(e->comm);
    e->comm = nullptr;
  }
  ncclUniqueId id;
  std::memcpy(id.internal, id_bytes, ARTIS_AMD_COMM_ID_BYTES);
  RCCL_TRY(rccl_api().CommInitRank(&e->comm, nranks, id, rank));
  return ARTIS_OK;
}

int artis_amd_comm_count(artis_amd_engine *e, void *nccl_comm, int *nranks) {
  if (!e || !nranks) return ARTIS_ERR_ARG;
  ncclComm_t comm = nccl_comm ? (ncclComm_t)nccl_comm : e->comm;
  if (!comm || !rccl_api().ok || !rccl_api().CommCount) {
    g_last_error = "no communicator (artis_amd_comm_init), or librccl without ncclCommCount";
    return ARTIS_ERR_RCCL;
  }
  RCCL_TRY(rccl_api().CommCount(comm, nranks));
  return ARTIS_OK;
}

int artis_amd_allreduce_estimators(artis_amd_engine *e, void *nccl_comm, void *hip_stream) {
  if (!e) return ARTIS_ERR_ARG;
  ncclComm_t comm = nccl_comm ? (ncclComm_t)nccl_comm : e->comm;
  if (!comm) {
    g_last_error = "no communicator: pass an ncclComm_t or call artis_amd_comm_init() first";
    return ARTIS_ERR_ARG;
  }
  if (!rccl_api().ok) {
    g_last_error = "librccl could not be loaded";
    return ARTIS_ERR_RCCL;
  }
  HIP_TRY(hipSetDevice(e->device));
  // one in-place sum over the whole block [J | nuJ | ffheat | colheat | gamma | bfheat | dep_* | scalars]
  RCCL_TRY(rccl_api().AllReduce(e->d_est, e->d_est, (size_t)e->est_ndoubles, ncclDouble, ncclSum, comm, (hipStream_t)hip_stream));
  return ARTIS_OK;
}

int artis_amd_update_packets(artis_amd_engine *e, artis_packet *packets, int64_t npackets, artis_estimators *est) {
  int rc = artis_amd_packets_upload(e, packets, npackets);
  if (rc != ARTIS_OK) return rc;
  rc = artis_amd_estimators_zero(e, nullptr);
  if (rc != ARTIS_OK) return rc;
  {
    // keep UPDATECELL of the populate that belongs to this timestep (with several cache tiles the populates happen
    // inside the update and count themselves)
    unsigned long long ncell = (e->cc.ntiles == 1) ? (unsigned long long)e->Mh.npts_nonempty : 0ull;
    HIP_TRY(hipMemcpy(e->d_stats + ARTIS_STAT_UPDATECELL, &ncell, sizeof(ncell), hipMemcpyHostToDevice));
  }
  rc = artis_amd_update_packets_device(e, nullptr);
  if (rc != ARTIS_OK) return rc;
  rc = artis_amd_packets_download(e, packets, npackets);
  if (rc != ARTIS_OK) return rc;
  if (est) rc = artis_amd_estimators_download(e, est);
  return rc;
}

int artis_amd_last_kernel_ms(artis_amd_engine *e, double *propagate_ms, int64_t *nlaunches) {
  if (!e) return ARTIS_ERR_ARG;
  if (propagate_ms) *propagate_ms = e->last.propagate_ms;
  if (nlaunches) *nlaunches = e->last.nlaunches;
  return ARTIS_OK;
}

int artis_amd_last_kernel_launches(artis_amd_engine *e, int64_t *rpkt_launches, int64_t *thermal_launches) {
  if (!e) return ARTIS_ERR_ARG;
  if (rpkt_launches) *rpkt_launches = e->last.klaunches[NEXT_RPKT];
  if (thermal_launches) *thermal_launches = e->last.klaunches[NEXT_MA] + e->last.klaunches[NEXT_KPKT];
  return ARTIS_OK;
}

int artis_amd_last_kernel_breakdown(artis_amd_engine *e, double *rpkt_ms, int64_t *rpkt_threads, double *thermal_ms,
                                    int64_t *thermal_threads) {
  if (!e) return ARTIS_ERR_ARG;
  if (rpkt_ms) *rpkt_ms = e->last.kms[NEXT_RPKT];
  if (rpkt_threads) *rpkt_threads = e->last.kthreads[NEXT_RPKT];
  if (thermal_ms) *thermal_ms = e->last.kms[NEXT_MA] + e->last.kms[NEXT_KPKT];
  if (thermal_threads) *thermal_threads = e->last.kthreads[NEXT_MA] + e->last.kthreads[NEXT_KPKT];
  return ARTIS_OK;
}

int artis_amd_last_tiling_fills(artis_amd_engine *e, int64_t *sparse_fills, int64_t *cells_filled) {
  if (!e) return ARTIS_ERR_ARG;
  if (sparse_fills) *sparse_fills = e->last.sparse_fills;
  if (cells_filled) *cells_filled = e->last.cells_filled;
  return ARTIS_OK;
}

int artis_amd_last_pool_resets(artis_amd_engine *e, int64_t *resets) {
  if (!e) return ARTIS_ERR_ARG;
  if (resets) *resets = e->last.pool_resets;
  return ARTIS_OK;
}

int artis_amd_record_tiers(artis_amd_engine *e, double *hot_fraction, int32_t *ncold_levels, int64_t *pool_slots) {
  if (!e) return ARTIS_ERR_ARG;
  if (hot_fraction) *hot_fraction = e->ma_hotfrac;
  if (ncold_levels) *ncold_levels = e->Mh.ncold;
  if (pool_slots) *pool_slots = e->Mh.ma_pool_slots;
  return ARTIS_OK;
}
int artis_amd_last_pool_usage(artis_amd_engine *e, int64_t *units_used, int64_t *units_cap) {
  if (!e) return ARTIS_ERR_ARG;
  if (units_used) *units_used = e->last_pool_used;
  if (units_cap) *units_cap = e->last_pool_cap;
  return ARTIS_OK;
}
int artis_amd_last_absent_records(artis_amd_engine *e, int64_t *skipped, int64_t *filled) {
  if (!e) return ARTIS_ERR_ARG;
  if (skipped) *skipped = e->last_absent_skipped;
  if (filled) *filled = e->last_absent_filled;
  return ARTIS_OK;
}
int artis_amd_last_thermal_variants(artis_amd_engine *e, int32_t *mask) {
  if (!e || !mask) return ARTIS_ERR_ARG;
  *mask = e->last.thermal_variants;
  return ARTIS_OK;
}
int artis_amd_last_estimator_forms(artis_amd_engine *e, int32_t *mask) {
  if (!e || !mask) return ARTIS_ERR_ARG;
  *mask = e->last.est_forms;
  return ARTIS_OK;
}
int artis_amd_last_tiling_parked(artis_amd_engine *e, int64_t *parked) {
  if (!e) return ARTIS_ERR_ARG;
  if (parked) *parked = e->last.parked;
  return ARTIS_OK;
}

int artis_amd_last_tiling(artis_amd_engine *e, int64_t *sweeps, int64_t *tile_fills, double *fill_ms, int64_t *listed) {
  if (!e) return ARTIS_ERR_ARG;
  if (sweeps) *sweeps = e->last.sweeps;
  if (tile_fills) *tile_fills = e->last.tile_fills;
  if (fill_ms) *fill_ms = e->last.fill_ms;
  if (listed) *listed = e->last.listed;
  return ARTIS_OK;
}

int artis_amd_last_kernel_table(artis_amd_engine *e, double ms[4], int64_t launches[4], int64_t packets[4]) {
  if (!e) return ARTIS_ERR_ARG;
  const int kinds[4] = {NEXT_RPKT, NEXT_MA, NEXT_KPKT, NEXT_SLOW};
  for (int i = 0; i < 4; i++) {
    if (ms) ms[i] = e->last.kms[kinds[i]];
    if (launches) launches[i] = e->last.klaunches[kinds[i]];
    if (packets) packets[i] = e->last.kthreads[kinds[i]];
  }
  return ARTIS_OK;
}

int artis_amd_last_kernel_ms_by_kind(artis_amd_engine *e, double ms[8], int64_t launches[8]) {
  if (!e || !ms) return ARTIS_ERR_ARG;
  const int kinds[5] = {NEXT_RPKT, NEXT_MA, NEXT_SLOW, NEXT_GAMMA, NEXT_BB};
  for (int i = 0; i < 8; i++) {
    ms[i] = 0.;
    if (launches) launches[i] = 0;
  }
  for (int i = 0; i < 5; i++) {
    ms[i] = e->last.kms[kinds[i]];
    if (launches) launches[i] = e->last.klaunches[kinds[i]];
  }
  ms[5] = e->last.kms_tail;
  ms[6] = e->last.fill_ms;
  ms[7] = e->last.kms_late;
  if (launches) {
    launches[5] = e->last.tail_launches;
    launches[7] = e->last.late_launches;
  }
  return ARTIS_OK;
}

int artis_amd_debug_visit_counts(artis_amd_engine *e, uint32_t *counts, int64_t n) {
  if (!e || !counts || n != (int64_t)e->Mh.npts_nonempty * e->Mh.nlevels) {
    g_last_error = "visit counts: [npts_nonempty][nlevels] uint32 expected";
    return ARTIS_ERR_ARG;
  }
  if (e->d_visit_counts == nullptr) {
    g_last_error = "this library was not built with -DARTIS_VISIT_COUNTS (or no propagation call has run yet)";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpy(counts, e->d_visit_counts, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
  return ARTIS_OK;
}

int artis_amd_debug_sort_list(artis_amd_engine *e, const int32_t *keys, const int32_t *list, int32_t n, int64_t nkeys, int32_t *out) {
  if (!e || n < 0 || (n > 0 && (!keys || !list || !out))) {
    g_last_error = "null argument or negative length";
    return ARTIS_ERR_ARG;
  }
  if (nkeys <= SORT_LDS_KEYS) {
    g_last_error = "debug_sort_list runs the many-keys sort: nkeys has to be above " + std::to_string(SORT_LDS_KEYS);
    return ARTIS_ERR_ARG;
  }
  if (nkeys > SORT_MAX_KEYS) {
    g_last_error = sort_too_many_keys_text(nkeys);
    return ARTIS_ERR_UNSUPPORTED;
  }
  for (int32_t i = 0; i < n; i++)
    if (keys[i] < 0 || keys[i] >= nkeys) {
      g_last_error = "a key is outside [0, nkeys)";
      return ARTIS_ERR_ARG;
    }
  if (n < 2 * BLOCK) {  // sort_by_key() leaves so short a list as it is
    if (n > 0) std::memcpy(out, list, sizeof(int32_t) * (size_t)n);
    return ARTIS_OK;
  }
  HIP_TRY(hipSetDevice(e->device));
  // the engine's own sort scratch (grown if this list is longer than its packet lists: it holds nothing between two sorts), buffers of the
  // call's own for keys, list and output: the engine's lists are not touched
  SortScratch &S = e->sort_scratch;
  int32_t *d_io = nullptr;  // keys, list, out
  int rc = (S.capacity >= n) ? ARTIS_OK : sort_scratch_alloc(S, n);
  if (rc == ARTIS_OK && hipMalloc((void **)&d_io, sizeof(int32_t) * 3 * (size_t)n) != hipSuccess) {
    g_last_error = "debug_sort_list: out of device memory";
    rc = ARTIS_ERR_HIP;
  }
  auto copy = [&](void *dst, const void *src, hipMemcpyKind kind) {
    if (rc == ARTIS_OK && hipMemcpy(dst, src, sizeof(int32_t) * (size_t)n, kind) != hipSuccess) {
      g_last_error = "debug_sort_list: copy failed";
      rc = ARTIS_ERR_HIP;
    }
  };
  copy(d_io, keys, hipMemcpyHostToDevice);
  copy(d_io + n, list, hipMemcpyHostToDevice);
  if (rc == ARTIS_OK) rc = sort_many_keys(e, S, nullptr, d_io + n, d_io, n, nkeys, d_io + 2 * (size_t)n);
  if (rc == ARTIS_OK && (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)) {
    g_last_error = "debug_sort_list: a sort kernel failed";
    rc = ARTIS_ERR_HIP;
  }
  copy(out, d_io + 2 * (size_t)n, hipMemcpyDeviceToHost);
  if (d_io) (void)hipFree(d_io);
  return rc;
}

}  // extern "C"

// ------------------------------------------------------------------ the cell cache's host side; the propagation driver; the timestep-end stages: spectra, radiation-field fit, ion balance, decay update, deposition rates; the pellet initialisation; thermal balance and its bound-free heating coefficients
#include "stage_cellcache.h"
#include "stage_propagate.h"
#include "stage_common.h"
#include "stage_spectra.h"
#include "stage_radfield.h"
#include "stage_ionbal.h"
#include "stage_decay.h"
#include "stage_deposition.h"
#include "stage_packet_init.h"
#include "stage_initial.h"
#include "stage_thermal.h"
#include "stage_bfheat.h"
#include "stage_ratecoeff.h"
#include "stage_photoion.h"
