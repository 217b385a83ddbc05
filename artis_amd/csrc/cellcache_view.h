// cellcache_view.h -- where one array of a cell's row lies, for the views that show a row as stored (artis_amd_debug_cellcache_array of
// stage_cellcache.h; the same view of the host emulation's rows, tests/hostemu). Pointers are the owner's: device pointers in the engine.
#pragma once
#include "tables.h"

namespace artis {

struct CcArrayView {
  const void *base;  // element 0 of row 0
  size_t elem;       // bytes per element
  int64_t per;       // elements per row
  bool by_row;       // a cache array: the row of a cell is physics.h krow(); false: an array of DevCells, indexed by the cell
};

// false: the array does not exist in this build or model, or `which` is no enumerator. expopac_own: the expansion-opacity tables are the
// engine's own (the host handed none over).
inline bool cc_array_view(const DevModel &M, const DevCells &C, const DevCache &K, bool expopac_own, int which, CcArrayView *v) {
#define CC_VIEW(ptr, T, n, by_row)                              \
  {                                                             \
    if ((n) <= 0 || (ptr) == nullptr) return false;             \
    *v = CcArrayView{(ptr), sizeof(T), (int64_t)(n), (by_row)}; \
    return true;                                                \
  }
#define CC_ROW(ptr, T, n) CC_VIEW(ptr, T, n, true)
#define CC_CELL(ptr, T, n) CC_VIEW(ptr, T, n, false)
  switch (which) {
    case ARTIS_AMD_CC_LINE_DPOP: CC_ROW(K.line_dpop, double, M.ndpop)
    case ARTIS_AMD_CC_BF_RADRECOMB: CC_ROW(K.bf_radrecomb, double, M.nphixstargets_total)
    case ARTIS_AMD_CC_BF_COLRECOMB: CC_ROW(K.bf_colrecomb, double, M.nphixstargets_total)
    case ARTIS_AMD_CC_BF_COLION: CC_ROW(K.bf_colion, double, M.nphixstargets_total)
    case ARTIS_AMD_CC_BF_COOLING: CC_ROW(K.bf_cooling, double, M.nphixstargets_total)
    case ARTIS_AMD_CC_ALLCONT_PAIR: CC_ROW(K.allcont_pair, D2, M.nbfcontinua)
    case ARTIS_AMD_CC_ALLCONT_KEPTLIST: CC_ROW(K.allcont_keptlist, int32_t, M.nbfcontinua)
    case ARTIS_AMD_CC_ALLCONT_KEEPPREFIX: CC_ROW(K.allcont_keepprefix, int32_t, M.nbfcontinua > 0 ? M.nkeepwords : 0)
    case ARTIS_AMD_CC_ALLCONT_KEPTPAIR: CC_ROW(K.allcont_keptpair, D2, M.nbfcontinua)
    case ARTIS_AMD_CC_ALLCONT_KEEPBITS: CC_ROW(K.allcont_keepbits, uint64_t, M.nbfcontinua > 0 ? M.nkeepwords : 0)
    case ARTIS_AMD_CC_COOL_GUIDE: CC_ROW(K.cool_guide, uint16_t, M.nguide)
    case ARTIS_AMD_CC_ION_COOLING_C: CC_ROW(K.ion_cooling_C, double, M.nions)
#if ARTIS_EXPOPAC_TABLES
    case ARTIS_AMD_CC_EXPANSIONOPACITIES: CC_CELL(expopac_own ? C.expansionopacities : nullptr, float, ARTIS_EXPOPAC_NBINS)
    case ARTIS_AMD_CC_EXPANSIONOPACITY_PLANCK_CUMULATIVE:
      CC_CELL((expopac_own && ARTIS_OPT_RPKT_BB_THERMALISATION) ? C.expansionopacity_planck_cumulative : nullptr, double, ARTIS_EXPOPAC_NBINS)
#endif
#if ARTIS_OPT_NT_ON
    case ARTIS_AMD_CC_NT_IONRATECOEFF: CC_CELL(C.nt_ionratecoeff, double, M.nions)
    case ARTIS_AMD_CC_NT_IONENRATE_CUM: CC_CELL(C.nt_ionenrate_cum, double, M.nions)
#endif
    default: break;
  }
#undef CC_ROW
#undef CC_CELL
#undef CC_VIEW
  (void)expopac_own;
  return false;
}

}  // namespace artis
