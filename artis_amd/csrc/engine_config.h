// engine_config.h -- the engine's configuration (include/artis_amd.h artis_amd_config): the caller's struct copied and checked, then resolved
// ONCE -- struct field, else ARTIS_AMD_* variable, else built-in default -- into the values the engine's sizing code and driver read.
// Host code only (no HIP, no model tables): included by artis_engine.hip, and small enough to be compiled into a stand-alone program.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/artis_amd.h"

namespace artis {

// X(field) for every field of artis_amd_config after struct_size, in the struct's order
#define ARTIS_CONFIG_FIELDS(X) \
  X(cache_budget_bytes)        \
  X(cache_headroom_bytes)      \
  X(pop_scratch_bytes)         \
  X(ma_hot_fraction)           \
  X(ma_pool_fraction)          \
  X(tail_threshold)            \
  X(tile_park_at)              \
  X(keep_line_dpop)            \
  X(reserved)

// every field "automatic / default"
inline void config_set_default(artis_amd_config *cfg) {
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->struct_size = sizeof(artis_amd_config);
  cfg->cache_budget_bytes = 0;
  cfg->cache_headroom_bytes = -1;
  cfg->pop_scratch_bytes = -1;
  cfg->ma_hot_fraction = -1.;
  cfg->ma_pool_fraction = -1.;
  cfg->tail_threshold = -1;
  cfg->tile_park_at = -1;
  cfg->keep_line_dpop = -1;
  cfg->reserved = 0;
}

// The caller's struct (null: the defaults) into the library's: the fields that lie wholly inside the caller's struct_size are copied -- nothing
// beyond it is read --, the others keep their defaults (an older caller's smaller struct); then every value is checked. Returns ARTIS_OK, or
// ARTIS_ERR_ARG with the reason in *err.
inline int config_copy_checked(const artis_amd_config *in, artis_amd_config *out, std::string *err) {
  config_set_default(out);
  if (in) {
    size_t n = 0;
    std::memcpy(&n, in, sizeof(n));  // (struct_size is the first member)
    if (n > sizeof(artis_amd_config)) {
      *err = "artis_amd_config.struct_size (" + std::to_string(n) + ") is larger than this library's (" + std::to_string(sizeof(artis_amd_config)) +
             "): the caller was built against a newer header";
      return ARTIS_ERR_ARG;
    }
    if (n < sizeof(size_t)) {
      *err = "artis_amd_config.struct_size (" + std::to_string(n) + ") does not cover struct_size itself: call artis_amd_config_default() first";
      return ARTIS_ERR_ARG;
    }
#define COPY(f) \
  if (offsetof(artis_amd_config, f) + sizeof(out->f) <= n) std::memcpy(&out->f, (const char *)in + offsetof(artis_amd_config, f), sizeof(out->f));
    ARTIS_CONFIG_FIELDS(COPY)
#undef COPY
  }
  const artis_amd_config &c = *out;
  if (c.reserved != 0) {
    *err = "artis_amd_config.reserved must be 0";
    return ARTIS_ERR_ARG;
  }
  if (c.cache_budget_bytes < 0) {
    *err = "artis_amd_config.cache_budget_bytes is negative (0 = automatic)";
    return ARTIS_ERR_ARG;
  }
  if (c.cache_headroom_bytes < -1 || c.pop_scratch_bytes < -1 || c.tail_threshold < -1 || c.tile_park_at < -1) {
    *err = "artis_amd_config: cache_headroom_bytes, pop_scratch_bytes, tail_threshold and tile_park_at are -1 (default) or >= 0";
    return ARTIS_ERR_ARG;
  }
  if (!(c.ma_hot_fraction < 0.) && !(c.ma_hot_fraction > 0. && c.ma_hot_fraction <= 1.)) {  // (a NaN is neither)
    *err = "artis_amd_config.ma_hot_fraction must lie in (0, 1] (< 0 = automatic)";
    return ARTIS_ERR_ARG;
  }
  if (!(c.ma_pool_fraction == -1.) && !(c.ma_pool_fraction >= 0.)) {
    *err = "artis_amd_config.ma_pool_fraction must be >= 0 (-1 = default)";
    return ARTIS_ERR_ARG;
  }
  if (c.keep_line_dpop < -1 || c.keep_line_dpop > 1) {
    *err = "artis_amd_config.keep_line_dpop must be -1 (automatic), 0 or 1";
    return ARTIS_ERR_ARG;
  }
  return ARTIS_OK;
}

// where a resolved value came from
enum ConfigSource : uint8_t { CONFIG_DEFAULT = 0, CONFIG_ENV = 1, CONFIG_STRUCT = 2 };
inline const char *config_source_name(uint8_t s) { return s == CONFIG_STRUCT ? "struct" : (s == CONFIG_ENV ? "environment" : "default"); }

constexpr double MA_ABSENT_EPS_DEFAULT = 1e-12;  // (the shortest headline step of the values measured: profiles/r12/absent_ions.md)
// The resolved configuration: what cache_budget_bytes(), the record-tier choice, the population scratch and the driver read. Bytes are kept as
// doubles, the form the sizing rule computes in (a variable in MB times 2^20 is exact).
struct EngineConfig {
  bool budget_given = false;       // cache_budget is the whole answer; else the automatic rule (80 % of free memory less scratch and head-room)
  double cache_budget = 0.;        // [B]
  double cache_headroom = 0.;      // [B]
  double pop_scratch = 2048. * 1048576.;  // [B]
  bool hot_given = false;          // ma_hot is the record tiers' hot share; else the sizing code chooses it (fewest tiles)
  double ma_hot = 1.;
  double ma_pool = 0.15;
  bool tail_given = false;         // else the build's own default (artis_amd_engine::tail_max)
  int tail_threshold = 0;
  bool park_given = false;
  int64_t tile_park_at = 0;
  int keep_line_dpop = -1;         // -1: dropped when that saves tiles; 0: dropped; 1: kept
  bool dpop_strict = false;        // ... kept or the creation fails (asked for through the struct)
  // k_thermal's unit budget BEFORE its list is used up, in launches that hand over at list exhaustion (stage_propagate.h launch_thermal): 0 = none,
  // a packet keeps its lane while the list lasts (the default); > 0: that many units (the launch's own budget, 2048 or 1024, gives the rule of
  // before). No struct field: a placement switch like the other budgets (ARTIS_AMD_BUDGET_T_BULK), resolved here with the rest.
  bool bulk_given = false;
  int budget_t_bulk = 0;
  // ABSENT IONS (tables.h): the population leaves out the static macro-atom records of an ion whose population in the cell is <= eps * its element's;
  // the first visit fills such a record (results do not depend on it). < 0: everything is populated; 0: ions without any population only; 1: every
  // ion, every record filled at its first visit (tests). No struct field: a placement switch (ARTIS_AMD_MA_ABSENT_EPS).
  double ma_absent_eps = MA_ABSENT_EPS_DEFAULT;
  uint8_t src_budget = 0, src_headroom = 0, src_scratch = 0, src_hot = 0, src_pool = 0, src_tail = 0, src_park = 0, src_dpop = 0, src_bulk = 0, src_absent = 0;
};

// THE resolution point: a field set in the (checked) struct wins; a field left at "automatic / default" takes its ARTIS_AMD_* variable if that is
// set, with the clamps those variables always had; otherwise the built-in default. No other place reads these variables.
inline EngineConfig resolve_config(const artis_amd_config &c) {
  EngineConfig r;
  if (c.cache_budget_bytes > 0) {
    r.budget_given = true, r.cache_budget = (double)c.cache_budget_bytes, r.src_budget = CONFIG_STRUCT;
  } else if (const char *b = std::getenv("ARTIS_AMD_CACHE_BUDGET_MB")) {
    r.budget_given = true, r.cache_budget = std::atof(b) * 1048576.0, r.src_budget = CONFIG_ENV;
  }
  if (c.cache_headroom_bytes >= 0) {
    r.cache_headroom = (double)c.cache_headroom_bytes, r.src_headroom = CONFIG_STRUCT;
  } else if (const char *b = std::getenv("ARTIS_AMD_CACHE_HEADROOM_MB")) {
    r.cache_headroom = std::max(0., std::atof(b)) * 1048576.0, r.src_headroom = CONFIG_ENV;
  }
  if (c.pop_scratch_bytes >= 0) {
    r.pop_scratch = (double)c.pop_scratch_bytes, r.src_scratch = CONFIG_STRUCT;
  } else if (const char *b = std::getenv("ARTIS_AMD_POP_SCRATCH_MB")) {
    r.pop_scratch = std::max(1., std::atof(b)) * 1048576.0, r.src_scratch = CONFIG_ENV;
  }
  if (c.ma_hot_fraction > 0.) {
    r.hot_given = true, r.ma_hot = c.ma_hot_fraction, r.src_hot = CONFIG_STRUCT;
  } else if (const char *b = std::getenv("ARTIS_AMD_MA_HOTFRAC")) {
    r.hot_given = true, r.ma_hot = std::min(1., std::max(0., std::atof(b))), r.src_hot = CONFIG_ENV;
  }
  if (c.ma_pool_fraction >= 0.) {
    r.ma_pool = std::min(1., c.ma_pool_fraction), r.src_pool = CONFIG_STRUCT;  // (the whole of the cold records: nothing above it to hold)
  } else if (const char *b = std::getenv("ARTIS_AMD_MA_POOLFRAC")) {
    r.ma_pool = std::min(1., std::max(0., std::atof(b))), r.src_pool = CONFIG_ENV;
  }
  if (c.tail_threshold >= 0) {
    r.tail_given = true, r.tail_threshold = (int)std::min<int64_t>(c.tail_threshold, INT_MAX), r.src_tail = CONFIG_STRUCT;
  } else if (const char *b = std::getenv("ARTIS_AMD_TAIL")) {
    r.tail_given = true, r.tail_threshold = std::max(0, std::atoi(b)), r.src_tail = CONFIG_ENV;
  }
  if (c.tile_park_at >= 0) {
    r.park_given = true, r.tile_park_at = c.tile_park_at, r.src_park = CONFIG_STRUCT;
  } else if (const char *b = std::getenv("ARTIS_AMD_TILE_PARK_AT")) {
    r.park_given = true, r.tile_park_at = std::max<int64_t>(0, std::atoll(b)), r.src_park = CONFIG_ENV;
  }
  if (c.keep_line_dpop >= 0) {
    r.keep_line_dpop = c.keep_line_dpop, r.dpop_strict = c.keep_line_dpop == 1, r.src_dpop = CONFIG_STRUCT;
  } else if (const char *b = std::getenv("ARTIS_AMD_DPOP")) {
    r.keep_line_dpop = std::atoi(b) == 0 ? 0 : 1, r.src_dpop = CONFIG_ENV;
  }
  if (const char *b = std::getenv("ARTIS_AMD_BUDGET_T_BULK")) {
    r.bulk_given = true, r.budget_t_bulk = std::max(0, std::atoi(b)), r.src_bulk = CONFIG_ENV;
  }
  if (const char *b = std::getenv("ARTIS_AMD_MA_ABSENT_EPS")) {
    const double v = std::atof(b);
    r.ma_absent_eps = (v >= 0.) ? std::min(1., v) : -1., r.src_absent = CONFIG_ENV;  // (a NaN: populate everything)
  }
  return r;
}

// Bytes the cell-cache rows may take. artis_amd_config.cache_budget_bytes when it is set: the whole answer, whatever else is on the device.
// Left at 0: 80 % of what is free once the population's scratch (pop_scratch_bytes) and a head-room for everything that is allocated later
// (cache_headroom_bytes, default 0: the packets at ~1 KB each with their work lists, the caller's structs and a snapshot -- 10 GB at 1e7 packets --
// fit the remaining fifth of a 288 GB card; a smaller GPU, or two engines on one device, set it) are taken off. ARTIS_AMD_CACHE_BUDGET_MB,
// _CACHE_HEADROOM_MB and _POP_SCRATCH_MB stand in for a field that is left at its default (resolve_config). One rule for the tile count and for the
// decision to drop line_dpop.
inline double cache_budget_bytes(const EngineConfig &cfg, double free_b) {
  if (cfg.budget_given) return cfg.cache_budget;
  return std::max(0., 0.8 * (free_b - (cfg.pop_scratch + cfg.cache_headroom)));
}

}  // namespace artis
