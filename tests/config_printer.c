/* Test helper: prints sizeof and every field's offsetof of artis_amd_config and artis_amd_plan as the C compiler lays them out from
 * include/artis_amd.h (tests/test_config_abi.py compares artis_amd/abi.py's ctypes mirrors and the library's own sizes with it). */
#include <stddef.h>
#include <stdio.h>

#include "../include/artis_amd.h"

#define C(f) printf("config.%s %zu %zu\n", #f, offsetof(artis_amd_config, f), sizeof(((artis_amd_config *)0)->f))
#define P(f) printf("plan.%s %zu %zu\n", #f, offsetof(artis_amd_plan, f), sizeof(((artis_amd_plan *)0)->f))

int main(void) {
  printf("config.sizeof %zu 0\n", sizeof(artis_amd_config));
  C(struct_size);
  C(cache_budget_bytes);
  C(cache_headroom_bytes);
  C(pop_scratch_bytes);
  C(ma_hot_fraction);
  C(ma_pool_fraction);
  C(tail_threshold);
  C(tile_park_at);
  C(keep_line_dpop);
  C(reserved);
  printf("plan.sizeof %zu 0\n", sizeof(artis_amd_plan));
  P(struct_size);
  P(bytes_per_cell);
  P(cells_resident);
  P(ntiles);
  P(ncold_levels);
  P(hot_fraction);
  P(pool_slots);
  P(cache_bytes);
  P(pool_bytes);
  P(pop_scratch_bytes);
  P(model_bytes);
  P(free_bytes_assumed);
  P(line_dpop_kept);
  P(reserved);
  return 0;
}
