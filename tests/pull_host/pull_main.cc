// Test-only: the work-pulling rules of artis_amd/csrc/work_pull.h compiled for x86 (ARTIS_HOST_EMU). A stand-alone program: it simulates the waves of
// a launch pulling from a list of n entries -- lanes keep an entry for a few turns, the waves take turns in a random order -- and checks that every
// index of [0, n) is handed out exactly once, that every wave ends up exhausted, and that nothing outside the launch's cursor slots is written.
//   pull_main            runs the built-in cases, prints a summary line, exits 0 when all hold
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define ARTIS_HOST_EMU 1
#include "../../artis_amd/csrc/work_pull.h"

namespace {
struct Wave {
  Puller q;
  unsigned long long have = 0;  // lanes that hold an entry
  int left[64] = {};            // ... and for how many more turns
};
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}
// one launch: nblocks workgroups of waves_per_block waves; a lane keeps an entry for 1..hold turns
bool run_case(int32_t n, int nchunks, int nblocks, int waves_per_block, int hold) {
  const int guard = 64;  // slots behind the allocation that must stay untouched
  std::vector<int32_t> cursors(PULL_SLOTS + guard, 0);
  for (int i = PULL_SLOTS; i < PULL_SLOTS + guard; i++) cursors[i] = 0x5A5A5A5A;
  std::vector<int> handed((size_t)(n > 0 ? n : 1), 0);
  std::vector<Wave> waves((size_t)nblocks * waves_per_block);
  std::vector<int> live(waves.size());
  for (int b = 0; b < nblocks; b++)
    for (int w = 0; w < waves_per_block; w++) {
      const int i = b * waves_per_block + w;
      puller_place(waves[(size_t)i].q, b & 7, (b >> 3) * waves_per_block + w, n, nchunks);
      live[(size_t)i] = i;
    }
  long long turns = 0;
  while (!live.empty()) {
    if (++turns > 50000000LL) {
      printf("  no end\n");
      return false;
    }
    const size_t pick = rnd() % live.size();
    Wave &w = waves[(size_t)live[pick]];
    // lanes finish; then the free lanes ask, as the kernels' loops do
    for (int l = 0; l < 64; l++)
      if ((w.have >> l & 1) && --w.left[l] <= 0) w.have &= ~(1ull << l);
    const unsigned long long mask = w.q.exhausted ? 0 : ~w.have;
    if (mask != 0) {
      int64_t first = 0, end = 0;
      pull_wave(w.q, mask, cursors.data(), &first, &end);
      int p = 0;
      for (int l = 0; l < 64; l++) {
        if (!(mask >> l & 1)) continue;
        const int64_t mine = first + p++;
        if (mine >= end) continue;
        if (mine < 0 || mine >= n) {
          printf("  index %lld outside the list\n", (long long)mine);
          return false;
        }
        handed[(size_t)mine]++;
        w.have |= 1ull << l;
        w.left[l] = 1 + (int)(rnd() % (uint32_t)hold);
      }
    }
    if (w.q.exhausted && w.have == 0) {
      live[pick] = live.back();
      live.pop_back();
    }
  }
  for (int32_t i = 0; i < n; i++)
    if (handed[(size_t)i] != 1) {
      printf("  index %d handed out %d times\n", i, handed[(size_t)i]);
      return false;
    }
  for (int i = PULL_SLOTS; i < PULL_SLOTS + guard; i++)
    if (cursors[i] != 0x5A5A5A5A) {
      printf("  slot %d behind the cursors was written\n", i);
      return false;
    }
  if (cursors[MAX_CHUNKS] != 0) {  // the "list used up" flag is the kernels' to set, never the puller's
    printf("  the puller wrote the launch's flag\n");
    return false;
  }
  return true;
}
}  // namespace

int main() {
  // chunk counts as chunks_for() gives them: multiples of 8 up to MAX_CHUNKS; lengths: empty, below and around a wave, fewer entries than chunks,
  // no multiple of 64 or of the chunk count
  const int chunk_counts[] = {8, 16, 256, 1024, MAX_CHUNKS};
  const int32_t lengths[] = {0, 1, 63, 64, 65, 1000, 4097, 50000};
  int failed = 0, cases = 0;
  for (const int nchunks : chunk_counts)
    for (const int32_t n : lengths)
      for (const int hold : {1, 5}) {
        const int nblocks = (nchunks <= 16) ? 16 : 40, wpb = (nchunks <= 16) ? 4 : 16;
        cases++;
        if (!run_case(n, nchunks, nblocks, wpb, hold)) {
          failed++;
          printf("FAILED: n %d nchunks %d hold %d\n", n, nchunks, hold);
        }
      }
  printf("%d cases, %d failed\n", cases, failed);
  return failed == 0 ? 0 : 1;
}
