// Prints what matchmaker_amd/csrc/launch_geometry.h computes, for tests/test_launch_geometry_cpu.py:
//   launch_geometry_check split n max [n max ...]        -> "split n max pairs_per_wave grid"
//   launch_geometry_check maps Bq Bd NQT [Bq Bd NQT ...] -> "tiled Bq Bd NQT gw t grid" and "ring Bq Bd NQT gw t grid"
// Plain C++17, no HIP: the header must compile on its own.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "launch_geometry.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  printf("kCUs %d\n", mm::kCUs);
  if (!strcmp(argv[1], "split")) {
    for (int i = 2; i + 1 < argc; i += 2) {
      const long long n = atoll(argv[i]), max = atoll(argv[i + 1]);
      const mm::WaveSplit s = mm::wave_split(n, max);
      printf("split %lld %lld %lld %lld\n", n, max, (long long)s.pairs_per_wave, (long long)s.grid);
    }
    return 0;
  }
  if (!strcmp(argv[1], "maps")) {
    for (int i = 2; i + 2 < argc; i += 3) {
      const long long Bq = atoll(argv[i]), Bd = atoll(argv[i + 1]);
      const int nqt = atoi(argv[i + 2]);
      const mm::AllPairsMap t = mm::all_pairs_tiled(Bq, Bd, nqt), r = mm::all_pairs_ring(Bq, Bd, nqt);
      printf("tiled %lld %lld %d %d %d %lld\n", Bq, Bd, nqt, t.gw, t.t, (long long)t.grid);
      printf("ring %lld %lld %d %d %d %lld\n", Bq, Bd, nqt, r.gw, r.t, (long long)r.grid);
    }
    return 0;
  }
  return 2;
}
