// Prints what matchmaker_amd/csrc/launch_geometry.h computes, for tests/test_launch_geometry_cpu.py:
//   launch_geometry_check split n max [n max ...]        -> "split n max pairs_per_wave grid"
//   launch_geometry_check maps Bq Bd NQT [Bq Bd NQT ...] -> "tiled Bq Bd NQT gw t grid" and "ring Bq Bd NQT gw t grid"
//   launch_geometry_check cursor count size [count size ...] -> per block "take count size measured carved offset nullret", then
//                                                                "total measured carved left"; one layout per run, blocks of
//                                                                `count` elements of `size` bytes (1, 2, 3, 4, 8 or 12)
// Plain C++17, no HIP: the header must compile on its own.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "launch_geometry.h"

template <int N>
struct Bytes {
  char c[N];
};

// take<T>(count) for the T of `size` bytes; false: no such T here
static bool take(mm::WsCursor& ws, long long count, int size, void** out) {
  switch (size) {
    case 1: *out = ws.take<Bytes<1>>((size_t)count); return true;
    case 2: *out = ws.take<Bytes<2>>((size_t)count); return true;
    case 3: *out = ws.take<Bytes<3>>((size_t)count); return true;
    case 4: *out = ws.take<Bytes<4>>((size_t)count); return true;
    case 8: *out = ws.take<Bytes<8>>((size_t)count); return true;
    case 12: *out = ws.take<Bytes<12>>((size_t)count); return true;
    default: return false;
  }
}

// The layout argv names, run twice as an operator does: on a measuring cursor, then on a buffer of exactly the measured size.
// Every carved block is written end to end, so a block that leaves the buffer is a finding of a sanitizer build.
static int cursor_mode(int argc, char** argv) {
  mm::WsCursor measure;
  for (int i = 2; i + 1 < argc; i += 2) {
    void* p = nullptr;
    if (!take(measure, atoll(argv[i]), atoi(argv[i + 1]), &p)) return 2;
    if (p) return 3;   // a cursor with no base returns only null
  }
  const size_t total = measure.used;
  char* base = (char*)aligned_alloc(256, total ? total : 256);
  if (!base) return 4;
  mm::WsCursor carve(base, total), again;
  for (int i = 2; i + 1 < argc; i += 2) {
    const long long count = atoll(argv[i]);
    const int size = atoi(argv[i + 1]);
    void *p = nullptr, *q = nullptr;
    take(carve, count, size, &p);
    take(again, count, size, &q);
    if (!p) return 5;
    memset(p, 0x5a, (size_t)count * size);
    printf("take %lld %d %zu %zu %lld %d\n", count, size, again.used, carve.used, (long long)((char*)p - base), q == nullptr);
  }
  printf("total %zu %zu %zu\n", total, carve.used, carve.left);
  free(base);
  return 0;
}

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
  if (!strcmp(argv[1], "cursor")) return cursor_mode(argc, argv);
  return 2;
}
