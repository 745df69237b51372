// Prints what the host-callable functions of matchmaker_amd/csrc/bitonic_device.h and elem_device.h compute, for
// tests/test_device_primitives_cpu.py.  Floats go in and out as hexadecimal bit patterns.
//   device_primitives_check keys x [x ...]  -> "keys x desc_key unkey(desc_key) asc_key unkey(asc_key) desc_key_nan_last"
//   device_primitives_check bf16 x [x ...]  -> "bf16 x bf16_rne_bits bf16_rne_bits_nan"
//   device_primitives_check pow2 width v [width v ...] -> "pow2 width v pow2_ge(v)"  (width 32: int, 64: int64_t)
// Plain C++17, no HIP: the headers must compile on their own.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bitonic_device.h"
#include "elem_device.h"

static float from_bits(const char* hex) { return __builtin_bit_cast(float, (uint32_t)strtoul(hex, nullptr, 16)); }
static uint32_t bits(float f) { return __builtin_bit_cast(uint32_t, f); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "keys")) {
    for (int i = 2; i < argc; ++i) {
      const float x = from_bits(argv[i]);
      const uint32_t d = mm::desc_key(x), a = mm::asc_key(x);
      printf("keys %08x %08x %08x %08x %08x %08x\n", bits(x), d, bits(mm::desc_unkey(d)), a, bits(mm::asc_unkey(a)),
             mm::desc_key_nan_last(x));
    }
  } else if (!strcmp(argv[1], "bf16")) {
    for (int i = 2; i < argc; ++i) {
      const float x = from_bits(argv[i]);
      printf("bf16 %08x %04x %04x\n", bits(x), mm::bf16_rne_bits(x), mm::bf16_rne_bits_nan(x));
    }
  } else if (!strcmp(argv[1], "pow2")) {
    for (int i = 2; i + 1 < argc; i += 2) {
      const long long v = atoll(argv[i + 1]);
      if (!strcmp(argv[i], "32")) printf("pow2 32 %lld %lld\n", v, (long long)mm::pow2_ge((int)v));
      else printf("pow2 64 %lld %lld\n", v, (long long)mm::pow2_ge((int64_t)v));
    }
  } else {
    return 2;
  }
  return 0;
}
