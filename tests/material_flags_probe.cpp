// Stand-alone probe of csrc/material_flags.h (tests/test_shading_update_abi.py): reads material rows from standard input, 11
// hexadecimal float32 words per line (colour rgb, shininess rgb, trans rgb, ior, roughness), and prints material_flags of each,
// one number per line.  Plain host C++: the header needs no HIP.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../cuda_ray_tracer_amd/csrc/material_flags.h"

int main()
{
  for (;;) {
    float m[11];
    for (int k = 0; k < 11; ++k) {
      unsigned word = 0;
      if (scanf("%x", &word) != 1) return k == 0 ? 0 : 2;      // (a short row is an error)
      const uint32_t w = word;
      memcpy(&m[k], &w, sizeof(float));
    }
    printf("%u\n", mirt::material_flags(m));
  }
}
