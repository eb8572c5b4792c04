// Stand-alone probe of csrc/query_launch.h for tests/test_group_launch.py: no HIP, no GPU, never loaded into python.
// stdin: one case per line, "n lanes_per_row cached_blocks".  stdout: "gshift=.. blocks=.. row_blocks=.. block=.. stack_lds=.." per case
// (row_blocks: row_launch(n, cached_blocks), whatever lanes_per_row is).
#include <cstdio>

#include "../cuda_ray_tracer_amd/csrc/query_launch.h"

int main()
{
  using namespace mirt;
  for (;;) {
    long long n = 0;
    int lanes = 0, cached = 0;
    const int got = scanf("%lld %d %d", &n, &lanes, &cached);
    if (got != 3) return got == EOF ? 0 : 1;
    const GroupLaunch g = group_launch(n, lanes, cached);
    printf("gshift=%d blocks=%d row_blocks=%d block=%d stack_lds=%d\n", g.gshift, g.blocks, row_launch(n, cached), QUERY_BLOCK, QUERY_STACK_LDS);
  }
}
