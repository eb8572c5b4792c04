// Stand-alone probe of csrc/render_plan.h for tests/test_stack_plan.py: no HIP, no GPU, never loaded into python.
// stdin: one case per line -- tree_depth stack_lds_depth wavefront traversal qnodes N Nt grid_ok has_quantised has_wide.
// stdout: the stack decisions of each case, one line of name=value.
#include <cstdio>

#include "../cuda_ray_tracer_amd/csrc/render_plan.h"

int main()
{
  using namespace mirt;
  for (;;) {
    Options o; SceneFacts s; CallShape c;
    int g = 0, q = 0, w = 0;
    const int n = scanf("%d %d %d %d %d %d %d %d %d %d", &s.tree_depth, &o.stack_lds_depth, &o.wavefront, &o.traversal, &o.qnodes, &s.N, &s.Nt, &g, &q, &w);
    if (n != 10) return n == EOF ? 0 : 1;
    s.grid_ok = g; s.has_quantised = q; s.has_wide = w;
    c.npix = 64 * 64; c.sample_count = 4; c.spp = 4;
    const CallPlan p = plan_call(s, o, c);
    printf("lds_only=%d lds_depth=%d qn=%d notri=%d capacity=%d stack_lds=%d\n", (int)p.lds_only, p.lds_depth, (int)p.qn, (int)p.notri, STACK_LDS_CAPACITY, STACK_LDS);
  }
}
