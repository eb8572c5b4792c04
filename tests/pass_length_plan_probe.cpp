// Stand-alone probe of csrc/render_plan.h for tests/test_plan_pass_length.py: no HIP, no GPU, never loaded into python.
// stdin: one case per line -- prim_ratio (a float; negative: not known) reps batch_k Nt N qnodes traversal wavefront tree_depth.
// stdout: the pass length and batch threshold of each case and the kind of kernel, one line of name=value.
#include <cstdio>

#include "../cuda_ray_tracer_amd/csrc/render_plan.h"

int main()
{
  using namespace mirt;
  for (;;) {
    Options o; SceneFacts s; CallShape c;
    const int n = scanf("%f %d %d %d %d %d %d %d %d", &s.prim_ratio, &o.reps, &o.batch_k, &s.Nt, &s.N, &o.qnodes, &o.traversal, &o.wavefront, &s.tree_depth);
    if (n != 9) return n == EOF ? 0 : 1;
    s.grid_ok = true; s.has_quantised = s.Nt == 0; s.has_wide = s.Nt != 0; s.num_suns = 1;
    c.npix = 64 * 36; c.sample_count = 4; c.spp = 4;
    const CallPlan p = plan_call(s, o, c);
    printf("reps=%d batch_k=%d qn=%d notri=%d start_lds=%d\n", p.reps, p.batch_k, (int)p.qn, (int)p.notri, (int)p.start_lds);
  }
}
