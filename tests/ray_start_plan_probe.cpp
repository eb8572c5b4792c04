// Stand-alone probe of csrc/render_plan.h for tests/test_ray_start_plan.py: no HIP, no GPU, never loaded into python.
// stdin: one case per line -- tree_depth stack_lds_depth ray_start_lds specialise num_suns num_bulbs any_trans gi Nt wavefront traversal.
// stdout: the kernel decisions of each case, one line of name=value.
#include <cstdio>

#include "../cuda_ray_tracer_amd/csrc/render_plan.h"

int main()
{
  using namespace mirt;
  for (;;) {
    Options o; SceneFacts s; CallShape c;
    int trans = 0;
    const int n = scanf("%d %d %d %d %d %d %d %d %d %d %d", &s.tree_depth, &o.stack_lds_depth, &o.ray_start_lds, &o.specialise, &s.num_suns, &s.num_bulbs, &trans,
                        &s.gi, &s.Nt, &o.wavefront, &o.traversal);
    if (n != 11) return n == EOF ? 0 : 1;
    s.any_trans = trans != 0;
    s.N = 10000; s.grid_ok = true; s.has_quantised = s.Nt == 0; s.has_wide = s.Nt != 0;
    c.npix = 96 * 54; c.sample_count = 4; c.spp = 4;
    const CallPlan p = plan_call(s, o, c);
    printf("start_lds=%d lds_only=%d qn=%d notri=%d nobulb=%d nopend=%d slots=%d suns=%d stack_lds=%d\n", (int)p.start_lds, (int)p.lds_only, (int)p.qn, (int)p.notri,
           (int)p.nobulb, (int)p.nopend, START_LDS_SLOTS, START_LDS_SUNS, STACK_LDS);
  }
}
