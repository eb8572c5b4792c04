// Stand-alone probe of csrc/render_plan.h for tests/test_render_plan.py: no HIP, no GPU, never loaded into python.
// stdin: one case per line, 34 integers in the order of the reads below.  stdout: the plan of each case, one line of name=value.
#include <cstdio>

#include "../cuda_ray_tracer_amd/csrc/render_plan.h"

int main()
{
  using namespace mirt;
  for (;;) {
    Options o; SceneFacts s; CallShape c;
    int b[10], blocks = 0;
    int n = scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &o.traversal, &o.wavefront, &o.qnodes, &o.specialise, &o.sched, &o.slab_log2, &o.stack_lds_depth,
                  &o.refill_k, &o.init_k, &o.leaf_k, &o.reps, &o.skip_unlit, &o.shadow_anyhit, &o.chunk_shift);
    if (n != 14) return n == EOF ? 0 : 1;
    if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &s.N, &s.Nt, &b[0], &b[1], &b[2], &b[3], &b[4], &b[5], &s.gi, &s.bounces, &s.num_suns, &s.num_bulbs) != 12) return 1;
    s.grid_ok = b[0]; s.has_quantised = b[1]; s.has_wide = b[2]; s.colors_finite = b[3]; s.any_trans = b[4]; s.any_rough = b[5];
    if (scanf("%lld %d %d %d %d %lld %d %d", &c.npix, &c.sample_first, &c.sample_count, &c.spp, &b[6], &c.num_listed, &b[7], &blocks) != 8) return 1;
    c.accumulate = b[6]; c.counters = b[7];
    const CallPlan p = plan_call(s, o, c);
    printf("slab_pixels=%lld nslabs=%d slab_samples_max=%lld listed_max=%lld launch_samples_max=%lld total_samples=%lld per_pixel_seed=%d args_spp=%d "
           "rng_sample_tables=%d shading_rng=%d notri=%d qn=%d swap_mask=%u reach_check=%d node_bytes=%d nobulb=%d nopend=%d need_pending=%d pending_slots=%d "
           "skip_unlit=%d shadow_anyhit=%d refill_k=%d init_k=%d leaf_k=%d reps=%d lds_depth=%d hand_out=%d chunk_shift=%d stack_lds=%d\n",
           p.slab_pixels, p.nslabs, p.slab_samples_max, p.listed_max, p.launch_samples_max, p.total_samples, (int)p.per_pixel_seed, p.args_spp,
           p.rng_sample_tables, (int)p.shading_rng, (int)p.notri, (int)p.qn, p.swap_mask, p.reach_check, p.node_bytes, (int)p.nobulb, (int)p.nopend,
           (int)p.need_pending, p.pending_slots, p.skip_unlit, p.shadow_anyhit, p.refill_k, p.init_k, p.leaf_k, p.reps, p.lds_depth, (int)p.hand_out,
           plan_chunk_shift(p.launch_samples_max, blocks, o.chunk_shift), STACK_LDS);
  }
}
