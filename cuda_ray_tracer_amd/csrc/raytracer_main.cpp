// raytracer -- the reference's command line (main.cu:25-94) over libmirt's C ABI:
//
//     raytracer scene.txt [--width W] [--height H] [--spp N] [--out file.png] [--device D] [--gpus N] [--frames K]
//                         [--traversal 0|1|2] [--bounds-as-shipped] [--adaptive V [--min-spp N] [--step N]] [--denoise K]
//
// Same contract: one positional scene file, the PNG is named by the scene's `png W H name` line and written to the
// current directory, the same lines go to stdout -- the phase timings (main.cu:39,61,71,80,93, with the reference's labels:
// the last one reads "cudaFree time:"), the build lines and, for at most 16 primitives, the "Node Info" dump of every node
// (lbvh_builder.cu:489-520), the "[DEBUG Render]" line of the many-samples kernel (draw.cu:232) -- and the reference's error
// messages + exit codes are kept ("Error opening file...", "One of the lines are not valid.": exit 1; device errors:
// EXIT_FAILURE).  The optional flags override resolution / samples per pixel of the scene file (BASELINE.json's configs do).
// --gpus N renders the frame on N GPUs of this node (image stripes, replicated BVH, RCCL framebuffer gather: mirt_multi_*);
// --frames K renders K frames back to back (consecutive frames overlap on every device) and reports ms per frame.
// --adaptive V: adaptive sampling (mirt_render_accumulate_pixels / mirt_select_pixels / mirt_finalize_counts): --min-spp samples
// (default 4) for every pixel, then rounds of --step more (default: --min-spp) for the pixels whose estimated variance of the mean
// exceeds V, up to --spp samples per pixel; one line reports the samples used.  One GPU only.
// --denoise K: the frame's sample moments (all --spp samples of every pixel, or what --adaptive leaves) are filtered by K iterations
// of mirt_denoise with the default scales, guided by the closest hits of the frame's camera rays (mirt_camera_rays ->
// mirt_trace_rays -> mirt_hit_features); the image is the filtered mean.  One GPU only.
// --bounds-as-shipped builds the tree of the shipped reference (scene bounds never stored, parse.cpp:28: every Morton code 0).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/mirt.h"

static void die_on(int rc, const char* what)
{
  if (rc == MIRT_OK) return;
  if (rc == MIRT_ERR_IO || rc == MIRT_ERR_PARSE) { std::cout << mirt_last_error() << std::endl; exit(1); }
  std::cerr << "Error in " << what << " : " << mirt_last_error() << std::endl;
  exit(EXIT_FAILURE);
}
#define HIP_CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::cerr << "HIP Error in " << __FILE__ << " at line " << __LINE__ << " : " << hipGetErrorString(e_) << std::endl; exit(EXIT_FAILURE); } } while (0)

// The reference's debug dump of a small tree (lbvh_builder.cu:496-520), same format.  visited_atomic_counter: the refit leaves 2
// in every internal node (both children arrived, lbvh_builder.cu:343-359); a leaf's counter and child offsets are never written
// by the reference (fresh cudaMalloc memory) and print as 0 here, an internal node's primitive_offset likewise.
static void print_node_info(MirtScene* sc, int n)
{
  std::vector<MirtTreeNode> nodes(2 * (size_t)n - 1);
  if (mirt_get_tree(sc, nodes.data(), nullptr, nullptr, nullptr) != MIRT_OK) return;
  printf("Node Info:\n");
  for (int i = 0; i < 2 * n - 1; ++i) {
    const MirtTreeNode& t = nodes[i];
    printf("  Node %d: num_primitives_in_leaf=%d, primitive_offset=%d, left_child_offset=%d, right_child_offset=%d, visited_atomic_counter=%u, bbox=(min: %.2f, %.2f, %.2f, max: %.2f, %.2f, %.2f)\n",
           i, (int)t.count, (int)t.prim_offset, (int)t.left, (int)t.right, t.count ? 0u : 2u, t.xmin, t.ymin, t.zmin, t.xmax, t.ymax, t.zmax);
  }
}

// draw.cu:222-232: the kernel for aa > 1 announces its launch (one thread per sample, blocks of 128)
static void print_debug_render(int width, int height, int spp)
{
  if (spp <= 1) return;
  const int block_size = 128;
  const int total_threads = width * height * spp;
  printf("[DEBUG Render] Launching AA Kernel. Total Threads: %d, Grid: %d, Block: %d\n", total_threads, (total_threads + block_size - 1) / block_size, block_size);
}

int main(int argc, char* argv[])
{
  if (argc < 2) { std::cout << "Error opening file..." << std::endl; return 1; }
  int ow = 0, oh = 0, ospp = -1, device = 0, gpus = 1, traversal = -1, frames = 1, shipped = 0;
  int min_spp = 4, step = 0, denoise = -1;
  bool adaptive = false;
  float max_variance = 0.0f;
  std::string out_override;
  for (int i = 2; i < argc; ++i) {
    std::string a = argv[i];
    auto need = [&](int k) { if (i + k >= argc) { std::cerr << "missing value for " << a << std::endl; exit(2); } };
    if (a == "--width") { need(1); ow = atoi(argv[++i]); }
    else if (a == "--height") { need(1); oh = atoi(argv[++i]); }
    else if (a == "--spp") { need(1); ospp = atoi(argv[++i]); }
    else if (a == "--out") { need(1); out_override = argv[++i]; }
    else if (a == "--device") { need(1); device = atoi(argv[++i]); }
    else if (a == "--gpus") { need(1); gpus = atoi(argv[++i]); }
    else if (a == "--traversal") { need(1); traversal = atoi(argv[++i]); }
    else if (a == "--frames") { need(1); frames = atoi(argv[++i]); if (frames < 1) frames = 1; }
    else if (a == "--bounds-as-shipped") shipped = 1;
    else if (a == "--adaptive") { need(1); adaptive = true; max_variance = (float)atof(argv[++i]); }
    else if (a == "--min-spp") { need(1); min_spp = atoi(argv[++i]); }
    else if (a == "--step") { need(1); step = atoi(argv[++i]); }
    else if (a == "--denoise") { need(1); denoise = atoi(argv[++i]); if (denoise < 0 || denoise > 8) { std::cerr << "--denoise takes 0 to 8 iterations" << std::endl; return 2; } }
    else { std::cerr << "unknown option " << a << std::endl; return 2; }
  }

  if (adaptive && gpus > 1) { std::cerr << "--adaptive renders on one GPU: it cannot be combined with --gpus " << gpus << std::endl; return 2; }
  if (denoise >= 0 && gpus > 1) { std::cerr << "--denoise filters a whole frame on one GPU: it cannot be combined with --gpus " << gpus << std::endl; return 2; }
  if (step <= 0) step = min_spp;
  if (adaptive && (min_spp < 2 || (ospp >= 0 && ospp < min_spp))) { std::cerr << "--adaptive needs 2 <= --min-spp <= --spp" << std::endl; return 2; }

  MirtHostScene* hs = nullptr;
  die_on(mirt_parse_scene_file(argv[1], &hs), "parseInput");
  MirtSceneDesc desc;
  die_on(mirt_host_scene_desc(hs, &desc), "mirt_host_scene_desc");
  const int width = ow > 0 ? ow : desc.width, height = oh > 0 ? oh : desc.height;
  const int spp = ospp >= 0 ? ospp : desc.aa;

  if (gpus > 1) {
    // several GPUs: the same phases, each over all devices
    auto start = std::chrono::high_resolution_clock::now();
    MirtMulti* mm = nullptr;
    die_on(mirt_multi_create(&desc, gpus, nullptr, &mm), "copyConfigDataToDevice");
    if (traversal >= 0) die_on(mirt_multi_set_option(mm, "traversal", traversal), "mirt_multi_set_option");
    auto end = std::chrono::high_resolution_clock::now();
    std::chrono::duration<double> elapsed = end - start;
    std::cout << "Initialize raw config time: " << elapsed.count() << " seconds" << std::endl;
    std::vector<uint8_t> img((size_t)width * height * 4);
    MirtMultiStats st;
    float ms_per_frame = 0.0f;
    start = std::chrono::high_resolution_clock::now();
    print_debug_render(width, height, spp);
    // (a capacity overflow on any device fails the call: mirt_multi_wait checks every device's scene)
    die_on(mirt_render_frames_multi(mm, width, height, spp, 4, frames, frames > 1 ? 2 : 1, img.data(), &st, &ms_per_frame), "render");
    end = std::chrono::high_resolution_clock::now();
    elapsed = end - start;
    if (desc.num_prims > 0) {
      printf("LBVH Build time (N=%d): %.3f ms\n", desc.num_prims, st.build_ms);
      printf("LBVH Build (Karas algorithm) complete. Total nodes: %u\n", 2u * (unsigned)desc.num_prims - 1u);
    }
    std::cout << "Render time: " << elapsed.count() << " seconds" << std::endl;
    printf("GPUs: %d, frames: %d (%.3f ms per frame), framebuffer gather: %.3f ms, per-GPU render ms of the last frame:", st.num_gpus, frames, ms_per_frame, st.gather_ms);
    for (int r = 0; r < st.num_gpus && r < MIRT_MULTI_MAX_GPUS; ++r) printf(" %.3f", st.render_ms[r]);
    printf("\n");
    const std::string out = out_override.empty() ? std::string(mirt_host_scene_filename(hs)) : out_override;
    die_on(mirt_write_png(out.c_str(), img.data(), width, height), "Image::save");
    mirt_multi_destroy(mm);
    mirt_host_scene_destroy(hs);
    return 0;
  }

  auto start = std::chrono::high_resolution_clock::now();
  MirtScene* sc = nullptr;
  die_on(mirt_scene_create(&desc, device, &sc), "copyConfigDataToDevice");
  if (traversal >= 0) die_on(mirt_scene_set_option(sc, "traversal", traversal), "mirt_scene_set_option");
  if (shipped) die_on(mirt_scene_set_option(sc, "bounds_as_shipped", 1), "mirt_scene_set_option");
  auto end = std::chrono::high_resolution_clock::now();
  std::chrono::duration<double> elapsed = end - start;
  std::cout << "Initialize raw config time: " << elapsed.count() << " seconds" << std::endl;

  if (desc.num_prims > 0) {
    float ms = 0.0f;
    die_on(mirt_build_lbvh(sc, nullptr, &ms), "build_lbvh_karas");
    printf("LBVH Build time (N=%d): %.3f ms\n", desc.num_prims, ms);
    printf("LBVH Build (Karas algorithm) complete. Total nodes: %u\n", 2u * (unsigned)desc.num_prims - 1u);
    if (desc.num_prims <= 16) print_node_info(sc, desc.num_prims);
  } else {
    die_on(mirt_build_lbvh(sc, nullptr, nullptr), "build_lbvh_karas");
  }

  start = std::chrono::high_resolution_clock::now();
  MirtRenderParams p;
  p.width = width; p.height = height; p.spp = spp; p.stripe_rows = height; p.num_parts = 1; p.part = 0; p.flags = 0;
  const size_t bytes = (size_t)width * height * 4;
  void* d_image = nullptr;
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipMalloc(&d_image, bytes));
  end = std::chrono::high_resolution_clock::now();
  elapsed = end - start;
  std::cout << "Malloc and transfer to device time: " << elapsed.count() << " seconds" << std::endl;

  start = std::chrono::high_resolution_clock::now();
  if (!adaptive) print_debug_render(width, height, spp);
  if (adaptive || denoise >= 0) {
    // the loop of DESIGN.md section 6e: every pixel gets samples [0, min_spp), then the pixels mirt_select_pixels still finds noisy
    // get the samples of one more round, the same range for all of them.  --denoise alone: every pixel gets samples [0, spp).
    if (adaptive && spp < min_spp) { std::cerr << "--adaptive needs 2 <= --min-spp <= --spp" << std::endl; return 2; }
    const int first_count = adaptive ? min_spp : (spp > 1 ? spp : 1);
    const size_t n = (size_t)width * height;
    void *accum = nullptr, *accum_sq = nullptr;
    uint32_t *counts = nullptr, *pixels = nullptr, *num = nullptr;
    HIP_CHECK(hipMalloc(&accum, 16 * n)); HIP_CHECK(hipMalloc(&accum_sq, 16 * n));
    HIP_CHECK(hipMalloc(&counts, 4 * n)); HIP_CHECK(hipMalloc(&pixels, 4 * n)); HIP_CHECK(hipMalloc(&num, 4));
    HIP_CHECK(hipMemset(accum, 0, 16 * n)); HIP_CHECK(hipMemset(accum_sq, 0, 16 * n)); HIP_CHECK(hipMemset(counts, 0, 4 * n));
    p.spp = spp > 2 ? spp : 2;
    die_on(mirt_render_accumulate_pixels(sc, &p, nullptr, 0, accum, accum_sq, counts, 0, first_count, nullptr), "render");
    for (int r = 0; adaptive && min_spp + (r + 1) * step <= spp; ++r) {
      die_on(mirt_select_pixels(&p, accum, accum_sq, counts, min_spp, spp, max_variance, pixels, num, nullptr), "render");
      uint32_t k = 0;
      HIP_CHECK(hipMemcpy(&k, num, 4, hipMemcpyDeviceToHost));
      if (k == 0) break;
      die_on(mirt_render_accumulate_pixels(sc, &p, pixels, k, accum, accum_sq, counts, min_spp + r * step, step, nullptr), "render");
    }
    if (denoise >= 0) {
      // sample 0's primary hits steer the filter (p.spp > 1: the rays mirt_render_accumulate_pixels started with)
      void *rays = nullptr, *hits = nullptr, *features = nullptr, *work = nullptr, *mean = nullptr;
      HIP_CHECK(hipMalloc(&rays, 32 * n)); HIP_CHECK(hipMalloc(&hits, 24 * n)); HIP_CHECK(hipMalloc(&features, 32 * n));
      HIP_CHECK(hipMalloc(&work, mirt_denoise_work_bytes(&p))); HIP_CHECK(hipMalloc(&mean, 16 * n));
      die_on(mirt_camera_rays(sc, &p, rays, nullptr), "render");
      die_on(mirt_trace_rays(sc, rays, (int64_t)n, hits, 0, nullptr), "render");
      die_on(mirt_hit_features(sc, rays, hits, (int64_t)n, features, nullptr), "render");
      die_on(mirt_denoise(&p, accum, accum_sq, counts, features, denoise, MIRT_DENOISE_SIGMA_C, MIRT_DENOISE_SIGMA_N, MIRT_DENOISE_SIGMA_P, work, mean, nullptr),
             "render");
      die_on(mirt_finalize(&p, mean, 1, d_image, nullptr), "render");
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipFree(rays)); HIP_CHECK(hipFree(hits)); HIP_CHECK(hipFree(features)); HIP_CHECK(hipFree(work)); HIP_CHECK(hipFree(mean));
      printf("Denoise: %d iterations\n", denoise);
    } else {
      die_on(mirt_finalize_counts(&p, accum, counts, d_image, nullptr), "render");
    }
    if (adaptive) {
      std::vector<uint32_t> host_counts(n);
      HIP_CHECK(hipMemcpy(host_counts.data(), counts, 4 * n, hipMemcpyDeviceToHost));
      unsigned long long used = 0;
      for (uint32_t c : host_counts) used += c;
      printf("Adaptive sampling: %llu samples used (min-spp x pixels: %llu, spp x pixels: %llu)\n", used, (unsigned long long)min_spp * n, (unsigned long long)spp * n);
    }
    HIP_CHECK(hipFree(accum)); HIP_CHECK(hipFree(accum_sq)); HIP_CHECK(hipFree(counts)); HIP_CHECK(hipFree(pixels)); HIP_CHECK(hipFree(num));
  } else {
    for (int f = 0; f < frames; ++f) die_on(mirt_render(sc, &p, d_image, nullptr, nullptr), "render");
  }
  HIP_CHECK(hipDeviceSynchronize());
  {
    MirtStats st;      // (a capacity overflow during the render is an error, not a warning on stdout as bvh_traversal.cu:154-164)
    die_on(mirt_get_stats(sc, &st), "render");
  }
  end = std::chrono::high_resolution_clock::now();
  elapsed = end - start;
  std::cout << "Render time: " << elapsed.count() << " seconds" << std::endl;
  if (frames > 1) printf("frames: %d (%.3f ms per frame)\n", frames, elapsed.count() * 1e3 / frames);

  start = std::chrono::high_resolution_clock::now();
  std::vector<uint8_t> img(bytes);
  HIP_CHECK(hipMemcpy(img.data(), d_image, bytes, hipMemcpyDeviceToHost));
  end = std::chrono::high_resolution_clock::now();
  elapsed = end - start;
  std::cout << "Transfer to host time: " << elapsed.count() << " seconds" << std::endl;

  const std::string out = out_override.empty() ? std::string(mirt_host_scene_filename(hs)) : out_override;
  die_on(mirt_write_png(out.c_str(), img.data(), width, height), "Image::save");

  start = std::chrono::high_resolution_clock::now();
  HIP_CHECK(hipFree(d_image));
  mirt_scene_destroy(sc);
  mirt_host_scene_destroy(hs);
  end = std::chrono::high_resolution_clock::now();
  elapsed = end - start;
  std::cout << "cudaFree time: " << elapsed.count() << " seconds" << std::endl;      // (the reference's label, main.cu:93: the contract is the text)
  return 0;
}
