"""cuda_ray_tracer_amd -- MI355X-native LBVH ray tracer (hot path of GJ0407790/cuda_ray_tracer).

Host side: binding.py (include/mirt.h restated for ctypes) and api.py (the calls over it); lighting.py (include/mirt_light.h);
visibility.py (include/mirt_visibility.h); indirect.py (include/mirt_indirect.h); closest.py (include/mirt_closest.h);
multihit.py (include/mirt_multihit.h); contacts.py (include_ext/mirt_contacts.h); spherecast.py (include_ext/mirt_spherecast.h);
overlap.py (include_ext/mirt_overlap.h); overlap_list.py (include_ext/mirt_overlap_list.h); query_lists.py (include_ext/mirt_query_lists.h);
overlap_tris.py (include_ext2/mirt_overlap_tris.h); cast_lists.py (include_ext3/mirt_cast_lists.h).
Device side: csrc/*.hip, built by build.py into _build/libmirt.so.
"""
from .api import (MirtError, StlConfig, RawConfig, parseInput, parseText, syntheticScene, initRawConfigFromStl,
                  copyConfigDataToDevice, freeRawConfigDeviceMemory, build_lbvh_karas, render, render_params,
                  num_pixels, scatter_part, write_png, lib, render_accumulate, finalize, Ray, Hit, trace_rays,
                  camera_rays, pack_rays, unpack_hits, Camera, update_spheres, update_triangles, render_accumulate_pixels,
                  select_pixels, finalize_counts, render_adaptive, hit_features, denoise,
                  denoise_work_bytes, denoise_frame, get_spheres, get_triangles, prev_features, temporal_accumulate,
                  TemporalAccumulator, Shading, make_plane, update_sphere_materials, update_triangle_materials,
                  get_sphere_materials, get_triangle_materials, direct_light, pack_features, direct_light_frame,
                  hemisphere_visibility, cosine_directions, rotations, ambient_occlusion_frame,
                  indirect_light, indirect_light_frame, closest_points, pack_points, trace_rays_multi, count_hits,
                  closest_points_multi, count_within, cast_spheres, pack_casts,
                  overlap_boxes, count_overlaps, pack_boxes, voxel_rows, occupancy_grid,
                  list_offsets, list_offsets_work_bytes, overlap_list, overlap_lists, unpack_words, voxel_lists,
                  ray_list, ball_list, ray_lists, ball_lists,
                  overlap_triangles, triangle_list, triangle_lists, pack_triangles, scene_triangle_rows,
                  count_casts, cast_list, cast_lists)

__all__ = ["MirtError", "StlConfig", "RawConfig", "parseInput", "parseText", "syntheticScene", "initRawConfigFromStl",
           "copyConfigDataToDevice", "freeRawConfigDeviceMemory", "build_lbvh_karas", "render", "render_params",
           "num_pixels", "scatter_part", "write_png", "lib", "render_accumulate", "finalize", "Ray", "Hit", "trace_rays",
           "camera_rays", "pack_rays", "unpack_hits", "Camera", "update_spheres", "update_triangles", "render_accumulate_pixels",
           "select_pixels", "finalize_counts", "render_adaptive", "hit_features", "denoise", "denoise_work_bytes", "denoise_frame",
           "get_spheres", "get_triangles", "prev_features", "temporal_accumulate", "TemporalAccumulator",
           "Shading", "make_plane", "update_sphere_materials", "update_triangle_materials", "get_sphere_materials",
           "get_triangle_materials", "direct_light", "pack_features", "direct_light_frame",
           "hemisphere_visibility", "cosine_directions", "rotations", "ambient_occlusion_frame",
           "indirect_light", "indirect_light_frame", "closest_points", "pack_points", "trace_rays_multi", "count_hits",
           "closest_points_multi", "count_within", "cast_spheres", "pack_casts",
           "overlap_boxes", "count_overlaps", "pack_boxes", "voxel_rows", "occupancy_grid",
           "list_offsets", "list_offsets_work_bytes", "overlap_list", "overlap_lists", "unpack_words", "voxel_lists",
           "ray_list", "ball_list", "ray_lists", "ball_lists",
           "overlap_triangles", "triangle_list", "triangle_lists", "pack_triangles", "scene_triangle_rows",
           "count_casts", "cast_list", "cast_lists"]
