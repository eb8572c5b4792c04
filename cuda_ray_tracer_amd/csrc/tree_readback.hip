// What a built scene hands back to the host: the tree in the reference's numbering (mirt_get_tree) and the records the traversal
// kernels read (mirt_get_records).  Copies only: lbvh_build.hip made all of it.
#include "scene_dev.h"
#include "host_scene.h"

namespace mirt {

int get_tree(MirtScene* sc, MirtTreeNode* nodes, uint32_t* codes, MirtPrimRef* refs, float* bounds)
{
  const int n = sc->N;
  if (!sc->built) { set_error("mirt_get_tree: LBVH not built"); return MIRT_ERR_STATE; }
  if (n == 0) return MIRT_OK;
  MIRT_HIP(hipDeviceSynchronize());
  std::vector<uint32_t> order(n), cl(n > 1 ? n - 1 : 0), cr(n > 1 ? n - 1 : 0);
  std::vector<MirtPrimRef> rin(n);
  std::vector<float> boxes(6 * (2 * (size_t)n - 1));
  MIRT_HIP(hipMemcpy(order.data(), sc->order, 4 * (size_t)n, hipMemcpyDeviceToHost));
  MIRT_HIP(hipMemcpy(rin.data(), sc->refs_in, sizeof(MirtPrimRef) * (size_t)n, hipMemcpyDeviceToHost));
  MIRT_HIP(hipMemcpy(boxes.data(), sc->boxes, 4 * boxes.size(), hipMemcpyDeviceToHost));
  if (n > 1) {
    MIRT_HIP(hipMemcpy(cl.data(), sc->child_l, 4 * (size_t)(n - 1), hipMemcpyDeviceToHost));
    MIRT_HIP(hipMemcpy(cr.data(), sc->child_r, 4 * (size_t)(n - 1), hipMemcpyDeviceToHost));
  }
  if (codes) MIRT_HIP(hipMemcpy(codes, sc->codes, 4 * (size_t)n, hipMemcpyDeviceToHost));
  if (refs) for (int i = 0; i < n; ++i) refs[i] = rin[order[i]];
  if (nodes) {
    for (int i = 0; i < 2 * n - 1; ++i) {
      MirtTreeNode& t = nodes[i];
      const float* b = &boxes[6 * (size_t)i];
      t.xmin = b[0]; t.xmax = b[1]; t.ymin = b[2]; t.ymax = b[3]; t.zmin = b[4]; t.zmax = b[5];
      if (i < n - 1) { t.left = cl[i]; t.right = cr[i]; t.prim_offset = 0; t.count = 0; }
      else { t.left = 0; t.right = 0; t.prim_offset = (uint32_t)(i - (n - 1)); t.count = 1; }
    }
  }
  if (bounds) {
    uint32_t k[6];
    MIRT_HIP(hipMemcpy(k, sc->bounds_keys, sizeof(k), hipMemcpyDeviceToHost));
    for (int i = 0; i < 6; ++i) bounds[i] = key2f(k[i]);
  }
  return MIRT_OK;
}

// mirt_get_records: the heap and its side tables as the traversal kernels read them.  A region the build did not make (or, after
// a rebuild with bounds_as_shipped, no longer offers) has count 0 and is not copied.
int get_records(MirtScene* sc, MirtRecordInfo* info, void* nodes, void* qnodes, void* wnodes, void* prims, uint32_t* unit_prim,
                uint32_t* tris_before, float* tri_boxes, float* qparams)
{
  const int n = sc->N;
  if (!sc->built) { set_error("mirt_get_records: LBVH not built"); return MIRT_ERR_STATE; }
  MIRT_HIP(hipDeviceSynchronize());
  const bool have_q = sc->root_ref_q != REF_NONE, have_w = sc->root_ref_w != REF_NONE;
  MirtRecordInfo r{};
  r.num_nodes = n > 1 ? (uint32_t)(n - 1) : 0u;
  r.num_qnodes = have_q ? r.num_nodes : 0u;
  r.num_wnodes = have_w ? r.num_nodes : 0u;
  r.prim_units = n > 0 ? (uint32_t)sc->Ns + 3u * (uint32_t)sc->Nt : 0u;
  r.num_tris_before = n > 0 ? (uint32_t)n + 1u : 0u;
  r.num_tri_boxes = n > 0 ? (uint32_t)sc->Nt : 0u;
  r.num_qparams = (have_q || have_w) ? 9u : 0u;
  r.prim_base16 = sc->prim_base / 16u; r.qnode_base16 = sc->qnode_base / 16u; r.wnode_base16 = sc->wnode_base / 16u;
  r.root_ref = sc->root_ref; r.root_ref_q = sc->root_ref_q; r.root_ref_w = sc->root_ref_w;
  r.grid_ok = sc->grid_ok ? 1 : 0; r.tree_depth = sc->tree_depth; r.coord_max = sc->coord_max;
  if (info) *info = r;
  const unsigned char* heap = sc->heap;
  if (nodes && r.num_nodes) MIRT_HIP(hipMemcpy(nodes, heap, 64 * (size_t)r.num_nodes, hipMemcpyDeviceToHost));
  if (qnodes && r.num_qnodes) MIRT_HIP(hipMemcpy(qnodes, heap + sc->qnode_base, 32 * (size_t)r.num_qnodes, hipMemcpyDeviceToHost));
  if (wnodes && r.num_wnodes) MIRT_HIP(hipMemcpy(wnodes, heap + sc->wnode_base, 64 * (size_t)r.num_wnodes, hipMemcpyDeviceToHost));
  if (prims && r.prim_units) MIRT_HIP(hipMemcpy(prims, heap + sc->prim_base, 16 * (size_t)r.prim_units, hipMemcpyDeviceToHost));
  if (unit_prim && r.prim_units) MIRT_HIP(hipMemcpy(unit_prim, sc->unit_prim, 4 * (size_t)r.prim_units, hipMemcpyDeviceToHost));
  if (tris_before && r.num_tris_before) MIRT_HIP(hipMemcpy(tris_before, sc->tris_before, 4 * (size_t)r.num_tris_before, hipMemcpyDeviceToHost));
  if (tri_boxes && r.num_tri_boxes) MIRT_HIP(hipMemcpy(tri_boxes, sc->tri_boxes, 32 * (size_t)r.num_tri_boxes, hipMemcpyDeviceToHost));
  if (qparams && r.num_qparams) MIRT_HIP(hipMemcpy(qparams, sc->qparams, 4 * (size_t)r.num_qparams, hipMemcpyDeviceToHost));
  return MIRT_OK;
}

} // namespace mirt
