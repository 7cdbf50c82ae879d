// hso_octree_dev.h — the oct-tree distribution on the device (hso_octree_dev.hip), shared with the detection chain
// (hso_edgelet.hip) that feeds it key lists it assembled on the device.
#pragma once
#include "hso_ctx.h"

#define HSO_OCTREE_MAX_FEATURES 4096   // n_features the kernel takes (its sort arrays live in LDS)
#define HSO_OCTREE_MAX_COLUMNS 64      // initial column nodes: round(width / height) of the rectangle

struct OctreePlan {
  int n_ini; float hX;          // computed on the host exactly as hso_gpu_select_octree computes them
  int min_y, max_y, n_features;
  int ncap;                     // node records per set and list buffer
  size_t per_set;               // scratch bytes per set
};
// HSO_E_INVALID for a rectangle hso_gpu_select_octree refuses, HSO_E_UNSUPPORTED beyond the limits above
int hso_octree_plan(hso_gpu_ctx* ctx, int min_x, int max_x, int min_y, int max_y, int n_features, OctreePlan* plan);
// bytes of scratch (node_of + per-set work) for n_sets sets holding total_keys keys
size_t hso_octree_scratch_bytes(const OctreePlan& plan, int n_sets, size_t total_keys);
// ctx->d_octree with room for `bytes` (grow-only; waits for the stream before it re-allocates)
int hso_octree_reserve(hso_gpu_ctx* ctx, size_t bytes, char** d);
// one launch, one workgroup per set, on ctx->stream; everything is device memory: keys of set i are
// d_keys[d_key_begin[i] .. d_key_begin[i + 1]), its selection goes to d_out + i * out_cap, its count (or HSO_E_*) to d_n_out[i]
int hso_octree_launch(hso_gpu_ctx* ctx, const OctreePlan& plan, const hso_keypoint* d_keys, const int* d_key_begin, int n_sets, size_t total_keys,
                      hso_keypoint* d_out, int out_cap, int* d_n_out, char* d_scratch);
