// hso_export.hip — map export (include/hso_gpu.h: hso_gpu_seqmap_export_points, hso_gpu_seed_table_export): the live point rows of
// sequence maps and the live seeds of a resident seed table, filtered, coloured and packed on the device, in table order.
//
// What the reference's one consumer of the map draws (Viewer::DrawMapRegionPoints, src/viewer.cpp:109-136: point->pos_ in
// point->color_ for every keyframe feature with a point) and where it takes the colour from (src/depth_filter.cpp:440-460: the host
// image's level-0 pixel at the host feature, read when a seed becomes a point).  The tables are mostly dead rows after a long run
// and are indexed by the caller's ids, so the selection happens here and only the selected records cross PCIe.
//
// Three short launches, none of which waits for another workgroup (no spin, no flag, no atomic cursor: a cursor would also lose the
// order):
//   count    one workgroup per (map, chunk of EXPORT_CHUNK rows): the number of selected rows of the chunk;
//   offsets  ONE workgroup: exclusive scan over the chunk list (maps in call order, chunks ascending), the per-map begins;
//   emit     the count pass's grid again: a selected lane's place = its chunk's offset + the selected lanes below it in the
//            workgroup (wave ballot + the counts of the waves below); the colour gather is fused in.
// A lane stores its record as whole 8-byte (points, 40 B) or 16-byte (seeds, 48 B) words: see DESIGN.md section 3.17.
#include "hso_ctx.h"
#include "hso_dev_math.h"
#include <climits>
#include <cmath>
#include <cstring>

using namespace hso_dev;

#define EXPORT_CHUNK 256          // rows per workgroup = threads per workgroup (tests/test_map_export_gpu.py walks its edges)
#define EXPORT_NO_COLOR 128       // Point::color_'s initial value, include/hso/point.h:121

static_assert(sizeof(hso_point_export) == 40 && sizeof(hso_seed_export) == 48, "record sizes are part of the ABI");
static_assert(offsetof(hso_point_export, point) == 24 && offsetof(hso_point_export, n_obs) == 32 && offsetof(hso_point_export, color) == 36,
              "k_export_emit_points packs the record's words by hand");
static_assert(offsetof(hso_seed_export, mu) == 24 && offsetof(hso_seed_export, slot) == 32 && offsetof(hso_seed_export, color) == 40,
              "k_export_emit_seeds packs the record's words by hand");

// hso_align.hip / hso_seed.hip: the tables as the export kernels read them
int hso_seqmap_export_view(hso_gpu_ctx* ctx, int map, const hso_map_point** pts, int* n_pts, const hso_obs** obs, int* n_obs, const hso_kf** kfs, int* n_kfs);
int hso_seed_table_export_view(hso_gpu_ctx* ctx, int table, const char** rows, size_t* stride, size_t* seed_offset, size_t* group_offset, int* n_slots,
                               int* max_group, PyrGeom* g);

struct ExportKf {               // a keyframe row as the colour lookup needs it
  const uint8_t* img;           // level 0 of the resident frame; null: the frame is not resident
  int32_t keyframe_id, w, h, pad_;
};
struct ExportMap {
  const hso_map_point* pts; const hso_obs* obs; const ExportKf* kfs;
  int32_t n_pts, n_obs, n_kfs;
  int32_t chunk_begin;          // the map's first entry in the call's chunk list
};

// level-0 byte ((int)px[1], (int)px[0]); a pixel outside the image (no keyframe feature has one) keeps the default instead of reading past it
HSO_DEV unsigned pixel_at(const uint8_t* img, int w, int h, double px0, double px1)
{
  if (!img || !(px0 >= 0.0 && px0 < (double)w && px1 >= 0.0 && px1 < (double)h)) return EXPORT_NO_COLOR;
  return img[(size_t)(int)px1 * (size_t)w + (size_t)(int)px0];
}

HSO_DEV bool point_selected(uint32_t word, int obs_count, uint32_t type_mask, int min_obs)
{
  const uint32_t type = (word >> 4) & 0xfu;
  return type != 0 && ((type_mask >> type) & 1u) && !(word & HSO_PT_BAD) && obs_count >= min_obs;
}

// place of a selected lane among the selected lanes of its workgroup (thread order) and their number; all threads must call
HSO_DEV int block_rank(bool sel, int* s_wave, int& total)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(sel);
  const int rank = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) s_wave[wave] = __popcll(b);
  __syncthreads();
  int base = 0; total = 0;
#pragma unroll
  for (int w = 0; w < EXPORT_CHUNK / 64; w++) { if (w < wave) base += s_wave[w]; total += s_wave[w]; }
  return base + rank;
}

static __global__ __launch_bounds__(EXPORT_CHUNK) void k_export_count_points(const ExportMap* __restrict__ maps, uint32_t type_mask, int min_obs,
                                                                             int32_t* __restrict__ counts)
{
  __shared__ int s_wave[EXPORT_CHUNK / 64];
  const ExportMap M = maps[blockIdx.y];
  if ((int)blockIdx.x >= (M.n_pts + EXPORT_CHUNK - 1) / EXPORT_CHUNK) return;   // the grid is as wide as the longest map
  const int row = (int)blockIdx.x * EXPORT_CHUNK + (int)threadIdx.x;
  bool sel = false;
  if (row < M.n_pts) sel = point_selected((uint32_t)M.pts[row].pad_, M.pts[row].obs_count, type_mask, min_obs);
  int total;
  (void)block_rank(sel, s_wave, total);
  if (threadIdx.x == 0) counts[M.chunk_begin + (int)blockIdx.x] = total;
}

// offsets[i] = counts[0] + ... + counts[i - 1], offsets[n_chunks] = the total; begin[m] = offsets[map_chunk[m]] (map_chunk[n_maps] =
// n_chunks).  One workgroup: a thread sums a contiguous span of the list, the spans' sums are scanned, the span is walked again.
static __global__ __launch_bounds__(256) void k_export_offsets(const int32_t* __restrict__ counts, int32_t* __restrict__ offsets, int n_chunks,
                                                               const int32_t* __restrict__ map_chunk, int32_t* __restrict__ begin, int n_maps)
{
  __shared__ int s_wave[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (n_chunks + 255) / 256;
  const int lo = min((int)threadIdx.x * per, n_chunks), hi = min(lo + per, n_chunks);
  int sum = 0;
  for (int i = lo; i < hi; i++) sum += counts[i];
  const int incl = wave_inclusive_scan(sum, lane);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int run = incl - sum;
  for (int w = 0; w < wave; w++) run += s_wave[w];
  for (int i = lo; i < hi; i++) { offsets[i] = run; run += counts[i]; }
  if (threadIdx.x == 255) offsets[n_chunks] = run;   // the last span ends the list (or is empty behind it)
  __threadfence();
  __syncthreads();
  for (int m = threadIdx.x; m <= n_maps; m += 256) begin[m] = offsets[map_chunk[m]];
}

static __global__ __launch_bounds__(EXPORT_CHUNK) void k_export_emit_points(const ExportMap* __restrict__ maps, uint32_t type_mask, int min_obs,
                                                                            const int32_t* __restrict__ offsets, unsigned long long* __restrict__ out, int cap)
{
  __shared__ int s_wave[EXPORT_CHUNK / 64];
  const ExportMap M = maps[blockIdx.y];
  if ((int)blockIdx.x >= (M.n_pts + EXPORT_CHUNK - 1) / EXPORT_CHUNK) return;
  const int row = (int)blockIdx.x * EXPORT_CHUNK + (int)threadIdx.x;
  hso_map_point p{};
  bool sel = false;
  if (row < M.n_pts) { p = M.pts[row]; sel = point_selected((uint32_t)p.pad_, p.obs_count, type_mask, min_obs); }
  int total;
  const int rank = block_rank(sel, s_wave, total);
  if (!sel) return;
  const int at = offsets[M.chunk_begin + (int)blockIdx.x] + rank;
  if (at >= cap) return;                                           // the first `cap` records and nothing beyond them
  // the host observation: the first entry of the point's chain made in its host keyframe
  unsigned color = EXPORT_NO_COLOR;
  int keyframe_id = -1;
  const int hk = p.host_kf;
  const bool kf_ok = hk >= 0 && hk < M.n_kfs;
  if (kf_ok) keyframe_id = M.kfs[hk].keyframe_id;
  int o = p.obs_begin;
  for (int step = 0; step < p.obs_count; step++) {
    if (o < 0 || o >= M.n_obs) break;
    const hso_obs* ob = M.obs + o;
    if (ob->kf == hk) {
      if (kf_ok) { const ExportKf K = M.kfs[hk]; color = pixel_at(K.img, K.w, K.h, ob->px[0], ob->px[1]); }
      break;
    }
    o = ob->pad_;
  }
  const uint32_t word = (uint32_t)p.pad_;
  unsigned long long* r = out + (size_t)at * 5;
  r[0] = (unsigned long long)__double_as_longlong(p.pos[0]);
  r[1] = (unsigned long long)__double_as_longlong(p.pos[1]);
  r[2] = (unsigned long long)__double_as_longlong(p.pos[2]);
  r[3] = (unsigned long long)(uint32_t)row | ((unsigned long long)(uint32_t)keyframe_id << 32);
  r[4] = (unsigned long long)(uint32_t)p.obs_count | ((unsigned long long)(color & 0xffu) << 32) | ((unsigned long long)((word >> 4) & 0xfu) << 40) |
         ((unsigned long long)(word & 0xfu) << 48);
}

// ---- seeds --------------------------------------------------------------------------------------------------------------------
struct ExportSeeds {
  const char* rows; size_t stride, seed_offset, group_offset;
  const uint32_t* group_mask;   // bit g: group g is named; null: every group
  int32_t n_slots, n_mask_bits, level0_off, w, h;
};

HSO_DEV bool seed_selected(const ExportSeeds& S, int slot)
{
  const char* row = S.rows + (size_t)slot * S.stride;
  if (*reinterpret_cast<const uint8_t* const*>(row) == nullptr) return false;              // erased
  if (S.group_mask) {
    const int g = *reinterpret_cast<const int32_t*>(row + S.group_offset);
    if (g < 0 || g >= S.n_mask_bits || !((S.group_mask[g >> 5] >> (g & 31)) & 1u)) return false;
  }
  const float mu = reinterpret_cast<const hso_seed*>(row + S.seed_offset)->mu;
  return mu > 0.0f && mu < INFINITY;                                                       // NaN fails both
}

static __global__ __launch_bounds__(EXPORT_CHUNK) void k_export_count_seeds(ExportSeeds S, int32_t* __restrict__ counts)
{
  __shared__ int s_wave[EXPORT_CHUNK / 64];
  const int slot = (int)blockIdx.x * EXPORT_CHUNK + (int)threadIdx.x;
  const bool sel = slot < S.n_slots && seed_selected(S, slot);
  int total;
  (void)block_rank(sel, s_wave, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

static __global__ __launch_bounds__(EXPORT_CHUNK) void k_export_emit_seeds(ExportSeeds S, const int32_t* __restrict__ offsets, uint4* __restrict__ out, int cap)
{
  __shared__ int s_wave[EXPORT_CHUNK / 64];
  const int slot = (int)blockIdx.x * EXPORT_CHUNK + (int)threadIdx.x;
  const bool sel = slot < S.n_slots && seed_selected(S, slot);
  int total;
  const int rank = block_rank(sel, s_wave, total);
  if (!sel) return;
  const int at = offsets[blockIdx.x] + rank;
  if (at >= cap) return;
  const char* row = S.rows + (size_t)slot * S.stride;
  const uint8_t* base = *reinterpret_cast<const uint8_t* const*>(row);
  const int group = *reinterpret_cast<const int32_t*>(row + S.group_offset);
  const hso_seed sd = *reinterpret_cast<const hso_seed*>(row + S.seed_offset);
  // T_ref_w^-1 * (f * (1 / mu)): the expression of the upgrade loop, src/depth_filter.cpp:440-451
  const double inv = 1.0 / (double)sd.mu;
  const Se3 T_w_ref = se3_inverse(se3_from(sd.T_ref_w));
  double x, y, z;
  se3_apply(T_w_ref, sd.f[0] * inv, sd.f[1] * inv, sd.f[2] * inv, x, y, z);
  const unsigned color = pixel_at(base + S.level0_off, S.w, S.h, sd.px[0], sd.px[1]);
  const unsigned long long bx = (unsigned long long)__double_as_longlong(x), by = (unsigned long long)__double_as_longlong(y),
                           bz = (unsigned long long)__double_as_longlong(z);
  uint4* r = out + (size_t)at * 3;
  r[0] = make_uint4((unsigned)bx, (unsigned)(bx >> 32), (unsigned)by, (unsigned)(by >> 32));
  r[1] = make_uint4((unsigned)bz, (unsigned)(bz >> 32), __float_as_uint(sd.mu), __float_as_uint(sd.sigma2));
  r[2] = make_uint4((unsigned)slot, (unsigned)group, (color & 0xffu) | (((unsigned)sd.type & 0xffu) << 8) | (((unsigned)sd.level & 0xffu) << 16), 0u);
}

extern "C" {

int hso_gpu_seqmap_export_points(hso_gpu_ctx* ctx, const int32_t* maps, int n_maps, uint32_t type_mask, int min_obs, hso_point_export* out, int cap,
                                 int32_t* begin_out)
{
  if (!ctx) return HSO_E_INVALID;
  if (n_maps < 0 || n_maps > 65535 || cap < 0 || !begin_out || (n_maps > 0 && !maps) || (cap > 0 && !out))
    return hso_fail(ctx, HSO_E_INVALID, "seqmap_export_points: bad argument");
  // everything is checked, and the call's tables are laid out, before anything is queued
  std::vector<ExportMap> em((size_t)n_maps);
  std::vector<int32_t> map_chunk((size_t)n_maps + 1, 0), kf_begin((size_t)n_maps + 1, 0);
  std::vector<ExportKf> ek;
  size_t total_rows = 0;
  int widest = 0;
  for (int i = 0; i < n_maps; i++) {
    ExportMap& M = em[(size_t)i];
    const hso_kf* kfs = nullptr;
    if (int rc = hso_seqmap_export_view(ctx, maps[i], &M.pts, &M.n_pts, &M.obs, &M.n_obs, &kfs, &M.n_kfs)) return rc;
    const int chunks = (M.n_pts + EXPORT_CHUNK - 1) / EXPORT_CHUNK;
    M.chunk_begin = map_chunk[(size_t)i];
    map_chunk[(size_t)i + 1] = map_chunk[(size_t)i] + chunks;
    widest = std::max(widest, chunks);
    total_rows += (size_t)M.n_pts;
    if (total_rows > (size_t)INT_MAX) return hso_fail(ctx, HSO_E_INVALID, "seqmap_export_points: more than 2^31 - 1 rows in one call");
    kf_begin[(size_t)i + 1] = kf_begin[(size_t)i] + M.n_kfs;
    for (int k = 0; k < M.n_kfs; k++) {
      ExportKf K{};
      K.keyframe_id = kfs[k].keyframe_id;
      auto it = ctx->frames.find(kfs[k].frame_id);
      if (it != ctx->frames.end()) { K.img = it->second.base + it->second.g.off[0]; K.w = it->second.g.w[0]; K.h = it->second.g.h[0]; }
      ek.push_back(K);
    }
  }
  const int n_chunks = map_chunk[(size_t)n_maps];
  if (n_chunks == 0) { for (int i = 0; i <= n_maps; i++) begin_out[i] = 0; return HSO_OK; }
  HSO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // [maps | first chunk per map | keyframe rows] go up in one copy; [counts | offsets | begins | records] stay on the device
  const size_t n_rec = std::min((size_t)cap, total_rows);
  const size_t b_maps = hso_al256(sizeof(ExportMap) * (size_t)n_maps), b_mc = hso_al256(sizeof(int32_t) * ((size_t)n_maps + 1)),
               b_kfs = hso_al256(sizeof(ExportKf) * ek.size()), b_in = b_maps + b_mc + b_kfs;
  const size_t b_cnt = hso_al256(sizeof(int32_t) * (size_t)n_chunks), b_off = hso_al256(sizeof(int32_t) * ((size_t)n_chunks + 1)),
               b_beg = hso_al256(sizeof(int32_t) * ((size_t)n_maps + 1)), b_rec = hso_al256(sizeof(hso_point_export) * n_rec);
  if (int rc = hso_batch_reserve(ctx, b_in + b_cnt + b_off + b_beg + b_rec)) return rc;
  char* d = ctx->d_batch;
  const ExportKf* d_kfs = reinterpret_cast<const ExportKf*>(d + b_maps + b_mc);
  for (int i = 0; i < n_maps; i++) em[(size_t)i].kfs = d_kfs + kf_begin[(size_t)i];
  std::vector<char> image(b_in, 0);
  memcpy(image.data(), em.data(), sizeof(ExportMap) * (size_t)n_maps);
  memcpy(image.data() + b_maps, map_chunk.data(), sizeof(int32_t) * ((size_t)n_maps + 1));
  if (!ek.empty()) memcpy(image.data() + b_maps + b_mc, ek.data(), sizeof(ExportKf) * ek.size());
  HSO_HIP_CHECK(ctx, hipMemcpyAsync(d, image.data(), b_in, hipMemcpyHostToDevice, ctx->stream));   // staged by the copy wrapper: `image` may go
  const ExportMap* d_maps = reinterpret_cast<const ExportMap*>(d);
  const int32_t* d_mc = reinterpret_cast<const int32_t*>(d + b_maps);
  int32_t* d_cnt = reinterpret_cast<int32_t*>(d + b_in);
  int32_t* d_off = reinterpret_cast<int32_t*>(d + b_in + b_cnt);
  int32_t* d_beg = reinterpret_cast<int32_t*>(d + b_in + b_cnt + b_off);
  char* d_rec = d + b_in + b_cnt + b_off + b_beg;
  const dim3 grid((unsigned)widest, (unsigned)n_maps);
  hipLaunchKernelGGL(k_export_count_points, grid, dim3(EXPORT_CHUNK), 0, ctx->stream, d_maps, type_mask, min_obs, d_cnt);
  hipLaunchKernelGGL(k_export_offsets, dim3(1), dim3(256), 0, ctx->stream, d_cnt, d_off, n_chunks, d_mc, d_beg, n_maps);
  hipLaunchKernelGGL(k_export_emit_points, grid, dim3(EXPORT_CHUNK), 0, ctx->stream, d_maps, type_mask, min_obs, d_off,
                     reinterpret_cast<unsigned long long*>(d_rec), (int)n_rec);
  HSO_HIP_CHECK(ctx, hipGetLastError());
  HSO_HIP_CHECK(ctx, hipMemcpyAsync(begin_out, d_beg, sizeof(int32_t) * ((size_t)n_maps + 1), hipMemcpyDeviceToHost, ctx->stream));
  HSO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t total = (size_t)begin_out[n_maps], n_write = std::min(total, (size_t)cap);
  if (n_write > 0) {
    HSO_HIP_CHECK(ctx, hipMemcpyAsync(out, d_rec, sizeof(hso_point_export) * n_write, hipMemcpyDeviceToHost, ctx->stream));
    HSO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (total > (size_t)cap) { ctx->err = "seqmap_export_points: cap is smaller than the number of selected rows (begin_out holds the full counts)"; return HSO_E_TRUNCATED; }
  return HSO_OK;
}

int hso_gpu_seed_table_export(hso_gpu_ctx* ctx, int table, const int32_t* groups, int n_groups, hso_seed_export* out, int cap, int32_t* n_out)
{
  if (!ctx) return HSO_E_INVALID;
  if (cap < 0 || !n_out || (cap > 0 && !out) || (groups && n_groups < 0)) return hso_fail(ctx, HSO_E_INVALID, "seed_table_export: bad argument");
  for (int i = 0; groups && i < n_groups; i++) if (groups[i] < 0) return hso_fail(ctx, HSO_E_INVALID, "seed_table_export: negative group");
  ExportSeeds S{};
  int max_group = -1;
  PyrGeom g{};
  if (int rc = hso_seed_table_export_view(ctx, table, &S.rows, &S.stride, &S.seed_offset, &S.group_offset, &S.n_slots, &max_group, &g)) return rc;   // waits for a pass in flight
  *n_out = 0;
  if (S.n_slots == 0) return HSO_OK;
  HSO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  S.level0_off = (int32_t)g.off[0]; S.w = g.w[0]; S.h = g.h[0];
  const int n_chunks = (S.n_slots + EXPORT_CHUNK - 1) / EXPORT_CHUNK;
  // the named groups as a bit mask over the groups the table has seen (a name beyond them selects nothing)
  S.n_mask_bits = max_group + 1;
  std::vector<uint32_t> mask(((size_t)S.n_mask_bits + 31) / 32 + 1, 0u);
  for (int i = 0; groups && i < n_groups; i++) if (groups[i] <= max_group) mask[(size_t)groups[i] >> 5] |= 1u << (groups[i] & 31);
  const int32_t map_chunk[2] = {0, n_chunks};
  const size_t n_rec = std::min((size_t)cap, (size_t)S.n_slots);
  const size_t b_mask = hso_al256(sizeof(uint32_t) * mask.size()), b_mc = hso_al256(sizeof(map_chunk)), b_in = b_mask + b_mc;
  const size_t b_cnt = hso_al256(sizeof(int32_t) * (size_t)n_chunks), b_off = hso_al256(sizeof(int32_t) * ((size_t)n_chunks + 1)), b_beg = hso_al256(2 * sizeof(int32_t)),
               b_rec = hso_al256(sizeof(hso_seed_export) * n_rec);
  if (int rc = hso_batch_reserve(ctx, b_in + b_cnt + b_off + b_beg + b_rec)) return rc;
  char* d = ctx->d_batch;
  std::vector<char> image(b_in, 0);
  memcpy(image.data(), mask.data(), sizeof(uint32_t) * mask.size());
  memcpy(image.data() + b_mask, map_chunk, sizeof(map_chunk));
  HSO_HIP_CHECK(ctx, hipMemcpyAsync(d, image.data(), b_in, hipMemcpyHostToDevice, ctx->stream));
  S.group_mask = groups ? reinterpret_cast<const uint32_t*>(d) : nullptr;
  int32_t* d_cnt = reinterpret_cast<int32_t*>(d + b_in);
  int32_t* d_off = reinterpret_cast<int32_t*>(d + b_in + b_cnt);
  int32_t* d_beg = reinterpret_cast<int32_t*>(d + b_in + b_cnt + b_off);
  char* d_rec = d + b_in + b_cnt + b_off + b_beg;
  hipLaunchKernelGGL(k_export_count_seeds, dim3((unsigned)n_chunks), dim3(EXPORT_CHUNK), 0, ctx->stream, S, d_cnt);
  hipLaunchKernelGGL(k_export_offsets, dim3(1), dim3(256), 0, ctx->stream, d_cnt, d_off, n_chunks, reinterpret_cast<const int32_t*>(d + b_mask), d_beg, 1);
  hipLaunchKernelGGL(k_export_emit_seeds, dim3((unsigned)n_chunks), dim3(EXPORT_CHUNK), 0, ctx->stream, S, d_off, reinterpret_cast<uint4*>(d_rec), (int)n_rec);
  HSO_HIP_CHECK(ctx, hipGetLastError());
  int32_t beg[2] = {0, 0};
  HSO_HIP_CHECK(ctx, hipMemcpyAsync(beg, d_beg, sizeof(beg), hipMemcpyDeviceToHost, ctx->stream));
  HSO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  *n_out = beg[1];
  const size_t total = (size_t)beg[1], n_write = std::min(total, (size_t)cap);
  if (n_write > 0) {
    HSO_HIP_CHECK(ctx, hipMemcpyAsync(out, d_rec, sizeof(hso_seed_export) * n_write, hipMemcpyDeviceToHost, ctx->stream));
    HSO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (total > (size_t)cap) { ctx->err = "seed_table_export: cap is smaller than the number of selected seeds (n_out holds the full count)"; return HSO_E_TRUNCATED; }
  return HSO_OK;
}

}  // extern "C"
