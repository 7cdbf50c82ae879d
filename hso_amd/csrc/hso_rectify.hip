// hso_rectify.hip — image rectification on gfx950: cv::remap(raw, rectified, undist_map1_, undist_map2_, INTER_LINEAR) of
// FOVCamera / EquidistantCamera::undistortImage (reference src/camera.cpp:267-271, :366-370), which the harness runs on every
// image between ImageReader::readImage and `new Frame` (test/test_dataset.cpp:275-276).  The definition is hso_gpu_rectify_host
// (hso_rectify_host.cpp); this kernel is held to it byte for byte (integer arithmetic only).
//
// One launch rectifies n frames of one size through one map.  A lane owns four adjacent output pixels of a row: it loads their map
// entries once (16 bytes of xy, 8 bytes of frac), turns them into four tap offsets and four weights per pixel, and then walks
// RECT_FPL frames of the batch with those registers — per frame 16 byte loads and one dword store straight into the frame's
// level-0 plane.  The map (6 bytes per pixel) and the weight arithmetic are thus paid once per RECT_FPL frames, not per frame.
//
// One formula serves the three cases of the definition: a tap outside the image gets weight 0 and offset 0 (a load that is always
// in bounds), so "inlier" is all four weights live, "fully outside" none — (0 + 16384) >> 15 = 0, the border value — and
// everything between is what remapBilinear's BORDER_CONSTANT branch computes.  No lane branches on its pixel's class.
//
// Gathers: plain byte loads (global_load_ubyte) served by L1 / L2.  The source rows of a rectifying map are nearly row-coherent —
// the 64 lanes of a wavefront cover 256 consecutive output pixels, whose sources lie on two or three neighbouring source rows — so
// the lines a wavefront touches are the lines its neighbours touch.  This is the only form that was built and measured
// (profiles/rectify.md: 4096 frames of 752x480 in 4.27 ms, 1.2 TB/s of algorithmic bytes, 7.7 x k_pyramid's time — bound by the
// issue rate of the byte gathers, not by HBM); an LDS row tile and two-byte tap loads were not tried.
#include "hso_ctx.h"

#define RECT_FPL 4   // frames per lane pass

typedef const __attribute__((address_space(1))) uint8_t* RectGlbCU8;
typedef __attribute__((address_space(1))) uint32_t* RectGlbU32;

__global__ __launch_bounds__(256) void k_rectify(const uint4* __restrict__ xy, const uint2* __restrict__ frac, int W, int H, uint32_t off0,
                                                 uint8_t* const* __restrict__ bases, const uint8_t* const* __restrict__ srcs, int n)
{
  const int q = blockIdx.x * blockDim.x + threadIdx.x;   // the lane's group of four pixels; W % 4 == 0, so it lies in one row
  if (q >= (W >> 2) * H) return;
  const uint4 m = xy[q];
  const uint2 fr = frac[q];
  const uint32_t mw[4] = {m.x, m.y, m.z, m.w};
  int off[4][4], wt[4][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int sx = (int16_t)(mw[k] & 0xffffu), sy = (int16_t)(mw[k] >> 16);
    const uint32_t f = ((k < 2 ? fr.x : fr.y) >> (16 * (k & 1))) & 1023u;
    const int ax = (int)(f & 31u), ay = (int)(f >> 5);
    const int wgt[4] = {(32 - ax) * (32 - ay) * 32, ax * (32 - ay) * 32, (32 - ax) * ay * 32, ax * ay * 32};
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int tx = sx + (t & 1), ty = sy + (t >> 1);
      const bool in = (unsigned)tx < (unsigned)W && (unsigned)ty < (unsigned)H;
      off[k][t] = in ? ty * W + tx : 0;
      wt[k][t] = in ? wgt[t] : 0;
    }
  }
  const int f0 = blockIdx.y * RECT_FPL;
#pragma unroll
  for (int j = 0; j < RECT_FPL; j++) {
    const int fi = f0 + j;
    if (fi >= n) break;
    // pointers read from a table are generic; say "global" so that the accesses are global_load / global_store
    const RectGlbCU8 S = (RectGlbCU8)srcs[fi];
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int v = (int)S[off[k][0]] * wt[k][0] + (int)S[off[k][1]] * wt[k][1] + (int)S[off[k][2]] * wt[k][2] + (int)S[off[k][3]] * wt[k][3];
      word |= (uint32_t)((v + 16384) >> 15) << (8 * k);   // <= 255: the weights sum to at most 32768
    }
    *(RectGlbU32)(bases[fi] + off0 + (size_t)q * 4) = word;
  }
}

// ------------------------------------------------------------------------------------------------ maps
struct RectifyMap { int w = 0, h = 0; char* d = nullptr; };   // d: xy (4 w h bytes) followed by frac (2 w h bytes); null = destroyed
struct RectifyMaps { std::vector<RectifyMap> maps; };

void hso_rectify_free(hso_gpu_ctx* ctx)
{
  if (!ctx->rectify) return;
  for (RectifyMap& m : ctx->rectify->maps) if (m.d) (void)hipFree(m.d);
  delete ctx->rectify;
  ctx->rectify = nullptr;
}

static const RectifyMap* find_map(hso_gpu_ctx* ctx, int32_t map)
{
  if (!ctx->rectify || map < 0 || (size_t)map >= ctx->rectify->maps.size() || !ctx->rectify->maps[map].d) return nullptr;
  return &ctx->rectify->maps[map];
}

// n frames whose raw images lie at d_srcs[i] (device memory, w x h of the map) -> level 0 of the frames at d_bases[i]
static int rectify_launch(hso_gpu_ctx* ctx, const RectifyMap& m, const PyrGeom& g, uint8_t* const* d_bases, const uint8_t* const* d_srcs, int n)
{
  const int quads = (m.w >> 2) * m.h;
  const int per_launch = 32768 * RECT_FPL;   // blockIdx.y is a 16-bit quantity
  for (int c0 = 0; c0 < n; c0 += per_launch) {
    const int c = std::min(per_launch, n - c0);
    hipLaunchKernelGGL(k_rectify, dim3((quads + 255) / 256, (c + RECT_FPL - 1) / RECT_FPL), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const uint4*>(m.d), reinterpret_cast<const uint2*>(m.d + (size_t)4 * m.w * m.h), m.w, m.h, g.off[0],
                       d_bases + c0, d_srcs + c0, c);
  }
  HSO_HIP_CHECK(ctx, hipGetLastError());
  return HSO_OK;
}

extern "C" {

int hso_gpu_rectify_map_create_tables(hso_gpu_ctx* ctx, int width, int height, const int16_t* xy, const uint16_t* frac, int32_t* map_out)
{
  if (!ctx) return HSO_E_INVALID;
  if (!xy || !frac || !map_out) return hso_fail(ctx, HSO_E_INVALID, "rectify_map_create: null argument");
  if (width <= 0 || height <= 0 || (width % 4) != 0 || width < 64 || height < 64)
    return hso_fail(ctx, HSO_E_INVALID, "rectify_map_create: width must be a multiple of 4, width and height >= 64");
  HSO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t px = (size_t)width * height;
  RectifyMap m;
  m.w = width; m.h = height;
  HSO_HIP_CHECK(ctx, hipMalloc(reinterpret_cast<void**>(&m.d), 6 * px));
  hipError_t e = hipMemcpyAsync(m.d, xy, 4 * px, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m.d + 4 * px, frac, 2 * px, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { (void)hipFree(m.d); HSO_HIP_CHECK(ctx, e); }
  if (!ctx->rectify) ctx->rectify = new RectifyMaps();
  ctx->rectify->maps.push_back(m);
  *map_out = (int32_t)ctx->rectify->maps.size() - 1;
  return HSO_OK;
}

int hso_gpu_rectify_map_create(hso_gpu_ctx* ctx, const hso_camera* cam, int32_t* map_out)
{
  if (!ctx) return HSO_E_INVALID;
  if (!cam || !map_out) return hso_fail(ctx, HSO_E_INVALID, "rectify_map_create: null argument");
  if (cam->width <= 0 || cam->height <= 0 || (cam->width % 4) != 0 || cam->width < 64 || cam->height < 64)
    return hso_fail(ctx, HSO_E_INVALID, "rectify_map_create: width must be a multiple of 4, width and height >= 64");
  const size_t px = (size_t)cam->width * cam->height;
  std::vector<int16_t> xy(2 * px);
  std::vector<uint16_t> frac(px);
  if (hso_gpu_rectify_build_map(cam, xy.data(), frac.data()) < 0)
    return hso_fail(ctx, HSO_E_INVALID, "rectify_map_create: the reference rectifies for FOV cameras with undistort = true and Equidistant cameras only");
  return hso_gpu_rectify_map_create_tables(ctx, cam->width, cam->height, xy.data(), frac.data(), map_out);
}

int hso_gpu_rectify_map_destroy(hso_gpu_ctx* ctx, int32_t map)
{
  if (!ctx) return HSO_E_INVALID;
  if (!find_map(ctx, map)) return hso_fail(ctx, HSO_E_INVALID, "rectify_map_destroy: no such map");
  HSO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HSO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));   // a remap queued earlier may still read it
  RectifyMap& m = ctx->rectify->maps[map];
  (void)hipFree(m.d);
  m.d = nullptr;
  return HSO_OK;
}

// include/hso_gpu_debug.h
int hso_gpu_rectify_map_read(hso_gpu_ctx* ctx, int32_t map, int16_t* xy, uint16_t* frac)
{
  if (!ctx) return HSO_E_INVALID;
  if (!xy || !frac) return hso_fail(ctx, HSO_E_INVALID, "rectify_map_read: null argument");
  const RectifyMap* m = find_map(ctx, map);
  if (!m) return hso_fail(ctx, HSO_E_INVALID, "rectify_map_read: no such map");
  const size_t px = (size_t)m->w * m->h;
  HSO_HIP_CHECK(ctx, hipMemcpyAsync(xy, m->d, 4 * px, hipMemcpyDeviceToHost, ctx->stream));
  HSO_HIP_CHECK(ctx, hipMemcpyAsync(frac, m->d + 4 * px, 2 * px, hipMemcpyDeviceToHost, ctx->stream));
  HSO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return HSO_OK;
}

int hso_gpu_frame_upload_rectified(hso_gpu_ctx* ctx, int64_t frame_id, const uint8_t* img, int src_width, int src_height, int32_t map,
                                   int img_is_device, hso_frame_stats* stats_out)
{
  if (!ctx) return HSO_E_INVALID;
  if (!img || src_width <= 0 || src_height <= 0) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_rectified: null image or bad size");
  const RectifyMap* m = find_map(ctx, map);
  if (!m) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_rectified: no such map");
  const int width = m->w, height = m->h;
  if ((width % 4) != 0 || width < 64 || height < 64)
    return hso_fail(ctx, HSO_E_INVALID, "frame_upload_rectified: width must be a multiple of 4, width and height >= 64");
  if (ctx->frames.count(frame_id)) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_rectified: frame id already resident");
  HSO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // work area: [the raw image, when it comes from the host | the image at the map's size, when the raw one has another]
  const bool resize = src_width != width || src_height != height;
  const size_t raw = img_is_device ? 0 : hso_al256((size_t)src_width * src_height);
  const size_t need = raw + (resize ? (size_t)width * height : 0);
  if (need) if (int rc = hso_batch_reserve(ctx, need)) return rc;
  const uint8_t* d_src = img;
  if (!img_is_device) {
    HSO_HIP_CHECK(ctx, hipMemcpyAsync(ctx->d_batch, img, (size_t)src_width * src_height, hipMemcpyHostToDevice, ctx->stream));
    d_src = reinterpret_cast<const uint8_t*>(ctx->d_batch);
  }
  if (resize) {   // ImageReader::readImage's cv::resize (src/ImageReader.cpp:79) comes first, as in the harness
    uint8_t* d_small = reinterpret_cast<uint8_t*>(ctx->d_batch + raw);
    if (int rc = hso_frame_resize_into(ctx, d_src, src_width, src_height, d_small, width, height)) return rc;
    d_src = d_small;
  }
  FrameRec rec;
  rec.id = frame_id;
  rec.g = make_geom(width, height);
  rec.base = nullptr;
  if (int rc = hso_frame_alloc(ctx, rec.g, &rec.base)) return rc;
  auto give_back = [&]() { (void)hipStreamSynchronize(ctx->stream); hso_frame_free(ctx, rec.g, rec.base); };
#define HSO_RECT_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { ctx->err = std::string(#expr) + ": " + hipGetErrorString(_e); give_back(); return HSO_E_HIP; } } while (0)
  // the kernels take device arrays of frame base / source pointers (batched form); one entry each here
  const void* tab[2] = {rec.base, d_src};
  uint8_t** d_tab = reinterpret_cast<uint8_t**>(rec.base + rec.g.stats_off + 128);
  HSO_RECT_TRY(hipMemcpyAsync(d_tab, tab, sizeof(tab), hipMemcpyHostToDevice, ctx->stream));
  int rc = rectify_launch(ctx, *m, rec.g, d_tab, const_cast<const uint8_t* const*>(d_tab + 1), 1);
  if (rc < 0) { give_back(); return rc; }
  rec.grad_ready = ctx->opt.eager_gradients != 0;
  rc = hso_frame_build(ctx, rec.g, d_tab, nullptr, nullptr, 1, rec.grad_ready);
  if (rc < 0) { give_back(); return rc; }
  if (stats_out)
    HSO_RECT_TRY(hipMemcpyAsync(stats_out, rec.base + rec.g.stats_off, sizeof(hso_frame_stats), hipMemcpyDeviceToHost, ctx->stream));
  HSO_RECT_TRY(hipStreamSynchronize(ctx->stream));   // the work area is reused by later calls
#undef HSO_RECT_TRY
  ctx->frames[frame_id] = rec;
  return HSO_OK;
}

int hso_gpu_frame_upload_batch_rectified(hso_gpu_ctx* ctx, const int64_t* frame_ids, const uint8_t* const* imgs, int n, int32_t map,
                                         int img_is_device, hso_frame_stats* stats_out)
{
  if (!ctx) return HSO_E_INVALID;
  if (!frame_ids || !imgs || n <= 0) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_rectified: null argument or n <= 0");
  const RectifyMap* m = find_map(ctx, map);
  if (!m) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_rectified: no such map");
  const int width = m->w, height = m->h;
  if ((width % 4) != 0 || width < 64 || height < 64)
    return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_rectified: width must be a multiple of 4, width and height >= 64");
  HSO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const PyrGeom g = make_geom(width, height);
  // as hso_gpu_frame_upload_batch: validate every entry, then allocate the new ones; ctx->frames is only touched once nothing
  // can fail any more, so an error in the middle of a batch leaves no half-built frame resident
  std::vector<uint8_t*> bases(n);
  std::vector<int> fresh;
  for (int i = 0; i < n; i++) {
    if (!imgs[i]) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_rectified: null image");
    auto it = ctx->frames.find(frame_ids[i]);
    if (it != ctx->frames.end() && !same_geom(it->second.g, g))
      return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_rectified: resident frame has another size");
    for (int k = 0; k < i && it == ctx->frames.end(); k++)
      if (frame_ids[k] == frame_ids[i]) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_rectified: a new frame id appears twice");
  }
  auto undo = [&]() { hso_stream_abandon(ctx->stream); for (int i : fresh) hso_frame_free(ctx, g, bases[i]); };
  for (int i = 0; i < n; i++) {
    auto it = ctx->frames.find(frame_ids[i]);
    if (it != ctx->frames.end()) {   // refresh in place: from here on the gradient images are no longer this frame's
      bases[i] = it->second.base; it->second.grad_ready = false;
      continue;
    }
    if (int rc = hso_frame_alloc(ctx, g, &bases[i])) { undo(); return rc; }
    fresh.push_back(i);
  }
#define HSO_BATCH_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { ctx->err = std::string(#expr) + ": " + hipGetErrorString(_e); undo(); return HSO_E_HIP; } } while (0)
  // work area: [bases | srcs | stats | the raw images, when they come from the host]
  const size_t b_ptr = hso_al256((size_t)n * sizeof(void*)), b_stats = hso_al256((size_t)n * sizeof(hso_frame_stats));
  const size_t img_bytes = (size_t)width * height, img_stride = hso_al256(img_bytes);
  const size_t need = 2 * b_ptr + b_stats + (img_is_device ? 0 : (size_t)n * img_stride);
  if (int rc = hso_batch_reserve(ctx, need)) { undo(); return rc; }
  uint8_t** d_bases = reinterpret_cast<uint8_t**>(ctx->d_batch);
  const uint8_t** d_srcs = reinterpret_cast<const uint8_t**>(ctx->d_batch + b_ptr);
  hso_frame_stats* d_stats = reinterpret_cast<hso_frame_stats*>(ctx->d_batch + 2 * b_ptr);
  uint8_t* d_raw = reinterpret_cast<uint8_t*>(ctx->d_batch + 2 * b_ptr + b_stats);
  HSO_BATCH_TRY(hipMemcpyAsync(d_bases, bases.data(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
  if (img_is_device) {
    HSO_BATCH_TRY(hipMemcpyAsync(d_srcs, imgs, (size_t)n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
  } else {
    std::vector<const uint8_t*> staged(n);
    for (int i = 0; i < n; i++) {
      staged[i] = d_raw + (size_t)i * img_stride;
      HSO_BATCH_TRY(hipMemcpyAsync(d_raw + (size_t)i * img_stride, imgs[i], img_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    HSO_BATCH_TRY(hipMemcpyAsync(d_srcs, staged.data(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));   // staged now: `staged` may go
  }
  int rc = rectify_launch(ctx, *m, g, d_bases, d_srcs, n);
  if (rc < 0) { undo(); return rc; }
  const bool eager = ctx->opt.eager_gradients != 0;
  rc = hso_frame_build(ctx, g, d_bases, nullptr, stats_out ? d_stats : nullptr, n, eager);
  if (rc < 0) { undo(); return rc; }
  if (stats_out) {
    HSO_BATCH_TRY(hipMemcpyAsync(stats_out, d_stats, (size_t)n * sizeof(hso_frame_stats), hipMemcpyDeviceToHost, ctx->stream));
    HSO_BATCH_TRY(hipStreamSynchronize(ctx->stream));
  }
#undef HSO_BATCH_TRY
  for (int i : fresh) {   // commit
    FrameRec rec;
    rec.id = frame_ids[i]; rec.g = g; rec.base = bases[i];
    ctx->frames[frame_ids[i]] = rec;
  }
  for (int i = 0; i < n; i++) ctx->frames[frame_ids[i]].grad_ready = eager;
  return HSO_OK;
}

// ImageReader::readImage's cv::resize(image, image, m_img_new_size) (reference src/ImageReader.cpp:79) for a batch, in front of the
// optional undistortImage (test/test_dataset.cpp:275-276) and `new Frame`: one k_resize_batch launch, one k_rectify launch when a
// map is named, the batched build, one wait when the statistics are wanted.
int hso_gpu_frame_upload_batch_resized(hso_gpu_ctx* ctx, const int64_t* frame_ids, const uint8_t* const* imgs, int n, int src_width,
                                       int src_height, int width, int height, int32_t map, int img_is_device, hso_frame_stats* stats_out)
{
  if (!ctx) return HSO_E_INVALID;
  if (!frame_ids || !imgs || n <= 0) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_resized: null argument or n <= 0");
  if (src_width <= 0 || src_height <= 0) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_resized: bad source size");
  if ((width % 4) != 0 || width < 64 || height < 64)
    return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_resized: width must be a multiple of 4, width and height >= 64");
  const RectifyMap* m = nullptr;
  if (map >= 0) {
    m = find_map(ctx, map);
    if (!m) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_resized: no such map");
    if (m->w != width || m->h != height) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_resized: the map has another size than the destination");
  }
  if (src_width == width && src_height == height)   // nothing to resize: the two entries this one stands in front of
    return m ? hso_gpu_frame_upload_batch_rectified(ctx, frame_ids, imgs, n, map, img_is_device, stats_out)
             : hso_gpu_frame_upload_batch(ctx, frame_ids, imgs, n, width, height, img_is_device, stats_out);
  HSO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const PyrGeom g = make_geom(width, height);
  // as hso_gpu_frame_upload_batch: validate every entry, then allocate the new ones; ctx->frames is only touched once nothing
  // can fail any more, so an error in the middle of a batch leaves no half-built frame resident
  std::vector<uint8_t*> bases(n);
  std::vector<int> fresh;
  for (int i = 0; i < n; i++) {
    if (!imgs[i]) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_resized: null image");
    auto it = ctx->frames.find(frame_ids[i]);
    if (it != ctx->frames.end() && !same_geom(it->second.g, g))
      return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_resized: resident frame has another size");
    for (int k = 0; k < i && it == ctx->frames.end(); k++)
      if (frame_ids[k] == frame_ids[i]) return hso_fail(ctx, HSO_E_INVALID, "frame_upload_batch_resized: a new frame id appears twice");
  }
  // work area: [bases | srcs | mids | stats | the source images, when they come from the host | the camera-size images, when they
  // are rectified].  Reserved before anything is allocated or marked: a work area that cannot be had is HSO_E_NOMEM and nothing changed.
  const size_t b_ptr = hso_al256((size_t)n * sizeof(void*)), b_stats = hso_al256((size_t)n * sizeof(hso_frame_stats));
  const size_t src_bytes = (size_t)src_width * src_height, src_stride = hso_al256(src_bytes);
  const size_t mid_stride = hso_al256((size_t)width * height);
  const size_t b_raw = img_is_device ? 0 : (size_t)n * src_stride;
  const size_t need = 3 * b_ptr + b_stats + b_raw + (m ? (size_t)n * mid_stride : 0);
  if (hso_batch_reserve(ctx, need)) {
    (void)hipGetLastError();
    return hso_fail(ctx, HSO_E_NOMEM, "frame_upload_batch_resized: no device memory for the work area (n source images, and n camera-size images when rectifying)");
  }
  auto undo = [&]() { hso_stream_abandon(ctx->stream); for (int i : fresh) hso_frame_free(ctx, g, bases[i]); };
  for (int i = 0; i < n; i++) {
    auto it = ctx->frames.find(frame_ids[i]);
    if (it != ctx->frames.end()) {   // refresh in place: from here on the gradient images are no longer this frame's
      bases[i] = it->second.base; it->second.grad_ready = false;
      continue;
    }
    if (int rc = hso_frame_alloc(ctx, g, &bases[i])) { undo(); return rc; }
    fresh.push_back(i);
  }
#define HSO_BATCH_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { ctx->err = std::string(#expr) + ": " + hipGetErrorString(_e); undo(); return HSO_E_HIP; } } while (0)
  uint8_t** d_bases = reinterpret_cast<uint8_t**>(ctx->d_batch);
  const uint8_t** d_srcs = reinterpret_cast<const uint8_t**>(ctx->d_batch + b_ptr);
  uint8_t** d_mids = reinterpret_cast<uint8_t**>(ctx->d_batch + 2 * b_ptr);
  hso_frame_stats* d_stats = reinterpret_cast<hso_frame_stats*>(ctx->d_batch + 3 * b_ptr);
  uint8_t* d_raw = reinterpret_cast<uint8_t*>(ctx->d_batch + 3 * b_ptr + b_stats);
  uint8_t* d_mid = d_raw + b_raw;
  HSO_BATCH_TRY(hipMemcpyAsync(d_bases, bases.data(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
  if (img_is_device) {
    HSO_BATCH_TRY(hipMemcpyAsync(d_srcs, imgs, (size_t)n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
  } else {
    std::vector<const uint8_t*> staged(n);
    for (int i = 0; i < n; i++) {
      staged[i] = d_raw + (size_t)i * src_stride;
      HSO_BATCH_TRY(hipMemcpyAsync(d_raw + (size_t)i * src_stride, imgs[i], src_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    HSO_BATCH_TRY(hipMemcpyAsync(d_srcs, staged.data(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));   // staged now: `staged` may go
  }
  int rc;
  if (m) {   // resize into the work area's camera-size slots, remap from there into level 0
    std::vector<uint8_t*> mids(n);
    for (int i = 0; i < n; i++) mids[i] = d_mid + (size_t)i * mid_stride;
    HSO_BATCH_TRY(hipMemcpyAsync(d_mids, mids.data(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    rc = hso_frame_resize_batch(ctx, d_srcs, src_width, src_height, d_mids, 0, width, height, n);
    if (rc >= 0) rc = rectify_launch(ctx, *m, g, d_bases, const_cast<const uint8_t* const*>(d_mids), n);
  } else {   // resize straight into level 0
    rc = hso_frame_resize_batch(ctx, d_srcs, src_width, src_height, d_bases, g.off[0], width, height, n);
  }
  if (rc < 0) { undo(); return rc; }
  const bool eager = ctx->opt.eager_gradients != 0;
  rc = hso_frame_build(ctx, g, d_bases, nullptr, stats_out ? d_stats : nullptr, n, eager);
  if (rc < 0) { undo(); return rc; }
  if (stats_out) {
    HSO_BATCH_TRY(hipMemcpyAsync(stats_out, d_stats, (size_t)n * sizeof(hso_frame_stats), hipMemcpyDeviceToHost, ctx->stream));
    HSO_BATCH_TRY(hipStreamSynchronize(ctx->stream));
  }
#undef HSO_BATCH_TRY
  for (int i : fresh) {   // commit
    FrameRec rec;
    rec.id = frame_ids[i]; rec.g = g; rec.base = bases[i];
    ctx->frames[frame_ids[i]] = rec;
  }
  for (int i = 0; i < n; i++) ctx->frames[frame_ids[i]].grad_ready = eager;
  return HSO_OK;
}

}  // extern "C"
