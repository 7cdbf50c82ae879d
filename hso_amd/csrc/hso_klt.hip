// hso_klt.hip — the image side of the two-view initialisation on the device: initialization::trackKlt
// (reference src/initialization.cpp:225-300) = cv::calcOpticalFlowPyrLK(img_prev, img_cur, px_prev, px_cur, .., Size(30, 30), 4,
// TermCriteria(COUNT + EPS, 30, 1e-4), OPTFLOW_USE_INITIAL_FLOW) followed by patchCheck (:476-563) per point.
//
// OpenCV is not part of the reference tree; the arithmetic follows its published pyramidal LK (14-bit fixed-point bilinear
// windows, Scharr derivatives, Gaussian 5x5 pyramid; oracle/hso_oracle_klt.c restates it on the CPU and states what is and is
// not pinned).  Data flow per call:
//   k_pyr_down4  level l of both frames' Gaussian pyramids for every pair of the call (level 0 = the resident frame's level-0
//                image, not copied); one launch per level
//   k_scharr4    interleaved int16 (Ix, Iy) of one level of every pair's PREVIOUS frame; one launch per level
//   k_klt        one 256-thread workgroup per point, coarse to fine: the 30x30 template window and its gradients live in LDS as
//                int16 (5.4 KB), the 2x2 matrix and the right-hand side are summed as exact 64-bit integers (OpenCV's float
//                accumulation order differs between its scalar and SIMD paths; the exact sum is the value both approximate),
//                then the 8x8 patch check on level 0.
// A call carries any number of frame pairs (hso_gpu_klt_track_multi: the sequences of a bank start together; hso_gpu_klt_track is
// a batch of one pair through the same code).  The pairs' level tables (KltLevels) sit in a device table; the image kernels take
// the pair from blockIdx.z, and k_klt finds its point's pair in a per-row int32 that the upload carries.  That index rather than
// a binary search of first[]: the ranges arrive in any order and may leave rows unowned, so a search would need a sorted copy
// beside the table and would put log2(n_pairs) dependent loads in front of every workgroup's work; the index is one 4-byte load
// per workgroup, and 4 bytes per row of upload beside the 16 of the two point tables.
// Per call: one upload [level tables | pair index | px_prev | px_init], assembled in page-locked staging; one launch per level
// for the pyramids and one per level for the derivatives; one k_klt launch over all rows; one download; one wait.
// Work area (hso_batch_reserve only).  P = pairs with n > 0, N = n_total, levels 0..L of w_l x h_l, every term rounded up to 256:
//   sizeof(KltLevels) P + 4 N + 8 N + 8 N + 16 N + P (2 sum_{l=1..L} w_l h_l + 4 sum_{l=0..L} w_l h_l)
// = 2.16 MB per pair + 36 bytes per point at 752x480 (L = 3).  A frame named by several pairs gets its pyramid once per pair.
// The image kernels: a lane owns four adjacent output pixels; it reads its source columns as aligned dwords where the row and the
// columns allow, and byte by byte through reflect101 indices computed once otherwise (borders, and rows of levels whose width is
// no multiple of 4 such as 94 or 47); it stores one dword (pyrDown) or one 16-byte vector of four (Ix, Iy) (Scharr) where that
// store is aligned and whole, single pixels on the row tail.  Integer arithmetic: bit for bit what one thread per pixel computes.
// All of it is HBM/L2-latency bound integer work; a sequence runs it a handful to a few dozen times (until the median disparity
// reaches Config::initMinDisparity), a bank once per step for all its starting sequences.
#include "hso_ctx.h"
#include "hso_wave.h"
#include "hso_klt_ranges.h"
#include <string.h>

namespace {

constexpr int KLT_THREADS = 256;
constexpr int KLT_MAX_WIN = 32;
constexpr int KLT_MAX_LEVELS = 8;
constexpr int IMG_TX = 32, IMG_TY = 8;   // the image kernels' workgroup: 32 x 8 lanes = 128 x 8 output pixels

__device__ __forceinline__ int reflect101(int i, int n)
{
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

// one frame pair's levels as the kernels see them; the call's device table holds one per pair with points
// A plain pointer read from a device table is a generic one to the compiler, and what is loaded through it a flat load, which
// waits on the LDS counter as well as the memory counter.  The table holds addresses of device memory only, and its members say
// so: the kernels' loads are global loads, as they were when the pointers were kernel arguments.
typedef const __attribute__((address_space(1))) uint8_t* KltImage;
typedef const __attribute__((address_space(1))) short2* KltDeriv;
struct KltLevels {
  KltImage prev[KLT_MAX_LEVELS];
  KltImage cur[KLT_MAX_LEVELS];
  KltDeriv deriv[KLT_MAX_LEVELS];
  int w[KLT_MAX_LEVELS], h[KLT_MAX_LEVELS];
  int last;       // index of the coarsest level
};

// cv::pyrDown, 8-bit, BORDER_REFLECT_101: [1 4 6 4 1]^2 / 256 with rounding.  Level l (dw x dh) from level l - 1 (w x h) of image
// z of the call: z >> 1 the pair, z & 1 the frame (0 previous, 1 current).  The lane's outputs x0 .. x0 + 3 read the source
// columns 2 x0 - 2 .. 2 x0 + 8.
__global__ __launch_bounds__(IMG_TX * IMG_TY) void k_pyr_down4(const KltLevels* __restrict__ tab, int n_img, int l, int w, int h, int dw, int dh)
{
  const int x0 = 4 * (blockIdx.x * IMG_TX + threadIdx.x), y = blockIdx.y * IMG_TY + threadIdx.y;
  if (x0 >= dw || y >= dh) return;
  int xs[11], ry[5];
#pragma unroll
  for (int k = 0; k < 11; k++) xs[k] = reflect101(2 * x0 - 2 + k, w);
#pragma unroll
  for (int k = 0; k < 5; k++) ry[k] = reflect101(2 * y - 2 + k, h);
  const bool wide = x0 >= 2 && 2 * x0 + 12 <= w;       // the four dwords at columns 2 x0 - 4 .. 2 x0 + 11 lie inside the row
  const int wk[5] = {1, 4, 6, 4, 1};
  for (int z = blockIdx.z; z < n_img; z += gridDim.z) {
    const KltLevels& L = tab[z >> 1];
    const uint8_t* __restrict__ src = (const uint8_t*)((z & 1) ? L.cur[l - 1] : L.prev[l - 1]);
    uint8_t* dst = (uint8_t*)((z & 1) ? L.cur[l] : L.prev[l]) + (size_t)y * dw + x0;
    int v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const uint8_t* s = src + (size_t)ry[k] * w;
      int c[11];
      if (wide && ((uintptr_t)s & 3) == 0) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(s + 2 * x0 - 4);
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
        c[0] = (d0 >> 16) & 255; c[1] = d0 >> 24;
        c[2] = d1 & 255; c[3] = (d1 >> 8) & 255; c[4] = (d1 >> 16) & 255; c[5] = d1 >> 24;
        c[6] = d2 & 255; c[7] = (d2 >> 8) & 255; c[8] = (d2 >> 16) & 255; c[9] = d2 >> 24;
        c[10] = d3 & 255;
      } else {
#pragma unroll
        for (int i = 0; i < 11; i++) c[i] = s[xs[i]];
      }
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] += wk[k] * (c[2 * j + 2] * 6 + (c[2 * j + 1] + c[2 * j + 3]) * 4 + c[2 * j] + c[2 * j + 4]);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = (v[j] + 128) >> 8;
    if (x0 + 3 < dw && ((uintptr_t)dst & 3) == 0)
      *reinterpret_cast<uint32_t*>(dst) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    else {
#pragma unroll
      for (int j = 0; j < 4; j++) if (x0 + j < dw) dst[j] = (uint8_t)v[j];
    }
  }
}

// calcSharrDeriv of level l (w x h) of every pair's previous frame: d[2 * (y * w + x)] = Ix, + 1 = Iy.  The lane's outputs
// x0 .. x0 + 3 read the source columns x0 - 1 .. x0 + 4 of three rows.
__global__ __launch_bounds__(IMG_TX * IMG_TY) void k_scharr4(const KltLevels* __restrict__ tab, int n_pairs, int l, int w, int h)
{
  const int x0 = 4 * (blockIdx.x * IMG_TX + threadIdx.x), y = blockIdx.y * IMG_TY + threadIdx.y;
  if (x0 >= w || y >= h) return;
  int xs[6];
#pragma unroll
  for (int k = 0; k < 6; k++) xs[k] = reflect101(x0 - 1 + k, w);
  const int ry[3] = {reflect101(y - 1, h), y, reflect101(y + 1, h)};
  const bool wide = x0 >= 4 && x0 + 8 <= w;            // the three dwords at columns x0 - 4 .. x0 + 7 lie inside the row
  for (int z = blockIdx.z; z < n_pairs; z += gridDim.z) {
    const KltLevels& L = tab[z];
    const uint8_t* __restrict__ src = (const uint8_t*)L.prev[l];
    short2* d = (short2*)L.deriv[l] + (size_t)y * w + x0;
    int a[3][6];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const uint8_t* s = src + (size_t)ry[r] * w;
      if (wide && ((uintptr_t)s & 3) == 0) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(s + x0 - 4);
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
        a[r][0] = d0 >> 24;
        a[r][1] = d1 & 255; a[r][2] = (d1 >> 8) & 255; a[r][3] = (d1 >> 16) & 255; a[r][4] = d1 >> 24;
        a[r][5] = d2 & 255;
      } else {
#pragma unroll
        for (int i = 0; i < 6; i++) a[r][i] = s[xs[i]];
      }
    }
    int t0[6], t1[6];
#pragma unroll
    for (int i = 0; i < 6; i++) { t0[i] = (a[0][i] + a[2][i]) * 3 + a[1][i] * 10; t1[i] = a[2][i] - a[0][i]; }
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const short ix = (short)(t0[j + 2] - t0[j]), iy = (short)((t1[j] + t1[j + 2]) * 3 + t1[j + 1] * 10);
      o[j] = (uint32_t)(uint16_t)ix | ((uint32_t)(uint16_t)iy << 16);
    }
    if (x0 + 3 < w && ((uintptr_t)d & 15) == 0)
      *reinterpret_cast<uint4*>(d) = make_uint4(o[0], o[1], o[2], o[3]);
    else {
#pragma unroll
      for (int j = 0; j < 4; j++) if (x0 + j < w) d[j] = make_short2((short)(o[j] & 0xffff), (short)(o[j] >> 16));
    }
  }
}

__device__ __forceinline__ long long wave_sum_i64(long long v)
{
  for (int o = 32; o > 0; o >>= 1) v += hso_dev::wave_shfl_xor(v, o);
  return v;
}

#define DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))

struct KltShared {
  short I[KLT_MAX_WIN * KLT_MAX_WIN];
  short2 dI[KLT_MAX_WIN * KLT_MAX_WIN];
  long long part[3][KLT_THREADS / 64];
  float patch[2][64];
  int ok[2];
};

// block-wide exact sums of up to three 64-bit values; every thread receives the totals
__device__ __forceinline__ void block_sum3(KltShared& s, long long& a, long long& b, long long& c)
{
  a = wave_sum_i64(a); b = wave_sum_i64(b); c = wave_sum_i64(c);
  const int wv = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { s.part[0][wv] = a; s.part[1][wv] = b; s.part[2][wv] = c; }
  __syncthreads();
  a = b = c = 0;
  for (int k = 0; k < KLT_THREADS / 64; k++) { a += s.part[0][k]; b += s.part[1][k]; c += s.part[2][k]; }
}

__device__ __forceinline__ void bilinear_weights(float a, float b, int& iw00, int& iw01, int& iw10, int& iw11)
{
  const int W_BITS = 14;
  iw00 = __float2int_rn((1.f - a) * (1.f - b) * (1 << W_BITS));
  iw01 = __float2int_rn(a * (1.f - b) * (1 << W_BITS));
  iw10 = __float2int_rn((1.f - a) * b * (1 << W_BITS));
  iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
}

// a derivative tap, 0 outside the image (BORDER_CONSTANT).  Written as a guarded load: `in ? dI[at] : zero` with the zero a local
// short2 made the compiler select between two ADDRESSES and keep the zero in scratch memory (8 bytes per lane, one store per tap)
__device__ __forceinline__ short2 deriv_tap(const short2* __restrict__ dI, bool in, size_t at)
{
  short2 v = make_short2(0, 0);
  if (in) v = dI[at];
  return v;
}

// row i of the call's tables; pair_of[i] = the row's pair in `tab`, -1: no pair owns the row (its result is all zero)
__global__ __launch_bounds__(KLT_THREADS) void k_klt(const KltLevels* __restrict__ tab, const int32_t* __restrict__ pair_of,
                                                     const float2* __restrict__ px_prev, const float2* __restrict__ px_init,
                                                     hso_klt_result* __restrict__ out, int n, int win, int max_count, double eps2,
                                                     int use_initial)
{
  __shared__ KltShared s;
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i >= n) return;
  const int pair = __builtin_amdgcn_readfirstlane(pair_of[i]);   // the same in every lane: the table reads below are scalar loads
  if (pair < 0) {                                        // uniform over the workgroup
    if (tid == 0) { hso_klt_result o; o.px[0] = o.px[1] = 0.f; o.ncc = 0.f; o.status = 0; out[i] = o; }
    return;
  }
  const KltLevels& L = tab[pair];
  const int area = win * win;
  const float half = (win - 1) * 0.5f;
  const float FLT_SCALE = 1.f / (1 << 20);
  const float2 p0 = px_prev[i];
  float2 next = px_init[i];
  int status = 1;
  for (int level = L.last; level >= 0; level--) {
    const int w = L.w[level], h = L.h[level];
    const uint8_t* __restrict__ I = (const uint8_t*)L.prev[level];
    const uint8_t* __restrict__ J = (const uint8_t*)L.cur[level];
    const short2* __restrict__ dI = (const short2*)L.deriv[level];
    float2 prev = make_float2(p0.x * (float)(1. / (1 << level)), p0.y * (float)(1. / (1 << level)));
    float2 nxt;
    if (level == L.last) nxt = use_initial ? make_float2(next.x * (float)(1. / (1 << level)), next.y * (float)(1. / (1 << level))) : prev;
    else nxt = make_float2(next.x * 2.f, next.y * 2.f);
    next = nxt;
    prev.x -= half; prev.y -= half;
    const int ipx = (int)floorf(prev.x), ipy = (int)floorf(prev.y);
    if (ipx < -win || ipx >= w || ipy < -win || ipy >= h) { if (level == 0) status = 0; continue; }   // uniform over the workgroup
    int iw00, iw01, iw10, iw11;
    bilinear_weights(prev.x - ipx, prev.y - ipy, iw00, iw01, iw10, iw11);
    long long a11 = 0, a12 = 0, a22 = 0;
    __syncthreads();                                    // the previous level's readers of s.I / s.dI are done
    for (int k = tid; k < area; k += KLT_THREADS) {
      const int y = k / win, x = k - y * win;
      const int X0 = ipx + x, Y0 = ipy + y, X1 = X0 + 1, Y1 = Y0 + 1;
      // intensity outside the image: BORDER_REFLECT_101; derivative outside: 0 (BORDER_CONSTANT)
      const int rx0 = reflect101(X0, w), rx1 = reflect101(X1, w);
      const uint8_t* row0 = I + (size_t)reflect101(Y0, h) * w;
      const uint8_t* row1 = I + (size_t)reflect101(Y1, h) * w;
      const int ival = DESCALE(row0[rx0] * iw00 + row0[rx1] * iw01 + row1[rx0] * iw10 + row1[rx1] * iw11, 14 - 5);
      const bool x0in = X0 >= 0 && X0 < w, x1in = X1 >= 0 && X1 < w, y0in = Y0 >= 0 && Y0 < h, y1in = Y1 >= 0 && Y1 < h;
      const short2 d00 = deriv_tap(dI, x0in && y0in, (size_t)Y0 * w + X0), d01 = deriv_tap(dI, x1in && y0in, (size_t)Y0 * w + X1);
      const short2 d10 = deriv_tap(dI, x0in && y1in, (size_t)Y1 * w + X0), d11 = deriv_tap(dI, x1in && y1in, (size_t)Y1 * w + X1);
      const int ixval = DESCALE(d00.x * iw00 + d01.x * iw01 + d10.x * iw10 + d11.x * iw11, 14);
      const int iyval = DESCALE(d00.y * iw00 + d01.y * iw01 + d10.y * iw10 + d11.y * iw11, 14);
      s.I[k] = (short)ival; s.dI[k] = make_short2((short)ixval, (short)iyval);
      a11 += (long long)ixval * ixval; a12 += (long long)ixval * iyval; a22 += (long long)iyval * iyval;
    }
    block_sum3(s, a11, a12, a22);
    const float A11 = (float)a11 * FLT_SCALE, A12 = (float)a12 * FLT_SCALE, A22 = (float)a22 * FLT_SCALE;
    float D = A11 * A22 - A12 * A12;
    const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (2 * win * win);
    if (minEig < 1e-4f || D < 1.1920929e-07f) { if (level == 0) status = 0; continue; }
    D = 1.f / D;
    nxt.x -= half; nxt.y -= half;
    float pdx = 0, pdy = 0;
    for (int j = 0; j < max_count; j++) {
      const int inx = (int)floorf(nxt.x), iny = (int)floorf(nxt.y);
      if (inx < -win || inx >= w || iny < -win || iny >= h) { if (level == 0) status = 0; break; }
      bilinear_weights(nxt.x - inx, nxt.y - iny, iw00, iw01, iw10, iw11);
      long long b1 = 0, b2 = 0, unused = 0;
      for (int k = tid; k < area; k += KLT_THREADS) {
        const int y = k / win, x = k - y * win;
        const int rx0 = reflect101(inx + x, w), rx1 = reflect101(inx + x + 1, w);
        const uint8_t* row0 = J + (size_t)reflect101(iny + y, h) * w;
        const uint8_t* row1 = J + (size_t)reflect101(iny + y + 1, h) * w;
        const int diff = DESCALE(row0[rx0] * iw00 + row0[rx1] * iw01 + row1[rx0] * iw10 + row1[rx1] * iw11, 14 - 5) - s.I[k];
        const short2 d = s.dI[k];
        b1 += (long long)diff * d.x; b2 += (long long)diff * d.y;
      }
      block_sum3(s, b1, b2, unused);
      const float fb1 = (float)b1 * FLT_SCALE, fb2 = (float)b2 * FLT_SCALE;
      const float dx = (A12 * fb2 - A22 * fb1) * D, dy = (A12 * fb1 - A11 * fb2) * D;
      nxt.x += dx; nxt.y += dy;
      next = make_float2(nxt.x + half, nxt.y + half);
      if ((double)dx * dx + (double)dy * dy <= eps2) break;
      if (j > 0 && fabsf(dx + pdx) < 0.01f && fabsf(dy + pdy) < 0.01f) { next.x -= dx * 0.5f; next.y -= dy * 0.5f; break; }
      pdx = dx; pdy = dy;
    }
  }
  // patchCheck (src/initialization.cpp:476-563) on the level-0 images: 8x8 bilinear patches, zero-mean NCC > 0.8.  The patch
  // values are computed by 64 lanes per image; the sums run serially on one lane in the reference's order.
  __syncthreads();
  const int w = L.w[0], h = L.h[0];
  if (tid < 128) {
    const int which = tid >> 6, k = tid & 63;
    const float u = which ? next.x : p0.x, v = which ? next.y : p0.y;
    const uint8_t* img = (const uint8_t*)(which ? L.cur[0] : L.prev[0]);
    const int ui = (int)floorf(u), vi = (int)floorf(v);
    const bool in = !(ui < 4 || ui >= w - 4 || vi < 4 || vi >= h - 4);     // NaN positions fail here: floorf(NaN) converts to INT_MIN
    if (k == 0) s.ok[which] = in ? 1 : 0;
    if (in) {
      const float su = u - ui, sv = v - vi;
      const float wtl = (float)((1.0 - su) * (1.0 - sv)), wtr = (float)(su * (1.0 - sv)), wbl = (float)((1.0 - su) * sv), wbr = su * sv;
      const uint8_t* p = img + (size_t)(vi - 4 + (k >> 3)) * w + (ui - 4 + (k & 7));
      s.patch[which][k] = wtl * p[0] + wtr * p[1] + wbl * p[w] + wbr * p[w + 1];
    }
  }
  __syncthreads();
  if (tid == 0) {
    float ncc = -2.f;
    int patch_ok = 0;
    if (s.ok[0] && s.ok[1]) {
      float ma = 0, mb = 0;
      for (int k = 0; k < 64; k++) { ma += s.patch[0][k]; mb += s.patch[1][k]; }
      ma /= 64; mb /= 64;
      float num = 0, d1 = 0, d2 = 0;
      for (int k = 0; k < 64; k++) {
        const float a = s.patch[0][k] - ma, b = s.patch[1][k] - mb;
        num += a * b; d1 += a * a; d2 += b * b;
      }
      const double r = (double)num / ((double)sqrtf(d1 * d2) + 1e-12);
      ncc = (float)r;
      patch_ok = r > (double)0.8f;
    }
    hso_klt_result o;
    o.px[0] = next.x; o.px[1] = next.y; o.ncc = ncc;
    o.status = (status ? HSO_KLT_TRACKED : 0) | (patch_ok ? HSO_KLT_PATCH_OK : 0);
    out[i] = o;
  }
}

dim3 image_grid(int w, int h, int n_z)
{
  return dim3(((w + 3) / 4 + IMG_TX - 1) / IMG_TX, (h + IMG_TY - 1) / IMG_TY, std::min(n_z, 65535));
}

}  // namespace

extern "C" int hso_gpu_klt_levels(int width, int height, int win, int max_level)
{
  for (int level = 0; level <= max_level; level++) {
    width = (width + 1) / 2; height = (height + 1) / 2;
    if (width <= win || height <= win) return level;
  }
  return max_level;
}

extern "C" int hso_gpu_klt_track_multi(hso_gpu_ctx* ctx, const hso_klt_pair* pairs, int n_pairs, const float* px_prev, const float* px_init,
                                       int n_total, const hso_klt_params* params, hso_klt_result* out)
{
  // every check before the first launch: a call that fails has queued nothing
  if (!ctx || !params || n_pairs < 0 || n_total < 0 || (n_pairs > 0 && !pairs) || (n_total > 0 && (!px_prev || !px_init || !out))) return HSO_E_INVALID;
  if (params->win_size < 3 || params->win_size > KLT_MAX_WIN || params->max_level < 0 || params->max_level >= KLT_MAX_LEVELS)
    return hso_fail(ctx, HSO_E_INVALID, "klt_track: window size must be 3..32 and max_level 0..7");
  std::vector<int32_t> active;
  if (hso_klt_check_ranges(pairs, n_pairs, n_total, active) != HSO_OK)
    return hso_fail(ctx, HSO_E_INVALID, "klt_track: a pair's rows lie outside the tables or overlap another pair's");
  const FrameRec* first = nullptr;
  for (int p = 0; p < n_pairs; p++) {
    auto ip = ctx->frames.find(pairs[p].frame_prev), ic = ctx->frames.find(pairs[p].frame_cur);
    if (ip == ctx->frames.end() || ic == ctx->frames.end()) return hso_fail(ctx, HSO_E_NOFRAME, "klt_track: frame not resident");
    if (!first) first = &ip->second;
    if (!same_geom(first->g, ip->second.g) || !same_geom(first->g, ic->second.g)) return hso_fail(ctx, HSO_E_INVALID, "klt_track: the frames differ in size");
  }
  if (active.empty()) {
    if (n_total > 0) memset(out, 0, sizeof(hso_klt_result) * (size_t)n_total);   // rows nobody owns come back zero
    return HSO_OK;
  }
  const PyrGeom& g = first->g;
  const int win = params->win_size, na = (int)active.size();
  KltLevels G;                                           // the geometry every pair shares
  G.last = hso_gpu_klt_levels(g.w[0], g.h[0], win, params->max_level);
  G.w[0] = g.w[0]; G.h[0] = g.h[0];
  for (int l = 1; l <= G.last; l++) { G.w[l] = (G.w[l - 1] + 1) / 2; G.h[l] = (G.h[l - 1] + 1) / 2; }
  for (int l = G.last + 1; l < KLT_MAX_LEVELS; l++) G.w[l] = G.h[l] = 0;
  // one allocation: [level tables | pair index | px_prev | px_init] (the upload) | results | per pair: levels 1.. of prev,
  // levels 1.. of cur, derivatives of every prev level
  size_t off = 0, img_off[2][KLT_MAX_LEVELS], der_off[KLT_MAX_LEVELS];
  auto take = [&](size_t bytes) { const size_t o = off; off += hso_al256(bytes); return o; };
  const size_t N = (size_t)n_total;
  const size_t o_tab = take(sizeof(KltLevels) * (size_t)na), o_pair = take(sizeof(int32_t) * N), o_prev = take(sizeof(float2) * N),
               o_init = take(sizeof(float2) * N), up_bytes = off, o_out = take(sizeof(hso_klt_result) * N), o_img = off;
  off = 0;
  for (int f = 0; f < 2; f++) for (int l = 1; l <= G.last; l++) img_off[f][l] = take((size_t)G.w[l] * G.h[l]);
  for (int l = 0; l <= G.last; l++) der_off[l] = take(sizeof(short2) * (size_t)G.w[l] * G.h[l]);
  const size_t per_pair = off;
  // the context's grow-only work area (no allocation per call: hipFree synchronises the device)
  if (int rc = hso_batch_reserve(ctx, o_img + per_pair * (size_t)na)) return rc;
  char* d = ctx->d_batch;
  char* up = hso_stage_reserve(ctx->stream, up_bytes);
  if (!up) return hso_fail(ctx, HSO_E_NOMEM, "klt_track: no staging memory");
  KltLevels* tab = reinterpret_cast<KltLevels*>(up + o_tab);
  for (int a = 0; a < na; a++) {
    const hso_klt_pair& P = pairs[active[(size_t)a]];
    char* area = d + o_img + per_pair * (size_t)a;
    KltLevels L = G;
    for (int l = 0; l < KLT_MAX_LEVELS; l++) { L.prev[l] = L.cur[l] = nullptr; L.deriv[l] = nullptr; }
    L.prev[0] = (KltImage)(ctx->frames.find(P.frame_prev)->second.base + g.off[0]); L.cur[0] = (KltImage)(ctx->frames.find(P.frame_cur)->second.base + g.off[0]);
    for (int l = 1; l <= G.last; l++) { L.prev[l] = (KltImage)(area + img_off[0][l]); L.cur[l] = (KltImage)(area + img_off[1][l]); }
    for (int l = 0; l <= G.last; l++) L.deriv[l] = (KltDeriv)(area + der_off[l]);
    memcpy(&tab[a], &L, sizeof(L));
  }
  hso_klt_fill_pair_of(pairs, active, n_total, reinterpret_cast<int32_t*>(up + o_pair));
  memcpy(up + o_prev, px_prev, sizeof(float2) * N);
  memcpy(up + o_init, px_init, sizeof(float2) * N);
  int rc = HSO_OK;
  auto body = [&]() -> int {
    HSO_HIP_CHECK(ctx, hipMemcpyAsync(d, up, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    const KltLevels* d_tab = reinterpret_cast<const KltLevels*>(d + o_tab);
    const dim3 tb(IMG_TX, IMG_TY);
    for (int l = 1; l <= G.last; l++)
      k_pyr_down4<<<image_grid(G.w[l], G.h[l], 2 * na), tb, 0, ctx->stream>>>(d_tab, 2 * na, l, G.w[l - 1], G.h[l - 1], G.w[l], G.h[l]);
    for (int l = 0; l <= G.last; l++)
      k_scharr4<<<image_grid(G.w[l], G.h[l], na), tb, 0, ctx->stream>>>(d_tab, na, l, G.w[l], G.h[l]);
    int max_count = params->max_iter;                    // TermCriteria clamping of calcOpticalFlowPyrLK
    if (max_count < 0) max_count = 0;
    if (max_count > 100) max_count = 100;
    double eps = params->epsilon;
    if (eps < 0) eps = 0;
    if (eps > 10) eps = 10;
    k_klt<<<n_total, KLT_THREADS, 0, ctx->stream>>>(d_tab, (const int32_t*)(d + o_pair), (const float2*)(d + o_prev), (const float2*)(d + o_init),
                                                    (hso_klt_result*)(d + o_out), n_total, win, max_count, eps * eps, params->use_initial_flow ? 1 : 0);
    HSO_HIP_CHECK(ctx, hipGetLastError());
    HSO_HIP_CHECK(ctx, hipMemcpyAsync(out, d + o_out, sizeof(hso_klt_result) * N, hipMemcpyDeviceToHost, ctx->stream));
    HSO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return HSO_OK;
  };
  rc = body();
  if (rc != HSO_OK) (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

// a batch of one pair
extern "C" int hso_gpu_klt_track(hso_gpu_ctx* ctx, int64_t frame_prev, int64_t frame_cur, const float* px_prev, const float* px_init, int n,
                                 const hso_klt_params* params, hso_klt_result* out)
{
  if (n < 0) return HSO_E_INVALID;
  const hso_klt_pair pair{frame_prev, frame_cur, 0, n};
  return hso_gpu_klt_track_multi(ctx, &pair, 1, px_prev, px_init, n, params, out);
}

// the Gaussian pyramid level / Scharr image the tracker would use, for the parity tests of the two kernels
extern "C" int hso_gpu_klt_debug_level(hso_gpu_ctx* ctx, int64_t frame, int level, uint8_t* img_out, int16_t* deriv_out)
{
  if (!ctx || level < 0 || level >= KLT_MAX_LEVELS) return HSO_E_INVALID;
  auto it = ctx->frames.find(frame);
  if (it == ctx->frames.end()) return hso_fail(ctx, HSO_E_NOFRAME, "klt_debug_level: frame not resident");
  const PyrGeom& g = it->second.g;
  // a table of one pair whose two frames are this one: [table | levels 1..level | derivatives of `level`]
  KltLevels L;
  memset(&L, 0, sizeof(L));
  L.last = level;
  L.w[0] = g.w[0]; L.h[0] = g.h[0];
  for (int l = 1; l <= level; l++) { L.w[l] = (L.w[l - 1] + 1) / 2; L.h[l] = (L.h[l - 1] + 1) / 2; }
  size_t off = hso_al256(sizeof(KltLevels)), lvl_off[KLT_MAX_LEVELS];
  for (int l = 1; l <= level; l++) { lvl_off[l] = off; off += hso_al256((size_t)L.w[l] * L.h[l]); }
  const size_t der_off = off;
  off += hso_al256(sizeof(short2) * (size_t)L.w[level] * L.h[level]);
  char* d = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d), off) != hipSuccess) return hso_fail(ctx, HSO_E_NOMEM, "klt_debug_level");
  L.prev[0] = L.cur[0] = (KltImage)(it->second.base + g.off[0]);
  for (int l = 1; l <= level; l++) L.prev[l] = L.cur[l] = (KltImage)(d + lvl_off[l]);
  L.deriv[level] = (KltDeriv)(d + der_off);
  const KltLevels* d_tab = reinterpret_cast<const KltLevels*>(d);
  const dim3 tb(IMG_TX, IMG_TY);
  hipError_t e = hipMemcpyAsync(d, &L, sizeof(L), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    for (int l = 1; l <= level; l++) k_pyr_down4<<<image_grid(L.w[l], L.h[l], 1), tb, 0, ctx->stream>>>(d_tab, 1, l, L.w[l - 1], L.h[l - 1], L.w[l], L.h[l]);
    k_scharr4<<<image_grid(L.w[level], L.h[level], 1), tb, 0, ctx->stream>>>(d_tab, 1, level, L.w[level], L.h[level]);
    e = hipGetLastError();
  }
  if (e == hipSuccess && img_out) e = hipMemcpyAsync(img_out, (const void*)L.prev[level], (size_t)L.w[level] * L.h[level], hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && deriv_out) e = hipMemcpyAsync(deriv_out, (const void*)L.deriv[level], sizeof(short2) * (size_t)L.w[level] * L.h[level], hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  else (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  if (e != hipSuccess) { ctx->err = std::string("klt_debug_level: ") + hipGetErrorString(e); hso_stream_abandon(ctx->stream); return HSO_E_HIP; }
  return HSO_OK;
}
