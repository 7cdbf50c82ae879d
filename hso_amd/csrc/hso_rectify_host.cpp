// hso_rectify_host.cpp — image rectification, the step the reference's harness runs between ImageReader::readImage and
// FrameHandlerMono::addImage: `if(cam_->getUndistort()) cam_->undistortImage(image, image);` (reference
// test/test_dataset.cpp:276).  Two of its three camera classes take that branch: FOVCamera built with undistort = true
// (src/camera.cpp:163-165) and EquidistantCamera, whose undistort_ is always true (:289) and whose world2cam / cam2world are
// plain pinhole (:297-315) — the whole model lives in the remap.
//
// Host code behind the C-ABI, no context needed, and the definition of both halves:
//   hso_gpu_rectify_build_map   getRemap + distortPixelFOV (:223-265) / getRemap + distortPixelEquidistant (:317-364), followed by
//                               cv::convertMaps(float, float -> CV_16SC2 + CV_16UC1) — once per camera;
//   hso_gpu_rectify_host        cv::remap(src, dst, map1 CV_16SC2, map2 CV_16UC1, INTER_LINEAR) for CV_8UC1 with the default
//                               BORDER_CONSTANT, value 0 (:267-271, :366-370) — the device kernel (hso_rectify.hip) is held to this
//                               function's output byte for byte.
// Every operation keeps the type the reference gives it; this file is compiled with -ffp-contract=off like the rest.
#include <cmath>
#include <cstdint>
#include <climits>
#include "../../include/hso_gpu.h"

namespace {

// cvRound(float) as OpenCV's SSE2 build evaluates it: cvtss2si — round half to even, the "integer indefinite" value for what does
// not fit.  lrintf rounds the same way in the default rounding mode.
inline int cv_round(float v)
{
  if (!(std::fabs(v) < 2147483648.f)) return INT_MIN;
  return (int)lrintf(v);
}

inline int16_t saturate_short(int v) { return (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// The reference's include/hso/camera.h:32 has `using namespace std;`, so its unqualified tan / sqrt / atan calls on float arguments
// resolve to the float overloads: tanf, sqrtf, atanf below are what it runs, not the double functions.

// FOVCamera::distortPixelFOV (src/camera.cpp:247-265): fx_, fy_, cx_, cy_, omega_ are doubles, everything declared float is float
inline void distort_fov(const hso_camera& c, int u, int v, float* ox, float* oy)
{
  const float dist = (float)c.d[0];
  const float d2t = 2 * tanf(dist / 2);
  const float x = (float)u, y = (float)v;
  float ix = (float)(((double)x - c.cx) / c.fx);
  float iy = (float)(((double)y - c.cy) / c.fy);
  const float r = sqrtf(ix * ix + iy * iy);
  const float fac = (r == 0 || dist == 0) ? 1 : atanf(r * d2t) / (dist * r);
  ix = (float)(c.fx * (double)fac * (double)ix + c.cx);
  iy = (float)(c.fy * (double)fac * (double)iy + c.cy);
  *ox = ix; *oy = iy;
}

// EquidistantCamera::distortPixelEquidistant (src/camera.cpp:342-364): d_[0..3] are doubles, so the polynomial is a double sum
// (added left to right) of double * float products, and theta * (...) is rounded to float once
inline void distort_equidistant(const hso_camera& c, int u, int v, float* ox, float* oy)
{
  const float x = (float)u, y = (float)v;
  const float ix = (float)(((double)x - c.cx) / c.fx);
  const float iy = (float)(((double)y - c.cy) / c.fy);
  const float r = sqrtf(ix * ix + iy * iy);
  const float theta = atanf(r);
  const float theta2 = theta * theta;
  const float theta4 = theta2 * theta2;
  const float theta6 = theta4 * theta2;
  const float theta8 = theta4 * theta4;
  const float thetad = (float)((double)theta * (1 + c.d[0] * (double)theta2 + c.d[1] * (double)theta4 + c.d[2] * (double)theta6 + c.d[3] * (double)theta8));
  const float scaling = ((double)r > 1e-8) ? thetad / r : 1.0f;
  *ox = (float)(c.fx * (double)ix * (double)scaling + c.cx);
  *oy = (float)(c.fy * (double)iy * (double)scaling + c.cy);
}

}  // namespace

extern "C" int hso_gpu_rectify_build_map(const hso_camera* cam, int16_t* xy, uint16_t* frac)
{
  if (!cam || !xy || !frac) return HSO_E_INVALID;
  if (cam->width <= 0 || cam->height <= 0) return HSO_E_INVALID;
  // the reference rectifies for these two and no other: PinholeCamera::undistort_ is always false, a FOV camera with
  // undistort = false keeps its distortion in world2cam / cam2world instead
  const bool fov = cam->model == HSO_CAM_FOV && cam->distortion == 0;
  const bool equi = cam->model == HSO_CAM_EQUIDISTANT;
  if (!fov && !equi) return HSO_E_INVALID;
  const int W = cam->width, H = cam->height;
  for (int v = 0; v < H; v++)
    for (int u = 0; u < W; u++) {
      float mx, my;
      if (fov) distort_fov(*cam, u, v, &mx, &my);
      else distort_equidistant(*cam, u, v, &mx, &my);
      // cv::convertMaps, CV_32FC1 x 2 -> CV_16SC2 + CV_16UC1 (INTER_BITS = 5, INTER_TAB_SIZE = 32)
      const int ix = cv_round(mx * 32), iy = cv_round(my * 32);
      const size_t i = (size_t)v * W + u;
      xy[2 * i] = saturate_short(ix >> 5);
      xy[2 * i + 1] = saturate_short(iy >> 5);
      frac[i] = (uint16_t)((iy & 31) * 32 + (ix & 31));
    }
  return HSO_OK;
}

// cv::remap's fixed-point bilinear path (remapBilinear<FixedPtCast<int, uchar, 15>, short> with the table of
// initInterTab2D(INTER_LINEAR, true): the four weights of a cell, scaled by 32768).  OpenCV builds that table from float products
// and then moves the rounding error into the largest entry; for a bilinear cell the products (32 - ax)(32 - ay) / 1024 * 32768 are
// exact integers, so nothing is moved — except that saturate_cast<short> turns the one entry 32768 (ax = ay = 0) into 32767 and
// the correction puts the missing 1 into the cell's last slot: {32767, 0, 0, 1}.  (S00 * 32767 + S11 + 16384) >> 15 equals S00 for
// every pair of bytes — the remainder (S11 - S00 + 16384) stays inside [0, 32768) — so {32768, 0, 0, 0}, used here, gives the same
// byte, also when one of the two taps lies outside and reads 0.
// Taps outside the image read the border value 0: dropping their terms is the same sum.
extern "C" int hso_gpu_rectify_host(const int16_t* xy, const uint16_t* frac, int w, int h, const uint8_t* src, uint8_t* dst)
{
  if (!xy || !frac || !src || !dst || w <= 0 || h <= 0 || src == dst) return HSO_E_INVALID;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const size_t i = (size_t)y * w + x;
      const int sx = xy[2 * i], sy = xy[2 * i + 1];
      const int f = frac[i] & 1023;                       // FXY[x] & (INTER_TAB_SIZE2 - 1)
      const int ax = f & 31, ay = f >> 5;
      const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
      int v;
      if ((unsigned)sx < (unsigned)(w - 1) && (unsigned)sy < (unsigned)(h - 1)) {
        const uint8_t* S = src + (size_t)sy * w + sx;
        v = S[0] * w00 + S[1] * w01 + S[w] * w10 + S[w + 1] * w11;
      } else if (sx >= w || sx + 1 < 0 || sy >= h || sy + 1 < 0) {
        v = 0;
      } else {
        const bool x0 = (unsigned)sx < (unsigned)w, x1 = (unsigned)(sx + 1) < (unsigned)w;
        const bool y0 = (unsigned)sy < (unsigned)h, y1 = (unsigned)(sy + 1) < (unsigned)h;
        v = 0;
        if (x0 && y0) v += src[(size_t)sy * w + sx] * w00;
        if (x1 && y0) v += src[(size_t)sy * w + sx + 1] * w01;
        if (x0 && y1) v += src[(size_t)(sy + 1) * w + sx] * w10;
        if (x1 && y1) v += src[(size_t)(sy + 1) * w + sx + 1] * w11;
      }
      dst[i] = (uint8_t)((v + 16384) >> 15);
    }
  return HSO_OK;
}
