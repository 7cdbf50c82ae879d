// hso_wave.h — the wave64 lane-exchange primitives of the gfx950 device code, each defined once: fixed-distance exchanges,
// butterfly / DPP sums, the halving (reduce-scatter) sum, the inclusive scan, 64-bit shuffles.  Every sum has a fixed order of
// additions, so floating-point results are deterministic; the kernels' bit-for-bit promises (order statistics, the pose
// kernel's sums, the tracker's wave-order combine) rest on these.  tests/test_wave_gpu.py checks each one by itself.
// `lane` is always the lane inside the wavefront (threadIdx.x & 63), never the thread index.
#pragma once
#include <hip/hip_runtime.h>

#define HSO_DEV __device__ __forceinline__

namespace hso_dev {

// ---- DPP moves: the lane reads v from the lane the control code names (rows = 16 lanes, banks of the row mask)
enum : int {
  DPP_QUAD_XOR1 = 0xb1,         // quad_perm:[1,0,3,2]   lane ^ 1
  DPP_QUAD_XOR2 = 0x4e,         // quad_perm:[2,3,0,1]   lane ^ 2
  DPP_QUAD_XOR3 = 0x1b,         // quad_perm:[3,2,1,0]   lane ^ 3
  DPP_ROW_ROR4 = 0x124,         // row_ror:4             the row rotated by 4 lanes
  DPP_ROW_ROR8 = 0x128,         // row_ror:8             the row rotated by 8 lanes = lane ^ 8
  DPP_ROW_HALF_MIRROR = 0x141,  // row_half_mirror       lane ^ 7
  DPP_ROW_BCAST15 = 0x142,      // row_bcast:15          lane 15 of a row to the next row
  DPP_ROW_BCAST31 = 0x143,      // row_bcast:31          lane 31 to rows 2, 3
};
template <int CTRL, int ROW_MASK = 0xf> HSO_DEV int dpp_get(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false); }
template <int CTRL, int ROW_MASK = 0xf> HSO_DEV unsigned dpp_get(unsigned v) { return (unsigned)dpp_get<CTRL, ROW_MASK>((int)v); }
template <int CTRL, int ROW_MASK = 0xf> HSO_DEV float dpp_get(float v) { return __uint_as_float(dpp_get<CTRL, ROW_MASK>(__float_as_uint(v))); }
template <int CTRL, int ROW_MASK = 0xf> HSO_DEV double dpp_get(double v)
{
  const int lo = dpp_get<CTRL, ROW_MASK>(__double2loint(v)), hi = dpp_get<CTRL, ROW_MASK>(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// ---- lane exchanges at a fixed xor distance, cheapest gfx950 form per distance (no LDS crossbar trip):
//   32, 16  v_permlane32_swap / v_permlane16_swap (swap the upper half / odd rows of one register with the lower half /
//           even rows of another: called with the same value twice, the second result is the partner's value in the
//           lower lanes and the first result is it in the upper lanes);
//   8       DPP row_ror:8;   2, 1  DPP quad_perm;   4  two DPP moves (quad_perm [3,2,1,0] then row_half_mirror: 3 ^ 7 = 4).
// The value every lane receives is exactly what __shfl_xor(v, M) returns, so butterfly sums keep their bits.
typedef unsigned lane_u32x2 __attribute__((ext_vector_type(2)));
template <int M> HSO_DEV lane_u32x2 lane_swap(unsigned a, unsigned b)
{
  static_assert(M == 32 || M == 16, "swap distances");
  if constexpr (M == 32) return __builtin_amdgcn_permlane32_swap(a, b, false, false);
  else return __builtin_amdgcn_permlane16_swap(a, b, false, false);
}
template <int M> HSO_DEV unsigned lane_xor(unsigned v)
{
  if constexpr (M == 32 || M == 16) {
    const lane_u32x2 r = lane_swap<M>(v, v);
    const bool up = (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & M) != 0;
    return up ? r[0] : r[1];
  } else if constexpr (M == 8) {
    return dpp_get<DPP_ROW_ROR8>(v);
  } else if constexpr (M == 4) {
    return dpp_get<DPP_ROW_HALF_MIRROR>(dpp_get<DPP_QUAD_XOR3>(v));
  } else if constexpr (M == 2) {
    return dpp_get<DPP_QUAD_XOR2>(v);
  } else {
    static_assert(M == 1, "xor distance");
    return dpp_get<DPP_QUAD_XOR1>(v);
  }
}
template <int M> HSO_DEV float lane_xor(float v) { return __uint_as_float(lane_xor<M>(__float_as_uint(v))); }
template <int M> HSO_DEV int lane_xor(int v) { return (int)lane_xor<M>((unsigned)v); }
template <int M> HSO_DEV double lane_xor(double v)
{
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = lane_xor<M>((unsigned)b), hi = lane_xor<M>((unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Distances 32 and 16 straight from the swap: lanes with (lane & M) == 0 get lo + lo', the others hi + hi' (primes: the
// partner lane's values).  The swap leaves, in every lane, exactly the two values that lane has to add, so no select is
// needed; lane_swap_sum<M>(v, v) is v + partner in every lane.
template <int M> HSO_DEV float lane_swap_sum(float lo, float hi)
{
  const lane_u32x2 r = lane_swap<M>(__float_as_uint(lo), __float_as_uint(hi));
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
template <int M> HSO_DEV int lane_swap_sum(int lo, int hi)
{
  const lane_u32x2 r = lane_swap<M>((unsigned)lo, (unsigned)hi);
  return (int)(r[0] + r[1]);
}
template <int M> HSO_DEV double lane_swap_sum(double lo, double hi)
{
  const unsigned long long bl = (unsigned long long)__double_as_longlong(lo), bh = (unsigned long long)__double_as_longlong(hi);
  const lane_u32x2 r0 = lane_swap<M>((unsigned)bl, (unsigned)bh), r1 = lane_swap<M>((unsigned)(bl >> 32), (unsigned)(bh >> 32));
  return __longlong_as_double((long long)(((unsigned long long)r1[0] << 32) | r0[0])) +
         __longlong_as_double((long long)(((unsigned long long)r1[1] << 32) | r0[1]));
}

// v + partner at distances D, D / 2, ..., 1: every lane of a group of 2 D lanes ends with the group's total
template <int D, typename T> HSO_DEV T wave_butterfly_from(T v)
{
  if constexpr (D >= 1) {
    if constexpr (D == 32 || D == 16) v = lane_swap_sum<D>(v, v);
    else v += lane_xor<D>(v);
    return wave_butterfly_from<D / 2>(v);
  } else {
    return v;
  }
}
// every lane ends with the wave total, summed in the order (32, 16, 8, 4, 2, 1) of the __shfl_xor butterfly it replaces
template <typename T> HSO_DEV T wave_butterfly_sum(T v) { return wave_butterfly_from<32>(v); }

// Sum over the 64 lanes of a wavefront; the total lands in lane 63 (the other lanes hold partial sums).
template <typename T> HSO_DEV T wave_sum_to_lane63(T v)
{
  v += dpp_get<DPP_QUAD_XOR1>(v);
  v += dpp_get<DPP_QUAD_XOR2>(v);
  v += dpp_get<DPP_ROW_ROR4>(v);
  v += dpp_get<DPP_ROW_ROR8>(v);
  v += dpp_get<DPP_ROW_BCAST15, 0xa>(v);  // -> rows 1, 3
  v += dpp_get<DPP_ROW_BCAST31, 0xc>(v);  // -> rows 2, 3
  return v;
}

// Sums inside a DPP row of 16 lanes / inside a group of 8 lanes (half a row); every lane of the row / group ends with the same
// bits (each step adds the same two partial sums in both partners).
HSO_DEV float row_sum16(float v)
{
  v += dpp_get<DPP_ROW_ROR8>(v);
  v += dpp_get<DPP_ROW_ROR4>(v);
  v += dpp_get<DPP_QUAD_XOR2>(v);
  v += dpp_get<DPP_QUAD_XOR1>(v);
  return v;
}
HSO_DEV float row_sum8(float v)
{
  v += dpp_get<DPP_ROW_HALF_MIRROR>(v);   // l8 <-> 7 - l8
  v += dpp_get<DPP_QUAD_XOR1>(v);
  v += dpp_get<DPP_QUAD_XOR2>(v);
  return v;
}

// Sum N (a power of two) per-lane values over the 2 M lanes of a group (M = 32: the wavefront) by recursive halving
// (reduce-scatter): at each step (lane distance M, M / 2, ...) a lane hands the half of its values it is not responsible for
// to its partner and adds the partner's contribution to the half it keeps, so N values cost ~N exchanges instead of 6 N for N
// butterflies.  The swap instructions of distances 32 / 16 do exactly "hand over the half you do not keep".
// Contract: afterwards EVERY lane holds in `out` the total of value `slot`, with slot = (lane % 2M) / G < N and G = 2 M / N: the G
// adjacent lanes of a slot all hold the same slot and the same total.  A caller that stores each total once selects the
// slot's first lane, wave_halve_first<N, M>(lane).
template <typename T, int N, int M> HSO_DEV void wave_halve_step(T (&v)[N], int lane, int& slot, T& out)
{
  static_assert((N & (N - 1)) == 0 && N >= 2 && N <= 2 * M, "N must be a power of two, at most one value per lane left");
  constexpr int HALF = N / 2;
  const bool up = (lane & M) != 0;
  T keep[HALF];
#pragma unroll
  for (int i = 0; i < HALF; i++) {
    if constexpr (M == 32 || M == 16) {
      keep[i] = lane_swap_sum<M>(v[i], v[HALF + i]);
    } else {
      const T send = up ? v[i] : v[HALF + i];
      keep[i] = (up ? v[HALF + i] : v[i]) + lane_xor<M>(send);
    }
  }
  if (up) slot += HALF;
  // a single value left: plain butterflies over the remaining distances
  if constexpr (HALF == 1) out = wave_butterfly_from<M / 2>(keep[0]);
  else wave_halve_step<T, HALF, M / 2>(keep, lane, slot, out);
}
template <typename T, int N, int M> HSO_DEV void wave_halve(T (&v)[N], int lane, int& slot, T& out)
{
  slot = 0;
  wave_halve_step<T, N, M>(v, lane, slot, out);
}
template <int N, int M> HSO_DEV bool wave_halve_first(int lane) { return (lane & (2 * M / N - 1)) == 0; }

// inclusive prefix sum over the lanes of a wavefront (lane 63 ends with the total)
template <typename T> HSO_DEV T wave_inclusive_scan(T v, int lane)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const T o = __shfl_up(v, d); if (lane >= d) v += o; }
  return v;
}

// 64-bit values through the 32-bit shuffles, for lanes / distances known only at run time
HSO_DEV double wave_shfl(double v, int src)
{
  const int lo = __shfl(__double2loint(v), src), hi = __shfl(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}
HSO_DEV double wave_shfl_xor(double v, int m)
{
  const int lo = __shfl_xor(__double2loint(v), m), hi = __shfl_xor(__double2hiint(v), m);
  return __hiloint2double(hi, lo);
}
HSO_DEV long long wave_shfl_xor(long long v, int m)
{
  const int lo = __shfl_xor((int)(v & 0xffffffffll), m), hi = __shfl_xor((int)(v >> 32), m);
  return ((long long)hi << 32) | (unsigned)lo;
}

}  // namespace hso_dev
