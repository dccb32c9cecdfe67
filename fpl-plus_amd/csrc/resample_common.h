// What the resampling kernels share (resample.hip: spline orders 0 and 1; spline.hip: order 3): the geometry argument,
// scipy's coordinate sum and its outside rule, and the extent limits of the C ABI.  The arithmetic is scipy's, operation for
// operation (see resample.hip); both files compile with -ffp-contract=off and include this header under
// `#pragma clang fp contract(off)`, so no fused multiply-add enters the coordinate sum.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RS_THREADS = 256;
constexpr int64_t RS_MAX_ELEMS = (int64_t)1 << 31;      // 32-bit linear indices inside the kernels

struct RsGeo {
  double m[3][3];
  double t[3];
  int C, D, H, W, OD, OH, OW;
};

__device__ __forceinline__ double rs_coord(const double* __restrict__ m, double t, double o0, double o1, double o2) {
  double c = o0 * m[0];
  c = c + o1 * m[1];
  c = c + o2 * m[2];
  return c + t;
}

// !(c >= 0 && c <= n - 1): a NaN coordinate (non-finite matrix) counts as outside, so that no index is ever formed from it
__device__ __forceinline__ bool rs_inside(double c, int n) { return c >= 0.0 && c <= (double)(n - 1); }

inline bool rs_extents_ok(int c, int d, int h, int w) {
  if (c <= 0 || d <= 0 || h <= 0 || w <= 0) return false;
  int64_t n = c;                                              // every partial product stays below 2^62
  for (int e : {d, h, w}) {
    n *= e;
    if (n >= RS_MAX_ELEMS) return false;
  }
  return true;
}

inline RsGeo rs_geo(int c, int d, int h, int w, int od, int oh, int ow, const double* matrix9, const double* offset3) {
  RsGeo g;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) g.m[i][j] = matrix9[3 * i + j];
    g.t[i] = offset3[i];
  }
  g.C = c; g.D = d; g.H = h; g.W = w; g.OD = od; g.OH = oh; g.OW = ow;
  return g;
}

}  // namespace
