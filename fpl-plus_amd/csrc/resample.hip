// Resampling of a [C][D][H][W] volume at non-integer coordinates: the hot path of RandomRotate, Rescale and RandomRescale
// (PyMIC/pymic/transform/rotate.py:14-92, rescale.py:14-153), which the reference runs as scipy.ndimage.rotate /
// scipy.ndimage.zoom in its DataLoader workers.  y[c][o] = interp(x[c], M o + t) with scipy's semantics for spline orders
// 0 and 1 under mode='constant', cval=0; the matrix and the offset are built on the host (fplx/ops.py) in fp64.
//
// The arithmetic is scipy's, operation for operation, so that labels and fp32 images come out with scipy's bits:
//  - coordinates in fp64: c_i = ((o_0 M[i][0] + o_1 M[i][1]) + o_2 M[i][2]) + t_i, the offset added LAST (starting the sum
//    from t_i moves nearest-neighbour ties at 45 and 135 degrees);
//  - outside (any c_i < 0 or c_i > n_i - 1) -> 0, for order 0 too;
//  - order 0: index floor(c_i + 0.5), ties up;
//  - order 1: f = floor(c), y = c - f, weights (1 - y, 1 - (1 - y)) (scipy forms the last weight as 1 minus the others: not
//    y to the last bit); fp64 sum of ((x[f + k] * w_d) * w_h) * w_w over the 8 neighbours - the value is multiplied by one
//    axis weight after the other - k_d outermost, k_w innermost; an index one past the end carries weight 0 and is
//    clamped; one cast to fp32.
// No fused multiply-add may enter either sum (a contracted sum moves a coordinate by an fp64 ulp, which flips voxels on
// the border and at rounding ties).  hipcc's default is -ffp-contract=fast, and HIP's __dmul_rn / __dadd_rn are plain
// operators in a header compiled under that default - sums written with them came out as v_fmac_f64.  So the sums below
// are plain operators under `#pragma clang fp contract(off)`, and the Makefile compiles this file with -ffp-contract=off;
// tests/test_gpu_resample.py holds the result to scipy's bits.
//
// One thread per output voxel, W fastest (coalesced stores), all channels in one launch; the gather side relies on L2.
#include "resample_common.h"      // RsGeo, rs_coord, rs_inside, rs_extents_ok: shared with spline.hip

#pragma clang fp contract(off)     // (the header sets it too: it holds the coordinate sum)

namespace {

template <typename T, int ORDER>
__global__ void __launch_bounds__(RS_THREADS)
resample_affine_k(const T* __restrict__ x, T* __restrict__ y, const RsGeo g) {
  const uint32_t total = (uint32_t)g.C * g.OD * g.OH * g.OW;
  const uint32_t i = blockIdx.x * RS_THREADS + threadIdx.x;
  if (i >= total) return;
  uint32_t r = i;
  const int ow = (int)(r % (uint32_t)g.OW); r /= (uint32_t)g.OW;
  const int oh = (int)(r % (uint32_t)g.OH); r /= (uint32_t)g.OH;
  const int od = (int)(r % (uint32_t)g.OD); r /= (uint32_t)g.OD;
  const T* __restrict__ xc = x + (size_t)r * g.D * g.H * g.W;
  const double o0 = (double)od, o1 = (double)oh, o2 = (double)ow;
  const double cd = rs_coord(g.m[0], g.t[0], o0, o1, o2);
  const double ch = rs_coord(g.m[1], g.t[1], o0, o1, o2);
  const double cw = rs_coord(g.m[2], g.t[2], o0, o1, o2);
  if (!(rs_inside(cd, g.D) && rs_inside(ch, g.H) && rs_inside(cw, g.W))) {
    y[i] = (T)0;
    return;
  }
  if (ORDER == 0) {
    const int id = (int)floor(cd + 0.5), ih = (int)floor(ch + 0.5), iw = (int)floor(cw + 0.5);
    y[i] = xc[((size_t)id * g.H + ih) * g.W + iw];           // 0 <= c <= n - 1  =>  0 <= floor(c + 0.5) <= n - 1
  } else {
    const double fd = floor(cd), fh = floor(ch), fw = floor(cw);
    const double yd = cd - fd, yh = ch - fh, yw = cw - fw;
    const double wd[2] = {1.0 - yd, 1.0 - (1.0 - yd)};
    const double wh[2] = {1.0 - yh, 1.0 - (1.0 - yh)};
    const double ww[2] = {1.0 - yw, 1.0 - (1.0 - yw)};
    const int d0 = (int)fd, h0 = (int)fh, w0 = (int)fw;      // in [0, n - 1]
    const int dd[2] = {d0, min(d0 + 1, g.D - 1)}, hh[2] = {h0, min(h0 + 1, g.H - 1)}, wx[2] = {w0, min(w0 + 1, g.W - 1)};
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (float)xc[((size_t)dd[k >> 2] * g.H + hh[(k >> 1) & 1]) * g.W + wx[k & 1]];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = acc + (((double)v[k] * wd[k >> 2]) * wh[(k >> 1) & 1]) * ww[k & 1];
    y[i] = (T)acc;
  }
}

}  // namespace

extern "C" {

int fplx_resample_affine(const void* x, void* y, int elem_bytes, int order, int c, int d, int h, int w, int od, int oh,
                         int ow, const double* matrix9, const double* offset3, fplx_stream_t stream) {
  FPLX_REQUIRE(x && y && matrix9 && offset3, FPLX_E_NULL, "resample_affine: null pointer");
  FPLX_REQUIRE(rs_extents_ok(c, d, h, w) && rs_extents_ok(c, od, oh, ow), FPLX_E_BADSHAPE,
               "resample_affine: bad extents [%d,%d,%d,%d] -> [%d,%d,%d,%d] (positive, fewer than 2^31 elements)", c, d, h, w,
               c, od, oh, ow);
  FPLX_REQUIRE(order == 0 || order == 1, FPLX_E_BADSHAPE, "resample_affine: order %d (0 nearest, 1 linear)", order);
  FPLX_REQUIRE(elem_bytes == 4 || elem_bytes == 1, FPLX_E_BADDTYPE, "resample_affine: element size %d (4 fp32, 1 uint8)",
               elem_bytes);
  FPLX_REQUIRE(elem_bytes == 4 || order == 0, FPLX_E_BADDTYPE, "resample_affine: uint8 volumes take order 0 only");
  const RsGeo g = rs_geo(c, d, h, w, od, oh, ow, matrix9, offset3);
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)c * od * oh * ow;
  const unsigned grid = (unsigned)((total + RS_THREADS - 1) / RS_THREADS);
  if (elem_bytes == 1)
    resample_affine_k<unsigned char, 0><<<grid, RS_THREADS, 0, st>>>((const unsigned char*)x, (unsigned char*)y, g);
  else if (order == 0)
    resample_affine_k<float, 0><<<grid, RS_THREADS, 0, st>>>((const float*)x, (float*)y, g);
  else
    resample_affine_k<float, 1><<<grid, RS_THREADS, 0, st>>>((const float*)x, (float*)y, g);
  return fplx_check_launch("resample_affine");
}

}  // extern "C"
