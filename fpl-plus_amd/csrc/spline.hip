// Cubic B-spline resampling of a [C][D][H][W] volume: what scipy.ndimage.zoom / rotate / affine_transform do at their default
// spline order 3, which the reference's dataset preparation uses (data/preprocess_vs.py: ndimage.zoom(img_sub, zoom);
// PyMIC/pymic/util/image_process.py:210-228: any order).  Two steps, as in scipy:
//
//  1. fplx_spline_prefilter: fp32 samples -> fp64 B-spline coefficients, a recursive filter along every line of every axis
//     (D, then H, then W, in place) with scipy's mirror boundary.  Per line of length n > 1, pole z, z_n = z^(n-1) (host pow):
//       c[i]  *= (1 - z)(1 - 1/z)                                                       the gain, all samples first
//       c[0]   = (c[0] + z_n c[n-1] + sum_{i=1..n-2} z^i (c[i] + z_n c[n-1-i])) / (1 - z_n z_n)     z^i by repeated product
//       c[i]  += z c[i-1]                      i = 1 .. n-1                              causal
//       c[n-1] = (z c[n-2] + c[n-1]) z / (z z - 1)
//       c[i]   = z (c[i+1] - c[i])             i = n-2 .. 0                              anticausal
//     A line of length 1 is left alone.  The recursion is sequential along a line; the parallelism is across lines, and the
//     sums run in this one order (no scan, no atomics): two runs give the same bits.
//      - D and H passes (sp_prefilter_strided_k): one thread per line, neighbouring threads neighbouring in W, so every step
//        of the walk is one coalesced row access of the wave.
//      - W pass (sp_prefilter_w_k): the lines lie along the fastest axis, a thread walking one would stride by a whole row.
//        A block of SP_LINES threads stages SP_LINES lines x SP_SEG columns through LDS: global accesses are SP_SEG
//        consecutive doubles (256 B) per line, and thread t walks LDS row t.  The row stride SP_SEG + 1 = 33 doubles is odd,
//        so the 32 lanes that ds_read_b64 serves together (bank = 8-byte slot mod 32 there) and the 16 that ds_write_b64
//        serves together hit distinct banks.  The carry (the previous coefficient) stays in a register from one segment to
//        the next: forwards for the causal pass, backwards for the anticausal one.
//  2. fplx_resample_spline: y[c][o] = sum over the 4x4x4 taps of coef * w_d * w_h * w_w at M o + t, in fp64, one cast to
//     fp32.  Coordinates and the outside rule are resample.hip's (resample_common.h).  Taps floor(c) - 1 + k, k = 0..3,
//     reflected about the first and last sample (period 2n - 2); weights with y = c - floor(c), zc = 1 - y:
//       w1 = (y y (y - 2) 3 + 4) / 6, w2 = (zc zc (zc - 2) 3 + 4) / 6, w0 = zc zc zc / 6, w3 = 1 - w0 - w1 - w2.
//     The value is multiplied by one axis weight after the other, k_d outermost and k_w innermost, as the order-1 kernel does.
//     One thread per output voxel, W fastest; the gather side relies on L2.
//
// No fused multiply-add: a contracted sum is another rounding than scipy's, and the tests' rounding bound counts
// operations (tests/splineoracle.py).  Hence `#pragma clang fp contract(off)` and -ffp-contract=off in the Makefile, for the
// reason resample.hip gives.
#include "resample_common.h"

#pragma clang fp contract(off)

namespace {

// one row per built spline order: the filter's pole and its gain (1 - z)(1 - 1/z).  Another order is a row here (orders 4
// and 5 have two poles: a second column then) and a weight function below.
struct SpOrder {
  int order;
  double pole, gain;
};
inline const SpOrder* sp_order_row(int order) {
  static const double z3 = sqrt(3.0) - 2.0;
  static const SpOrder table[] = {{3, z3, (1.0 - z3) * (1.0 - 1.0 / z3)}};
  for (const SpOrder& r : table)
    if (r.order == order) return &r;
  return nullptr;
}
constexpr char SP_BUILT_ORDERS[] = "3";

struct SpLine {
  double z, gain, zn1;     // zn1 = z^(n - 1) for this pass's line length
};

constexpr int SP_LINES = 64;             // lines per block of the W pass = its threads (one wave)
constexpr int SP_SEG = 32;               // columns staged per step
constexpr int SP_STRIDE = SP_SEG + 1;    // LDS row stride in doubles: odd -> conflict-free walks

// D and H passes.  Line l = (outer, in): elements at outer * n * inner + in + i * inner, i < n; `inner` consecutive lines are
// consecutive in memory.  TIN = float reads the samples and writes the coefficients (first pass; n == 1 only converts),
// TIN = double filters in place (src == dst: no __restrict__).
template <typename TIN>
__global__ void __launch_bounds__(RS_THREADS)
sp_prefilter_strided_k(const TIN* src, double* dst, int n, uint32_t inner, uint32_t nlines, const SpLine p) {
  const uint32_t l = blockIdx.x * RS_THREADS + threadIdx.x;
  if (l >= nlines) return;
  const size_t base = (size_t)(l / inner) * n * inner + (l % inner);
  const TIN* s = src + base;
  double* c = dst + base;
  if (n == 1) {
    c[0] = (double)s[0];
    return;
  }
  const double z = p.z, g = p.gain, zn1 = p.zn1;
  double acc = (double)s[0] * g + zn1 * ((double)s[(size_t)(n - 1) * inner] * g);
  double zi = z;
  for (int i = 1; i < n - 1; ++i) {
    acc = acc + zi * ((double)s[(size_t)i * inner] * g + zn1 * ((double)s[(size_t)(n - 1 - i) * inner] * g));
    zi = zi * z;
  }
  acc = acc / (1.0 - zn1 * zn1);
  double prev = acc, prev2 = 0.0;
  c[0] = prev;
  for (int i = 1; i < n; ++i) {
    prev2 = prev;
    prev = (double)s[(size_t)i * inner] * g + z * prev;          // in place: s[i] is read before c[i] is written
    c[(size_t)i * inner] = prev;
  }
  double nxt = (z * prev2 + prev) * z / (z * z - 1.0);
  c[(size_t)(n - 1) * inner] = nxt;
  for (int i = n - 2; i >= 0; --i) {
    nxt = z * (nxt - c[(size_t)i * inner]);
    c[(size_t)i * inner] = nxt;
  }
}

// tile[l][j] = scale * c[line0 + l][col(j)], col(j) = col0 + j, or n - 1 - (col0 + j) when MIRROR; 0 outside the volume.
// A wave instruction covers two lines x SP_SEG consecutive doubles.
template <bool MIRROR>
__device__ __forceinline__ void sp_load_tile(double* tile, const double* c, uint32_t line0, uint32_t nlines, int n, int col0,
                                             double scale) {
#pragma unroll                  // all SP_SEG loads of a thread in flight at once: the tile costs one memory latency, not eight
  for (int r = 0; r < SP_SEG; ++r) {
    const int idx = r * SP_LINES + (int)threadIdx.x;
    const int l = idx / SP_SEG, j = idx % SP_SEG;
    const int col = MIRROR ? n - 1 - (col0 + j) : col0 + j;
    double v = 0.0;
    if (line0 + l < nlines && col >= 0 && col < n) v = c[(size_t)(line0 + l) * n + col] * scale;
    tile[l * SP_STRIDE + j] = v;
  }
}

__device__ __forceinline__ void sp_store_tile(const double* tile, double* c, uint32_t line0, uint32_t nlines, int n, int col0) {
#pragma unroll 4
  for (int r = 0; r < SP_SEG; ++r) {
    const int idx = r * SP_LINES + (int)threadIdx.x;
    const int l = idx / SP_SEG, j = idx % SP_SEG;
    const int col = col0 + j;
    if (line0 + l < nlines && col < n) c[(size_t)(line0 + l) * n + col] = tile[l * SP_STRIDE + j];
  }
}

// W pass, in place, n > 1.  Block b owns lines [b * SP_LINES, +SP_LINES) (rows of n consecutive doubles); thread t walks line t.
__global__ void __launch_bounds__(SP_LINES)
sp_prefilter_w_k(double* c, int n, uint32_t nlines, const SpLine p) {
  __shared__ double ta[SP_LINES * SP_STRIDE];
  __shared__ double tb[SP_LINES * SP_STRIDE];
  const int t = (int)threadIdx.x;
  const uint32_t line0 = blockIdx.x * SP_LINES;
  const bool live = line0 + t < nlines;
  const int nseg = (n + SP_SEG - 1) / SP_SEG;
  const double z = p.z, g = p.gain, zn1 = p.zn1;
  double* row = ta + t * SP_STRIDE;
  const double* rowb = tb + t * SP_STRIDE;

  // start-up sum: c[i] from the segment, c[n-1-i] from its mirror image
  double acc = 0.0, zi = z;
  if (live) {
    const double* lc = c + (size_t)(line0 + t) * n;
    acc = lc[0] * g + zn1 * (lc[n - 1] * g);
  }
  for (int s = 0; s < nseg; ++s) {
    sp_load_tile<false>(ta, c, line0, nlines, n, s * SP_SEG, g);
    sp_load_tile<true>(tb, c, line0, nlines, n, s * SP_SEG, g);
    __syncthreads();
    if (live) {
      for (int j = 0; j < SP_SEG; ++j) {
        const int i = s * SP_SEG + j;
        if (i >= 1 && i <= n - 2) {
          acc = acc + zi * (row[j] + zn1 * rowb[j]);
          zi = zi * z;
        }
      }
    }
    __syncthreads();
  }
  acc = acc / (1.0 - zn1 * zn1);

  // causal pass, segments forwards; the carry is `prev`
  double prev = acc, prev2 = 0.0;
  for (int s = 0; s < nseg; ++s) {
    sp_load_tile<false>(ta, c, line0, nlines, n, s * SP_SEG, g);
    __syncthreads();
    if (live) {
      for (int j = 0; j < SP_SEG; ++j) {
        const int i = s * SP_SEG + j;
        if (i >= n) break;
        if (i > 0) {
          prev2 = prev;
          prev = row[j] + z * prev;
        }
        row[j] = prev;
      }
    }
    __syncthreads();
    sp_store_tile(ta, c, line0, nlines, n, s * SP_SEG);
    __syncthreads();
  }

  // anticausal pass, segments backwards; the carry is `nxt`
  double nxt = (z * prev2 + prev) * z / (z * z - 1.0);
  for (int s = nseg - 1; s >= 0; --s) {
    sp_load_tile<false>(ta, c, line0, nlines, n, s * SP_SEG, 1.0);
    __syncthreads();
    if (live) {
      for (int j = SP_SEG - 1; j >= 0; --j) {
        const int i = s * SP_SEG + j;
        if (i >= n) continue;
        if (i < n - 1) nxt = z * (nxt - row[j]);
        row[j] = nxt;
      }
    }
    __syncthreads();
    sp_store_tile(ta, c, line0, nlines, n, s * SP_SEG);
    __syncthreads();
  }
}

// taps floor(c) - 1 + k reflected about the first and the last sample, and scipy's cubic weights
__device__ __forceinline__ int sp_reflect(int i, int n) {
  if (n == 1) return 0;
  const int period = 2 * n - 2;
  i = (i < 0 ? -i : i) % period;
  return i >= n ? period - i : i;
}

__device__ __forceinline__ void sp_taps3(double c, int n, double* w, int* idx) {
  const double f = floor(c);
  const double y = c - f, zc = 1.0 - y;
  w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
  w[2] = (zc * zc * (zc - 2.0) * 3.0 + 4.0) / 6.0;
  w[0] = zc * zc * zc / 6.0;
  w[3] = 1.0 - w[0] - w[1] - w[2];
  const int i0 = (int)f - 1;                                  // 0 <= c <= n - 1  =>  -1 <= i0 + k <= n + 1
#pragma unroll
  for (int k = 0; k < 4; ++k) idx[k] = sp_reflect(i0 + k, n);
}

__global__ void __launch_bounds__(RS_THREADS)
resample_spline3_k(const double* __restrict__ coef, float* __restrict__ y, const RsGeo g) {
  const uint32_t total = (uint32_t)g.C * g.OD * g.OH * g.OW;
  const uint32_t i = blockIdx.x * RS_THREADS + threadIdx.x;
  if (i >= total) return;
  uint32_t r = i;
  const int ow = (int)(r % (uint32_t)g.OW); r /= (uint32_t)g.OW;
  const int oh = (int)(r % (uint32_t)g.OH); r /= (uint32_t)g.OH;
  const int od = (int)(r % (uint32_t)g.OD); r /= (uint32_t)g.OD;
  const double* __restrict__ xc = coef + (size_t)r * g.D * g.H * g.W;
  const double o0 = (double)od, o1 = (double)oh, o2 = (double)ow;
  const double cd = rs_coord(g.m[0], g.t[0], o0, o1, o2);
  const double ch = rs_coord(g.m[1], g.t[1], o0, o1, o2);
  const double cw = rs_coord(g.m[2], g.t[2], o0, o1, o2);
  if (!(rs_inside(cd, g.D) && rs_inside(ch, g.H) && rs_inside(cw, g.W))) {
    y[i] = 0.f;
    return;
  }
  double wd[4], wh[4], ww[4];
  int dd[4], hh[4], wx[4];
  sp_taps3(cd, g.D, wd, dd);
  sp_taps3(ch, g.H, wh, hh);
  sp_taps3(cw, g.W, ww, wx);
  double acc = 0.0;
#pragma unroll
  for (int kd = 0; kd < 4; ++kd) {
#pragma unroll
    for (int kh = 0; kh < 4; ++kh) {
      const double* __restrict__ row = xc + ((size_t)dd[kd] * g.H + hh[kh]) * g.W;
#pragma unroll
      for (int kw = 0; kw < 4; ++kw) acc = acc + ((row[wx[kw]] * wd[kd]) * wh[kh]) * ww[kw];
    }
  }
  y[i] = (float)acc;
}

}  // namespace

extern "C" {

int fplx_spline_prefilter(const float* x, double* coef, int c, int d, int h, int w, int order, fplx_stream_t stream) {
  FPLX_REQUIRE(x && coef, FPLX_E_NULL, "spline_prefilter: null pointer");
  FPLX_REQUIRE(rs_extents_ok(c, d, h, w), FPLX_E_BADSHAPE,
               "spline_prefilter: bad extents [%d,%d,%d,%d] (positive, fewer than 2^31 elements)", c, d, h, w);
  const SpOrder* row = sp_order_row(order);
  FPLX_REQUIRE(row, FPLX_E_BADSHAPE, "spline_prefilter: order %d (built: %s)", order, SP_BUILT_ORDERS);
  hipStream_t st = (hipStream_t)stream;
  auto line = [&](int n) { return SpLine{row->pole, row->gain, pow(row->pole, (double)(n - 1))}; };
  auto blocks = [](int64_t lines, int per) { return (unsigned)((lines + per - 1) / per); };
  // D: samples -> coefficients (D == 1 only converts); H and W in place
  const int64_t ld = (int64_t)c * h * w, lh = (int64_t)c * d * w, lw = (int64_t)c * d * h;
  sp_prefilter_strided_k<float><<<blocks(ld, RS_THREADS), RS_THREADS, 0, st>>>(x, coef, d, (uint32_t)(h * w), (uint32_t)ld, line(d));
  if (h > 1)
    sp_prefilter_strided_k<double><<<blocks(lh, RS_THREADS), RS_THREADS, 0, st>>>(coef, coef, h, (uint32_t)w, (uint32_t)lh, line(h));
  if (w > 1) sp_prefilter_w_k<<<blocks(lw, SP_LINES), SP_LINES, 0, st>>>(coef, w, (uint32_t)lw, line(w));
  return fplx_check_launch("spline_prefilter");
}

int fplx_resample_spline(const double* coef, float* y, int c, int d, int h, int w, int od, int oh, int ow,
                         const double* matrix9, const double* offset3, int order, fplx_stream_t stream) {
  FPLX_REQUIRE(coef && y && matrix9 && offset3, FPLX_E_NULL, "resample_spline: null pointer");
  FPLX_REQUIRE(rs_extents_ok(c, d, h, w) && rs_extents_ok(c, od, oh, ow), FPLX_E_BADSHAPE,
               "resample_spline: bad extents [%d,%d,%d,%d] -> [%d,%d,%d,%d] (positive, fewer than 2^31 elements)", c, d, h, w,
               c, od, oh, ow);
  FPLX_REQUIRE(sp_order_row(order), FPLX_E_BADSHAPE, "resample_spline: order %d (built: %s)", order, SP_BUILT_ORDERS);
  const RsGeo g = rs_geo(c, d, h, w, od, oh, ow, matrix9, offset3);
  const int64_t total = (int64_t)c * od * oh * ow;
  const unsigned grid = (unsigned)((total + RS_THREADS - 1) / RS_THREADS);
  resample_spline3_k<<<grid, RS_THREADS, 0, (hipStream_t)stream>>>(coef, y, g);
  return fplx_check_launch("resample_spline");
}

}  // extern "C"
