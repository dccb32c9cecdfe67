// Exact Euclidean distance transform of n uint8 masks [n][d][h][w] (nonzero = foreground; a 2D mask is ndim = 2, d = 1):
// what scipy.ndimage.distance_transform_edt computes, which the reference's get_euclidean_distance calls twice
// (PyMIC/pymic/util/image_process.py:165-192).  The float64 SQUARED distance is a separable minimum:
//
//   g0 = 0 on background voxels, +inf on foreground voxels
//   for axis 0, then 1, then 2:   g[j] = min_i ( g[i] + ((j - i) * s_axis)^2 )
//
// product first, then the square, then the sum, every one rounded to float64 and none contracted.  Rounding is monotone, so
// the three one-dimensional minima commute with it and the result is the minimum over the background voxels of
// ((dz sz)^2 + (dy sy)^2) + (dx sx)^2 - scipy's own association (dt *= sampling; dt *= dt; add.reduce(axis 0)), bit for
// bit (tests/edtoracle.py restates it).  A minimum has no order of evaluation: two runs give the same bits.
//
// One kernel serves the three passes (edt_pass_k).  A block owns EDT_LINES whole lines and stages them in LDS as
// tile[i * EDT_STRIDE + line] (dynamic LDS: n * EDT_STRIDE doubles, so the longest line FPLX_EDT_MAX_EXTENT = 620 takes 159.8
// of the CU's 160 KiB and short lines leave room for several blocks per CU); after the barrier it writes the same lines back,
// so the pass runs in place.
//  - D and H passes (ALONG = false): line l = (outer, in), elements at outer * n * inner + in + i * inner.  Neighbouring
//    threads take neighbouring lines, which are neighbours in memory (along W): loads and stores are rows of EDT_LINES
//    consecutive elements.
//  - W pass (ALONG = true, inner = 1): the lines lie along the fastest axis, so neighbouring threads take neighbouring
//    elements of a line; the block's lines are one contiguous range of memory.
//    The row stride EDT_STRIDE = 33 doubles is odd: lanes that differ in the line at one i, and lanes that differ in i on
//    one line, both fall on distinct 8-byte bank slots of ds_read_b64 (32 lanes served together) and ds_write_b64 (16).
//  - output j: the plain windowed search.  best = g[j]; for k = 1, 2, ...: stop as soon as fl((k s)^2) >= best, else try
//    g[j - k] + fl((k s)^2) and g[j + k] + fl((k s)^2).  The stop is exact: g >= 0 and rounding is monotone, so no farther
//    candidate can be smaller.  k < n bounds the loop.  A line without a finite entry stays +inf until a later pass.
//  - phantom: scipy's result for a mask WITHOUT any background voxel is the distance to one background voxel at index
//    (-1, 0, 0) (2D: (-1, 0)).  The caller establishes that a mask has no zero (phantom[mask] != 0); the axis-0 pass then
//    adds the candidate ((j + 1) s_0)^2 to the line (y = 0, x = 0) of that mask.
//  - feature transform (optional): the D and H passes store their argmin i per voxel (workspace), the W pass follows the
//    chain ix = argmin, iy = IY[z][y][ix], iz = IZ[z][iy][ix] and writes the int32 coordinates.  Ties go to the nearest i,
//    then to the smaller one; scipy may choose another voxel at the same distance.
// No atomics, no waiting between blocks, no loop without a bound.
//
// fplx_edt_finish: sqrt(sq_a), or sqrt(sq_b) - sqrt(sq_a), the signed map of get_euclidean_distance.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int EDT_LINES = 32;                      // lines per block
constexpr int EDT_STRIDE = EDT_LINES + 1;          // LDS row stride in doubles: odd -> conflict-free both ways
constexpr int EDT_LDS_BYTES = 160 * 1024;          // the LDS of a CU; one block may take all of it
constexpr int EDT_MAX_N = EDT_LDS_BYTES / (EDT_STRIDE * (int)sizeof(double));
static_assert(EDT_MAX_N == FPLX_EDT_MAX_EXTENT, "include/fplx.h states the limit the tile gives");
constexpr int EDT_MAX_THREADS = 1024;
constexpr int64_t EDT_MAX_ELEMS = (int64_t)1 << 31;      // 32-bit line numbers inside the kernel

struct EdtPass {
  int n;                   // line length
  uint32_t inner;          // distance between consecutive elements of a line = lines that are consecutive in memory
  uint32_t nlines;
  double s;                // sampling of this axis
  uint32_t ph_lines;       // axis-0 pass: lines per mask (the phantom seeds line 0 of a mask); else 0
  int nch;                 // W pass with indices: 2 or 3 coordinate channels; else 0
  uint32_t D, H;           // W pass with indices: extents (line = (mask * D + z) * H + y)
};

__device__ __forceinline__ double edt_load(const uint8_t* p, size_t a) { return p[a] ? (double)INFINITY : 0.0; }
__device__ __forceinline__ double edt_load(const double* p, size_t a) { return p[a]; }

// src == dst for TIN = double (in place: no __restrict__).  arg: this pass's argmin per voxel (D, H passes), or null.
// iz, iy, idx: W pass with indices, else null.
template <typename TIN, bool ALONG>
__global__ void __launch_bounds__(EDT_MAX_THREADS)
edt_pass_k(const TIN* src, double* dst, int* arg, const uint8_t* __restrict__ phantom, const int* __restrict__ iz,
           const int* __restrict__ iy, int* __restrict__ idx, const EdtPass p) {
  extern __shared__ double edt_tile[];
  const int n = p.n, cnt = EDT_LINES * n, T = (int)blockDim.x;
  const uint32_t line0 = blockIdx.x * EDT_LINES;
  for (int e = (int)threadIdx.x; e < cnt; e += T) {
    const int ln = ALONG ? e / n : e % EDT_LINES, i = ALONG ? e - ln * n : e / EDT_LINES;
    const uint32_t l = line0 + ln;
    double v = (double)INFINITY;
    if (l < p.nlines) v = edt_load(src, (size_t)(l / p.inner) * n * p.inner + (l % p.inner) + (size_t)i * p.inner);
    edt_tile[i * EDT_STRIDE + ln] = v;
  }
  __syncthreads();
  const double s = p.s;
  for (int e = (int)threadIdx.x; e < cnt; e += T) {
    const int ln = ALONG ? e / n : e % EDT_LINES, j = ALONG ? e - ln * n : e / EDT_LINES;
    const uint32_t l = line0 + ln;
    if (l >= p.nlines) continue;
    const double* g = edt_tile + ln;
    double best = g[j * EDT_STRIDE];
    int at = j;
    for (int k = 1; k < n; ++k) {
      const double dk = (double)k * s;
      const double d2 = dk * dk;
      if (d2 >= best) break;
      if (j - k >= 0) {
        const double c = g[(j - k) * EDT_STRIDE] + d2;
        if (c < best) { best = c; at = j - k; }
      }
      if (j + k < n) {
        const double c = g[(j + k) * EDT_STRIDE] + d2;
        if (c < best) { best = c; at = j + k; }
      }
    }
    if (p.ph_lines && phantom && l % p.ph_lines == 0 && phantom[l / p.ph_lines]) {
      const double dk = (double)(j + 1) * s;
      const double c = dk * dk;
      if (c < best) { best = c; at = -1; }
    }
    const size_t o = (size_t)(l / p.inner) * n * p.inner + (l % p.inner) + (size_t)j * p.inner;
    dst[o] = best;
    if (arg) arg[o] = at;
    if (p.nch) {                                   // ALONG: o = l * n + j, l = (mask * D + z) * H + y
      const uint32_t m = l / (p.D * p.H), zy = l % (p.D * p.H), z = zy / p.H;
      const size_t vox = (size_t)p.D * p.H * n;
      const int y1 = iy[(size_t)l * n + at];
      const int z1 = iz[(((size_t)m * p.D + z) * p.H + y1) * n + at];
      int* q = idx + (size_t)m * p.nch * vox + (size_t)zy * n + j;
      q[0] = z1;
      if (p.nch == 3) q[vox] = y1;
      q[(size_t)(p.nch - 1) * vox] = at;
    }
  }
}

__global__ void __launch_bounds__(256)
edt_finish_k(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const double ra = sqrt(a[i]);
  out[i] = b ? sqrt(b[i]) - ra : ra;
}

// threads per block: EDT_LINES lines x n outputs are dealt to them; long lines mean few blocks per CU, so each gets more waves
inline int edt_threads(int n) { return n <= 128 ? 256 : (n <= 256 ? 512 : EDT_MAX_THREADS); }

template <typename TIN, bool ALONG>
inline void edt_launch(const TIN* src, double* dst, int* arg, const uint8_t* phantom, const int* iz, const int* iy, int* idx,
                       const EdtPass& p, hipStream_t st) {
  const unsigned grid = (p.nlines + EDT_LINES - 1) / EDT_LINES;
  fplx_launch(edt_pass_k<TIN, ALONG>, dim3(grid), dim3(edt_threads(p.n)), (size_t)p.n * EDT_STRIDE * sizeof(double), st, src, dst,
              arg, phantom, iz, iy, idx, p);
}

// the lines of the pass along `axis` of n volumes [D][H][W]
inline EdtPass edt_geo(int axis, int n, int D, int H, int W, double s) {
  const uint32_t all = (uint32_t)n * D * H * W;
  const int len = axis == 0 ? D : (axis == 1 ? H : W);
  const uint32_t inner = axis == 0 ? (uint32_t)(H * W) : (axis == 1 ? (uint32_t)W : 1u);
  return EdtPass{len, inner, all / (uint32_t)len, s, 0u, 0, 0u, 0u};
}

}  // namespace

extern "C" {

int fplx_edt_squared(const uint8_t* mask, int n, int d, int h, int w, int ndim, const double* sampling3, const uint8_t* phantom,
                     double* sq, int* idx, int* ws, size_t ws_bytes, fplx_stream_t stream) {
  FPLX_REQUIRE(mask && sampling3 && sq, FPLX_E_NULL, "edt_squared: null pointer");
  FPLX_REQUIRE(ndim == 3 || (ndim == 2 && d == 1), FPLX_E_BADSHAPE, "edt_squared: ndim = %d, d = %d (ndim 3, or ndim 2 with d = 1)",
               ndim, d);
  FPLX_REQUIRE(n > 0 && d > 0 && h > 0 && w > 0, FPLX_E_BADSHAPE, "edt_squared: bad extents [%d,%d,%d,%d] (positive)", n, d, h, w);
  FPLX_REQUIRE(d <= FPLX_EDT_MAX_EXTENT && h <= FPLX_EDT_MAX_EXTENT && w <= FPLX_EDT_MAX_EXTENT, FPLX_E_BADSHAPE,
               "edt_squared: extents [%d,%d,%d] exceed the limit of %d per axis (a whole line is staged in the 160 KiB of LDS)", d,
               h, w, FPLX_EDT_MAX_EXTENT);
  const int64_t vox = (int64_t)d * h * w;
  FPLX_REQUIRE(vox * n < EDT_MAX_ELEMS, FPLX_E_BADSHAPE, "edt_squared: %lld elements (fewer than 2^31)", (long long)(vox * n));
  for (int a = 0; a < 3; ++a)
    FPLX_REQUIRE(sampling3[a] > 0.0 && sampling3[a] < (double)INFINITY, FPLX_E_BADSHAPE,
                 "edt_squared: sampling[%d] = %g (positive and finite)", a, sampling3[a]);
  if (idx) {
    FPLX_REQUIRE(ws, FPLX_E_NULL, "edt_squared: the feature transform needs a workspace");
    FPLX_REQUIRE(ws_bytes >= FPLX_EDT_WS_BYTES(n, vox), FPLX_E_WORKSPACE, "edt_squared: workspace of %zu bytes, need %zu", ws_bytes,
                 FPLX_EDT_WS_BYTES(n, vox));
  }
  hipStream_t st = (hipStream_t)stream;
  // a 2D mask [h][w] runs as the volume [h][1][w]: axis 0 (with the phantom at -1) is the D pass, the H pass copies
  const int D = ndim == 2 ? h : d, H = ndim == 2 ? 1 : h, W = w;
  const double s0 = sampling3[ndim == 2 ? 1 : 0], s1 = ndim == 2 ? 1.0 : sampling3[1], s2 = sampling3[2];
  int* izl = idx ? ws : nullptr;
  int* iyl = idx ? ws + (size_t)n * vox : nullptr;
  EdtPass pd = edt_geo(0, n, D, H, W, s0), ph = edt_geo(1, n, D, H, W, s1), pw = edt_geo(2, n, D, H, W, s2);
  if (phantom) pd.ph_lines = (uint32_t)(H * W);
  if (idx) { pw.nch = ndim; pw.D = (uint32_t)D; pw.H = (uint32_t)H; }
  edt_launch<uint8_t, false>(mask, sq, izl, phantom, nullptr, nullptr, nullptr, pd, st);
  edt_launch<double, false>(sq, sq, iyl, nullptr, nullptr, nullptr, nullptr, ph, st);
  edt_launch<double, true>(sq, sq, nullptr, nullptr, izl, iyl, idx, pw, st);
  return fplx_check_launch("edt_squared");
}

int fplx_edt_pass(double* g, int n, int d, int h, int w, int axis, double sampling, fplx_stream_t stream) {
  FPLX_REQUIRE(g, FPLX_E_NULL, "edt_pass: null pointer");
  FPLX_REQUIRE(n > 0 && d > 0 && h > 0 && w > 0, FPLX_E_BADSHAPE, "edt_pass: bad extents [%d,%d,%d,%d] (positive)", n, d, h, w);
  FPLX_REQUIRE(axis >= 0 && axis <= 2, FPLX_E_BADSHAPE, "edt_pass: axis %d (0, 1 or 2)", axis);
  const int len = axis == 0 ? d : (axis == 1 ? h : w);
  FPLX_REQUIRE(len <= FPLX_EDT_MAX_EXTENT, FPLX_E_BADSHAPE,
               "edt_pass: a line of %d elements exceeds the limit of %d (a whole line is staged in the 160 KiB of LDS)", len,
               FPLX_EDT_MAX_EXTENT);
  int64_t total = n;
  for (int e : {d, h, w}) {
    total *= e;
    FPLX_REQUIRE(total < EDT_MAX_ELEMS, FPLX_E_BADSHAPE, "edt_pass: 2^31 elements or more");
  }
  FPLX_REQUIRE(sampling > 0.0 && sampling < (double)INFINITY, FPLX_E_BADSHAPE, "edt_pass: sampling = %g (positive and finite)",
               sampling);
  const EdtPass p = edt_geo(axis, n, d, h, w, sampling);
  hipStream_t st = (hipStream_t)stream;
  if (axis == 2) edt_launch<double, true>(g, g, nullptr, nullptr, nullptr, nullptr, nullptr, p, st);
  else edt_launch<double, false>(g, g, nullptr, nullptr, nullptr, nullptr, nullptr, p, st);
  return fplx_check_launch("edt_pass");
}

int fplx_edt_finish(const double* sq_a, const double* sq_b, double* out, int64_t count, fplx_stream_t stream) {
  FPLX_REQUIRE(sq_a && out, FPLX_E_NULL, "edt_finish: null pointer");
  FPLX_REQUIRE(count > 0 && count < EDT_MAX_ELEMS, FPLX_E_BADSHAPE, "edt_finish: %lld elements (1 .. 2^31 - 1)", (long long)count);
  edt_finish_k<<<(unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream>>>(sq_a, sq_b, out, count);
  return fplx_check_launch("edt_finish");
}

}  // extern "C"
