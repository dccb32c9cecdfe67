// The 1x1x1 classification head of UNet3D (reference PyMIC/pymic/net/net3d/unet3d.py:131-135, 150-157: out_conv and the three
// deep-supervision heads out_conv1..3) and the trilinear interpolation that brings a coarse head's logits to full size
// (unet3d.py:152-158: torch.nn.functional.interpolate(x, size, mode='trilinear'), align_corners = False).
//
// Head: the activation a is NDHWC [N * V][lda] (fp32 or bf16; lda = 2 C where a is the left half of a concat buffer), the
// weights W[ncls][C] and the bias are fp32, the logits fp32 planar [N][ncls][V] - what the loss kernels read.  All three
// kernels stream a once with 16-byte loads along the channel axis; the arithmetic is a handful of FMAs per byte, so they are
// HBM-bound and carry no tuning.  Every sum is formed by one thread (or one fixed tree of threads) in a fixed order: no atomics.
//   fwd    one thread per voxel, channels ascending; W and the bias in LDS (every lane reads the same word: a broadcast)
//   dgrad  one thread per (voxel, 8 channels): consecutive lanes write consecutive 16-byte pieces; classes ascending;
//          accumulate = 1: da = da + sum (the level's other consumer wrote da first), in place
//   wgrad  stage 1: block b sums its voxels (a fixed function of the shape) per thread, then over the block's rows through LDS
//          in ascending row order, one partial row [ncls][C + 1] per block in the workspace (column C: the bias gradient);
//          stage 2: one thread per (class, channel) adds the partial rows in ascending block order
//
// Interpolation: planar fp32 [NC][d][h][w] -> [NC][f d][f h][f w], f in {2, 4, 8} on all three axes.  Source coordinate by
// ATen's rule (area_pixel_compute_source_index, align_corners = false): src = max((dst + 0.5) / f - 0.5, 0), i0 = (int)src,
// i1 = i0 + (i0 < in - 1), lambda1 = src - i0; the three axes are combined w, then h, then d as ATen's kernel does.
//   fwd    one thread per fine voxel (coalesced stores)
//   bwd    the exact transpose as a gather: one thread per coarse voxel sums the (at most (2 f)^3) fine voxels that touch it,
//          d, h, w ascending
#include "common.h"
#include "loss_common.h"

namespace {

constexpr int HEAD_THREADS = 256;
constexpr int HEAD_MAXC = 512;
constexpr int HEAD_MAXK = MAXC;          // loss_common.h: the loss kernels take at most this many classes

struct alignas(16) F4 { float x, y, z, w; };
struct alignas(16) U4 { uint32_t x, y, z, w; };

// 8 consecutive channels as fp32: two 16-byte loads (fp32) or one (bf16; a bf16 is the upper half of the fp32 word)
template <typename T> struct Row8;
template <> struct Row8<float> {
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const F4 a = *reinterpret_cast<const F4*>(p), b = *reinterpret_cast<const F4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  static __device__ __forceinline__ void st(float* p, const float* v) {
    *reinterpret_cast<F4*>(p) = F4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<F4*>(p + 4) = F4{v[4], v[5], v[6], v[7]};
  }
};
template <> struct Row8<bf16_t> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float* v) {
    const U4 a = *reinterpret_cast<const U4*>(p);
    const uint32_t u[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(u[i] << 16);
      v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ void st(bf16_t* p, const float* v) {
    uint32_t u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf16_t lo = (bf16_t)v[2 * i], hi = (bf16_t)v[2 * i + 1];            // round to nearest even
      u[i] = (uint32_t)__builtin_bit_cast(uint16_t, lo) | ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16);
    }
    *reinterpret_cast<U4*>(p) = U4{u[0], u[1], u[2], u[3]};
  }
};

inline int head_grid(int64_t items) {
  int64_t g = (items + HEAD_THREADS - 1) / HEAD_THREADS;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

// ------------------------------------------------------------------------------------------------ forward
template <typename T>
__global__ void __launch_bounds__(HEAD_THREADS)
head_fwd_k(const T* __restrict__ a, int64_t lda, const float* __restrict__ w, const float* __restrict__ bias,
           float* __restrict__ logits, int64_t NV, int64_t V, int C, int K) {
  __shared__ float ws[HEAD_MAXK * HEAD_MAXC];
  __shared__ float bs[HEAD_MAXK];
  for (int i = threadIdx.x; i < K * C; i += HEAD_THREADS) ws[i] = w[i];
  if (threadIdx.x < K) bs[threadIdx.x] = bias ? bias[threadIdx.x] : 0.f;
  __syncthreads();
  for (int64_t g = (int64_t)blockIdx.x * HEAD_THREADS + threadIdx.x; g < NV; g += (int64_t)gridDim.x * HEAD_THREADS) {
    float acc[HEAD_MAXK];
#pragma unroll
    for (int k = 0; k < HEAD_MAXK; ++k) acc[k] = k < K ? bs[k] : 0.f;
    const T* row = a + g * lda;
    for (int c = 0; c < C; c += 8) {
      float v[8];
      Row8<T>::ld(row + c, v);
#pragma unroll
      for (int k = 0; k < HEAD_MAXK; ++k) {
        if (k < K) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[k] = fmaf(ws[k * C + c + j], v[j], acc[k]);
        }
      }
    }
    const int64_t n = g / V, vv = g - n * V;
    float* out = logits + n * K * V + vv;
#pragma unroll
    for (int k = 0; k < HEAD_MAXK; ++k)
      if (k < K) out[(int64_t)k * V] = acc[k];
  }
}

// ------------------------------------------------------------------------------------------------ data gradient
template <typename T>
__global__ void __launch_bounds__(HEAD_THREADS)
head_dgrad_k(const float* __restrict__ dlogits, const float* __restrict__ w, T* __restrict__ da, int64_t lda, int64_t NV,
             int64_t V, int C, int K, int accumulate) {
  __shared__ float ws[HEAD_MAXK * HEAD_MAXC];
  for (int i = threadIdx.x; i < K * C; i += HEAD_THREADS) ws[i] = w[i];
  __syncthreads();
  const int nq = C >> 3;
  const int64_t items = NV * nq;
  for (int64_t i = (int64_t)blockIdx.x * HEAD_THREADS + threadIdx.x; i < items; i += (int64_t)gridDim.x * HEAD_THREADS) {
    const int64_t g = i / nq;
    const int c = (int)(i - g * nq) << 3;
    const int64_t n = g / V, vv = g - n * V;
    const float* dl = dlogits + n * K * V + vv;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; ++k) {
      const float d = dl[(int64_t)k * V];
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] = fmaf(ws[k * C + c + j], d, s[j]);
    }
    T* row = da + g * lda + c;
    if (accumulate) {
      float old[8];
      Row8<T>::ld(row, old);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] = old[j] + s[j];
    }
    Row8<T>::st(row, s);
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// threads of a block: nq = C / 8 channel pieces x rows = 256 / nq voxel rows (the remaining 256 - nq * rows threads idle)
struct WgPlan { int nq, rows, blocks; };
inline WgPlan wg_plan(int64_t NV, int C) {
  WgPlan p;
  p.nq = C >> 3;
  p.rows = HEAD_THREADS / p.nq;
  int64_t b = (NV + (int64_t)p.rows * 8 - 1) / ((int64_t)p.rows * 8);      // about 8 voxels per thread
  p.blocks = (int)(b > 512 ? 512 : (b < 1 ? 1 : b));
  return p;
}

template <typename T>
__global__ void __launch_bounds__(HEAD_THREADS)
head_wgrad_partial_k(const T* __restrict__ a, int64_t lda, const float* __restrict__ dlogits, float* __restrict__ part,
                     int64_t NV, int64_t V, int C, int K, int nq, int rows) {
  __shared__ float red[HEAD_THREADS * 8];
  __shared__ float redb[HEAD_THREADS];
  const int t = threadIdx.x;
  const int q = t % nq, r = t / nq;
  const bool live = r < rows;
  float acc[HEAD_MAXK][8];
  float accb[HEAD_MAXK];
#pragma unroll
  for (int k = 0; k < HEAD_MAXK; ++k) {
    accb[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
  }
  if (live) {
    for (int64_t g = (int64_t)blockIdx.x * rows + r; g < NV; g += (int64_t)gridDim.x * rows) {
      float v[8];
      Row8<T>::ld(a + g * lda + (q << 3), v);
      const int64_t n = g / V, vv = g - n * V;
      const float* dl = dlogits + n * K * V + vv;
#pragma unroll
      for (int k = 0; k < HEAD_MAXK; ++k) {
        if (k < K) {
          const float d = dl[(int64_t)k * V];
          accb[k] += d;
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(d, v[j], acc[k][j]);
        }
      }
    }
  }
  float* prow = part + (int64_t)blockIdx.x * K * (C + 1);
#pragma unroll
  for (int k = 0; k < HEAD_MAXK; ++k) {
    if (k < K) {                                         // (K is uniform: every thread reaches the barriers)
#pragma unroll
      for (int j = 0; j < 8; ++j) red[t * 8 + j] = acc[k][j];
      redb[t] = accb[k];
      __syncthreads();
      for (int ch = t; ch < C; ch += HEAD_THREADS) {     // channel ch: piece ch / 8, element ch % 8, rows ascending
        float s = 0.f;
        for (int rr = 0; rr < rows; ++rr) s += red[(rr * nq + (ch >> 3)) * 8 + (ch & 7)];
        prow[k * (C + 1) + ch] = s;
      }
      if (t == 0) {                                      // bias gradient: the q = 0 thread of every row saw each voxel once
        float s = 0.f;
        for (int rr = 0; rr < rows; ++rr) s += redb[rr * nq];
        prow[k * (C + 1) + C] = s;
      }
      __syncthreads();
    }
  }
}

__global__ void __launch_bounds__(HEAD_THREADS)
head_wgrad_final_k(const float* __restrict__ part, int blocks, float* __restrict__ dw, float* __restrict__ db, int C, int K) {
  const int i = blockIdx.x * HEAD_THREADS + threadIdx.x;
  if (i >= K * (C + 1)) return;
  const int k = i / (C + 1), c = i - k * (C + 1);
  float s = 0.f;
  for (int b = 0; b < blocks; ++b) s += part[(int64_t)b * K * (C + 1) + i];
  if (c < C) dw[k * C + c] = s;
  else if (db) db[k] = s;
}

// ------------------------------------------------------------------------------------------------ interpolation
struct Src { int i0, i1; float l0, l1; };

__device__ __forceinline__ Src interp_src(int o, int in, float inv_f) {
  Src s;
  float x = ((float)o + 0.5f) * inv_f - 0.5f;          // exact: inv_f is a power of two
  x = x < 0.f ? 0.f : x;
  s.i0 = (int)x;
  if (s.i0 > in - 1) s.i0 = in - 1;
  s.i1 = s.i0 + (s.i0 < in - 1 ? 1 : 0);
  s.l1 = x - (float)s.i0;
  s.l0 = 1.f - s.l1;
  return s;
}

__global__ void __launch_bounds__(HEAD_THREADS)
interp_fwd_k(const float* __restrict__ x, float* __restrict__ y, int64_t NC, int D, int H, int W, int f) {
  const int Do = D * f, Ho = H * f, Wo = W * f;
  const float inv_f = 1.f / (float)f;
  const int64_t total = NC * Do * Ho * Wo;
  for (int64_t i = (int64_t)blockIdx.x * HEAD_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * HEAD_THREADS) {
    int64_t r = i;
    const int ow = (int)(r % Wo); r /= Wo;
    const int oh = (int)(r % Ho); r /= Ho;
    const int od = (int)(r % Do);
    const int64_t nc = r / Do;
    const Src sd = interp_src(od, D, inv_f), sh = interp_src(oh, H, inv_f), sw = interp_src(ow, W, inv_f);
    const float* p = x + nc * D * H * W;
    auto at = [&](int dd, int hh, int ww) { return p[((int64_t)dd * H + hh) * W + ww]; };
    const float r00 = sw.l0 * at(sd.i0, sh.i0, sw.i0) + sw.l1 * at(sd.i0, sh.i0, sw.i1);
    const float r01 = sw.l0 * at(sd.i0, sh.i1, sw.i0) + sw.l1 * at(sd.i0, sh.i1, sw.i1);
    const float r10 = sw.l0 * at(sd.i1, sh.i0, sw.i0) + sw.l1 * at(sd.i1, sh.i0, sw.i1);
    const float r11 = sw.l0 * at(sd.i1, sh.i1, sw.i0) + sw.l1 * at(sd.i1, sh.i1, sw.i1);
    y[i] = sd.l0 * (sh.l0 * r00 + sh.l1 * r01) + sd.l1 * (sh.l0 * r10 + sh.l1 * r11);
  }
}

// weight of fine index o on coarse index i along one axis (i0 == i1 at the upper edge: both terms land on the same voxel)
__device__ __forceinline__ float interp_wt(int o, int i, int in, float inv_f) {
  const Src s = interp_src(o, in, inv_f);
  return (s.i0 == i ? s.l0 : 0.f) + (s.i1 == i ? s.l1 : 0.f);
}

__global__ void __launch_bounds__(HEAD_THREADS)
interp_bwd_k(const float* __restrict__ dy, float* __restrict__ dx, int64_t NC, int D, int H, int W, int f) {
  const int Do = D * f, Ho = H * f, Wo = W * f;
  const float inv_f = 1.f / (float)f;
  const int64_t total = NC * D * H * W;
  for (int64_t i = (int64_t)blockIdx.x * HEAD_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * HEAD_THREADS) {
    int64_t r = i;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H); r /= H;
    const int d = (int)(r % D);
    const int64_t nc = r / D;
    // fine indices whose source coordinate lies in (i - 1, i + 1): f i - f / 2 .. f i + 3 f / 2 - 1, inside the volume
    const int hf = f >> 1;
    const int d0 = max(0, f * d - hf), d1 = min(Do - 1, f * d + 3 * hf - 1);
    const int h0 = max(0, f * h - hf), h1 = min(Ho - 1, f * h + 3 * hf - 1);
    const int w0 = max(0, f * w - hf), w1 = min(Wo - 1, f * w + 3 * hf - 1);
    const float* p = dy + nc * Do * Ho * Wo;
    float acc = 0.f;
    for (int od = d0; od <= d1; ++od) {
      const float wd = interp_wt(od, d, D, inv_f);
      if (wd == 0.f) continue;
      for (int oh = h0; oh <= h1; ++oh) {
        const float wh = interp_wt(oh, h, H, inv_f);
        if (wh == 0.f) continue;
        const float wdh = wd * wh;
        const float* prow = p + ((int64_t)od * Ho + oh) * Wo;
        for (int ow = w0; ow <= w1; ++ow) acc += (wdh * interp_wt(ow, w, W, inv_f)) * prow[ow];
      }
    }
    dx[i] = acc;
  }
}

// ------------------------------------------------------------------------------------------------ host checks
int head_check(const char* what, const void* a, int64_t lda, int dt, const void* w, const void* lg, int n, int64_t v, int c,
               int ncls) {
  FPLX_REQUIRE(a && w && lg, FPLX_E_NULL, "%s: null pointer", what);
  FPLX_REQUIRE(dt == FPLX_F32 || dt == FPLX_BF16, FPLX_E_BADDTYPE, "%s: dtype %d", what, dt);
  FPLX_REQUIRE(n > 0 && v > 0 && (int64_t)n * v < ((int64_t)1 << 40), FPLX_E_BADSHAPE, "%s: n=%d voxels=%lld", what, n,
               (long long)v);
  FPLX_REQUIRE(c >= 8 && c <= HEAD_MAXC && c % 8 == 0, FPLX_E_BADSHAPE, "%s: C=%d (a multiple of 8, at most %d)", what, c,
               HEAD_MAXC);
  FPLX_REQUIRE(ncls >= 1 && ncls <= HEAD_MAXK, FPLX_E_BADSHAPE, "%s: %d classes (1..%d)", what, ncls, HEAD_MAXK);
  const int64_t elems16 = dt == FPLX_F32 ? 4 : 8;
  FPLX_REQUIRE(lda >= c && lda % elems16 == 0 && ((uintptr_t)a & 15) == 0, FPLX_E_BADSHAPE,
               "%s: lda=%lld (>= C, rows 16-byte aligned)", what, (long long)lda);
  return FPLX_OK;
}

int interp_check(const char* what, const void* x, const void* y, int64_t nc, int d, int h, int w, int f) {
  FPLX_REQUIRE(x && y, FPLX_E_NULL, "%s: null pointer", what);
  FPLX_REQUIRE(f == 2 || f == 4 || f == 8, FPLX_E_BADSHAPE, "%s: factor %d (2, 4 or 8)", what, f);
  FPLX_REQUIRE(nc > 0 && d > 0 && h > 0 && w > 0 && (int64_t)d * f < (1 << 20) && (int64_t)h * f < (1 << 20) &&
                   (int64_t)w * f < (1 << 20) && nc * d * h * w < ((int64_t)1 << 40) / ((int64_t)f * f * f),
               FPLX_E_BADSHAPE, "%s: bad shape %lld x %d x %d x %d", what, (long long)nc, d, h, w);
  return FPLX_OK;
}

}  // namespace

extern "C" {

int fplx_head_fwd(const void* a, int64_t lda, int dt, const float* w, const float* bias, float* logits, int n, int64_t v, int c,
                  int ncls, fplx_stream_t stream) {
  const int rc = head_check("head_fwd", a, lda, dt, w, logits, n, v, c, ncls);
  if (rc != FPLX_OK) return rc;
  const int64_t NV = (int64_t)n * v;
  hipStream_t st = (hipStream_t)stream;
  if (dt == FPLX_F32)
    head_fwd_k<float><<<head_grid(NV), HEAD_THREADS, 0, st>>>((const float*)a, lda, w, bias, logits, NV, v, c, ncls);
  else
    head_fwd_k<bf16_t><<<head_grid(NV), HEAD_THREADS, 0, st>>>((const bf16_t*)a, lda, w, bias, logits, NV, v, c, ncls);
  return fplx_check_launch("head_fwd");
}

int fplx_head_dgrad(const float* dlogits, const float* w, void* da, int64_t lda, int dt, int n, int64_t v, int c, int ncls,
                    int accumulate, fplx_stream_t stream) {
  const int rc = head_check("head_dgrad", da, lda, dt, w, dlogits, n, v, c, ncls);
  if (rc != FPLX_OK) return rc;
  const int64_t NV = (int64_t)n * v;
  hipStream_t st = (hipStream_t)stream;
  const int grid = head_grid(NV * (c >> 3));
  if (dt == FPLX_F32)
    head_dgrad_k<float><<<grid, HEAD_THREADS, 0, st>>>(dlogits, w, (float*)da, lda, NV, v, c, ncls, accumulate ? 1 : 0);
  else
    head_dgrad_k<bf16_t><<<grid, HEAD_THREADS, 0, st>>>(dlogits, w, (bf16_t*)da, lda, NV, v, c, ncls, accumulate ? 1 : 0);
  return fplx_check_launch("head_dgrad");
}

size_t fplx_head_wgrad_ws_bytes(int n, int64_t v, int c, int ncls) {
  if (n <= 0 || v <= 0 || c < 8 || c > HEAD_MAXC || c % 8 || ncls < 1 || ncls > HEAD_MAXK) return 0;
  const WgPlan p = wg_plan((int64_t)n * v, c);
  return (size_t)p.blocks * ncls * (c + 1) * sizeof(float);
}

int fplx_head_wgrad(const void* a, int64_t lda, int dt, const float* dlogits, float* dw, float* db, int n, int64_t v, int c,
                    int ncls, void* ws, size_t ws_bytes, fplx_stream_t stream) {
  const int rc = head_check("head_wgrad", a, lda, dt, dw, dlogits, n, v, c, ncls);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(ws, FPLX_E_NULL, "head_wgrad: null workspace");
  const size_t need = fplx_head_wgrad_ws_bytes(n, v, c, ncls);
  FPLX_REQUIRE(ws_bytes >= need, FPLX_E_WORKSPACE, "head_wgrad: workspace %zu < %zu bytes", ws_bytes, need);
  const int64_t NV = (int64_t)n * v;
  const WgPlan p = wg_plan(NV, c);
  hipStream_t st = (hipStream_t)stream;
  if (dt == FPLX_F32)
    head_wgrad_partial_k<float><<<p.blocks, HEAD_THREADS, 0, st>>>((const float*)a, lda, dlogits, (float*)ws, NV, v, c, ncls,
                                                                    p.nq, p.rows);
  else
    head_wgrad_partial_k<bf16_t><<<p.blocks, HEAD_THREADS, 0, st>>>((const bf16_t*)a, lda, dlogits, (float*)ws, NV, v, c, ncls,
                                                                     p.nq, p.rows);
  const int items = ncls * (c + 1);
  head_wgrad_final_k<<<(items + HEAD_THREADS - 1) / HEAD_THREADS, HEAD_THREADS, 0, st>>>((const float*)ws, p.blocks, dw, db, c,
                                                                                         ncls);
  return fplx_check_launch("head_wgrad");
}

int fplx_interp_fwd(const float* x, float* y, int64_t nc, int d, int h, int w, int f, fplx_stream_t stream) {
  const int rc = interp_check("interp_fwd", x, y, nc, d, h, w, f);
  if (rc != FPLX_OK) return rc;
  const int64_t total = nc * d * h * w * f * f * f;
  interp_fwd_k<<<head_grid(total), HEAD_THREADS, 0, (hipStream_t)stream>>>(x, y, nc, d, h, w, f);
  return fplx_check_launch("interp_fwd");
}

int fplx_interp_bwd(const float* dy, float* dx, int64_t nc, int d, int h, int w, int f, fplx_stream_t stream) {
  const int rc = interp_check("interp_bwd", dy, dx, nc, d, h, w, f);
  if (rc != FPLX_OK) return rc;
  const int64_t total = nc * d * h * w;
  interp_bwd_k<<<head_grid(total), HEAD_THREADS, 0, (hipStream_t)stream>>>(dy, dx, nc, d, h, w, f);
  return fplx_check_launch("interp_bwd");
}

}  // extern "C"
