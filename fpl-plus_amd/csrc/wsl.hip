// Weakly-supervised regularisers of the reference's third entry point (PyMIC/pymic/net_run_wsl/): GatedCRFLoss
// (loss/seg/gatedcrf.py), TotalVariationLoss (loss/seg/ssl.py:46-86) and MumfordShahLoss (loss/seg/mumford_shah.py), forward and
// backward.  Layouts and formulas: include/fplx.h, "weakly-supervised learning".  The kernels index [N][C][D][H][W] directly - a
// slice is the (n, d) plane - where the reference transposes and copies to [N D][C][H][W] and, for the CRF, unfolds every tensor to
// (2 r + 1)^2 copies of itself.  Reductions as in ssl.hip: a block's fp32 partial, the partials summed in double in a fixed order
// by one wave (no floating-point atomics: two runs give the same bits; TV's count tensor takes integer atomics, which commute).
// Compiled with -ffp-contract=off (Makefile): p' = 0.999 p + 5e-4 must round as torch's two fp32 operations do - TV compares
// these values for equality of minima - and no sum may depend on what the compiler fuses; the fused multiply-adds that are
// meant are written as fmaf.
#include "loss_common.h"

namespace {

constexpr int MAXCI = 4;
constexpr int CRF_T = 16;                     // a block's tile of a slice: 16 x 16 pixels, one per lane
constexpr int CRF_MAXR = 8, CRF_MAXK = 4;

struct CrfDesc {
  float w[CRF_MAXK], ixy[CRF_MAXK], irgb[CRF_MAXK];      // weight, 1 / sigma_xy^2, 1 / sigma_rgb^2 (0: the modality is absent)
  int nk;
};

// the block's sum of acc -> lane 0's return value (valid for threadIdx.x == 0 only)
__device__ __forceinline__ float block_sum(float acc) {
  __shared__ float red[LT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();                                        // red may still be read from an earlier call
  const float t = wave_sum(acc);
  if (lane == 0) red[wv] = t;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0)
    for (int i = 0; i < LT / 64; ++i) s += red[i];
  return s;
}

template <int C>
__device__ __forceinline__ void load_probs(const float* __restrict__ base, int64_t V, int64_t v, bool do_softmax, float (&p)[MAXC]) {
  float l[MAXC];
#pragma unroll
  for (int c = 0; c < C; ++c) l[c] = base[(int64_t)c * V + v];
  softmax_argmax<C>(l, p, do_softmax);
}

// dlogits_c = gs p_c (e_c - sum_j p_j e_j), the dot product as ssl.hip forms it; softmax = 0: gs e_c
template <int C>
__device__ __forceinline__ void store_jacobian(const float (&p)[MAXC], const float (&e)[MAXC], float gs, bool do_softmax,
                                               float* __restrict__ dg, int64_t V, int64_t v) {
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) dot = fmaf(e[c], p[c], dot);
#pragma unroll
  for (int c = 0; c < C; ++c) dg[(int64_t)c * V + v] = gs * (do_softmax ? p[c] * (e[c] - dot) : e[c]);
}

// one wave: columns 0 and (K == 2) 1 of the partial rows in double, lanes stride over them, then
// out = {s0, s1, (s0 + lambda s1) / numel, numel}
__global__ void wsl_finish_k(const float* __restrict__ part, int K, int64_t rows, double numel, double lambda,
                             double* __restrict__ out) {
  const int lane = threadIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t r = lane; r < rows; r += 64) {
    s0 += (double)part[r * K];
    if (K > 1) s1 += (double)part[r * K + 1];
  }
  s0 = wave_sum_d(s0);
  s1 = wave_sum_d(s1);
  if (lane == 0) { out[0] = s0; out[1] = s1; out[2] = (s0 + lambda * s1) / numel; out[3] = numel; }
}

// ---------------------------------------------------------------- GatedCRF
// LDS: the tile plus its halo of r as probabilities [C][NP] and intensities [Ci][NP] (zero outside the slice: the unfold's
// padding), then the xy factor of every window offset per descriptor, weight exp(-1/2 (dy^2 + dx^2) / sigma_xy^2) [nk][NT]: the
// one transcendental left per pair is the rgb exponential.  block b = (slice, tile); part[b] = the tile's share of out0.
template <int C>
__global__ void __launch_bounds__(LT)
wsl_crf_fwd_k(const float* __restrict__ logits, const float* __restrict__ image, int Ci, int D, int H, int W, int tx, int ty, int r,
              CrfDesc ds, int do_softmax, float* __restrict__ kp, float* __restrict__ part) {
  extern __shared__ float lds[];
  const int E = CRF_T + 2 * r, NP = E * E, dia = 2 * r + 1, NT = dia * dia;
  float* sp = lds;
  float* si = sp + C * NP;
  float* tab = si + Ci * NP;
  const int tiles = tx * ty;
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const int64_t s = blockIdx.x / (unsigned)tiles;
  const int d = (int)(s % D), n = (int)(s / D);
  const int h0 = (tile / tx) * CRF_T, w0 = (tile % tx) * CRF_T;
  const int64_t HW = (int64_t)H * W, V = HW * D;
  const float* lg = logits + (int64_t)n * C * V + (int64_t)d * HW;
  const float* im = image + (int64_t)n * Ci * V + (int64_t)d * HW;
  for (int i = threadIdx.x; i < NP; i += LT) {
    const int hh = h0 - r + i / E, ww = w0 - r + i % E;
    const bool in = hh >= 0 && hh < H && ww >= 0 && ww < W;
    float p[MAXC];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.f;
    const int64_t o = (int64_t)hh * W + ww;
    if (in) load_probs<C>(lg, V, o, do_softmax != 0, p);
#pragma unroll
    for (int c = 0; c < C; ++c) sp[c * NP + i] = p[c];
    for (int ch = 0; ch < Ci; ++ch) si[ch * NP + i] = in ? im[(int64_t)ch * V + o] : 0.f;
  }
  for (int i = threadIdx.x; i < ds.nk * NT; i += LT) {
    const int k = i / NT, j = i % NT;
    const int dy = j / dia - r, dx = j % dia - r;
    tab[i] = ds.w[k] * expf(-0.5f * ((float)(dy * dy + dx * dx) * ds.ixy[k]));
  }
  __syncthreads();
  const int ly = threadIdx.x / CRF_T, lx = threadIdx.x % CRF_T;
  const int h = h0 + ly, w = w0 + lx;
  float acc = 0.f;
  if (h < H && w < W) {
    const int ci = (ly + r) * E + lx + r;
    float pi[MAXC], kpc[MAXC], ii[MAXCI];
#pragma unroll
    for (int c = 0; c < C; ++c) { pi[c] = sp[c * NP + ci]; kpc[c] = 0.f; }
    float i2 = 0.f;
#pragma unroll
    for (int ch = 0; ch < MAXCI; ++ch) {
      ii[ch] = ch < Ci ? si[ch * NP + ci] : 0.f;
      i2 += ii[ch] * ii[ch];
    }
    // a neighbour outside the slice: its features are the padding's zeros, so the distance is the pixel's own (x, y) and I
    const float xy2 = (float)h * (float)h + (float)w * (float)w;
    float koob = 0.f;
    for (int k = 0; k < ds.nk; ++k) koob += ds.w[k] * expf(-0.5f * (xy2 * ds.ixy[k] + i2 * ds.irgb[k]));
    for (int dy = -r; dy <= r; ++dy) {
      const bool row_in = h + dy >= 0 && h + dy < H;
      for (int dx = -r; dx <= r; ++dx) {
        if (dy == 0 && dx == 0) continue;
        if (!(row_in && w + dx >= 0 && w + dx < W)) { acc += koob; continue; }
        const int cj = ci + dy * E + dx, tj = (dy + r) * dia + dx + r;
        float rgb2 = 0.f;
#pragma unroll
        for (int ch = 0; ch < MAXCI; ++ch)
          if (ch < Ci) { const float t = ii[ch] - si[ch * NP + cj]; rgb2 += t * t; }
        float kk = 0.f;
        for (int k = 0; k < ds.nk; ++k) {
          const float t = tab[k * NT + tj];
          kk += ds.irgb[k] != 0.f ? t * expf(-0.5f * (rgb2 * ds.irgb[k])) : t;
        }
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float pj = sp[c * NP + cj];
          dot += pi[c] * pj;
          kpc[c] += kk * pj;
        }
        acc += kk * (1.0f - dot);
      }
    }
    float* kg = kp + (int64_t)n * C * V + (int64_t)d * HW + (int64_t)h * W + w;
#pragma unroll
    for (int c = 0; c < C; ++c) kg[(int64_t)c * V] = kpc[c];
  }
  const float t = block_sum(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// e_c = coef kp_c, coef = -2 / (N D H W)
template <int C>
__global__ void __launch_bounds__(LT)
wsl_crf_bwd_k(const float* __restrict__ logits, const float* __restrict__ kp, const float* __restrict__ gscale, float coef, int64_t V,
              int do_softmax, float* __restrict__ dlogits) {
  const int64_t off = (int64_t)blockIdx.y * C * V;
  const float gs = *gscale;
  for (int64_t v = (int64_t)blockIdx.x * LT + threadIdx.x; v < V; v += (int64_t)gridDim.x * LT) {
    float p[MAXC], e[MAXC];
    load_probs<C>(logits + off, V, v, do_softmax != 0, p);
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = coef * kp[off + (int64_t)c * V + v];
    store_jacobian<C>(p, e, gs, do_softmax != 0, dlogits + off, V, v);
  }
}

// ---------------------------------------------------------------- TotalVariation
template <int C>
__global__ void __launch_bounds__(LT)
wsl_tv_prob_k(const float* __restrict__ logits, int64_t V, int do_softmax, float* __restrict__ pp) {
  const int64_t off = (int64_t)blockIdx.y * C * V;
  for (int64_t v = (int64_t)blockIdx.x * LT + threadIdx.x; v < V; v += (int64_t)gridDim.x * LT) {
    float p[MAXC];
    load_probs<C>(logits + off, V, v, do_softmax != 0, p);
#pragma unroll
    for (int c = 0; c < C; ++c) pp[off + (int64_t)c * V + v] = p[c] * 0.999f + 5e-4f;
  }
}

// the extreme value of the in-bounds 3x3x3 window of row[] around voxel v and its offset: the first one in (d, h, w) scan order
template <bool MAX>
__device__ __forceinline__ int window_extreme(const float* __restrict__ row, int v, int D, int H, int W, float* val) {
  const int HW = H * W;
  const int d = v / HW, h = (v - d * HW) / W, w = v - d * HW - h * W;
  float best = 0.f;
  int bi = -1;
  for (int dd = d > 0 ? d - 1 : 0; dd <= (d + 1 < D ? d + 1 : D - 1); ++dd)
    for (int hh = h > 0 ? h - 1 : 0; hh <= (h + 1 < H ? h + 1 : H - 1); ++hh)
      for (int ww = w > 0 ? w - 1 : 0; ww <= (w + 1 < W ? w + 1 : W - 1); ++ww) {
        const int u = (dd * H + hh) * W + ww;
        const float x = row[u];
        if (bi < 0 || (MAX ? x > best : x < best)) { best = x; bi = u; }
      }
  *val = best;
  return bi;
}

// blockIdx.y: the (n, c) row
__global__ void __launch_bounds__(LT)
wsl_tv_erode_k(const float* __restrict__ pp, int D, int H, int W, float* __restrict__ er, int32_t* __restrict__ amin) {
  const int V = D * H * W;
  const int64_t off = (int64_t)blockIdx.y * V;
  for (int64_t v = (int64_t)blockIdx.x * LT + threadIdx.x; v < V; v += (int64_t)gridDim.x * LT) {
    float x;
    const int u = window_extreme<false>(pp + off, (int)v, D, H, W, &x);
    er[off + v] = x;
    amin[off + v] = u;
  }
}

// part[row][blockIdx.x]: the block's sum of contour
__global__ void __launch_bounds__(LT)
wsl_tv_dilate_k(const float* __restrict__ er, const int32_t* __restrict__ amin, int D, int H, int W, int32_t* __restrict__ count,
                float* __restrict__ part) {
  const int V = D * H * W;
  const int64_t off = (int64_t)blockIdx.y * V;
  float acc = 0.f;
  for (int64_t v = (int64_t)blockIdx.x * LT + threadIdx.x; v < V; v += (int64_t)gridDim.x * LT) {
    float o;
    const int u = window_extreme<true>(er + off, (int)v, D, H, W, &o);
    const float ct = o - er[off + v];
    if (ct > 0.f) {                                       // relu and its derivative: nothing at 0
      acc += ct;
      atomicAdd(count + off + amin[off + u], 1);
      atomicAdd(count + off + amin[off + v], -1);
    }
  }
  const float t = block_sum(acc);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// e_c = coef count_c, coef = 0.999 / (N C D H W)
template <int C>
__global__ void __launch_bounds__(LT)
wsl_tv_bwd_k(const float* __restrict__ logits, const int32_t* __restrict__ count, const float* __restrict__ gscale, float coef,
             int64_t V, int do_softmax, float* __restrict__ dlogits) {
  const int64_t off = (int64_t)blockIdx.y * C * V;
  const float gs = *gscale;
  for (int64_t v = (int64_t)blockIdx.x * LT + threadIdx.x; v < V; v += (int64_t)gridDim.x * LT) {
    float p[MAXC], e[MAXC];
    load_probs<C>(logits + off, V, v, do_softmax != 0, p);
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = coef * (float)count[off + (int64_t)c * V + v];
    store_jacobian<C>(p, e, gs, do_softmax != 0, dlogits + off, V, v);
  }
}

// ---------------------------------------------------------------- Mumford-Shah
// blockIdx.y: the slice s = n D + d; blockIdx.x: a chunk of its pixels.  part[s][chunk][C (1 + Ci)]: sum p_c, then sum I_ch p_c
template <int C>
__global__ void __launch_bounds__(LT)
wsl_ms_moments_k(const float* __restrict__ logits, const float* __restrict__ image, int Ci, int D, int HW, int do_softmax,
                 float* __restrict__ part) {
  const int s = blockIdx.y, n = s / D, d = s % D;
  const int64_t V = (int64_t)HW * D;
  const float* lg = logits + (int64_t)n * C * V + (int64_t)d * HW;
  const float* im = image + (int64_t)n * Ci * V + (int64_t)d * HW;
  float s0[MAXC], s1[MAXCI][MAXC];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    s0[c] = 0.f;
#pragma unroll
    for (int ch = 0; ch < MAXCI; ++ch) s1[ch][c] = 0.f;
  }
  for (int i = blockIdx.x * LT + threadIdx.x; i < HW; i += gridDim.x * LT) {
    float p[MAXC];
    load_probs<C>(lg, V, i, do_softmax != 0, p);
#pragma unroll
    for (int c = 0; c < C; ++c) s0[c] += p[c];
#pragma unroll
    for (int ch = 0; ch < MAXCI; ++ch)
      if (ch < Ci) {
        const float x = im[(int64_t)ch * V + i];
#pragma unroll
        for (int c = 0; c < C; ++c) s1[ch][c] += x * p[c];
      }
  }
  const int K = C * (1 + Ci);
  float* row = part + ((int64_t)s * gridDim.x + blockIdx.x) * K;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float t = block_sum(s0[c]);
    if (threadIdx.x == 0) row[c] = t;
  }
#pragma unroll
  for (int ch = 0; ch < MAXCI; ++ch)
    if (ch < Ci) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float t = block_sum(s1[ch][c]);
        if (threadIdx.x == 0) row[C + ch * C + c] = t;
      }
    }
}

// cen[s][ch][c] = S1 / S0, the chunks added in double in their order
__global__ void __launch_bounds__(LT)
wsl_ms_centroid_k(const float* __restrict__ part, int slices, int chunks, int C, int Ci, float* __restrict__ cen) {
  const int K = C * (1 + Ci);
  const int64_t total = (int64_t)slices * Ci * C;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < total; i += (int64_t)gridDim.x * LT) {
    const int c = (int)(i % C), ch = (int)((i / C) % Ci);
    const int64_t s = i / ((int64_t)C * Ci);
    double a = 0.0, b = 0.0;
    for (int j = 0; j < chunks; ++j) {
      const float* row = part + (s * chunks + j) * K;
      a += (double)row[c];
      b += (double)row[C + ch * C + c];
    }
    cen[i] = (float)(b / a);
  }
}

template <int C>
__device__ __forceinline__ float ms_edge(const float (&a)[MAXC], const float (&b)[MAXC], int penalty) {
  float t = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float dlt = fabsf(a[c] - b[c]);
    t += penalty == 2 ? dlt * dlt : dlt;
  }
  return t;
}

// part[s][chunk][2]: sum (I_ch - cen)^2 p_c; sum over the forward differences inside the slice
template <int C>
__global__ void __launch_bounds__(LT)
wsl_ms_loss_k(const float* __restrict__ logits, const float* __restrict__ image, const float* __restrict__ cen, int Ci, int D, int H,
              int W, int penalty, int do_softmax, float* __restrict__ part) {
  const int s = blockIdx.y, n = s / D, d = s % D, HW = H * W;
  const int64_t V = (int64_t)HW * D;
  const float* lg = logits + (int64_t)n * C * V + (int64_t)d * HW;
  const float* im = image + (int64_t)n * Ci * V + (int64_t)d * HW;
  const float* cs = cen + (int64_t)s * Ci * C;
  float a0 = 0.f, a1 = 0.f;
  for (int i = blockIdx.x * LT + threadIdx.x; i < HW; i += gridDim.x * LT) {
    const int h = i / W, w = i - h * W;
    float p[MAXC], q[MAXC];
    load_probs<C>(lg, V, i, do_softmax != 0, p);
    for (int ch = 0; ch < Ci; ++ch) {
      const float x = im[(int64_t)ch * V + i];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float t = x - cs[ch * C + c];
        a0 += t * t * p[c];
      }
    }
    if (h + 1 < H) { load_probs<C>(lg, V, i + W, do_softmax != 0, q); a1 += ms_edge<C>(q, p, penalty); }
    if (w + 1 < W) { load_probs<C>(lg, V, i + 1, do_softmax != 0, q); a1 += ms_edge<C>(q, p, penalty); }
  }
  float* row = part + ((int64_t)s * gridDim.x + blockIdx.x) * 2;
  const float t0 = block_sum(a0);
  const float t1 = block_sum(a1);
  if (threadIdx.x == 0) { row[0] = t0; row[1] = t1; }
}

__device__ __forceinline__ float ms_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// the stencil's share of one difference a - b as seen from a (sgn = +1) or from b (sgn = -1)
template <int C>
__device__ __forceinline__ void ms_stencil(const float (&a)[MAXC], const float (&b)[MAXC], int penalty, float sgn, float (&st)[MAXC]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float dlt = a[c] - b[c];
    st[c] += sgn * (penalty == 2 ? 2.0f * dlt : ms_sign(dlt));
  }
}

template <int C>
__global__ void __launch_bounds__(LT)
wsl_ms_bwd_k(const float* __restrict__ logits, const float* __restrict__ image, const float* __restrict__ cen,
             const float* __restrict__ gscale, int Ci, int D, int H, int W, int penalty, float lambda, float inv_numel, int do_softmax,
             float* __restrict__ dlogits) {
  const int s = blockIdx.y, n = s / D, d = s % D, HW = H * W;
  const int64_t V = (int64_t)HW * D;
  const float* lg = logits + (int64_t)n * C * V + (int64_t)d * HW;
  const float* im = image + (int64_t)n * Ci * V + (int64_t)d * HW;
  float* dg = dlogits + (int64_t)n * C * V + (int64_t)d * HW;
  const float* cs = cen + (int64_t)s * Ci * C;
  const float gs = *gscale;
  const bool sm = do_softmax != 0;
  for (int i = blockIdx.x * LT + threadIdx.x; i < HW; i += gridDim.x * LT) {
    const int h = i / W, w = i - h * W;
    float p[MAXC], q[MAXC], lev[MAXC], st[MAXC], e[MAXC];
    load_probs<C>(lg, V, i, sm, p);
#pragma unroll
    for (int c = 0; c < C; ++c) { lev[c] = 0.f; st[c] = 0.f; }
    for (int ch = 0; ch < Ci; ++ch) {
      const float x = im[(int64_t)ch * V + i];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float t = x - cs[ch * C + c];
        lev[c] += t * t;
      }
    }
    if (h > 0) { load_probs<C>(lg, V, i - W, sm, q); ms_stencil<C>(p, q, penalty, 1.f, st); }
    if (h + 1 < H) { load_probs<C>(lg, V, i + W, sm, q); ms_stencil<C>(q, p, penalty, -1.f, st); }
    if (w > 0) { load_probs<C>(lg, V, i - 1, sm, q); ms_stencil<C>(p, q, penalty, 1.f, st); }
    if (w + 1 < W) { load_probs<C>(lg, V, i + 1, sm, q); ms_stencil<C>(q, p, penalty, -1.f, st); }
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = (lev[c] + lambda * st[c]) * inv_numel;
    store_jacobian<C>(p, e, gs, sm, dg, V, i);
  }
}

inline int wsl_shape_check(const char* what, int n, int c, int d, int h, int w) {
  FPLX_REQUIRE(n > 0 && c >= 2 && c <= MAXC && d > 0 && h > 0 && w > 0, FPLX_E_BADSHAPE,
               "%s: n=%d (>= 1) c=%d (2..%d) d=%d h=%d w=%d (>= 1)", what, n, c, MAXC, d, h, w);
  const int64_t v = (int64_t)d * h * w;
  // voxel offsets inside a sample are 32-bit (TV's argmin tensor, the slice loops); the (n, c) rows and the slices are grid.y
  FPLX_REQUIRE(v <= (1LL << 30) && (int64_t)n * c <= 65535 && (int64_t)n * d <= 65535, FPLX_E_BADSHAPE,
               "%s: d h w=%lld (<= 2^30) n c=%lld n d=%lld (<= 65535)", what, (long long)v, (long long)n * c, (long long)n * d);
  return FPLX_OK;
}

inline int wsl_ci_check(const char* what, int ci) {
  FPLX_REQUIRE(ci >= 1 && ci <= MAXCI, FPLX_E_BADSHAPE, "%s: ci=%d image channels (1..%d)", what, ci, MAXCI);
  return FPLX_OK;
}

inline int wsl_ms_check(const char* what, int penalty, float lambda) {
  FPLX_REQUIRE(penalty == 1 || penalty == 2, FPLX_E_BADSHAPE, "%s: penalty=%d (1: l1, 2: l2)", what, penalty);
  FPLX_REQUIRE(lambda >= 0.f, FPLX_E_BADSHAPE, "%s: lambda=%g is negative", what, (double)lambda);
  return FPLX_OK;
}

}  // namespace

#define WSL_DISPATCH(C, KERNEL, ...)               \
  switch (C) {                                     \
    case 2: KERNEL<2> __VA_ARGS__; break;          \
    case 3: KERNEL<3> __VA_ARGS__; break;          \
    case 4: KERNEL<4> __VA_ARGS__; break;          \
    case 5: KERNEL<5> __VA_ARGS__; break;          \
    case 6: KERNEL<6> __VA_ARGS__; break;          \
    case 7: KERNEL<7> __VA_ARGS__; break;          \
    default: KERNEL<8> __VA_ARGS__; break;         \
  }

extern "C" {

int fplx_wsl_gatedcrf_fwd(const float* logits, const float* image, int n, int c, int ci, int d, int h, int w, const float* desc,
                          int nk, int radius, int softmax, float* kp, float* part, double* out, fplx_stream_t stream) {
  int rc = wsl_shape_check("wsl_gatedcrf_fwd", n, c, d, h, w);
  if (rc != FPLX_OK) return rc;
  rc = wsl_ci_check("wsl_gatedcrf_fwd", ci);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(nk >= 1 && nk <= CRF_MAXK && radius >= 1 && radius <= CRF_MAXR, FPLX_E_BADSHAPE,
               "wsl_gatedcrf_fwd: nk=%d kernel descriptors (1..%d) radius=%d (1..%d)", nk, CRF_MAXK, radius, CRF_MAXR);
  FPLX_REQUIRE(logits && image && desc && kp && part && out, FPLX_E_NULL, "wsl_gatedcrf_fwd: null pointer");
  CrfDesc ds;
  ds.nk = nk;
  for (int k = 0; k < CRF_MAXK; ++k) ds.w[k] = ds.ixy[k] = ds.irgb[k] = 0.f;
  for (int k = 0; k < nk; ++k) {
    const float wt = desc[3 * k], sxy = desc[3 * k + 1], srgb = desc[3 * k + 2];
    FPLX_REQUIRE(sxy >= 0.f && srgb >= 0.f && (sxy > 0.f || srgb > 0.f), FPLX_E_BADSHAPE,
                 "wsl_gatedcrf_fwd: descriptor %d: sigma_xy=%g sigma_rgb=%g (>= 0, one of them > 0)", k, (double)sxy, (double)srgb);
    ds.w[k] = wt;
    ds.ixy[k] = sxy > 0.f ? (float)(1.0 / ((double)sxy * sxy)) : 0.f;
    ds.irgb[k] = srgb > 0.f ? (float)(1.0 / ((double)srgb * srgb)) : 0.f;
  }
  const int tx = (w + CRF_T - 1) / CRF_T, ty = (h + CRF_T - 1) / CRF_T;
  const int64_t blocks = (int64_t)n * d * tx * ty;
  FPLX_REQUIRE(blocks <= 0x7fffffffLL, FPLX_E_BADSHAPE, "wsl_gatedcrf_fwd: %lld tiles (< 2^31)", (long long)blocks);
  const int E = CRF_T + 2 * radius, dia = 2 * radius + 1;
  const size_t lds = sizeof(float) * ((size_t)(c + ci) * E * E + (size_t)nk * dia * dia);
  hipStream_t st = (hipStream_t)stream;
  WSL_DISPATCH(c, wsl_crf_fwd_k, <<<dim3((unsigned)blocks), LT, lds, st>>>(logits, image, ci, d, h, w, tx, ty, radius, ds, softmax,
                                                                            kp, part));
  wsl_finish_k<<<1, 64, 0, st>>>(part, 1, blocks, (double)n * d * (double)h * w, 0.0, out);
  return fplx_check_launch("wsl_gatedcrf_fwd");
}

int fplx_wsl_gatedcrf_bwd(const float* logits, const float* kp, const float* gscale, int n, int c, int d, int h, int w,
                          int softmax, float* dlogits, fplx_stream_t stream) {
  const int rc = wsl_shape_check("wsl_gatedcrf_bwd", n, c, d, h, w);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && kp && gscale && dlogits, FPLX_E_NULL, "wsl_gatedcrf_bwd: null pointer");
  const int64_t v = (int64_t)d * h * w;
  const float coef = (float)(-2.0 / ((double)n * (double)v));
  dim3 grid(grid1(v, 2048), n);
  WSL_DISPATCH(c, wsl_crf_bwd_k, <<<grid, LT, 0, (hipStream_t)stream>>>(logits, kp, gscale, coef, v, softmax, dlogits));
  return fplx_check_launch("wsl_gatedcrf_bwd");
}

int fplx_wsl_tv_fwd(const float* logits, int n, int c, int d, int h, int w, int softmax, int32_t* count, void* ws,
                    size_t ws_bytes, float* part, double* out, fplx_stream_t stream) {
  const int rc = wsl_shape_check("wsl_tv_fwd", n, c, d, h, w);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && count && ws && part && out, FPLX_E_NULL, "wsl_tv_fwd: null pointer");
  const int64_t v = (int64_t)d * h * w, e = (int64_t)n * c * v;
  FPLX_REQUIRE(ws_bytes >= (size_t)e * 12, FPLX_E_BADSHAPE, "wsl_tv_fwd: workspace of %zu bytes, %lld needed", ws_bytes,
               (long long)e * 12);
  FPLX_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15u) == 0, FPLX_E_BADSHAPE, "wsl_tv_fwd: the workspace is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float* pp = (float*)ws;
  float* er = pp + e;
  int32_t* amin = (int32_t*)(er + e);
  const int rows = loss_rows(v);
  if (hipMemsetAsync(count, 0, (size_t)e * sizeof(int32_t), st) != hipSuccess) return fplx_check_launch("wsl_tv_fwd");
  WSL_DISPATCH(c, wsl_tv_prob_k, <<<dim3(grid1(v, 2048), n), LT, 0, st>>>(logits, v, softmax, pp));
  wsl_tv_erode_k<<<dim3(grid1(v, 2048), n * c), LT, 0, st>>>(pp, d, h, w, er, amin);
  wsl_tv_dilate_k<<<dim3(rows, n * c), LT, 0, st>>>(er, amin, d, h, w, count, part);
  wsl_finish_k<<<1, 64, 0, st>>>(part, 1, (int64_t)n * c * rows, (double)e, 0.0, out);
  return fplx_check_launch("wsl_tv_fwd");
}

int fplx_wsl_tv_bwd(const float* logits, const int32_t* count, const float* gscale, int n, int c, int d, int h, int w,
                    int softmax, float* dlogits, fplx_stream_t stream) {
  const int rc = wsl_shape_check("wsl_tv_bwd", n, c, d, h, w);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && count && gscale && dlogits, FPLX_E_NULL, "wsl_tv_bwd: null pointer");
  const int64_t v = (int64_t)d * h * w;
  const float coef = (float)(0.999 / ((double)n * c * (double)v));
  dim3 grid(grid1(v, 2048), n);
  WSL_DISPATCH(c, wsl_tv_bwd_k, <<<grid, LT, 0, (hipStream_t)stream>>>(logits, count, gscale, coef, v, softmax, dlogits));
  return fplx_check_launch("wsl_tv_bwd");
}

int fplx_wsl_mumford_shah_fwd(const float* logits, const float* image, int n, int c, int ci, int d, int h, int w, int penalty,
                              float lambda, int softmax, float* cen, float* part, double* out, fplx_stream_t stream) {
  int rc = wsl_shape_check("wsl_mumford_shah_fwd", n, c, d, h, w);
  if (rc != FPLX_OK) return rc;
  rc = wsl_ci_check("wsl_mumford_shah_fwd", ci);
  if (rc != FPLX_OK) return rc;
  rc = wsl_ms_check("wsl_mumford_shah_fwd", penalty, lambda);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && image && cen && part && out, FPLX_E_NULL, "wsl_mumford_shah_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int hw = h * w, chunks = loss_rows(hw), slices = n * d;
  dim3 grid(chunks, slices);
  WSL_DISPATCH(c, wsl_ms_moments_k, <<<grid, LT, 0, st>>>(logits, image, ci, d, hw, softmax, part));
  wsl_ms_centroid_k<<<grid1((int64_t)slices * ci * c, 2048), LT, 0, st>>>(part, slices, chunks, c, ci, cen);
  WSL_DISPATCH(c, wsl_ms_loss_k, <<<grid, LT, 0, st>>>(logits, image, cen, ci, d, h, w, penalty, softmax, part));
  wsl_finish_k<<<1, 64, 0, st>>>(part, 2, (int64_t)slices * chunks, (double)n * c * (double)d * (double)hw, (double)lambda, out);
  return fplx_check_launch("wsl_mumford_shah_fwd");
}

int fplx_wsl_mumford_shah_bwd(const float* logits, const float* image, const float* cen, const float* gscale, int n, int c,
                              int ci, int d, int h, int w, int penalty, float lambda, int softmax, float* dlogits,
                              fplx_stream_t stream) {
  int rc = wsl_shape_check("wsl_mumford_shah_bwd", n, c, d, h, w);
  if (rc != FPLX_OK) return rc;
  rc = wsl_ci_check("wsl_mumford_shah_bwd", ci);
  if (rc != FPLX_OK) return rc;
  rc = wsl_ms_check("wsl_mumford_shah_bwd", penalty, lambda);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && image && cen && gscale && dlogits, FPLX_E_NULL, "wsl_mumford_shah_bwd: null pointer");
  const int hw = h * w;
  const float inv = (float)(1.0 / ((double)n * c * (double)d * (double)hw));
  dim3 grid(grid1(hw, 2048), n * d);
  WSL_DISPATCH(c, wsl_ms_bwd_k, <<<grid, LT, 0, (hipStream_t)stream>>>(logits, image, cen, gscale, ci, d, h, w, penalty, lambda, inv,
                                                                       softmax, dlogits));
  return fplx_check_launch("wsl_mumford_shah_bwd");
}

}  // extern "C"
