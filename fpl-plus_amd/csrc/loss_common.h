// What the two segmentation-loss families (loss_filter.hip, loss_ext.hip) share: the class / block limits and the dispatch on
// the class count, the shape check, the number of partial rows of a pass and where its double sums live, the softmax of one
// voxel, the kernel that reduces the partial rows (seg_loss_sums_k: an anonymous-namespace kernel, so each of the two files compiles
// its own copy of it into the library), the first family's part of the one-thread finalize and the first family's gradient
// terms of the backward voxel loop.  The rest of the voxel loops stays in their own files (loss_ext.hip says why).
// ssl.hip and nll.hip (the semi-supervised and noisy-label passes) take the limits, loss_rows / grid1, softmax_argmax and the
// voxel loads / stores from here and nothing else.
#pragma once
#include "common.h"

namespace {

constexpr int MAXC = 8;
constexpr int LT = 256;

inline int loss_rows(int64_t v) {
  int64_t r = (v + 4095) / 4096;
  if (r > 512) r = 512;
  if (r < 1) r = 1;
  return (int)r;
}

inline int grid1(int64_t v, int cap) {
  int64_t g = (v + LT - 1) / LT;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

inline int loss_shape_check(const char* what, int n, int c, int64_t v) {
  FPLX_REQUIRE(n > 0 && n <= 64 && c >= 1 && c <= MAXC && v > 0, FPLX_E_BADSHAPE, "%s: n=%d (<=64) c=%d (<=%d) v=%lld", what, n,
               c, MAXC, (long long)v);
  return FPLX_OK;
}

// rows to ALLOCATE per sample are the partial rows the kernels use plus LOSS_SPARE_ROWS: behind the N x rows x K partials of a
// call the spare N x 5 x K floats hold the per-sample sums and the batch totals as doubles ((N + 1) x K doubles = 2 (N + 1) K
// floats) plus the one float the 8-byte alignment of that region may cost (K is odd): 2 (N + 1) K + 1 <= 5 N K for every N >= 1.
// (With 4 spare rows N = 1 and an odd rows x K overran the buffer by one float: ADVICE r02.)
constexpr int LOSS_SPARE_ROWS = 5;
struct LossSums { double *sums, *totals; };      // [N][K], [K]
inline LossSums loss_sums_region(float* part, int n, int rows, int K) {
  double* sums = reinterpret_cast<double*>(part + (((size_t)n * rows * K + 1) / 2) * 2);
  return {sums, sums + (size_t)n * K};
}

template <int C>
__device__ __forceinline__ int softmax_argmax(const float (&l)[MAXC], float (&p)[MAXC], bool do_softmax) {
  // scipy.special.softmax / torch.softmax order of operations: max, exp(x - max), sum, divide.
  // Returns argmax (first maximum) of the PROBABILITIES, as np.argmax(prob) does.
  float m = l[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, l[c]);
  if (do_softmax) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { p[c] = expf(l[c] - m); s += p[c]; }
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = p[c] / s;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = l[c];
  }
  int a = 0;
  float best = p[0];
#pragma unroll
  for (int c = 1; c < C; ++c)
    if (p[c] > best) { best = p[c]; a = c; }
  return a;
}

// ---- what ssl.hip and nll.hip load and store voxels with: one voxel per lane, or four with 16-byte accesses
template <int W> struct VecLd;
template <> struct VecLd<1> {
  static __device__ __forceinline__ void ld(const float* p, float (&o)[1]) { o[0] = *p; }
  static __device__ __forceinline__ void st(float* p, const float (&o)[1]) { *p = o[0]; }
};
template <> struct VecLd<4> {
  static __device__ __forceinline__ void ld(const float* p, float (&o)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
  }
  static __device__ __forceinline__ void st(float* p, const float (&o)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
  }
};

// [C][V] rows of one sample at voxel v -> l[j][c] for the W voxels of this lane
template <int C, int W>
__device__ __forceinline__ void load_voxels(const float* __restrict__ base, int64_t V, int64_t v, float (&l)[W][MAXC]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float t[W];
    VecLd<W>::ld(base + (int64_t)c * V + v, t);
#pragma unroll
    for (int j = 0; j < W; ++j) l[j][c] = t[j];
  }
}
template <int C, int W>
__device__ __forceinline__ void store_voxels(float* __restrict__ base, int64_t V, int64_t v, const float (&l)[W][MAXC]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float t[W];
#pragma unroll
    for (int j = 0; j < W; ++j) t[j] = l[j][c];
    VecLd<W>::st(base + (int64_t)c * V + v, t);
  }
}

// The first family's gradient terms of one class at one voxel, before the softmax Jacobian (ent_sm: the entropy term shares
// the pass's softmax).
__device__ __forceinline__ float seg_loss_base_grad(bool use_dice, bool use_ce, bool ent_sm, float w, float A, float B, float cce,
                                                    float cent, float y, float p) {
  const float inv_ln2 = 1.4426950408889634f;
  float gc = 0.f;
  if (use_dice) gc += w * fmaf(A, y, B);
  if (use_ce) gc -= cce * w * y * 0.999f / (p * 0.999f + 5e-4f);
  if (ent_sm) gc -= cent * (log2f(p + 1e-10f) + p * inv_ln2 / (p + 1e-10f));
  return gc;
}

// the entropy term's gradient with respect to ITS softmax output q
__device__ __forceinline__ float seg_loss_ent_grad(float cent, float q) {
  const float inv_ln2 = 1.4426950408889634f;
  return -cent * (log2f(q + 1e-10f) + q * inv_ln2 / (q + 1e-10f));
}

// one block: reduce the partial rows part[N][rows][K] (double) to per-sample sums [N][K] and their total over the local samples [K]
__global__ void seg_loss_sums_k(const float* __restrict__ part, int rows, int N, int K, double* __restrict__ sums,
                                double* __restrict__ totals) {
  // one wave per (n, k) sum: lanes stride over rows
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int i = wv; i < N * K; i += nw) {
    const int n = i / K, k = i % K;
    double s = 0.0;
    for (int r = lane; r < rows; r += 64) s += (double)part[((int64_t)n * rows + r) * K + k];
    s = wave_sum_d(s);
    if (lane == 0) sums[i] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    double t = 0.0;
    for (int n = 0; n < N; ++n) t += sums[n * K + threadIdx.x];      // fixed order
    totals[threadIdx.x] = t;
  }
}

// The first family's part of the one-thread finalize: the loss terms and the backward coefficients from the per-sample sums of
// the LOCAL samples (rows of K doubles, the first 6C + 3 of each the first family's) and the totals over the WHOLE batch (= the
// local totals in one process; all-reduced over the ranks under data parallelism, where the reference's nn.DataParallel gathers
// the logits and evaluates ONE loss over the full batch, agent_seg.py:692-698).  Writes out[1..3], out[4 .. 4+C) and
// coef[0 .. 2NC+2); returns the weighted total of the four terms.
__device__ __forceinline__ double seg_loss_base_finalize(const double* __restrict__ sums, const double* __restrict__ tot, int N,
                                                         int NG, int C, int K, double V, int has_pw,
                                                         const float* __restrict__ image_weight, float w_dice, float w_ce,
                                                         float w_img, float w_ent, float* __restrict__ out,
                                                         float* __restrict__ coef) {
  double Ld = 0.0, Limg = 0.0, Lce = 0.0, Lent = 0.0;
  for (int i = 0; i < N * C * 2; ++i) coef[i] = 0.f;
  // global Dice over all voxels of the batch (dice.py:20-57)
  for (int c = 0; c < C; ++c) {
    const double* t = tot + 6 * c;
    const double den = t[0] + t[1] + 1e-5, num = 2.0 * t[2] + 1e-5;
    Ld += num / den;
    out[4 + c] = (float)((2.0 * t[5] + 1e-5) / (t[3] + t[4] + 1e-5));
    for (int n = 0; n < N; ++n) {
      coef[(n * C + c) * 2 + 0] += (float)(w_dice * (-2.0 / (C * den)));
      coef[(n * C + c) * 2 + 1] += (float)(w_dice * (num / (C * den * den)));
    }
  }
  Ld = 1.0 - Ld / C;
  // per-sample Dice times image weight, mean over the batch (dice.py:106-128): this rank's samples only; the terms of the
  // other ranks' samples are theirs (the value is completed by the caller's all-reduce when it wants the number)
  if (w_img != 0.f && image_weight) {
    for (int n = 0; n < N; ++n) {
      double dn = 0.0;
      const double f = (double)image_weight[n] / NG;
      for (int c = 0; c < C; ++c) {
        const double* s = sums + n * K + 6 * c;
        const double den = s[0] + s[1] + 1e-5, num = 2.0 * s[2] + 1e-5;
        dn += num / den;
        coef[(n * C + c) * 2 + 0] += (float)(w_img * f * (-2.0 / (C * den)));
        coef[(n * C + c) * 2 + 1] += (float)(w_img * f * (num / (C * den * den)));
      }
      Limg += f * (1.0 - dn / C);
    }
  }
  const double cenum = tot[6 * C + 0], wsum = tot[6 * C + 1], ent = tot[6 * C + 2];
  const double ce_norm = has_pw ? 1.0 / (wsum + 1e-5) : 1.0 / (NG * V);   // ce.py:39-43
  Lce = cenum * ce_norm;
  Lent = ent / (NG * V);                                                  // agent_seg.py:352-353
  coef[N * C * 2 + 0] = (float)(w_ce * ce_norm);
  coef[N * C * 2 + 1] = (float)(w_ent / (NG * V));
  out[1] = (float)(w_dice * Ld + w_img * Limg);
  out[2] = (float)Lce;
  out[3] = (float)Lent;
  return w_dice * Ld + w_img * Limg + w_ce * Lce + w_ent * Lent;
}

}  // namespace

#define DISPATCH_C(C, KERNEL, ...)                 \
  switch (C) {                                     \
    case 1: KERNEL<1> __VA_ARGS__; break;          \
    case 2: KERNEL<2> __VA_ARGS__; break;          \
    case 3: KERNEL<3> __VA_ARGS__; break;          \
    case 4: KERNEL<4> __VA_ARGS__; break;          \
    case 5: KERNEL<5> __VA_ARGS__; break;          \
    case 6: KERNEL<6> __VA_ARGS__; break;          \
    case 7: KERNEL<7> __VA_ARGS__; break;          \
    default: KERNEL<8> __VA_ARGS__; break;         \
  }
