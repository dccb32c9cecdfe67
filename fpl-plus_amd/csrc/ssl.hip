// Semi-supervised regularisers of the reference's second entry point (PyMIC/pymic/net_run_ssl/ssl_em.py, ssl_mt.py, ssl_uamt.py):
// the clamped-noise perturbation of a teacher input, the (uncertainty-masked) consistency loss between student and teacher,
// EntropyLoss (loss/seg/ssl.py:32-44) and the EMA of the parameters - each ONE pass over its tensors, forward and backward.
// Also URPC's pyramid consistency over K output scales (ssl_urpc.py:76-91) and CPS's one-hot pseudo labels (ssl_cps.py:103-106).
// Layouts and formulas: include/fplx.h, "semi-supervised learning".  Reductions as in the two loss families: a block's fp32
// partial row, the rows summed in double in a fixed order by one wave (no floating-point atomics: two runs give the same bits).
// A lane takes 4 consecutive voxels with 16-byte loads where every row of the tensors is 16-byte aligned (aligned bases and
// V a multiple of 4), else one voxel; the flat passes (perturb, EMA) take n / 4 quads and a scalar tail
// (VecLd, load_voxels, store_voxels: loss_common.h).
// Compiled with -ffp-contract=off (Makefile): x + clamp(sigma z) must round as torch's three fp32 operations do, and the
// sums of squares must not depend on what the compiler fuses; the fused multiply-adds that are meant are written as fmaf.
#include "loss_common.h"
#include "philox.h"

namespace {

// a block's K sums -> part[(n * gridDim.x + blockIdx.x) * K + k]
template <int K>
__device__ __forceinline__ void block_rows(const float (&acc)[K], float* __restrict__ part) {
  __shared__ float red[LT / 64][K];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float t = wave_sum(acc[k]);
    if (lane == 0) red[wv][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    float t = 0.f;
    for (int i = 0; i < LT / 64; ++i) t += red[i][threadIdx.x];
    part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * K + threadIdx.x] = t;
  }
}

// ---- consistency: sum over kept voxels of sum_c (p_c - q_c)^2 and the number of kept voxels.  part [N][rows][2]
template <int C, int W>
__global__ void __launch_bounds__(LT)
ssl_cons_fwd_k(const float* __restrict__ student, const float* __restrict__ teacher, const float* __restrict__ mc, int T, int N,
               int64_t V, float thr, int do_softmax, uint8_t* __restrict__ mask, float* __restrict__ part) {
  const int n = blockIdx.y;
  const float* sg = student + (int64_t)n * C * V;
  const float* tg = teacher + (int64_t)n * C * V;
  const float ft = (float)T;
  float acc[2] = {0.f, 0.f};
  const int64_t nq = V / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    const int64_t v = i * W;
    bool keep[W];
#pragma unroll
    for (int j = 0; j < W; ++j) keep[j] = true;
    if (T > 0) {
      // ssl_uamt.py:91-99: softmax per pass, mean over the passes, entropy with + 1e-6, kept where it is below the threshold
      float m[W][MAXC];
#pragma unroll
      for (int j = 0; j < W; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) m[j][c] = 0.f;
      for (int t = 0; t < T; ++t) {
        float l[W][MAXC], p[MAXC];
        load_voxels<C, W>(mc + ((int64_t)t * N + n) * C * V, V, v, l);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          softmax_argmax<C>(l[j], p, do_softmax != 0);
#pragma unroll
          for (int c = 0; c < C; ++c) m[j][c] += p[c];
        }
      }
      uint32_t bits = 0;
#pragma unroll
      for (int j = 0; j < W; ++j) {
        float unc = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float mm = m[j][c] / ft;
          unc -= mm * logf(mm + 1e-6f);
        }
        keep[j] = unc < thr;
        bits |= (keep[j] ? 1u : 0u) << (8 * j);
      }
      uint8_t* mk = mask + (int64_t)n * V + v;
      if (W == 4) *reinterpret_cast<uint32_t*>(mk) = bits;
      else *mk = (uint8_t)bits;
    }
    float s[W][MAXC], q[W][MAXC];
    load_voxels<C, W>(sg, V, v, s);
    load_voxels<C, W>(tg, V, v, q);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float p[MAXC], r[MAXC];
      softmax_argmax<C>(s[j], p, do_softmax != 0);
      softmax_argmax<C>(q[j], r, do_softmax != 0);
      float sq = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) { const float d = p[c] - r[c]; sq += d * d; }
      if (keep[j]) { acc[0] += sq; acc[1] += 1.f; }
    }
  }
  block_rows<2>(acc, part);
}

// one wave: the rows in double, lanes stride over them, then the loss.  mode 0: mean over N C V (torch.nn.MSELoss, ssl_mt.py:100),
// 1: out0 / (2 out1 + 1e-16) (ssl_uamt.py:100), 2: EntropyLoss, out0 / (ln C N V) with out1 = N V
__global__ void ssl_finish_k(const float* __restrict__ part, int K, int64_t rows_total, int mode, double nv, int C,
                             double* __restrict__ out) {
  const int lane = threadIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t r = lane; r < rows_total; r += 64) {
    s0 += (double)part[r * K];
    if (K > 1) s1 += (double)part[r * K + 1];
  }
  s0 = wave_sum_d(s0);
  s1 = wave_sum_d(s1);
  if (lane == 0) {
    double loss;
    if (mode == 0) { s1 = nv; loss = s0 / (nv * C); }
    else if (mode == 1) loss = s0 / (2.0 * s1 + 1e-16);
    else { s1 = nv; loss = s0 / (log((double)C) * nv); }
    out[0] = s0; out[1] = s1; out[2] = loss; out[3] = 0.0;
  }
}

template <int C, int W>
__global__ void __launch_bounds__(LT)
ssl_cons_bwd_k(const float* __restrict__ student, const float* __restrict__ teacher, const uint8_t* __restrict__ mask,
               const double* __restrict__ out, const float* __restrict__ gscale, int N, int64_t V, int T, int do_softmax,
               float* __restrict__ dstudent) {
  const int n = blockIdx.y;
  const float* sg = student + (int64_t)n * C * V;
  const float* tg = teacher + (int64_t)n * C * V;
  float* dg = dstudent + (int64_t)n * C * V;
  const double den = T > 0 ? 2.0 * out[1] + 1e-16 : (double)N * C * (double)V;
  const float k2 = (float)(2.0 / den), gs = *gscale;
  const int64_t nq = V / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    const int64_t v = i * W;
    uint32_t bits = 0x01010101u;
    if (T > 0) {
      const uint8_t* mk = mask + (int64_t)n * V + v;
      bits = W == 4 ? *reinterpret_cast<const uint32_t*>(mk) : (uint32_t)*mk;
    }
    float s[W][MAXC], q[W][MAXC], d[W][MAXC];
    load_voxels<C, W>(sg, V, v, s);
    load_voxels<C, W>(tg, V, v, q);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float p[MAXC], r[MAXC], e[MAXC];
      softmax_argmax<C>(s[j], p, do_softmax != 0);
      softmax_argmax<C>(q[j], r, do_softmax != 0);
      const float kj = ((bits >> (8 * j)) & 0xFFu) ? k2 : 0.f;
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        e[c] = (p[c] - r[c]) * kj;
        dot = fmaf(e[c], p[c], dot);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) d[j][c] = gs * (do_softmax ? p[c] * (e[c] - dot) : e[c]);
    }
    store_voxels<C, W>(dg, V, v, d);
  }
}

// ---- EntropyLoss (loss/seg/ssl.py:40-43): sum over the voxels of -sum_c p' ln p', p' = 0.999 p + 5e-4.  part [N][rows][1]
template <int C, int W>
__global__ void __launch_bounds__(LT)
ssl_ent_fwd_k(const float* __restrict__ logits, int64_t V, int do_softmax, float* __restrict__ part) {
  const float* lg = logits + (int64_t)blockIdx.y * C * V;
  float acc[1] = {0.f};
  const int64_t nq = V / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    float l[W][MAXC];
    load_voxels<C, W>(lg, V, i * W, l);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float p[MAXC];
      softmax_argmax<C>(l[j], p, do_softmax != 0);
      float h = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float pp = p[c] * 0.999f + 5e-4f;
        h -= pp * logf(pp);
      }
      acc[0] += h;
    }
  }
  block_rows<1>(acc, part);
}

template <int C, int W>
__global__ void __launch_bounds__(LT)
ssl_ent_bwd_k(const float* __restrict__ logits, const float* __restrict__ gscale, float coef, int64_t V, int do_softmax,
              float* __restrict__ dlogits) {
  const float* lg = logits + (int64_t)blockIdx.y * C * V;
  float* dg = dlogits + (int64_t)blockIdx.y * C * V;
  const float gs = *gscale;
  const int64_t nq = V / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    float l[W][MAXC], d[W][MAXC];
    load_voxels<C, W>(lg, V, i * W, l);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float p[MAXC], g[MAXC];
      softmax_argmax<C>(l[j], p, do_softmax != 0);
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float pp = p[c] * 0.999f + 5e-4f;
        g[c] = -coef * (logf(pp) + 1.0f);                  // coef = 0.999 / (ln C N V)
        dot = fmaf(g[c], p[c], dot);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) d[j][c] = gs * (do_softmax ? p[c] * (g[c] - dot) : g[c]);
    }
    store_voxels<C, W>(dg, V, i * W, d);
  }
}

// ---- URPC's pyramid consistency (ssl_urpc.py:76-91) over K = 2..4 full-resolution logit tensors, and CPS's pseudo labels.
// Per voxel K C probabilities are live at once, so the vector path is four voxels per lane only while K C <= 12 and two
// (8-byte accesses) beyond; the register counts per instantiation are in DESIGN 1n.
constexpr int PYR_K = 4;
struct PyrIn { const float* p[PYR_K]; };
struct PyrOut { float* p[PYR_K]; };

template <> struct VecLd<2> {
  static __device__ __forceinline__ void ld(const float* p, float (&o)[2]) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    o[0] = t.x; o[1] = t.y;
  }
  static __device__ __forceinline__ void st(float* p, const float (&o)[2]) { *reinterpret_cast<float2*>(p) = make_float2(o[0], o[1]); }
};

constexpr int pyr_width(int K, int C) { return K * C <= 12 ? 4 : 2; }
// the backward pass also holds the K C gradients of every voxel until their rows are stored
constexpr int pyr_width_bwd(int K, int C) { return K * C <= 4 ? 4 : (K * C <= 12 ? 2 : 1); }

// one voxel in the reference's order: p_k = softmax(z_k), m = (p_1 + .. + p_K) / K, a = 0.99 m + 0.005, q_k = 0.99 p_k + 0.005,
// dl_kc = ln a_c - ln q_kc, var_k = sum_c a_c dl_kc, e_k = exp(-var_k), s_k = sum_c (a_c - q_kc)^2
template <int K, int C>
__device__ __forceinline__ void pyr_voxel(const float (&l)[K][MAXC], float (&p)[K][MAXC], float (&a)[MAXC], float (&dl)[K][MAXC],
                                          float (&var)[K], float (&e)[K], float (&s)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) softmax_argmax<C>(l[k], p[k], true);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float m = p[0][c];
#pragma unroll
    for (int k = 1; k < K; ++k) m += p[k][c];
    a[c] = (m / (float)K) * 0.99f + 0.005f;
    const float la = logf(a[c]);
#pragma unroll
    for (int k = 0; k < K; ++k) dl[k][c] = la - logf(p[k][c] * 0.99f + 0.005f);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float vs = 0.f, ss = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float d = a[c] - (p[k][c] * 0.99f + 0.005f);
      vs += a[c] * dl[k][c];
      ss += d * d;
    }
    var[k] = vs;
    e[k] = expf(-vs);
    s[k] = ss;
  }
}

// part [N][rows][3 K]: per scale sum s_k e_k, sum e_k, sum var_k
template <int K, int C, int W>
__global__ void __launch_bounds__(LT)
ssl_pyramid_fwd_k(PyrIn lg, int64_t V, float* __restrict__ part) {
  const int64_t off = (int64_t)blockIdx.y * C * V;
  float acc[3 * K];
#pragma unroll
  for (int i = 0; i < 3 * K; ++i) acc[i] = 0.f;
  const int64_t nq = V / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    float l[K][W][MAXC];
#pragma unroll
    for (int k = 0; k < K; ++k) load_voxels<C, W>(lg.p[k] + off, V, i * W, l[k]);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float lv[K][MAXC], p[K][MAXC], a[MAXC], dl[K][MAXC], var[K], e[K], s[K];
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c) lv[k][c] = l[k][j][c];
      pyr_voxel<K, C>(lv, p, a, dl, var, e, s);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        acc[3 * k + 0] += s[k] * e[k];
        acc[3 * k + 1] += e[k];
        acc[3 * k + 2] += var[k];
      }
    }
  }
  block_rows<3 * K>(acc, part);
}

// one wave: the rows in double, lanes stride over them; out [K][4] (A_k, B_k, V_k, L_k) + [2] (loss_reg, 0), M = N V:
// L_k = (A_k / (C M)) / (B_k / M + 1e-8) + V_k / M (ssl_urpc.py:88-89), loss_reg = sum_k L_k / K
__global__ void ssl_pyramid_finish_k(const float* __restrict__ part, int K, int C, int64_t rows_total, double M,
                                     double* __restrict__ out) {
  const int lane = threadIdx.x;
  double total = 0.0;
  for (int k = 0; k < K; ++k) {
    double t[3];
    for (int i = 0; i < 3; ++i) {
      double s = 0.0;
      for (int64_t r = lane; r < rows_total; r += 64) s += (double)part[r * (3 * K) + 3 * k + i];
      t[i] = wave_sum_d(s);
    }
    const double L = (t[0] / (C * M)) / (t[1] / M + 1e-8) + t[2] / M;
    total += L;
    if (lane == 0) { out[4 * k + 0] = t[0]; out[4 * k + 1] = t[1]; out[4 * k + 2] = t[2]; out[4 * k + 3] = L; }
  }
  if (lane == 0) { out[4 * K] = total / K; out[4 * K + 1] = 0.0; }
}

// g_k = 1 / M - e_k (alpha_k s_k + beta_k) = dL_k / dvar_k, h_k = alpha_k e_k = dL_k / ds_k with alpha_k, beta_k from A_k, B_k
// of `out`; the mean over the scales carries gradient (the reference does not detach it); then the softmax Jacobian
template <int K, int C, int W>
__global__ void __launch_bounds__(LT)
ssl_pyramid_bwd_k(PyrIn lg, const double* __restrict__ out, const float* __restrict__ gscale, int N, int64_t V, PyrOut dlg) {
  const int64_t off = (int64_t)blockIdx.y * C * V;
  const double M = (double)N * (double)V, CM = (double)C * M;
  float al[K], be[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double den = out[4 * k + 1] / M + 1e-8;
    al[k] = (float)(1.0 / (CM * den));
    be[k] = (float)(-(out[4 * k] / CM) / (den * den) / M);
  }
  const float invM = (float)(1.0 / M), gs = *gscale, w = 0.99f / (float)K;
  const int64_t nq = V / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    float l[K][W][MAXC], d[K][W][MAXC];
#pragma unroll
    for (int k = 0; k < K; ++k) load_voxels<C, W>(lg.p[k] + off, V, i * W, l[k]);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float lv[K][MAXC], p[K][MAXC], a[MAXC], dl[K][MAXC], var[K], e[K], s[K], g[K], h2[K], t[MAXC];
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c) lv[k][c] = l[k][j][c];
      pyr_voxel<K, C>(lv, p, a, dl, var, e, s);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        g[k] = invM - e[k] * (al[k] * s[k] + be[k]);
        h2[k] = 2.f * (al[k] * e[k]);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float ts = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) ts += g[k] * (dl[k][c] + 1.f) + h2[k] * (a[c] - (p[k][c] * 0.99f + 0.005f));
        t[c] = ts / (float)K;
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float gp[MAXC], dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float q = p[k][c] * 0.99f + 0.005f;
          gp[c] = w * (t[c] - g[k] * a[c] / q - h2[k] * (a[c] - q));
          dot = fmaf(gp[c], p[k][c], dot);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) d[k][j][c] = gs * (p[k][c] * (gp[c] - dot));
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) store_voxels<C, W>(dlg.p[k] + off, V, i * W, d[k]);
  }
}

// fp32 one-hot of the first maximum of the LOGITS over C, K tensors in one launch (ssl_cps.py:103-106)
template <int C, int W>
__global__ void __launch_bounds__(LT)
ssl_pseudo_onehot_k(PyrIn lg, int K, int64_t V, PyrOut oh) {
  const int64_t off = (int64_t)blockIdx.y * C * V;
  const int64_t nq = V / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
#pragma unroll
    for (int k = 0; k < PYR_K - 1; ++k) {
      if (k < K) {
        float l[W][MAXC], o[W][MAXC];
        load_voxels<C, W>(lg.p[k] + off, V, i * W, l);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          int best = 0;
          float m = l[j][0];
#pragma unroll
          for (int c = 1; c < C; ++c)
            if (l[j][c] > m) { m = l[j][c]; best = c; }
#pragma unroll
          for (int c = 0; c < C; ++c) o[j][c] = c == best ? 1.f : 0.f;
        }
        store_voxels<C, W>(oh.p[k] + off, V, i * W, o);
      }
    }
  }
}

// ---- flat passes
__device__ __forceinline__ float perturb1(float x, float z, float sigma, float clip) {
  const float t = sigma * z;
  return x + fminf(fmaxf(t, -clip), clip);               // torch.clamp: max with the lower bound, then min with the upper
}

// noise [reps][n] given: W = 4 needs every row 16-byte aligned (n % 4 == 0 or reps == 1); the tail of n % 4 elements is scalar
template <int W>
__global__ void __launch_bounds__(LT)
ssl_perturb_k(const float* __restrict__ x, const float* __restrict__ noise, float* __restrict__ y, int64_t n, int reps,
              float sigma, float clip) {
  const int64_t nq = n / W, tail0 = nq * W;
  for (int r = 0; r < reps; ++r) {
    const float* z = noise + (int64_t)r * n;
    float* yr = y + (int64_t)r * n;
    for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
      float a[W], b[W], o[W];
      VecLd<W>::ld(x + i * W, a);
      VecLd<W>::ld(z + i * W, b);
#pragma unroll
      for (int j = 0; j < W; ++j) o[j] = perturb1(a[j], b[j], sigma, clip);
      VecLd<W>::st(yr + i * W, o);
    }
    if (blockIdx.x == 0)
      for (int64_t i = tail0 + threadIdx.x; i < n; i += LT) yr[i] = perturb1(x[i], z[i], sigma, clip);
  }
}

// device generator: the Box-Muller of add_noise_philox_k (intensity.hip) on the counter (i >> 1, r, stream, i >> 33): element i of
// repetition r takes words 2 (i & 1), 2 (i & 1) + 1; u = (word + 1) / 2^32 in (0, 1]; z = sqrt(-2 ln u1) cos(2 pi u2) in fp64,
// rounded to fp32 once, then the three fp32 operations of the injected route
__global__ void __launch_bounds__(LT)
ssl_perturb_philox_k(const float* __restrict__ x, float* __restrict__ y, int64_t n, int reps, float sigma, float clip, uint32_t k0,
                     uint32_t k1, uint32_t sid) {
  for (int r = 0; r < reps; ++r) {
    float* yr = y + (int64_t)r * n;
    for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < n; i += (int64_t)gridDim.x * LT) {
      const Philox4 ph = philox4x32_10((uint32_t)(i >> 1), (uint32_t)r, sid, (uint32_t)(i >> 33), k0, k1);
      const int w = (int)(i & 1) * 2;
      const double u1 = ((double)ph.v[w] + 1.0) * (1.0 / 4294967296.0);
      const double u2 = ((double)ph.v[w + 1] + 1.0) * (1.0 / 4294967296.0);
      const double rad = sqrt(-2.0 * log(u1));
      const float z = (float)(rad * cos(6.283185307179586 * u2));
      yr[i] = perturb1(x[i], z, sigma, clip);
    }
  }
}

template <int W>
__global__ void __launch_bounds__(LT)
ema_step_k(float* __restrict__ ema, const float* __restrict__ p, int64_t n, float alpha, float oma) {
  const int64_t nq = n / W, tail0 = nq * W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    float e[W], a[W];
    VecLd<W>::ld(ema + i * W, e);
    VecLd<W>::ld(p + i * W, a);
#pragma unroll
    for (int j = 0; j < W; ++j) e[j] = fmaf(alpha, e[j], oma * a[j]);
    VecLd<W>::st(ema + i * W, e);
  }
  if (blockIdx.x == 0)
    for (int64_t i = tail0 + threadIdx.x; i < n; i += LT) ema[i] = fmaf(alpha, ema[i], oma * p[i]);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int ssl_shape_check(const char* what, int n, int c, int64_t v) {
  FPLX_REQUIRE(n > 0 && n <= 65535 && c >= 2 && c <= MAXC && v > 0, FPLX_E_BADSHAPE, "%s: n=%d (1..65535) c=%d (2..%d) v=%lld (>= 1)",
               what, n, c, MAXC, (long long)v);
  return FPLX_OK;
}

inline int ssl_t_check(const char* what, int t) {
  FPLX_REQUIRE(t >= 0 && t <= 16 && (t & 1) == 0, FPLX_E_BADSHAPE, "%s: t=%d Monte-Carlo passes (even, 0..16)", what, t);
  return FPLX_OK;
}

// K and C to template arguments; the vector path's width is pyr_width(K, C)
template <int K, int C>
void pyr_launch_fwd(bool vec, dim3 grid, hipStream_t st, const PyrIn& in, int64_t v, float* part) {
  if (vec) ssl_pyramid_fwd_k<K, C, pyr_width(K, C)><<<grid, LT, 0, st>>>(in, v, part);
  else ssl_pyramid_fwd_k<K, C, 1><<<grid, LT, 0, st>>>(in, v, part);
}
template <int K, int C>
void pyr_launch_bwd(bool vec, int n, hipStream_t st, const PyrIn& in, const double* out, const float* gscale, int64_t v,
                    const PyrOut& o) {
  constexpr int W = pyr_width_bwd(K, C);
  if (vec) ssl_pyramid_bwd_k<K, C, W><<<dim3(grid1(v / W, 2048), n), LT, 0, st>>>(in, out, gscale, n, v, o);
  else ssl_pyramid_bwd_k<K, C, 1><<<dim3(grid1(v, 2048), n), LT, 0, st>>>(in, out, gscale, n, v, o);
}
#define PYR_C(K, C, FN, ...)                     \
  switch (C) {                                   \
    case 2: FN<K, 2>(__VA_ARGS__); break;        \
    case 3: FN<K, 3>(__VA_ARGS__); break;        \
    case 4: FN<K, 4>(__VA_ARGS__); break;        \
    case 5: FN<K, 5>(__VA_ARGS__); break;        \
    case 6: FN<K, 6>(__VA_ARGS__); break;        \
    case 7: FN<K, 7>(__VA_ARGS__); break;        \
    default: FN<K, 8>(__VA_ARGS__); break;       \
  }
#define PYR_DISPATCH(K, C, FN, ...)              \
  switch (K) {                                   \
    case 2: PYR_C(2, C, FN, __VA_ARGS__) break;  \
    case 3: PYR_C(3, C, FN, __VA_ARGS__) break;  \
    default: PYR_C(4, C, FN, __VA_ARGS__) break; \
  }

// the table's first k entries -> a by-value struct; refuses a NULL entry; *vec stays true while every base is 16-byte aligned
template <typename S, typename T>
int pyr_table(const char* what, T* const* table, int k, S* s, bool* vec) {
  for (int j = 0; j < PYR_K; ++j) s->p[j] = nullptr;
  for (int j = 0; j < k; ++j) {
    FPLX_REQUIRE(table[j], FPLX_E_NULL, "%s: null tensor %d", what, j);
    s->p[j] = table[j];
    *vec = *vec && aligned16(table[j]);
  }
  return FPLX_OK;
}

}  // namespace

#define SSL_DISPATCH(C, W, KERNEL, ...)              \
  switch (C) {                                       \
    case 2: KERNEL<2, W> __VA_ARGS__; break;         \
    case 3: KERNEL<3, W> __VA_ARGS__; break;         \
    case 4: KERNEL<4, W> __VA_ARGS__; break;         \
    case 5: KERNEL<5, W> __VA_ARGS__; break;         \
    case 6: KERNEL<6, W> __VA_ARGS__; break;         \
    case 7: KERNEL<7, W> __VA_ARGS__; break;         \
    default: KERNEL<8, W> __VA_ARGS__; break;        \
  }
#define SSL_DISPATCH_VEC(vec, C, KERNEL, ...)        \
  do {                                               \
    if (vec) { SSL_DISPATCH(C, 4, KERNEL, __VA_ARGS__) } else { SSL_DISPATCH(C, 1, KERNEL, __VA_ARGS__) } \
  } while (0)

extern "C" {

int fplx_ssl_perturb(const float* x, const float* noise, float* y, int64_t n, int reps, float sigma, float clip, uint64_t seed,
                     uint32_t stream_id, fplx_stream_t stream) {
  FPLX_REQUIRE(x && y, FPLX_E_NULL, "ssl_perturb: null pointer");
  FPLX_REQUIRE(n > 0 && reps >= 1 && reps <= 64, FPLX_E_BADSHAPE, "ssl_perturb: n=%lld (>= 1) reps=%d (1..64)", (long long)n, reps);
  FPLX_REQUIRE(clip >= 0.f, FPLX_E_BADSHAPE, "ssl_perturb: clip=%g is negative", (double)clip);
  hipStream_t st = (hipStream_t)stream;
  if (noise) {
    const bool vec = aligned16(x) && aligned16(noise) && aligned16(y) && (n % 4 == 0 || reps == 1) && n >= 4;
    if (vec) ssl_perturb_k<4><<<grid1(n / 4, 2048), LT, 0, st>>>(x, noise, y, n, reps, sigma, clip);
    else ssl_perturb_k<1><<<grid1(n, 2048), LT, 0, st>>>(x, noise, y, n, reps, sigma, clip);
  } else {
    ssl_perturb_philox_k<<<grid1(n, 2048), LT, 0, st>>>(x, y, n, reps, sigma, clip, (uint32_t)seed, (uint32_t)(seed >> 32),
                                                        stream_id);
  }
  return fplx_check_launch("ssl_perturb");
}

int fplx_ssl_consistency_fwd(const float* student, const float* teacher, const float* mc, int t, int n, int c, int64_t v, float thr,
                             int softmax, uint8_t* mask, float* part, double* out, fplx_stream_t stream) {
  int rc = ssl_shape_check("ssl_consistency_fwd", n, c, v);
  if (rc != FPLX_OK) return rc;
  rc = ssl_t_check("ssl_consistency_fwd", t);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(student && teacher && part && out, FPLX_E_NULL, "ssl_consistency_fwd: null pointer");
  FPLX_REQUIRE(t == 0 || (mc && mask), FPLX_E_NULL, "ssl_consistency_fwd: t=%d needs the Monte-Carlo stack and the mask", t);
  hipStream_t st = (hipStream_t)stream;
  const int rows = loss_rows(v);
  const bool vec = v % 4 == 0 && aligned16(student) && aligned16(teacher) && (t == 0 || (aligned16(mc) && aligned16(mask)));
  dim3 grid(rows, n);
  SSL_DISPATCH_VEC(vec, c, ssl_cons_fwd_k, <<<grid, LT, 0, st>>>(student, teacher, mc, t, n, v, thr, softmax, mask, part));
  ssl_finish_k<<<1, 64, 0, st>>>(part, 2, (int64_t)n * rows, t > 0 ? 1 : 0, (double)n * (double)v, c, out);
  return fplx_check_launch("ssl_consistency_fwd");
}

int fplx_ssl_consistency_bwd(const float* student, const float* teacher, const uint8_t* mask, const double* out,
                             const float* gscale, int n, int c, int64_t v, int t, int softmax, float* dstudent,
                             fplx_stream_t stream) {
  int rc = ssl_shape_check("ssl_consistency_bwd", n, c, v);
  if (rc != FPLX_OK) return rc;
  rc = ssl_t_check("ssl_consistency_bwd", t);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(student && teacher && gscale && dstudent, FPLX_E_NULL, "ssl_consistency_bwd: null pointer");
  FPLX_REQUIRE(t == 0 || (mask && out), FPLX_E_NULL, "ssl_consistency_bwd: t=%d needs the mask and the forward's out", t);
  const bool vec = v % 4 == 0 && aligned16(student) && aligned16(teacher) && aligned16(dstudent) && (t == 0 || aligned16(mask));
  dim3 grid(grid1(vec ? v / 4 : v, 2048), n);
  SSL_DISPATCH_VEC(vec, c, ssl_cons_bwd_k, <<<grid, LT, 0, (hipStream_t)stream>>>(student, teacher, mask, out, gscale, n, v, t,
                                                                                 softmax, dstudent));
  return fplx_check_launch("ssl_consistency_bwd");
}

int fplx_ssl_entropy_fwd(const float* logits, int n, int c, int64_t v, int softmax, float* part, double* out,
                         fplx_stream_t stream) {
  const int rc = ssl_shape_check("ssl_entropy_fwd", n, c, v);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && part && out, FPLX_E_NULL, "ssl_entropy_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int rows = loss_rows(v);
  const bool vec = v % 4 == 0 && aligned16(logits);
  dim3 grid(rows, n);
  SSL_DISPATCH_VEC(vec, c, ssl_ent_fwd_k, <<<grid, LT, 0, st>>>(logits, v, softmax, part));
  ssl_finish_k<<<1, 64, 0, st>>>(part, 1, (int64_t)n * rows, 2, (double)n * (double)v, c, out);
  return fplx_check_launch("ssl_entropy_fwd");
}

int fplx_ssl_entropy_bwd(const float* logits, const float* gscale, int n, int c, int64_t v, int softmax, float* dlogits,
                         fplx_stream_t stream) {
  const int rc = ssl_shape_check("ssl_entropy_bwd", n, c, v);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && gscale && dlogits, FPLX_E_NULL, "ssl_entropy_bwd: null pointer");
  const float coef = (float)(0.999 / (log((double)c) * (double)n * (double)v));
  const bool vec = v % 4 == 0 && aligned16(logits) && aligned16(dlogits);
  dim3 grid(grid1(vec ? v / 4 : v, 2048), n);
  SSL_DISPATCH_VEC(vec, c, ssl_ent_bwd_k, <<<grid, LT, 0, (hipStream_t)stream>>>(logits, gscale, coef, v, softmax, dlogits));
  return fplx_check_launch("ssl_entropy_bwd");
}

int fplx_ssl_pyramid_fwd(const float* const* logits, int k, int n, int c, int64_t v, float* part, double* out,
                         fplx_stream_t stream) {
  FPLX_REQUIRE(k >= 2 && k <= PYR_K, FPLX_E_BADSHAPE, "ssl_pyramid_fwd: k=%d scales (2..%d)", k, PYR_K);
  int rc = ssl_shape_check("ssl_pyramid_fwd", n, c, v);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && part && out, FPLX_E_NULL, "ssl_pyramid_fwd: null pointer");
  PyrIn in;
  bool vec = v % 4 == 0;
  rc = pyr_table("ssl_pyramid_fwd", logits, k, &in, &vec);
  if (rc != FPLX_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int rows = loss_rows(v);
  PYR_DISPATCH(k, c, pyr_launch_fwd, vec, dim3(rows, n), st, in, v, part);
  ssl_pyramid_finish_k<<<1, 64, 0, st>>>(part, k, c, (int64_t)n * rows, (double)n * (double)v, out);
  return fplx_check_launch("ssl_pyramid_fwd");
}

int fplx_ssl_pyramid_bwd(const float* const* logits, const double* out, const float* gscale, int k, int n, int c, int64_t v,
                         float* const* dlogits, fplx_stream_t stream) {
  FPLX_REQUIRE(k >= 2 && k <= PYR_K, FPLX_E_BADSHAPE, "ssl_pyramid_bwd: k=%d scales (2..%d)", k, PYR_K);
  int rc = ssl_shape_check("ssl_pyramid_bwd", n, c, v);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && out && gscale && dlogits, FPLX_E_NULL, "ssl_pyramid_bwd: null pointer");
  PyrIn in;
  PyrOut o;
  bool vec = v % 4 == 0;
  rc = pyr_table("ssl_pyramid_bwd", logits, k, &in, &vec);
  if (rc != FPLX_OK) return rc;
  rc = pyr_table("ssl_pyramid_bwd", dlogits, k, &o, &vec);
  if (rc != FPLX_OK) return rc;
  PYR_DISPATCH(k, c, pyr_launch_bwd, vec, n, (hipStream_t)stream, in, out, gscale, v, o);
  return fplx_check_launch("ssl_pyramid_bwd");
}

int fplx_ssl_pseudo_onehot(const float* const* logits, int k, int n, int c, int64_t v, float* const* onehot, fplx_stream_t stream) {
  FPLX_REQUIRE(k >= 1 && k < PYR_K, FPLX_E_BADSHAPE, "ssl_pseudo_onehot: k=%d tensors (1..%d)", k, PYR_K - 1);
  int rc = ssl_shape_check("ssl_pseudo_onehot", n, c, v);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && onehot, FPLX_E_NULL, "ssl_pseudo_onehot: null pointer");
  PyrIn in;
  PyrOut o;
  bool vec = v % 4 == 0;
  rc = pyr_table("ssl_pseudo_onehot", logits, k, &in, &vec);
  if (rc != FPLX_OK) return rc;
  rc = pyr_table("ssl_pseudo_onehot", onehot, k, &o, &vec);
  if (rc != FPLX_OK) return rc;
  dim3 grid(grid1(vec ? v / 4 : v, 2048), n);
  SSL_DISPATCH_VEC(vec, c, ssl_pseudo_onehot_k, <<<grid, LT, 0, (hipStream_t)stream>>>(in, k, v, o));
  return fplx_check_launch("ssl_pseudo_onehot");
}

int fplx_ema_step(float* ema, const float* p, int64_t n, float alpha, fplx_stream_t stream) {
  FPLX_REQUIRE(ema && p, FPLX_E_NULL, "ema_step: null pointer");
  FPLX_REQUIRE(n > 0, FPLX_E_BADSHAPE, "ema_step: n=%lld (>= 1)", (long long)n);
  FPLX_REQUIRE(alpha >= 0.f && alpha <= 1.f, FPLX_E_BADSHAPE, "ema_step: alpha=%g outside [0, 1]", (double)alpha);
  const float oma = (float)(1.0 - (double)alpha);      // formed in double, rounded once
  const bool vec = aligned16(ema) && aligned16(p) && n >= 4;
  if (vec) ema_step_k<4><<<grid1(n / 4, 2048), LT, 0, (hipStream_t)stream>>>(ema, p, n, alpha, oma);
  else ema_step_k<1><<<grid1(n, 2048), LT, 0, (hipStream_t)stream>>>(ema, p, n, alpha, oma);
  return fplx_check_launch("ema_step");
}

}  // extern "C"
