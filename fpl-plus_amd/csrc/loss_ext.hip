// Second family of segmentation losses (FocalDice, NoiseRobustDice, ExpLog, GeneralizedCE, MAE, MSE, SLSR) fused with the
// first one (loss_filter.hip): one forward pass makes the 6C + 3 sums of seg_loss_fwd_k - same arithmetic, same positions - and
// 4C + 4 new ones, one finalize thread turns the totals into values and a coefficient table, one backward pass writes dlogits for
// any mixture of the eleven terms.  Which terms run is a bit mask in the kernel arguments: wave-uniform branches, so the powf /
// logf work of a term that was not asked for is never issued.  Layouts: include/fplx.h, "segmentation loss, second family".
// Shared with loss_filter.hip through loss_common.h: dispatch, checks, the sums region, seg_loss_sums_k, the first family's
// finalize, and of the backward voxel loop seg_loss_base_grad and seg_loss_ent_grad.  The forward voxel loop and the rest of
// the backward one are two copies on purpose: a shared device function there stays only if every instantiation that uses it keeps its
// text or its counts of fused multiply-adds, multiplies and adds (-ffp-contract=fast fuses after inlining).
#include "loss_common.h"

namespace {

enum : int {
  T_DICE = 1 << 0, T_CE = 1 << 1, T_ENT = 1 << 2, T_FOCAL = 1 << 3, T_NR = 1 << 4, T_EXPLOG = 1 << 5, T_GCE = 1 << 6,
  T_MAE = 1 << 7, T_MSE = 1 << 8, T_SLSR = 1 << 9, T_GCE_PW = 1 << 10
};

// host cfg[] positions (include/fplx.h)
enum : int { CF_DICE = 0, CF_CE, CF_IMG, CF_ENT, CF_FOCAL, CF_NR, CF_EXPLOG, CF_GCE, CF_MAE, CF_MSE, CF_SLSR, CF_BETA, CF_GNR,
             CF_ELW, CF_GEL, CF_Q, CF_EPS, CF_USEPW, CF_CW };

// what the voxel loops need of cfg (kernel argument, by value)
struct ExtArgs {
  int flags;
  float gnr, gel, q, eps;     // gamma of NoiseRobustDice and of ExpLog, q of GeneralizedCE, epsilon of SLSR
  float cw[MAXC];             // class weights of GeneralizedCE
};

// the whole cfg for the one-thread finalize
struct ExtCfg { float f[CF_CW + MAXC]; };

inline ExtArgs ext_args(const float* cfg, int c) {
  ExtArgs a;
  int f = 0;
  if (cfg[CF_DICE] != 0.f || cfg[CF_IMG] != 0.f) f |= T_DICE;
  if (cfg[CF_CE] != 0.f) f |= T_CE;
  if (cfg[CF_ENT] != 0.f) f |= T_ENT;
  if (cfg[CF_FOCAL] != 0.f) f |= T_FOCAL;
  if (cfg[CF_NR] != 0.f) f |= T_NR;
  if (cfg[CF_EXPLOG] != 0.f) f |= T_EXPLOG;
  if (cfg[CF_GCE] != 0.f) f |= T_GCE;
  if (cfg[CF_MAE] != 0.f) f |= T_MAE;
  if (cfg[CF_MSE] != 0.f) f |= T_MSE;
  if (cfg[CF_SLSR] != 0.f) f |= T_SLSR;
  if (cfg[CF_GCE] != 0.f && cfg[CF_USEPW] != 0.f) f |= T_GCE_PW;
  a.flags = f;
  a.gnr = cfg[CF_GNR]; a.gel = cfg[CF_GEL]; a.q = cfg[CF_Q]; a.eps = cfg[CF_EPS];
  for (int k = 0; k < MAXC; ++k) a.cw[k] = k < c ? cfg[CF_CW + k] : 0.f;
  return a;
}

__device__ __forceinline__ float sign0(float d) { return (float)(d > 0.f) - (float)(d < 0.f); }     // torch.sign: 0 at 0

// the label SLSR takes: smoothed towards 1/2 where the mask is set (slsr.py:46-49)
__device__ __forceinline__ float slsr_label(float y, bool masked, float eps) {
  return masked ? (y - 0.5f) * (0.5f - eps) / 0.5f + 0.5f : y;
}

// part[n][row][10C+7]: the 6C + 3 entries of seg_loss_fwd_k, then per class (P, I unweighted, sum |p - y|^gamma, sum y L^gamma),
// then the GeneralizedCE numerator, sum (p - y)^2, sum |p - y|, the SLSR numerator
template <int C>
__global__ void __launch_bounds__(LT)
seg_loss_ext_fwd_k(const float* __restrict__ logits, const float* __restrict__ label, const float* __restrict__ pw,
                   int64_t V, int do_softmax, ExtArgs a, float* __restrict__ part) {
  constexpr int K0 = 6 * C + 3, K = 10 * C + 7, S0 = 10 * C + 3;
  const int n = blockIdx.y;
  const float* lg = logits + (int64_t)n * C * V;
  const float* lb = label + (int64_t)n * C * V;
  const float* wp = pw ? pw + (int64_t)n * V : nullptr;
  const int fl = a.flags;
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.f;
  for (int64_t v = (int64_t)blockIdx.x * LT + threadIdx.x; v < V; v += (int64_t)gridDim.x * LT) {
    float l[MAXC], p[MAXC], y[MAXC];
#pragma unroll
    for (int c = 0; c < C; ++c) { l[c] = lg[(int64_t)c * V + v]; y[c] = lb[(int64_t)c * V + v]; }
    const float w = wp ? wp[v] : 1.f;
    int am = 0;
    {
      float best = l[0];
#pragma unroll
      for (int c = 1; c < C; ++c)
        if (l[c] > best) { best = l[c]; am = c; }
    }
    softmax_argmax<C>(l, p, do_softmax != 0);
    float ce = 0.f, ent = 0.f;
    // the first 6C + 3 sums are seg_loss_fwd_k's lines (loss_filter.hip): two copies under the rule above
#pragma unroll
    for (int c = 0; c < C; ++c) {
      acc[6 * c + 0] += y[c] * w;
      acc[6 * c + 1] += p[c] * w;
      acc[6 * c + 2] += y[c] * p[c] * w;
      const float hc = (am == c) ? 1.f : 0.f;
      acc[6 * c + 3] += y[c];
      acc[6 * c + 4] += hc;
      acc[6 * c + 5] += y[c] * hc;
      acc[K0 + 4 * c + 0] += p[c];
      acc[K0 + 4 * c + 1] += y[c] * p[c];
    }
    // the CE numerator and the entropy sum are part of every pass: seg_loss_fwd_k's lines, its twin under the rule above
    float q[MAXC];
    if (do_softmax) {
#pragma unroll
      for (int c = 0; c < C; ++c) q[c] = p[c];
    } else {
      softmax_argmax<C>(l, q, true);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      ce -= y[c] * logf(p[c] * 0.999f + 5e-4f);
      ent -= q[c] * log2f(q[c] + 1e-10f);
    }
    acc[6 * C + 0] += w * ce;
    acc[6 * C + 1] += w;
    acc[6 * C + 2] += ent;
    if (fl & (T_MSE | T_MAE)) {
      float s2 = 0.f, s1 = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) { const float d = p[c] - y[c]; s2 += d * d; s1 += fabsf(d); }
      acc[S0 + 1] += s2;
      acc[S0 + 2] += s1;
    }
    if (fl & T_NR) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[K0 + 4 * c + 2] += powf(fabsf(p[c] - y[c]), a.gnr);
    }
    if (fl & T_EXPLOG) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[K0 + 4 * c + 3] += y[c] * powf(-logf(0.005f + p[c] * 0.99f), a.gel);
    }
    if (fl & T_GCE) {
      float g = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) g += (1.0f - powf(p[c], a.q)) / a.q * y[c] * a.cw[c];
      acc[S0 + 0] += (fl & T_GCE_PW) ? g * w : g;
    }
    if (fl & T_SLSR) {
      const bool masked = wp && w > 0.f;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) s -= slsr_label(y[c], masked, a.eps) * logf(p[c] * 0.999f + 5e-4f);
      acc[S0 + 3] += s;
    }
  }
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
    part[((int64_t)n * gridDim.x + blockIdx.x) * K + threadIdx.x] = t;
  }
}

// one thread: values and the backward coefficient table.  The first family's part is seg_loss_base_finalize (loss_common.h),
// as in seg_loss_coef_k.  coef: [N][C][2] (A, B of the pixel-weighted Dice terms), cce, cent; then per class (Au, Bu: the unweighted
// Dice-type terms as Au y + Bu, cnr, cel); then cgce, 2 cmse, cmae, cslsr.
__global__ void seg_loss_ext_coef_k(const double* __restrict__ sums, const double* __restrict__ tot, int N, int NG, int C,
                                    double V, int has_pw, const float* __restrict__ image_weight, ExtCfg cf,
                                    float* __restrict__ out, float* __restrict__ coef) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int K = 10 * C + 7, K0 = 6 * C + 3, S0 = 10 * C + 3;
  const double M = NG * V;
  float* ce2 = coef + N * C * 2;
  double total = seg_loss_base_finalize(sums, tot, N, NG, C, K, V, has_pw, image_weight, cf.f[CF_DICE], cf.f[CF_CE], cf.f[CF_IMG],
                                        cf.f[CF_ENT], out, coef);
  const double wsum = tot[6 * C + 1];
  // ---- second family
  const double w_focal = cf.f[CF_FOCAL], w_nr = cf.f[CF_NR], w_el = cf.f[CF_EXPLOG], w_gce = cf.f[CF_GCE], w_mae = cf.f[CF_MAE],
               w_mse = cf.f[CF_MSE], w_slsr = cf.f[CF_SLSR];
  const double beta = cf.f[CF_BETA], gnr = cf.f[CF_GNR], elw = cf.f[CF_ELW], gel = cf.f[CF_GEL];
  float* cc = ce2 + 2;
  double Lf = 0.0, Lnr = 0.0, Leld = 0.0, Lelc = 0.0;
  for (int c = 0; c < C; ++c) {
    const double Y = tot[6 * c + 3], P = tot[K0 + 4 * c + 0], I = tot[K0 + 4 * c + 1], NR = tot[K0 + 4 * c + 2],
                 E = tot[K0 + 4 * c + 3];
    const double den = Y + P + 1e-5, num = 2.0 * I + 1e-5, dice = num / den;      // util.py:97-106 without pix_w
    double Au = 0.0, Bu = 0.0, cnr = 0.0, cel = 0.0;
    if (w_focal != 0.0) {                                                           // dice.py:158-160
      Lf += pow(dice, 1.0 / beta);
      const double k = w_focal / (C * beta) * pow(dice, 1.0 / beta - 1.0);
      Au += k * (-2.0 / den);
      Bu += k * (num / (den * den));
    }
    if (w_nr != 0.0) {                                                              // dice.py:192-198
      Lnr += NR / den;
      cnr = w_nr * gnr / (C * den);
      Bu -= w_nr * NR / (C * den * den);
    }
    if (w_el != 0.0) {                                                              // exp_log.py:40-53
      const double s = 0.005 + dice * 0.99, ls = -log(s);
      Leld += pow(ls, gel);
      const double k = w_el * elw / C * gel * pow(ls, gel - 1.0) * 0.99 / s;
      Au += k * (-2.0 / den);
      Bu += k * (num / (den * den));
      const double wc = pow(1.0 / (Y / M + 0.1), 0.5);
      Lelc += wc * E;
      cel = w_el * (1.0 - elw) * wc / M * gel;
    }
    cc[4 * c + 0] = (float)Au;
    cc[4 * c + 1] = (float)Bu;
    cc[4 * c + 2] = (float)cnr;
    cc[4 * c + 3] = (float)cel;
  }
  Lf = 1.0 - Lf / C;
  Lnr = Lnr / C;
  const double Lel = Leld / C * elw + Lelc / M * (1.0 - elw);
  const double gce_norm = (cf.f[CF_USEPW] != 0.f && w_gce != 0.0) ? 1.0 / wsum : 1.0 / M;      // ce.py:85-92 as documented
  const double Lgce = tot[S0 + 0] * gce_norm;
  const double Lmse = tot[S0 + 1] / (M * C), Lmae = tot[S0 + 2] / (M * C), Lsl = tot[S0 + 3] / M;
  float* cs = cc + 4 * C;
  cs[0] = (float)(w_gce * gce_norm);
  cs[1] = (float)(2.0 * w_mse / (M * C));
  cs[2] = (float)(w_mae / (M * C));
  cs[3] = (float)(w_slsr / M);
  float* oe = out + 4 + C;
  oe[0] = oe[1] = oe[2] = oe[3] = oe[4] = oe[5] = oe[6] = 0.f;
  if (w_focal != 0.0) { total += w_focal * Lf; oe[0] = (float)Lf; }
  if (w_nr != 0.0) { total += w_nr * Lnr; oe[1] = (float)Lnr; }
  if (w_el != 0.0) { total += w_el * Lel; oe[2] = (float)Lel; }
  if (w_gce != 0.0) { total += w_gce * Lgce; oe[3] = (float)Lgce; }
  if (w_mae != 0.0) { total += w_mae * Lmae; oe[4] = (float)Lmae; }
  if (w_mse != 0.0) { total += w_mse * Lmse; oe[5] = (float)Lmse; }
  if (w_slsr != 0.0) { total += w_slsr * Lsl; oe[6] = (float)Lsl; }
  out[0] = (float)total;
}

template <int C>
__global__ void __launch_bounds__(LT)
seg_loss_ext_bwd_k(const float* __restrict__ logits, const float* __restrict__ label, const float* __restrict__ pw,
                   const float* __restrict__ coef, const float* __restrict__ gscale, int N, int64_t V, int do_softmax,
                   ExtArgs a, float* __restrict__ dlogits) {
  const int n = blockIdx.y;
  const float* lg = logits + (int64_t)n * C * V;
  const float* lb = label + (int64_t)n * C * V;
  const float* wp = pw ? pw + (int64_t)n * V : nullptr;
  float* dl = dlogits + (int64_t)n * C * V;
  const int fl = a.flags;
  const bool use_dice = fl & T_DICE, use_ce = fl & T_CE, use_ent = fl & T_ENT;
  const bool use_u = fl & (T_FOCAL | T_NR | T_EXPLOG), use_d = fl & (T_NR | T_MSE | T_MAE);
  float A[MAXC], B[MAXC], Au[MAXC], Bu[MAXC], cnr[MAXC], cel[MAXC];
  const float* ce2 = coef + N * C * 2;
  const float* cc = ce2 + 2;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    A[c] = coef[(n * C + c) * 2]; B[c] = coef[(n * C + c) * 2 + 1];
    Au[c] = cc[4 * c]; Bu[c] = cc[4 * c + 1]; cnr[c] = cc[4 * c + 2]; cel[c] = cc[4 * c + 3];
  }
  const float cce = ce2[0], cent = ce2[1], gs = *gscale;
  const float cgce = cc[4 * C + 0], cmse2 = cc[4 * C + 1], cmae = cc[4 * C + 2], cslsr = cc[4 * C + 3];
  const float gnr1 = a.gnr - 1.0f, gel1 = a.gel - 1.0f, q1 = a.q - 1.0f;
  for (int64_t v = (int64_t)blockIdx.x * LT + threadIdx.x; v < V; v += (int64_t)gridDim.x * LT) {
    float l[MAXC], p[MAXC], g[MAXC];
#pragma unroll
    for (int c = 0; c < C; ++c) l[c] = lg[(int64_t)c * V + v];
    const float w = wp ? wp[v] : 1.f;
    const float wg = (fl & T_GCE_PW) ? w : 1.f;
    const bool masked = wp && w > 0.f;
    softmax_argmax<C>(l, p, do_softmax != 0);
    // without loss_softmax every term but the entropy one sends its gradient to the outputs directly (the Jacobian below is
    // seg_loss_bwd_k's, its twin under the rule above)
    const bool ent_own = use_ent && !do_softmax;
    float q[MAXC], ge[MAXC], dote = 0.f;
    if (ent_own) softmax_argmax<C>(l, q, true);
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float y = lb[(int64_t)c * V + v];
      float gc = seg_loss_base_grad(use_dice, use_ce, use_ent && do_softmax, w, A[c], B[c], cce, cent, y, p[c]);
      if (ent_own) {
        ge[c] = seg_loss_ent_grad(cent, q[c]);
        dote = fmaf(ge[c], q[c], dote);
      }
      if (use_u) gc += fmaf(Au[c], y, Bu[c]);
      if (use_d) {
        const float d = p[c] - y, sg = sign0(d);
        if (fl & T_NR) gc += cnr[c] * powf(fabsf(d), gnr1) * sg;
        if (fl & T_MSE) gc += cmse2 * d;
        if (fl & T_MAE) gc += cmae * sg;
      }
      if (fl & T_EXPLOG) {
        const float s = 0.005f + p[c] * 0.99f;
        gc -= cel[c] * y * powf(-logf(s), gel1) * 0.99f / s;
      }
      if (fl & T_GCE) gc -= cgce * wg * a.cw[c] * y * powf(p[c], q1);
      if (fl & T_SLSR) gc -= cslsr * slsr_label(y, masked, a.eps) * 0.999f / (p[c] * 0.999f + 5e-4f);
      g[c] = gc;
      dot = fmaf(gc, p[c], dot);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float d = do_softmax ? p[c] * (g[c] - dot) : g[c];
      if (ent_own) d += q[c] * (ge[c] - dote);
      dl[(int64_t)c * V + v] = gs * d;
    }
  }
}

int ext_check(const char* what, int n, int c, int64_t v, const float* cfg) {
  const int rc = loss_shape_check(what, n, c, v);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(cfg, FPLX_E_NULL, "%s: null cfg", what);
  return FPLX_OK;
}

}  // namespace

extern "C" {

int fplx_seg_loss_ext_sums(const float* logits, const float* label, const float* pixel_weight, int n, int c, int64_t v,
                           const float* cfg, int softmax, float* part, double* sums, double* totals, fplx_stream_t stream) {
  const int rc = ext_check("seg_loss_ext_sums", n, c, v, cfg);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && label && part && sums && totals, FPLX_E_NULL, "seg_loss_ext_sums: null pointer");
  const ExtArgs a = ext_args(cfg, c);
  FPLX_REQUIRE(!(a.flags & T_GCE_PW) || pixel_weight, FPLX_E_NULL, "seg_loss_ext_sums: use_pixel_weight without pixel_weight");
  hipStream_t st = (hipStream_t)stream;
  const int rows = loss_rows(v);
  dim3 grid(rows, n);
  DISPATCH_C(c, seg_loss_ext_fwd_k, <<<grid, LT, 0, st>>>(logits, label, pixel_weight, v, softmax, a, part));
  seg_loss_sums_k<<<1, 1024, 0, st>>>(part, rows, n, FPLX_LOSS_EXT_K(c), sums, totals);
  return fplx_check_launch("seg_loss_ext_sums");
}

int fplx_seg_loss_ext_from_sums(const double* sums, const double* totals, const float* image_weight, int n, int n_global, int c,
                                int64_t v, int has_pixel_weight, const float* cfg, float* out, float* coef,
                                fplx_stream_t stream) {
  const int rc = ext_check("seg_loss_ext_from_sums", n, c, v, cfg);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(sums && totals && out && coef, FPLX_E_NULL, "seg_loss_ext_from_sums: null pointer");
  FPLX_REQUIRE(n_global >= n, FPLX_E_BADSHAPE, "seg_loss_ext_from_sums: n_global=%d < n=%d", n_global, n);
  FPLX_REQUIRE(cfg[CF_IMG] == 0.f || (image_weight && has_pixel_weight), FPLX_E_NULL,
               "seg_loss_ext_from_sums: image-weighted Dice needs image_weight and pixel_weight");
  FPLX_REQUIRE(cfg[CF_GCE] == 0.f || cfg[CF_USEPW] == 0.f || has_pixel_weight, FPLX_E_NULL,
               "seg_loss_ext_from_sums: use_pixel_weight without pixel_weight");
  ExtCfg cf;
  for (int k = 0; k < CF_CW + MAXC; ++k) cf.f[k] = k < CF_CW + c ? cfg[k] : 0.f;
  seg_loss_ext_coef_k<<<1, 64, 0, (hipStream_t)stream>>>(sums, totals, n, n_global, c, (double)v, has_pixel_weight, image_weight,
                                                         cf, out, coef);
  return fplx_check_launch("seg_loss_ext_from_sums");
}

int fplx_seg_loss_ext_fwd(const float* logits, const float* label, const float* pixel_weight, const float* image_weight, int n,
                          int c, int64_t v, const float* cfg, int softmax, float* part, float* out, float* coef,
                          fplx_stream_t stream) {
  int rc = ext_check("seg_loss_ext_fwd", n, c, v, cfg);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && label && part && out && coef, FPLX_E_NULL, "seg_loss_ext_fwd: null pointer");
  FPLX_REQUIRE(cfg[CF_IMG] == 0.f || (image_weight && pixel_weight), FPLX_E_NULL,
               "seg_loss_ext_fwd: image-weighted Dice needs image_weight and pixel_weight");
  const LossSums s = loss_sums_region(part, n, loss_rows(v), FPLX_LOSS_EXT_K(c));
  rc = fplx_seg_loss_ext_sums(logits, label, pixel_weight, n, c, v, cfg, softmax, part, s.sums, s.totals, stream);
  if (rc != FPLX_OK) return rc;
  return fplx_seg_loss_ext_from_sums(s.sums, s.totals, image_weight, n, n, c, v, pixel_weight != nullptr, cfg, out, coef, stream);
}

int fplx_seg_loss_ext_bwd(const float* logits, const float* label, const float* pixel_weight, const float* coef,
                          const float* gscale, int n, int c, int64_t v, const float* cfg, int softmax, float* dlogits,
                          fplx_stream_t stream) {
  const int rc = ext_check("seg_loss_ext_bwd", n, c, v, cfg);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && label && coef && gscale && dlogits, FPLX_E_NULL, "seg_loss_ext_bwd: null pointer");
  const ExtArgs a = ext_args(cfg, c);
  FPLX_REQUIRE(!(a.flags & T_GCE_PW) || pixel_weight, FPLX_E_NULL, "seg_loss_ext_bwd: use_pixel_weight without pixel_weight");
  dim3 grid(grid1(v, 2048), n);
  DISPATCH_C(c, seg_loss_ext_bwd_k, <<<grid, LT, 0, (hipStream_t)stream>>>(logits, label, pixel_weight, coef, gscale, n, v,
                                                                           softmax, a, dlogits));
  return fplx_check_launch("seg_loss_ext_bwd");
}

}  // extern "C"
