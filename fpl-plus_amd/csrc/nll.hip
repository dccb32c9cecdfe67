// Noisy-label learning, the reference's fourth entry point (PyMIC/pymic/net_run_nll/nll_co_teaching.py:91-118, nll_trinet.py:66-120):
// the per-voxel cross entropy of up to three networks against one soft label, the selection of the small-loss voxels from the
// order statistics fplx_select_kth (intensity.hip) returns - no sort, no host round trip - and the means over the sets the OTHER
// network(s) chose, forward and backward.  Layouts and formulas: include/fplx.h, "noisy-label learning".
// Conventions of ssl.hip: a lane takes 4 consecutive voxels with 16-byte accesses where every base is 16-byte aligned and V is a
// multiple of 4, else one voxel; reductions are fp32 block partials summed in double in a fixed order by one wave; counts are
// integers; no floating-point atomics - two runs give the same bits.
// Compiled with -ffp-contract=off (Makefile): 0.999 p + 5e-4 is torch's product and sum, torch's lerp is a product and a sum, and
// no partial sum depends on what the compiler fuses; the fused multiply-adds that are meant are written as fmaf.
#include "loss_common.h"
#include "gfx950.h"

namespace {

constexpr int NLL_K = 3;                       // networks per call (CoTeaching 2, TriNet 3)
constexpr int NLL_BLOCKS = 1024;               // blocks of the flat passes over the N V losses
constexpr int64_t NLL_MAX_N = (int64_t)1 << 31;    // the bound of fplx_select_kth

struct NllIn { const float* p[NLL_K]; };
struct NllOut { float* p[NLL_K]; };
struct NllMask { const uint8_t* p[NLL_K]; };
struct NllUses { int u[NLL_K]; };

// ---- per-voxel cross entropy of K logit tensors against ONE label: loss_k [N V] and part [K][N][rows] (the block sums)
template <int C, int W>
__global__ void __launch_bounds__(LT)
nll_ce_fwd_k(NllIn lg, int K, const float* __restrict__ label, int64_t V, NllOut loss, float* __restrict__ part) {
  __shared__ float red[LT / 64][NLL_K];
  const int n = blockIdx.y;
  const float* yg = label + (int64_t)n * C * V;
  float acc[NLL_K] = {0.f, 0.f, 0.f};
  const int64_t nq = V / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    const int64_t v = i * W;
    float y[W][MAXC];
    load_voxels<C, W>(yg, V, v, y);
#pragma unroll
    for (int k = 0; k < NLL_K; ++k) {
      if (k < K) {
        float l[W][MAXC], ls[W];
        load_voxels<C, W>(lg.p[k] + (int64_t)n * C * V, V, v, l);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          float p[MAXC];
          softmax_argmax<C>(l[j], p, true);
          float s = 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) s += -y[j][c] * logf(p[c] * 0.999f + 5e-4f);     // - y_2d * log(prob_2d), summed over dim 1
          ls[j] = s;
          acc[k] += s;
        }
        VecLd<W>::st(loss.p[k] + (int64_t)n * V + v, ls);
      }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NLL_K; ++k) {
    const float t = wave_sum(acc[k]);
    if (lane == 0) red[wv][k] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    float t = 0.f;
    for (int i = 0; i < LT / 64; ++i) t += red[i][threadIdx.x];
    part[((int64_t)threadIdx.x * gridDim.y + n) * gridDim.x + blockIdx.x] = t;
  }
}

// ---- selection masks.  Every block owns the contiguous chunk [b chunk, (b + 1) chunk) of the array in all three passes.
// ws words: less[G] | eq[G] | eq_before[G] | total less
__device__ __forceinline__ uint32_t block_usum(uint32_t v, uint32_t* red) {        // the sum in every thread; red: LT / 64 words
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
  for (int i = 0; i < LT / 64; ++i) t += red[i];
  return t;
}

__global__ void __launch_bounds__(LT)
nll_rank_count_k(const float* __restrict__ loss, int64_t n, int64_t chunk, const float* __restrict__ sk, uint32_t* __restrict__ ws) {
  __shared__ uint32_t red[LT / 64];
  const uint32_t tk = key_nan_high(sk[0]);
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  uint32_t less = 0, eq = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += LT) {
    const uint32_t k = key_nan_high(loss[i]);
    less += k < tk;
    eq += k == tk;
  }
  less = block_usum(less, red);
  eq = block_usum(eq, red);
  if (threadIdx.x == 0) { ws[blockIdx.x] = less; ws[gridDim.x + blockIdx.x] = eq; }
}

// one block: the exclusive prefix of eq[] over the blocks and the total of less[]; G <= NLL_BLOCKS = 4 LT
__global__ void __launch_bounds__(LT)
nll_rank_scan_k(uint32_t* __restrict__ ws, int G) {
  __shared__ uint32_t sc[LT];
  __shared__ uint32_t red[LT / 64];
  constexpr int PER = NLL_BLOCKS / LT;
  uint32_t e[PER], own = 0, less = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int b = threadIdx.x * PER + j;
    e[j] = b < G ? ws[G + b] : 0u;
    own += e[j];
    less += b < G ? ws[b] : 0u;
  }
  sc[threadIdx.x] = own;
  __syncthreads();
  for (int o = 1; o < LT; o <<= 1) {                                   // inclusive scan over the threads' sums
    const uint32_t t = (int)threadIdx.x >= o ? sc[threadIdx.x - o] : 0u;
    __syncthreads();
    sc[threadIdx.x] += t;
    __syncthreads();
  }
  uint32_t run = sc[threadIdx.x] - own;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int b = threadIdx.x * PER + j;
    if (b < G) ws[2 * G + b] = run;
    run += e[j];
  }
  less = block_usum(less, red);
  if (threadIdx.x == 0) ws[3 * G] = less;
}

// kept: key < t, and of the voxels with key == t the first num_remb - #less in index order (a stable ascending argsort's
// first num_remb entries).  A chunk with no voxel at t skips the ranking.
__global__ void __launch_bounds__(LT)
nll_rank_write_k(const float* __restrict__ loss, int64_t n, int64_t chunk, const float* __restrict__ sk, int64_t num_remb,
                 const uint32_t* __restrict__ ws, uint8_t* __restrict__ mask) {
  __shared__ uint32_t wtot[2][LT / 64];
  const int G = gridDim.x;
  const uint32_t tk = key_nan_high(sk[0]);
  const int64_t need = num_remb - (int64_t)ws[3 * G];                   // how many of the voxels at t are taken
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  if (ws[G + blockIdx.x] == 0u) {
    for (int64_t i = lo + threadIdx.x; i < hi; i += LT) mask[i] = key_nan_high(loss[i]) < tk ? 1 : 0;
    return;
  }
  int64_t run = (int64_t)ws[2 * G + blockIdx.x];                        // voxels at t in the chunks before this one
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int buf = 0;
  for (int64_t base = lo; base < hi; base += LT, buf ^= 1) {            // uniform over the block: hi - lo is the same for all
    const int64_t i = base + threadIdx.x;
    const bool valid = i < hi;
    const uint32_t k = valid ? key_nan_high(loss[i]) : 0u;
    const bool eq = valid && k == tk;
    const unsigned long long b = __ballot(eq);
    if (lane == 0) wtot[buf][wv] = (uint32_t)__popcll(b);
    __syncthreads();                                                    // the other buffer is rewritten only after the next barrier
    int64_t rank = run + __popcll(b & ((1ull << lane) - 1ull));
    uint32_t tile = 0;
    for (int w = 0; w < LT / 64; ++w) {
      const uint32_t t = wtot[buf][w];
      if (w < wv) rank += t;
      tile += t;
    }
    if (valid) mask[i] = (k < tk || (eq && rank < need)) ? 1 : 0;
    run += tile;
  }
}

// torch.quantile's interpolation (lerp of s[k] and s[ceil(pos)], all fp32), then `loss < threshold` as fp32 values
__global__ void __launch_bounds__(LT)
nll_below_k(const float* __restrict__ loss, int64_t n, const float* __restrict__ sk, const float* __restrict__ smax, float w,
            uint8_t* __restrict__ mask) {
  const float a = sk[0], b = w == 0.f ? a : sk[1];                      // w = 0: ceil(pos) = k, the pair is (s[k], s[k])
  const float d = b - a;
  float thr = w < 0.5f ? a + w * d : b - d * (1.0f - w);
  if (smax && *smax != *smax) thr = *smax;                              // a NaN anywhere: torch.quantile returns NaN
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < n; i += (int64_t)gridDim.x * LT) mask[i] = loss[i] < thr ? 1 : 0;
}

// ---- selected means.  ws: ticket | 3 pad words | fp32 sums [K][G] | uint32 counts [K][G].  The block that draws the last
// ticket sums the rows in double, lanes striding over them in a fixed order, and writes out [K][4].
template <int W>
__device__ __forceinline__ void nll_take(const NllIn& loss, const NllMask& mask, const NllUses& uses, int K, int64_t i,
                                         float (&acc)[NLL_K], uint32_t (&cnt)[NLL_K]) {
  uint32_t bits[W];
#pragma unroll
  for (int j = 0; j < W; ++j) bits[j] = 0u;
#pragma unroll
  for (int k = 0; k < NLL_K; ++k) {
    if (k < K) {
      uint32_t m = W == 4 ? *reinterpret_cast<const uint32_t*>(mask.p[k] + i) : (uint32_t)mask.p[k][i];
#pragma unroll
      for (int j = 0; j < W; ++j) bits[j] |= ((m >> (8 * j)) & 0xFFu) ? (1u << k) : 0u;
    }
  }
#pragma unroll
  for (int k = 0; k < NLL_K; ++k) {
    if (k < K) {
      float l[W];
      VecLd<W>::ld(loss.p[k] + i, l);
#pragma unroll
      for (int j = 0; j < W; ++j)
        if ((bits[j] & (uint32_t)uses.u[k]) == (uint32_t)uses.u[k]) { acc[k] += l[j]; cnt[k] += 1u; }
    }
  }
}

template <int W>
__global__ void __launch_bounds__(LT)
nll_select_fwd_k(NllIn loss, NllMask mask, NllUses uses, int K, int64_t n, const float* __restrict__ ce_part, int64_t ce_rows,
                 uint32_t* __restrict__ ws, double* __restrict__ out) {
  __shared__ uint32_t red[LT / 64][2 * NLL_K + 1];                      // the block's one LDS object: sums, counts, "I am last"
  const int G = gridDim.x;
  float* psum = reinterpret_cast<float*>(ws + 4);
  uint32_t* pcnt = ws + 4 + NLL_K * G;
  float acc[NLL_K] = {0.f, 0.f, 0.f};
  uint32_t cnt[NLL_K] = {0u, 0u, 0u};
  const int64_t nq = n / W, tail0 = nq * W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)G * LT) nll_take<W>(loss, mask, uses, K, i * W, acc, cnt);
  if (W > 1 && blockIdx.x == 0)
    for (int64_t i = tail0 + threadIdx.x; i < n; i += LT) nll_take<1>(loss, mask, uses, K, i, acc, cnt);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NLL_K; ++k) {
    const float s = wave_sum(acc[k]);
    uint32_t c = cnt[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
    if (lane == 0) { red[wv][k] = __float_as_uint(s); red[wv][NLL_K + k] = c; }
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    float s = 0.f;
    uint32_t c = 0u;
    for (int i = 0; i < LT / 64; ++i) { s += __uint_as_float(red[i][threadIdx.x]); c += red[i][NLL_K + threadIdx.x]; }
    psum[(int64_t)threadIdx.x * G + blockIdx.x] = s;
    pcnt[(int64_t)threadIdx.x * G + blockIdx.x] = c;
  }
  // publish the rows, draw a ticket: agent-scope release before the relaxed add, agent-scope acquire in the last block
  wait_vmcnt0();
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    wait_vmcnt0();
    const uint32_t t = __hip_atomic_fetch_add(ws, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = t == (uint32_t)G - 1u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      wait_vmcnt0();
    }
    red[0][2 * NLL_K] = last ? 1u : 0u;
  }
  __syncthreads();
  if (red[0][2 * NLL_K] == 0u || wv != 0) return;
  for (int k = 0; k < K; ++k) {
    double s = 0.0, all = 0.0;
    unsigned long long c = 0ull;
    for (int r = lane; r < G; r += 64) { s += (double)psum[(int64_t)k * G + r]; c += pcnt[(int64_t)k * G + r]; }
    for (int64_t r = lane; r < ce_rows; r += 64) all += (double)ce_part[(int64_t)k * ce_rows + r];
    s = wave_sum_d(s);
    all = wave_sum_d(all);
    double cd = wave_sum_d((double)c);                                   // exact: fewer than 2^31 voxels
    if (lane == 0) {
      out[4 * k + 0] = s;
      out[4 * k + 1] = cd;
      out[4 * k + 2] = s / cd;                                           // 0 / 0 = NaN: the mean of an empty selection
      out[4 * k + 3] = all;
    }
  }
}

template <int C, int W>
__global__ void __launch_bounds__(LT)
nll_select_bwd_k(NllIn lg, int K, const float* __restrict__ label, NllMask mask, NllUses uses, const double* __restrict__ out,
                 const float* __restrict__ gscale, float wj, int64_t V, NllOut dl) {
  const int n = blockIdx.y;
  const float* yg = label + (int64_t)n * C * V;
  const float g = *gscale * wj;
  float invc[NLL_K];
#pragma unroll
  for (int k = 0; k < NLL_K; ++k) invc[k] = (k < K && out[4 * k + 1] > 0.0) ? (float)(1.0 / out[4 * k + 1]) : 0.f;
  const int64_t nq = V / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    const int64_t v = i * W;
    float y[W][MAXC];
    load_voxels<C, W>(yg, V, v, y);
    uint32_t bits[W];
#pragma unroll
    for (int j = 0; j < W; ++j) bits[j] = 0u;
#pragma unroll
    for (int k = 0; k < NLL_K; ++k) {
      if (k < K) {
        const uint8_t* mk = mask.p[k] + (int64_t)n * V + v;
        const uint32_t m = W == 4 ? *reinterpret_cast<const uint32_t*>(mk) : (uint32_t)*mk;
#pragma unroll
        for (int j = 0; j < W; ++j) bits[j] |= ((m >> (8 * j)) & 0xFFu) ? (1u << k) : 0u;
      }
    }
#pragma unroll
    for (int k = 0; k < NLL_K; ++k) {
      if (k < K) {
        float l[W][MAXC], d[W][MAXC];
        load_voxels<C, W>(lg.p[k] + (int64_t)n * C * V, V, v, l);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          float p[MAXC], e[MAXC];
          softmax_argmax<C>(l[j], p, true);
          const float kj = (bits[j] & (uint32_t)uses.u[k]) == (uint32_t)uses.u[k] ? invc[k] : 0.f;
          float dot = 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            e[c] = -0.999f * y[j][c] / (p[c] * 0.999f + 5e-4f) * kj;
            dot = fmaf(e[c], p[c], dot);
          }
#pragma unroll
          for (int c = 0; c < C; ++c) d[j][c] = g * (p[c] * (e[c] - dot));
        }
        store_voxels<C, W>(dl.p[k] + (int64_t)n * C * V, V, v, d);
      }
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int nll_shape_check(const char* what, int k, int n, int c, int64_t v) {
  FPLX_REQUIRE(k >= 1 && k <= NLL_K, FPLX_E_BADSHAPE, "%s: %d networks (1..%d)", what, k, NLL_K);
  FPLX_REQUIRE(n > 0 && n <= 65535 && c >= 2 && c <= MAXC && v > 0, FPLX_E_BADSHAPE, "%s: n=%d (1..65535) c=%d (2..%d) v=%lld (>= 1)",
               what, n, c, MAXC, (long long)v);
  FPLX_REQUIRE((int64_t)n * v < NLL_MAX_N, FPLX_E_BADSHAPE, "%s: n v = %lld voxels, fewer than 2^31 supported (select_kth's bound)",
               what, (long long)((int64_t)n * v));
  return FPLX_OK;
}

inline int nll_uses_check(const char* what, const int* uses, int k, NllUses* u) {
  FPLX_REQUIRE(uses, FPLX_E_NULL, "%s: null uses", what);
  for (int j = 0; j < NLL_K; ++j) u->u[j] = 0;
  for (int j = 0; j < k; ++j) {
    FPLX_REQUIRE(uses[j] >= 0 && uses[j] < (1 << k), FPLX_E_BADSHAPE, "%s: uses[%d] = %d names a mask beyond the %d given", what, j,
                 uses[j], k);
    u->u[j] = uses[j];
  }
  return FPLX_OK;
}

// the chunk a block owns in the three RANK passes, and the grid that covers n with it
inline int64_t nll_chunk(int64_t n) {
  const int64_t per = (n + NLL_BLOCKS - 1) / NLL_BLOCKS;
  return ((per + LT - 1) / LT) * LT;
}

inline int nll_flat_grid(int64_t n) {
  const int64_t g = (n + LT - 1) / LT;
  return (int)(g > NLL_BLOCKS ? NLL_BLOCKS : (g < 1 ? 1 : g));
}

}  // namespace

#define NLL_DISPATCH(C, W, KERNEL, ...)              \
  switch (C) {                                       \
    case 2: KERNEL<2, W> __VA_ARGS__; break;         \
    case 3: KERNEL<3, W> __VA_ARGS__; break;         \
    case 4: KERNEL<4, W> __VA_ARGS__; break;         \
    case 5: KERNEL<5, W> __VA_ARGS__; break;         \
    case 6: KERNEL<6, W> __VA_ARGS__; break;         \
    case 7: KERNEL<7, W> __VA_ARGS__; break;         \
    default: KERNEL<8, W> __VA_ARGS__; break;        \
  }
#define NLL_DISPATCH_VEC(vec, C, KERNEL, ...)        \
  do {                                               \
    if (vec) { NLL_DISPATCH(C, 4, KERNEL, __VA_ARGS__) } else { NLL_DISPATCH(C, 1, KERNEL, __VA_ARGS__) } \
  } while (0)

extern "C" {

int fplx_nll_ce_rows(int64_t voxels_per_sample) { return loss_rows(voxels_per_sample); }

int fplx_nll_voxel_ce_fwd(const float* const* logits, int k, const float* label, int n, int c, int64_t v, float* const* loss,
                          float* part, fplx_stream_t stream) {
  const int rc = nll_shape_check("nll_voxel_ce_fwd", k, n, c, v);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && label && loss && part, FPLX_E_NULL, "nll_voxel_ce_fwd: null pointer");
  NllIn in = {{nullptr, nullptr, nullptr}};
  NllOut o = {{nullptr, nullptr, nullptr}};
  bool vec = v % 4 == 0 && aligned16(label);
  for (int j = 0; j < k; ++j) {
    FPLX_REQUIRE(logits[j] && loss[j], FPLX_E_NULL, "nll_voxel_ce_fwd: null tensor %d", j);
    in.p[j] = logits[j];
    o.p[j] = loss[j];
    vec = vec && aligned16(logits[j]) && aligned16(loss[j]);
  }
  dim3 grid(loss_rows(v), n);
  NLL_DISPATCH_VEC(vec, c, nll_ce_fwd_k, <<<grid, LT, 0, (hipStream_t)stream>>>(in, k, label, v, o, part));
  return fplx_check_launch("nll_voxel_ce_fwd");
}

size_t fplx_nll_mask_ws_bytes(void) { return (3 * NLL_BLOCKS + 1) * sizeof(uint32_t); }

int fplx_nll_select_mask(const float* loss, int64_t n, int mode, int64_t num_remb, float w, const float* sk, const float* smax,
                         uint8_t* mask, void* ws, size_t ws_bytes, fplx_stream_t stream) {
  FPLX_REQUIRE(loss && mask, FPLX_E_NULL, "nll_select_mask: null pointer");
  FPLX_REQUIRE(n > 0 && n < NLL_MAX_N, FPLX_E_BADSHAPE, "nll_select_mask: n = %lld outside [1, 2^31)", (long long)n);
  FPLX_REQUIRE(mode == FPLX_NLL_RANK || mode == FPLX_NLL_BELOW, FPLX_E_BADSHAPE, "nll_select_mask: mode %d (0 RANK, 1 BELOW)", mode);
  hipStream_t st = (hipStream_t)stream;
  if (mode == FPLX_NLL_BELOW) {
    FPLX_REQUIRE(sk, FPLX_E_NULL, "nll_select_mask: BELOW needs the pair of select_kth");
    FPLX_REQUIRE(w >= 0.f && w < 1.f, FPLX_E_BADSHAPE, "nll_select_mask: weight %g outside [0, 1)", (double)w);
    nll_below_k<<<nll_flat_grid(n), LT, 0, st>>>(loss, n, sk, smax, w, mask);
    return fplx_check_launch("nll_select_mask");
  }
  FPLX_REQUIRE(num_remb >= 0 && num_remb <= n, FPLX_E_BADSHAPE, "nll_select_mask: num_remb = %lld outside [0, %lld]",
               (long long)num_remb, (long long)n);
  FPLX_REQUIRE(num_remb == 0 || (sk && ws), FPLX_E_NULL, "nll_select_mask: RANK needs the pair of select_kth and the workspace");
  FPLX_REQUIRE(num_remb == 0 || ws_bytes >= fplx_nll_mask_ws_bytes(), FPLX_E_WORKSPACE, "nll_select_mask: workspace %zu < %zu", ws_bytes,
               fplx_nll_mask_ws_bytes());
  if (num_remb == 0) {
    if (hipMemsetAsync(mask, 0, (size_t)n, st) != hipSuccess) return fplx_check_launch("nll_select_mask");
    return FPLX_OK;
  }
  const int64_t chunk = nll_chunk(n);
  const int G = (int)((n + chunk - 1) / chunk);
  uint32_t* wsu = (uint32_t*)ws;
  nll_rank_count_k<<<G, LT, 0, st>>>(loss, n, chunk, sk, wsu);
  nll_rank_scan_k<<<1, LT, 0, st>>>(wsu, G);
  nll_rank_write_k<<<G, LT, 0, st>>>(loss, n, chunk, sk, num_remb, wsu, mask);
  return fplx_check_launch("nll_select_mask");
}

size_t fplx_nll_select_ws_bytes(void) { return (4 + 2 * NLL_K * NLL_BLOCKS) * sizeof(uint32_t); }

int fplx_nll_select_fwd(const float* const* loss, const uint8_t* const* mask, const int* uses, int k, int64_t n,
                        const float* ce_part, int64_t ce_rows, double* out, void* ws, size_t ws_bytes, fplx_stream_t stream) {
  FPLX_REQUIRE(k >= 1 && k <= NLL_K, FPLX_E_BADSHAPE, "nll_select_fwd: %d networks (1..%d)", k, NLL_K);
  FPLX_REQUIRE(n > 0 && n < NLL_MAX_N, FPLX_E_BADSHAPE, "nll_select_fwd: n = %lld outside [1, 2^31)", (long long)n);
  FPLX_REQUIRE(ce_rows >= 1, FPLX_E_BADSHAPE, "nll_select_fwd: %lld partial rows per network (>= 1)", (long long)ce_rows);
  FPLX_REQUIRE(loss && mask && ce_part && out && ws, FPLX_E_NULL, "nll_select_fwd: null pointer");
  FPLX_REQUIRE(ws_bytes >= fplx_nll_select_ws_bytes(), FPLX_E_WORKSPACE, "nll_select_fwd: workspace %zu < %zu", ws_bytes,
               fplx_nll_select_ws_bytes());
  NllUses u;
  const int rc = nll_uses_check("nll_select_fwd", uses, k, &u);
  if (rc != FPLX_OK) return rc;
  NllIn in = {{nullptr, nullptr, nullptr}};
  NllMask mk = {{nullptr, nullptr, nullptr}};
  bool vec = n >= 4;
  for (int j = 0; j < k; ++j) {
    FPLX_REQUIRE(loss[j] && mask[j], FPLX_E_NULL, "nll_select_fwd: null array %d", j);
    in.p[j] = loss[j];
    mk.p[j] = mask[j];
    vec = vec && aligned16(loss[j]) && aligned16(mask[j]);
  }
  hipStream_t st = (hipStream_t)stream;
  // the ticket is cleared by a memset node in front of the one launch (a counter that only the last block resets would be
  // wrong on a workspace used for the first time)
  if (hipMemsetAsync(ws, 0, 4 * sizeof(uint32_t), st) != hipSuccess) return fplx_check_launch("nll_select_fwd");
  if (vec) nll_select_fwd_k<4><<<nll_flat_grid(n / 4), LT, 0, st>>>(in, mk, u, k, n, ce_part, ce_rows, (uint32_t*)ws, out);
  else nll_select_fwd_k<1><<<nll_flat_grid(n), LT, 0, st>>>(in, mk, u, k, n, ce_part, ce_rows, (uint32_t*)ws, out);
  return fplx_check_launch("nll_select_fwd");
}

int fplx_nll_select_bwd(const float* const* logits, const float* label, const uint8_t* const* mask, const int* uses, int k,
                        const double* out, const float* gscale, float wj, int n, int c, int64_t v, float* const* dlogits,
                        fplx_stream_t stream) {
  int rc = nll_shape_check("nll_select_bwd", k, n, c, v);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(logits && label && mask && out && gscale && dlogits, FPLX_E_NULL, "nll_select_bwd: null pointer");
  NllUses u;
  rc = nll_uses_check("nll_select_bwd", uses, k, &u);
  if (rc != FPLX_OK) return rc;
  NllIn in = {{nullptr, nullptr, nullptr}};
  NllMask mk = {{nullptr, nullptr, nullptr}};
  NllOut o = {{nullptr, nullptr, nullptr}};
  bool vec = v % 4 == 0 && aligned16(label);
  for (int j = 0; j < k; ++j) {
    FPLX_REQUIRE(logits[j] && mask[j] && dlogits[j], FPLX_E_NULL, "nll_select_bwd: null tensor %d", j);
    in.p[j] = logits[j];
    mk.p[j] = mask[j];
    o.p[j] = dlogits[j];
    vec = vec && aligned16(logits[j]) && aligned16(mask[j]) && aligned16(dlogits[j]);
  }
  dim3 grid(grid1(vec ? v / 4 : v, 2048), n);
  NLL_DISPATCH_VEC(vec, c, nll_select_bwd_k, <<<grid, LT, 0, (hipStream_t)stream>>>(in, k, label, mk, u, out, gscale, wj, v, o));
  return fplx_check_launch("nll_select_bwd");
}

}  // extern "C"
