// Confident learning, the producer of SLSRLoss's "this label is suspect" mask (PyMIC/pymic/net_run_nll/nll_clslsr.py:19-46, which
// hands the softmax of every voxel of the training set to cleanlab 1.0's get_noise_indices): the class statistics, the confident
// joint, the keys of the order statistics fplx_select_kth (intensity.hip) takes and the mask, each as one streaming pass over
// psx fp32 planar [C][M] and the given labels s uint8 [M].  Formulas: include/fplx.h, "confident learning".
// Conventions of nll.hip: a lane takes 4 consecutive voxels with 16-byte accesses where every base is aligned and M is a multiple
// of 4, else one voxel; fp32 values are summed in double, the block partials of a sum added in a fixed order by one wave of the
// block that draws the last ticket; counts are integers (integer atomics on the histogram and the mask count); no floating-point
// atomics - two runs give the same bits.
// Compiled with -ffp-contract=off (Makefile): the margin psx[j] - psx[k] and the softmax round the same way in every kernel
// that forms them, whatever stands next to them.
#include "loss_common.h"
#include "gfx950.h"

namespace {

constexpr int CL_BLOCKS = 1024;                       // blocks of the passes, and rows of the statistics' partials
constexpr int64_t CL_MAX_M = (int64_t)1 << 31;        // the bound of fplx_select_kth
constexpr int CL_NCNT = MAXC + 2;                     // counters: the classes, labels >= C, voxels with a NaN

template <int W>
__device__ __forceinline__ void cl_labels(const uint8_t* __restrict__ s, int64_t i, int (&k)[W]) {
  if constexpr (W == 4) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(s + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = (int)((v >> (8 * j)) & 0xFFu);
  } else {
    k[0] = (int)s[i];
  }
}

// psx[k] of a voxel whose label is a run-time k, without indexed registers: the bits of the one plane whose number matches
// (a chain of selects is turned back into an indexed load of a private array by the compiler - 144 bytes of scratch per lane)
template <int C>
__device__ __forceinline__ float cl_pick(const float (&p)[MAXC], int k) {
  uint32_t r = 0u;
#pragma unroll
  for (int c = 0; c < C; ++c) r |= __float_as_uint(p[c]) & (k == c ? 0xFFFFFFFFu : 0u);
  return __uint_as_float(r);
}

template <int C>
__device__ __forceinline__ int cl_argmax(const float (&p)[MAXC]) {          // first maximum, as np.argmax
  int a = 0;
  float best = p[0];
#pragma unroll
  for (int c = 1; c < C; ++c)
    if (p[c] > best) { best = p[c]; a = c; }
  return a;
}

// ---- p[c][i] = softmax over c of x[.][i]: max, exp(x - max), sum (c ascending), divide
template <int C, int W>
__global__ void __launch_bounds__(LT)
cl_softmax_k(const float* __restrict__ x, int64_t m, float* __restrict__ p) {
  const int64_t nq = m / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    const int64_t v = i * W;
    float l[W][MAXC], o[W][MAXC];
    load_voxels<C, W>(x, m, v, l);
#pragma unroll
    for (int j = 0; j < W; ++j) softmax_argmax<C>(l[j], o[j], true);
    store_voxels<C, W>(p, m, v, o);
  }
}

// ---- class statistics.  ws: ticket | 3 pad words | double psum [MAXC][CL_BLOCKS] | uint32 pcnt [CL_NCNT][CL_BLOCKS]
template <int C, int W>
__global__ void __launch_bounds__(LT)
cl_stats_k(const float* __restrict__ psx, const uint8_t* __restrict__ s, int64_t m, uint32_t* __restrict__ ws,
           double* __restrict__ sums, int64_t* __restrict__ counts, double* __restrict__ thr) {
  __shared__ double rs[LT / 64][MAXC];
  __shared__ uint32_t rc[LT / 64][CL_NCNT];
  __shared__ uint32_t is_last;
  const int G = gridDim.x;
  double* psum = reinterpret_cast<double*>(ws + 4);
  uint32_t* pcnt = ws + 4 + 2 * MAXC * CL_BLOCKS;
  double acc[C];
  uint32_t cnt[C + 2];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0;
#pragma unroll
  for (int c = 0; c < C + 2; ++c) cnt[c] = 0u;
  const int64_t nq = m / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)G * LT) {
    const int64_t v = i * W;
    float l[W][MAXC];
    int k[W];
    load_voxels<C, W>(psx, m, v, l);
    cl_labels<W>(s, v, k);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      bool nan = false;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        nan = nan || l[j][c] != l[j][c];
        if (k[j] == c) { acc[c] += (double)l[j][c]; cnt[c] += 1u; }
      }
      cnt[C] += k[j] >= C ? 1u : 0u;
      cnt[C + 1] += nan ? 1u : 0u;
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double t = wave_sum_d(acc[c]);
    if (lane == 0) rs[wv][c] = t;
  }
#pragma unroll
  for (int c = 0; c < C + 2; ++c) {
    uint32_t t = cnt[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += (uint32_t)__shfl_xor((int)t, o, 64);
    if (lane == 0) rc[wv][c] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < C + 2) {
    uint32_t t = 0u;
    for (int i = 0; i < LT / 64; ++i) t += rc[i][threadIdx.x];
    pcnt[(int64_t)threadIdx.x * CL_BLOCKS + blockIdx.x] = t;
    if ((int)threadIdx.x < C) {
      double d = 0.0;
      for (int i = 0; i < LT / 64; ++i) d += rs[i][threadIdx.x];
      psum[(int64_t)threadIdx.x * CL_BLOCKS + blockIdx.x] = d;
    }
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
    is_last = last ? 1u : 0u;
  }
  __syncthreads();
  if (is_last == 0u) return;
  for (int c = wv; c < C + 2; c += LT / 64) {                            // one wave per sum, lanes striding over the rows
    double d = 0.0, n = 0.0;
    for (int r = lane; r < G; r += 64) {
      n += (double)pcnt[(int64_t)c * CL_BLOCKS + r];
      if (c < C) d += psum[(int64_t)c * CL_BLOCKS + r];
    }
    d = wave_sum_d(d);
    n = wave_sum_d(n);                                                  // exact: fewer than 2^31 voxels
    if (lane == 0) {
      counts[c] = (int64_t)n;
      if (c < C) {
        sums[c] = d;
        if (thr) thr[c] = d / n;                                        // an empty class: 0 / 0 = NaN, refused by the host
      }
    }
  }
}

// ---- confident joint: joint[s][guess] += 1 for the voxels with at least one confident class
template <int C, int W>
__global__ void __launch_bounds__(LT)
cl_joint_k(const float* __restrict__ psx, const uint8_t* __restrict__ s, int64_t m, const double* __restrict__ thr,
           unsigned long long* __restrict__ joint) {
  __shared__ uint32_t hist[MAXC * MAXC];
  if ((int)threadIdx.x < C * C) hist[threadIdx.x] = 0u;
  __syncthreads();
  double t[C];
#pragma unroll
  for (int c = 0; c < C; ++c) t[c] = thr[c] - 1e-6;
  const int64_t nq = m / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    const int64_t v = i * W;
    float l[W][MAXC];
    int k[W];
    load_voxels<C, W>(psx, m, v, l);
    cl_labels<W>(s, v, k);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      int nc = 0, only = 0;
#pragma unroll
      for (int c = 0; c < C; ++c)
        if ((double)l[j][c] >= t[c]) { nc += 1; only = c; }
      const int guess = nc == 1 ? only : cl_argmax<C>(l[j]);
      if (nc > 0 && k[j] < C) atomicAdd(&hist[k[j] * C + guess], 1u);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < C * C && hist[threadIdx.x] != 0u) atomicAdd(&joint[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

// ---- the keys of one order statistic: members of class k carry their value, everything else NaN (sorted last)
template <int C, int W>
__global__ void __launch_bounds__(LT)
cl_keys_k(const float* __restrict__ psx, const uint8_t* __restrict__ s, int64_t m, int k, int jc, float* __restrict__ keys) {
  const float* pk = psx + (int64_t)k * m;
  const float* pj = psx + (int64_t)(jc < 0 ? k : jc) * m;
  const float qnan = __uint_as_float(0x7FC00000u);
  const int64_t nq = m / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    const int64_t v = i * W;
    float a[W], b[W], o[W];
    int lab[W];
    VecLd<W>::ld(pk + v, a);
    cl_labels<W>(s, v, lab);
    VecLd<W>::ld(pj + v, b);                                            // j < 0: plane k again
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float val = jc < 0 ? a[j] : -(b[j] - a[j]);
      o[j] = lab[j] == k ? val : qnan;
    }
    VecLd<W>::st(keys + v, o);
  }
}

// ---- the mask: (by class | by noise rate | both) and pred != s.  The cuts sit in LDS, a row of MAXC per given label, NaN where
// a cut does not apply (a comparison with NaN is false): a lane reads the row of ITS label - no indexed registers, no scratch.
template <int C, int W>
__global__ void __launch_bounds__(LT)
cl_mask_k(const float* __restrict__ psx, const uint8_t* __restrict__ s, int64_t m, int method,
          const float* __restrict__ class_cut, const float* __restrict__ pair_cut, unsigned long long active,
          uint8_t* __restrict__ mask, unsigned long long* __restrict__ count) {
  __shared__ float cuts[MAXC][MAXC];                                     // [k][j]: pair_cut[k][j]; [k][k]: class_cut[k]
  __shared__ uint32_t red[LT / 64];
  if (threadIdx.x < MAXC * MAXC) {
    const int k = threadIdx.x / MAXC, j = threadIdx.x % MAXC;
    float v = __uint_as_float(0x7FC00000u);
    if (k < C && j < C) {
      if (k == j) { if (method != FPLX_CL_BY_NOISE_RATE) v = class_cut[k]; }
      else if ((active >> (k * MAXC + j)) & 1ull) v = pair_cut[k * C + j];
    }
    cuts[k][j] = v;
  }
  __syncthreads();
  uint32_t set = 0u;
  const int64_t nq = m / W;
  for (int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x; i < nq; i += (int64_t)gridDim.x * LT) {
    const int64_t v = i * W;
    float l[W][MAXC];
    int k[W];
    load_voxels<C, W>(psx, m, v, l);
    cl_labels<W>(s, v, k);
    uint32_t word = 0u;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int kk = k[j] < C ? k[j] : 0;
      const float pk = cl_pick<C>(l[j], kk);
      bool by_class = false, by_rate = false;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float cut = cuts[kk][c];
        by_class = by_class || (c == kk && pk < cut);
        by_rate = by_rate || (c != kk && l[j][c] - pk >= cut);
      }
      const bool sel = method == FPLX_CL_BY_CLASS ? by_class : (method == FPLX_CL_BY_NOISE_RATE ? by_rate : (by_class && by_rate));
      const bool on = sel && k[j] < C && cl_argmax<C>(l[j]) != kk;
      word |= (on ? 1u : 0u) << (8 * j);
      set += on ? 1u : 0u;
    }
    if constexpr (W == 4) *reinterpret_cast<uint32_t*>(mask + v) = word;
    else mask[v] = (uint8_t)word;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) set += (uint32_t)__shfl_xor((int)set, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = set;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0u;
    for (int i = 0; i < LT / 64; ++i) t += red[i];
    if (t != 0u) atomicAdd(count, (unsigned long long)t);
  }
}

inline bool cl_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

inline int cl_shape_check(const char* what, int c, int64_t m) {
  FPLX_REQUIRE(c >= 2 && c <= MAXC, FPLX_E_BADSHAPE, "%s: c=%d (2..%d)", what, c, MAXC);
  FPLX_REQUIRE(m >= 1 && m < CL_MAX_M, FPLX_E_BADSHAPE, "%s: m = %lld outside [1, 2^31) (select_kth's bound)", what, (long long)m);
  return FPLX_OK;
}

// four voxels per lane: the planes (base and m) and the byte arrays allow 16-byte / 4-byte accesses
inline bool cl_vec(int64_t m, const void* f0, const void* f1, const void* b0, const void* b1) {
  return m % 4 == 0 && cl_aligned(f0, 16) && (!f1 || cl_aligned(f1, 16)) && (!b0 || cl_aligned(b0, 4)) && (!b1 || cl_aligned(b1, 4));
}

inline int cl_grid(bool vec, int64_t m) { return grid1(vec ? m / 4 : m, CL_BLOCKS); }

}  // namespace

#define CL_DISPATCH(C, W, KERNEL, ...)               \
  switch (C) {                                       \
    case 2: KERNEL<2, W> __VA_ARGS__; break;         \
    case 3: KERNEL<3, W> __VA_ARGS__; break;         \
    case 4: KERNEL<4, W> __VA_ARGS__; break;         \
    case 5: KERNEL<5, W> __VA_ARGS__; break;         \
    case 6: KERNEL<6, W> __VA_ARGS__; break;         \
    case 7: KERNEL<7, W> __VA_ARGS__; break;         \
    default: KERNEL<8, W> __VA_ARGS__; break;        \
  }
#define CL_DISPATCH_VEC(vec, C, KERNEL, ...)         \
  do {                                               \
    if (vec) { CL_DISPATCH(C, 4, KERNEL, __VA_ARGS__) } else { CL_DISPATCH(C, 1, KERNEL, __VA_ARGS__) } \
  } while (0)

extern "C" {

int fplx_cl_softmax(const float* x, int c, int64_t m, float* p, fplx_stream_t stream) {
  const int rc = cl_shape_check("cl_softmax", c, m);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(x && p, FPLX_E_NULL, "cl_softmax: null pointer");
  const bool vec = cl_vec(m, x, p, nullptr, nullptr);
  CL_DISPATCH_VEC(vec, c, cl_softmax_k, <<<cl_grid(vec, m), LT, 0, (hipStream_t)stream>>>(x, m, p));
  return fplx_check_launch("cl_softmax");
}

size_t fplx_cl_stats_ws_bytes(void) { return (4 + 2 * MAXC * CL_BLOCKS + CL_NCNT * CL_BLOCKS) * sizeof(uint32_t); }

int fplx_cl_class_stats(const float* psx, const uint8_t* s, int c, int64_t m, void* ws, size_t ws_bytes, double* sums,
                        int64_t* counts, double* thr, fplx_stream_t stream) {
  const int rc = cl_shape_check("cl_class_stats", c, m);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(psx && s && ws && sums && counts, FPLX_E_NULL, "cl_class_stats: null pointer");
  FPLX_REQUIRE(cl_aligned(ws, 8), FPLX_E_BADSHAPE, "cl_class_stats: the workspace is not 8-byte aligned");
  FPLX_REQUIRE(ws_bytes >= fplx_cl_stats_ws_bytes(), FPLX_E_WORKSPACE, "cl_class_stats: workspace %zu < %zu", ws_bytes,
               fplx_cl_stats_ws_bytes());
  hipStream_t st = (hipStream_t)stream;
  // the ticket is cleared by a memset node in front of the one launch, as in nll_select_fwd
  if (hipMemsetAsync(ws, 0, 4 * sizeof(uint32_t), st) != hipSuccess) return fplx_check_launch("cl_class_stats");
  const bool vec = cl_vec(m, psx, nullptr, s, nullptr);
  CL_DISPATCH_VEC(vec, c, cl_stats_k, <<<cl_grid(vec, m), LT, 0, st>>>(psx, s, m, (uint32_t*)ws, sums, counts, thr));
  return fplx_check_launch("cl_class_stats");
}

int fplx_cl_confident_joint(const float* psx, const uint8_t* s, int c, int64_t m, const double* thr, int64_t* joint,
                            fplx_stream_t stream) {
  const int rc = cl_shape_check("cl_confident_joint", c, m);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(psx && s && thr && joint, FPLX_E_NULL, "cl_confident_joint: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(joint, 0, (size_t)c * c * sizeof(int64_t), st) != hipSuccess) return fplx_check_launch("cl_confident_joint");
  const bool vec = cl_vec(m, psx, nullptr, s, nullptr);
  CL_DISPATCH_VEC(vec, c, cl_joint_k, <<<cl_grid(vec, m), LT, 0, st>>>(psx, s, m, thr, (unsigned long long*)joint));
  return fplx_check_launch("cl_confident_joint");
}

int fplx_cl_select_keys(const float* psx, const uint8_t* s, int c, int64_t m, int k, int j, float* keys, fplx_stream_t stream) {
  const int rc = cl_shape_check("cl_select_keys", c, m);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(psx && s && keys, FPLX_E_NULL, "cl_select_keys: null pointer");
  FPLX_REQUIRE(k >= 0 && k < c && j < c && j != k, FPLX_E_BADSHAPE, "cl_select_keys: k=%d j=%d for %d classes (0 <= k < c, j < c, j != k)",
               k, j, c);
  const bool vec = cl_vec(m, psx, keys, s, nullptr);
  CL_DISPATCH_VEC(vec, c, cl_keys_k, <<<cl_grid(vec, m), LT, 0, (hipStream_t)stream>>>(psx, s, m, k, j, keys));
  return fplx_check_launch("cl_select_keys");
}

int fplx_cl_noise_mask(const float* psx, const uint8_t* s, int c, int64_t m, int method, const float* class_cut,
                       const float* pair_cut, const uint8_t* pair_active, uint8_t* mask, int64_t* count, fplx_stream_t stream) {
  const int rc = cl_shape_check("cl_noise_mask", c, m);
  if (rc != FPLX_OK) return rc;
  FPLX_REQUIRE(method == FPLX_CL_BY_CLASS || method == FPLX_CL_BY_NOISE_RATE || method == FPLX_CL_BOTH, FPLX_E_BADSHAPE,
               "cl_noise_mask: method %d (0 by class, 1 by noise rate, 2 both)", method);
  FPLX_REQUIRE(psx && s && mask && count, FPLX_E_NULL, "cl_noise_mask: null pointer");
  FPLX_REQUIRE(method == FPLX_CL_BY_NOISE_RATE || class_cut, FPLX_E_NULL, "cl_noise_mask: this method needs class_cut");
  FPLX_REQUIRE(method == FPLX_CL_BY_CLASS || (pair_cut && pair_active), FPLX_E_NULL, "cl_noise_mask: this method needs pair_cut and pair_active");
  unsigned long long active = 0ull;                                      // bit k MAXC + j: pair_cut[k][j] applies
  if (method != FPLX_CL_BY_CLASS)
    for (int k = 0; k < c; ++k)
      for (int j = 0; j < c; ++j)
        if (j != k && pair_active[k * c + j]) active |= 1ull << (k * MAXC + j);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(count, 0, sizeof(int64_t), st) != hipSuccess) return fplx_check_launch("cl_noise_mask");
  const bool vec = cl_vec(m, psx, nullptr, s, mask);
  CL_DISPATCH_VEC(vec, c, cl_mask_k, <<<cl_grid(vec, m), LT, 0, st>>>(psx, s, m, method, class_cut, pair_cut, active, mask,
                                                                     (unsigned long long*)count));
  return fplx_check_launch("cl_noise_mask");
}

}  // extern "C"
