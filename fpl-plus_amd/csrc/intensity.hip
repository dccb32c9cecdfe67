// Intensity transforms on the GPU: the reference's numpy passes NormalizeWithMinMax / NormalizeWithPercentiles
// (PyMIC/pymic/transform/normalize.py:155-237), ChannelWiseThreshold / ChannelWiseThresholdWithNormalize (threshold.py:14-132),
// GammaCorrection / GaussianNoise (intensity.py:14-86) on one channel volume of fp32 voxels.  The random draws stay on the
// host (fplx/transform.py); these kernels are the reductions, the exact order statistics behind numpy.percentile and the
// fused element passes.  Every fp32 expression is written operation for operation as numpy evaluates it on a float32 array
// under NumPy 2 (Python-float parameters enter as float32), and this file is compiled with -ffp-contract=off: a fused
// multiply-add would round p * (vmax - vmin) + vmin once where numpy rounds twice.
#include "common.h"
#include "philox.h"
#include <math.h>

namespace {

constexpr int IT_THREADS = 256;
constexpr int IT_MAX_BLOCKS = 1024;
constexpr int IT_ROWS = 256;                   // partial rows of the masked moments (as sample.hip's SP_BLOCKS)

inline int it_grid(int64_t total) {
  int64_t g = (total + IT_THREADS - 1) / IT_THREADS;
  return (int)(g > IT_MAX_BLOCKS ? IT_MAX_BLOCKS : (g < 1 ? 1 : g));
}

// (the order-preserving integer keys key_nan_high / key_nan_low / key_to_float: common.h)
__device__ __forceinline__ uint32_t wave_umin(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64); v = t < v ? t : v; }
  return v;
}
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64); v = t > v ? t : v; }
  return v;
}

// ---- per-channel min / max, and min / max of the data clipped as numpy clips it (x < lo -> lo, then x > hi -> hi)
// keys: [min, max, clipped min, clipped max]
__global__ void minmax_init_k(uint32_t* __restrict__ keys) {
  if (threadIdx.x < 4) keys[threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xFFFFFFFFu;
}

__global__ void __launch_bounds__(IT_THREADS)
minmax_k(const float* __restrict__ x, int64_t n, float lo, int use_lo, float hi, int use_hi, uint32_t* __restrict__ keys) {
  __shared__ uint32_t red[IT_THREADS / 64][4];
  uint32_t kmin = 0xFFFFFFFFu, kmax = 0u, cmin = 0xFFFFFFFFu, cmax = 0u;
  for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS) {
    const float v = x[i];
    float c = v;
    if (use_lo && c < lo) c = lo;
    if (use_hi && c > hi) c = hi;
    const uint32_t a = key_nan_low(v), b = key_nan_high(v), ca = key_nan_low(c), cb = key_nan_high(c);
    kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax;
    cmin = ca < cmin ? ca : cmin; cmax = cb > cmax ? cb : cmax;
  }
  kmin = wave_umin(kmin); kmax = wave_umax(kmax); cmin = wave_umin(cmin); cmax = wave_umax(cmax);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave][0] = kmin; red[wave][1] = kmax; red[wave][2] = cmin; red[wave][3] = cmax; }
  __syncthreads();
  if (threadIdx.x < 4) {
    uint32_t v = red[0][threadIdx.x];
    const bool is_max = threadIdx.x & 1;
    for (int w = 1; w < IT_THREADS / 64; ++w) {
      const uint32_t t = red[w][threadIdx.x];
      v = is_max ? (t > v ? t : v) : (t < v ? t : v);
    }
    // at most one device-scope atomic per block and statistic, and none when the block cannot improve the key: the relaxed
    // load may return an older value, which is never better than the current one, so skipping on it is safe.  A thousand
    // atomics on one cache line cost more than the pass over the data (26 us against 10).
    const uint32_t seen = __hip_atomic_load(keys + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (is_max) { if (v > seen) atomicMax(keys + threadIdx.x, v); }
    else { if (v < seen) atomicMin(keys + threadIdx.x, v); }
  }
}

__global__ void minmax_final_k(const uint32_t* __restrict__ keys, float* __restrict__ out4) {
  if (threadIdx.x < 4) out4[threadIdx.x] = key_to_float(keys[threadIdx.x]);
}

// ---- exact order statistics: radix selection, 4 passes of 8 bits over the key (most significant first).
// Workspace words: prefix[8] | remaining rank[8] | histogram group[8] | count, status | pad to 32 | histograms [8][256].
// A "rank" here is an internal one: caller's rank j becomes 2j (k_j) and 2j + 1 (k_j + 1, clamped to n - 1).
// Ranks whose prefixes agree so far share one histogram (group = the lowest such rank): all of them in the first pass, and
// k_j / k_j + 1 almost always to the last.
constexpr int SEL_MAX = 8;
constexpr int SEL_PREFIX = 0, SEL_KREM = 8, SEL_GRP = 16, SEL_NR = 24, SEL_STATUS = 25, SEL_HIST = 32;
constexpr int SEL_WORDS = SEL_HIST + SEL_MAX * 256;

struct SelRanks { uint32_t k[SEL_MAX]; int nr; };

__global__ void __launch_bounds__(IT_THREADS)
select_init_k(uint32_t* __restrict__ ws, SelRanks r) {
  for (int i = threadIdx.x; i < SEL_WORDS; i += IT_THREADS) {
    uint32_t v = 0u;
    if (i >= SEL_KREM && i < SEL_KREM + SEL_MAX) v = r.k[i - SEL_KREM];
    if (i == SEL_NR) v = (uint32_t)r.nr;
    ws[i] = v;
  }
}

__global__ void __launch_bounds__(IT_THREADS)
select_hist_k(const float* __restrict__ x, int64_t n, uint32_t* __restrict__ ws, int pass) {
  __shared__ uint32_t lh[SEL_MAX][256];
  const int nr = min((int)ws[SEL_NR], SEL_MAX);
  uint32_t prefix[SEL_MAX];
  bool lead[SEL_MAX];
#pragma unroll
  for (int r = 0; r < SEL_MAX; ++r) {
    prefix[r] = ws[SEL_PREFIX + r];
    lead[r] = r < nr && ws[SEL_GRP + r] == (uint32_t)r;
  }
#pragma unroll
  for (int r = 0; r < SEL_MAX; ++r) lh[r][threadIdx.x] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS) {
    const uint32_t key = key_nan_high(x[i]);
    const uint32_t top = pass == 0 ? 0u : key >> (shift + 8);
    const uint32_t bin = (key >> shift) & 255u;
#pragma unroll
    for (int r = 0; r < SEL_MAX; ++r)
      if (lead[r] && top == prefix[r]) atomicAdd(&lh[r][bin], 1u);
  }
  __syncthreads();
  // flush: one device-scope atomic per non-empty bin; the next kernel in the stream reads the sums
#pragma unroll
  for (int r = 0; r < SEL_MAX; ++r) {
    const uint32_t v = lh[r][threadIdx.x];
    if (lead[r] && v) atomicAdd(ws + SEL_HIST + r * 256 + threadIdx.x, v);
  }
}

// one block: narrows every rank's prefix by the bin that holds it, regroups, clears the histograms for the next pass.
// The bin is found with a block-wide prefix sum (one bin per thread): a serial walk over the 256 bins by one thread per rank
// cost 14 us per pass, more than the pass over the data.
__global__ void __launch_bounds__(IT_THREADS)
select_scan_k(uint32_t* __restrict__ ws, int pass, float* __restrict__ out) {
  __shared__ uint32_t h[SEL_MAX][256];                         // counts, then inclusive sums within each wave
  __shared__ uint32_t wsum[SEL_MAX][IT_THREADS / 64];
  __shared__ uint32_t fbin[SEL_MAX], fcum[SEL_MAX], np[SEL_MAX];
  const int nr = min((int)ws[SEL_NR], SEL_MAX);                // the clamps keep every index inside the workspace whatever it holds
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t cnt[SEL_MAX];
#pragma unroll
  for (int r = 0; r < SEL_MAX; ++r) {
    cnt[r] = 0u;
    if (r < nr) {                                              // block-uniform
      const uint32_t c = ws[SEL_HIST + (int)(ws[SEL_GRP + r] & (SEL_MAX - 1)) * 256 + t];
      uint32_t v = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
        if (lane >= o) v += u;
      }
      cnt[r] = c;
      h[r][t] = v;
      if (lane == 63) wsum[r][wave] = v;
    }
  }
  if (t < SEL_MAX) fbin[t] = 0xFFFFFFFFu;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SEL_MAX; ++r) {
    if (r < nr) {
      uint32_t incl = h[r][t];
      for (int w = 0; w < wave; ++w) incl += wsum[r][w];
      const uint32_t excl = incl - cnt[r], k = ws[SEL_KREM + r];
      if (excl <= k && k < incl) { fbin[r] = (uint32_t)t; fcum[r] = excl; }    // at most one bin holds rank k
    }
  }
  __syncthreads();
  if (t < nr) {
    const uint32_t k = ws[SEL_KREM + t];
    uint32_t bin = fbin[t], cum = fcum[t];
    if (bin > 255u) { bin = 255u; cum = k; ws[SEL_STATUS] = 1u; }   // cannot happen for 0 <= k < n; reported, never followed
    const uint32_t p = (pass == 0 ? 0u : ws[SEL_PREFIX + t] << 8) | bin;
    np[t] = p;
    ws[SEL_PREFIX + t] = p;
    ws[SEL_KREM + t] = k - cum;
    if (pass == 3) out[t] = key_to_float(p);
  }
  __syncthreads();
  if (t < nr) {
    int g = t;
    for (int r = t - 1; r >= 0; --r) if (np[r] == np[t]) g = r;
    ws[SEL_GRP + t] = (uint32_t)g;
  }
  for (int r = 0; r < SEL_MAX; ++r) ws[SEL_HIST + r * 256 + t] = 0u;
}

// ---- element passes (y may alias x everywhere)

// numpy: img[img < v0] = v0; img[img > v1] = v1; (img - a) / b.  The comparisons are numpy's, so a NaN passes through.
__global__ void __launch_bounds__(IT_THREADS)
clip_affine_k(const float* __restrict__ x, float* __restrict__ y, int64_t n, float v0, float v1, float a, float b) {
  for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS) {
    float v = x[i];
    if (v < v0) v = v0;
    if (v > v1) v = v1;
    y[i] = (v - a) / b;
  }
}

__global__ void __launch_bounds__(IT_THREADS)
clip_affine_dev_k(const float* __restrict__ x, float* __restrict__ y, int64_t n, const float* __restrict__ pv0,
                  const float* __restrict__ pv1, const float* __restrict__ pa, const float* __restrict__ phi) {
  const float v0 = *pv0, v1 = *pv1, a = *pa, b = *phi - a;       // fp32 difference, as numpy forms v1 - v0
  for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS) {
    float v = x[i];
    if (v < v0) v = v0;
    if (v > v1) v = v1;
    y[i] = (v - a) / b;
  }
}

// threshold.py:46-61: the upper test sees the value the lower replacement left
__global__ void __launch_bounds__(IT_THREADS)
threshold_replace_k(const float* __restrict__ x, float* __restrict__ y, int64_t n, float t_lo, float r_lo, int use_lo,
                    float t_hi, float r_hi, int use_hi) {
  for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS) {
    float v = x[i];
    if (use_lo && v < t_lo) v = r_lo;
    if (use_hi && v > t_hi) v = r_hi;
    y[i] = v;
  }
}

// ---- masked moments: normalize_positive's three passes (sample.hip) with the mask v0 < x < v1, each bound optional.
// threshold.py:103-114: a voxel outside the mask (a NaN included: both comparisons are false) takes the noise volume.
struct Range { float v0, v1; int use0, use1; };
__device__ __forceinline__ bool inside(float v, const Range& r) {
  return (!r.use0 || v > r.v0) && (!r.use1 || v < r.v1);
}

__device__ __forceinline__ double rows_total(const double* __restrict__ part) {   // fixed order
  double t = 0.0;
  for (int i = 0; i < IT_ROWS; ++i) t += part[i];
  return t;
}

__device__ __forceinline__ void block_sum2(double s, double c, double* __restrict__ ps, double* __restrict__ pc) {
  __shared__ double red[IT_THREADS], redc[IT_THREADS];
  red[threadIdx.x] = s; redc[threadIdx.x] = c;
  __syncthreads();
  for (int o = IT_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { red[threadIdx.x] += red[threadIdx.x + o]; redc[threadIdx.x] += redc[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { ps[blockIdx.x] = red[0]; if (pc) pc[blockIdx.x] = redc[0]; }
}

__global__ void __launch_bounds__(IT_THREADS)
range_sum_k(const float* __restrict__ x, int64_t n, Range rg, double* __restrict__ part, double* __restrict__ cnt) {
  double s = 0.0, c = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS)
    if (inside(x[i], rg)) { s += (double)x[i]; c += 1.0; }
  block_sum2(s, c, part, cnt);
}

__global__ void __launch_bounds__(IT_THREADS)
range_dev_k(const float* __restrict__ x, int64_t n, Range rg, const double* __restrict__ sums, const double* __restrict__ cnt,
            double* __restrict__ part) {
  const double mean = rows_total(sums) / rows_total(cnt);
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS)
    if (inside(x[i], rg)) { const double d = (double)x[i] - mean; s += d * d; }
  block_sum2(s, 0.0, part, nullptr);
}

__global__ void __launch_bounds__(IT_THREADS)
range_apply_k(const float* __restrict__ x, const float* __restrict__ noise, float* __restrict__ y, int64_t n, Range rg,
              const double* __restrict__ sums, const double* __restrict__ cnt, const double* __restrict__ devs,
              float* __restrict__ out_ms) {
  const double m = rows_total(cnt);                            // 0 for an empty mask: NaN moments, every voxel replaced
  const float mean = (float)(rows_total(sums) / m);
  const float sd = (float)sqrt(rows_total(devs) / m);
  if (out_ms && blockIdx.x == 0 && threadIdx.x == 0) { out_ms[0] = mean; out_ms[1] = sd; }
  for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS) {
    const float v = x[i];
    y[i] = inside(v, rg) ? (v - mean) / sd : noise[i];
  }
}

// ---- intensity.py:37-51.  n = (x - vmin) / (vmax - vmin), p = n ** gamma, y = p * (vmax - vmin) + vmin, all float32 in
// numpy.  p is the correctly rounded power here (fp64 pow, one rounding), numpy's powf is within 1 ulp of that.
__global__ void __launch_bounds__(IT_THREADS)
gamma_k(const float* __restrict__ x, float* __restrict__ y, int64_t n, const float* __restrict__ pmin,
        const float* __restrict__ pmax, float gamma) {
  const float vmin = *pmin, vmax = *pmax;
  const float d = vmax - vmin;
  const double g = (double)gamma;
  for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS) {
    const float nv = (x[i] - vmin) / d;
    const float p = (float)pow((double)nv, g);
    const float s = p * d;
    y[i] = s + vmin;
  }
}

// intensity.py:78-84: float32 image + float64 noise is a float64 sum, stored back into the float32 image
__global__ void __launch_bounds__(IT_THREADS)
add_noise_f64_k(const float* __restrict__ x, const double* __restrict__ noise, float* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS)
    y[i] = (float)((double)x[i] + noise[i]);
}

// device generator.  Element i: words 2 (i & 1), 2 (i & 1) + 1 of philox(counter = (i >> 1, 0, stream, 0), key = seed) -
// the dropout stream's counter layout with two words per element instead of one; u = (word + 1) / 2^32 in (0, 1];
// z = sqrt(-2 ln u1) cos(2 pi u2) in fp64; y = float32((double(x) + mean) + std * z).
__global__ void __launch_bounds__(IT_THREADS)
add_noise_philox_k(const float* __restrict__ x, float* __restrict__ y, int64_t n, uint32_t k0, uint32_t k1, uint32_t sid,
                   double mean, double sd, double* __restrict__ out_u) {
  for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS) {
    const Philox4 r = philox4x32_10((uint32_t)(i >> 1), 0u, sid, 0u, k0, k1);
    const int w = (int)(i & 1) * 2;
    const double u1 = ((double)r.v[w] + 1.0) * (1.0 / 4294967296.0);
    const double u2 = ((double)r.v[w + 1] + 1.0) * (1.0 / 4294967296.0);
    if (out_u) { out_u[2 * i] = u1; out_u[2 * i + 1] = u2; }
    const double rad = sqrt(-2.0 * log(u1));
    const double z = rad * cos(6.283185307179586 * u2);
    const double t = sd * z;
    y[i] = (float)(((double)x[i] + mean) + t);
  }
}

constexpr int64_t IT_MAX_N = (int64_t)1 << 31;

}  // namespace

extern "C" {

int fplx_channel_minmax(const float* x, int64_t n, float lo, int use_lo, float hi, int use_hi, void* ws, size_t ws_bytes,
                        float* out4, fplx_stream_t stream) {
  FPLX_REQUIRE(x && out4 && ws, FPLX_E_NULL, "channel_minmax: null pointer");
  FPLX_REQUIRE(n > 0 && n < IT_MAX_N, FPLX_E_BADSHAPE, "channel_minmax: n = %lld outside [1, 2^31)", (long long)n);
  FPLX_REQUIRE(ws_bytes >= 4 * sizeof(uint32_t), FPLX_E_WORKSPACE, "channel_minmax: workspace %zu < 16", ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* keys = (uint32_t*)ws;
  minmax_init_k<<<1, 64, 0, st>>>(keys);
  minmax_k<<<min(it_grid(n), IT_MAX_BLOCKS / 2), IT_THREADS, 0, st>>>(x, n, lo, use_lo, hi, use_hi, keys);
  minmax_final_k<<<1, 64, 0, st>>>(keys, out4);
  return fplx_check_launch("channel_minmax");
}

size_t fplx_select_ws_bytes(void) { return SEL_WORDS * sizeof(uint32_t); }

int fplx_select_kth(const float* x, int64_t n, const int64_t* ranks, int nranks, float* out, void* ws, size_t ws_bytes,
                    fplx_stream_t stream) {
  FPLX_REQUIRE(x && ranks && out && ws, FPLX_E_NULL, "select_kth: null pointer");
  FPLX_REQUIRE(n > 0 && n < IT_MAX_N, FPLX_E_BADSHAPE, "select_kth: n = %lld outside [1, 2^31)", (long long)n);
  FPLX_REQUIRE(nranks >= 1 && 2 * nranks <= SEL_MAX, FPLX_E_BADSHAPE, "select_kth: %d ranks, 1..%d supported", nranks,
               SEL_MAX / 2);
  FPLX_REQUIRE(ws_bytes >= fplx_select_ws_bytes(), FPLX_E_WORKSPACE, "select_kth: workspace %zu < %zu", ws_bytes,
               fplx_select_ws_bytes());
  SelRanks r;
  memset(&r, 0, sizeof(r));
  r.nr = 2 * nranks;
  for (int j = 0; j < nranks; ++j) {
    FPLX_REQUIRE(ranks[j] >= 0 && ranks[j] < n, FPLX_E_BADSHAPE, "select_kth: rank %lld outside [0, %lld)", (long long)ranks[j],
                 (long long)n);
    r.k[2 * j] = (uint32_t)ranks[j];
    r.k[2 * j + 1] = (uint32_t)(ranks[j] + 1 < n ? ranks[j] + 1 : n - 1);
  }
  hipStream_t st = (hipStream_t)stream;
  uint32_t* w = (uint32_t*)ws;
  select_init_k<<<1, IT_THREADS, 0, st>>>(w, r);
  for (int pass = 0; pass < 4; ++pass) {
    select_hist_k<<<it_grid(n), IT_THREADS, 0, st>>>(x, n, w, pass);
    select_scan_k<<<1, IT_THREADS, 0, st>>>(w, pass, out);
  }
  return fplx_check_launch("select_kth");
}

int fplx_clip_affine(const float* x, float* y, int64_t n, float v0, float v1, float a, float b, fplx_stream_t stream) {
  FPLX_REQUIRE(x && y, FPLX_E_NULL, "clip_affine: null pointer");
  FPLX_REQUIRE(n > 0, FPLX_E_BADSHAPE, "clip_affine: empty volume");
  clip_affine_k<<<it_grid(n), IT_THREADS, 0, (hipStream_t)stream>>>(x, y, n, v0, v1, a, b);
  return fplx_check_launch("clip_affine");
}

int fplx_clip_affine_dev(const float* x, float* y, int64_t n, const float* v0, const float* v1, const float* a,
                         const float* hi, fplx_stream_t stream) {
  FPLX_REQUIRE(x && y && v0 && v1 && a && hi, FPLX_E_NULL, "clip_affine_dev: null pointer");
  FPLX_REQUIRE(n > 0, FPLX_E_BADSHAPE, "clip_affine_dev: empty volume");
  clip_affine_dev_k<<<it_grid(n), IT_THREADS, 0, (hipStream_t)stream>>>(x, y, n, v0, v1, a, hi);
  return fplx_check_launch("clip_affine_dev");
}

int fplx_threshold_replace(const float* x, float* y, int64_t n, float t_lo, float r_lo, int use_lo, float t_hi, float r_hi,
                           int use_hi, fplx_stream_t stream) {
  FPLX_REQUIRE(x && y, FPLX_E_NULL, "threshold_replace: null pointer");
  FPLX_REQUIRE(n > 0, FPLX_E_BADSHAPE, "threshold_replace: empty volume");
  threshold_replace_k<<<it_grid(n), IT_THREADS, 0, (hipStream_t)stream>>>(x, y, n, t_lo, r_lo, use_lo, t_hi, r_hi, use_hi);
  return fplx_check_launch("threshold_replace");
}

int fplx_normalize_range(const float* x, const float* noise, float* y, int64_t n, float v0, int use_v0, float v1, int use_v1,
                         void* ws, size_t ws_bytes, float* out_mean_std, fplx_stream_t stream) {
  FPLX_REQUIRE(x && noise && y, FPLX_E_NULL, "normalize_range: null pointer");
  FPLX_REQUIRE(n > 0, FPLX_E_BADSHAPE, "normalize_range: empty volume");
  FPLX_REQUIRE(ws && ws_bytes >= 3 * IT_ROWS * sizeof(double), FPLX_E_WORKSPACE, "normalize_range: workspace %zu < %zu",
               ws_bytes, 3 * IT_ROWS * sizeof(double));
  hipStream_t st = (hipStream_t)stream;
  double* sums = (double*)ws;
  double* devs = sums + IT_ROWS;
  double* cnt = devs + IT_ROWS;
  Range rg;
  rg.v0 = v0; rg.v1 = v1; rg.use0 = use_v0; rg.use1 = use_v1;
  range_sum_k<<<IT_ROWS, IT_THREADS, 0, st>>>(x, n, rg, sums, cnt);
  range_dev_k<<<IT_ROWS, IT_THREADS, 0, st>>>(x, n, rg, sums, cnt, devs);
  range_apply_k<<<it_grid(n), IT_THREADS, 0, st>>>(x, noise, y, n, rg, sums, cnt, devs, out_mean_std);
  return fplx_check_launch("normalize_range");
}

int fplx_gamma(const float* x, float* y, int64_t n, const float* vmin, const float* vmax, float gamma, fplx_stream_t stream) {
  FPLX_REQUIRE(x && y && vmin && vmax, FPLX_E_NULL, "gamma: null pointer");
  FPLX_REQUIRE(n > 0, FPLX_E_BADSHAPE, "gamma: empty volume");
  gamma_k<<<it_grid(n), IT_THREADS, 0, (hipStream_t)stream>>>(x, y, n, vmin, vmax, gamma);
  return fplx_check_launch("gamma");
}

int fplx_add_noise_f64(const float* x, const double* noise, float* y, int64_t n, fplx_stream_t stream) {
  FPLX_REQUIRE(x && noise && y, FPLX_E_NULL, "add_noise_f64: null pointer");
  FPLX_REQUIRE(n > 0, FPLX_E_BADSHAPE, "add_noise_f64: empty volume");
  add_noise_f64_k<<<it_grid(n), IT_THREADS, 0, (hipStream_t)stream>>>(x, noise, y, n);
  return fplx_check_launch("add_noise_f64");
}

int fplx_add_noise_philox(const float* x, float* y, int64_t n, uint64_t seed, uint32_t stream_id, double mean, double sigma,
                          double* out_uniforms, fplx_stream_t stream) {
  FPLX_REQUIRE(x && y, FPLX_E_NULL, "add_noise_philox: null pointer");
  FPLX_REQUIRE(n > 0 && n < IT_MAX_N, FPLX_E_BADSHAPE, "add_noise_philox: n = %lld outside [1, 2^31)", (long long)n);
  add_noise_philox_k<<<it_grid(n), IT_THREADS, 0, (hipStream_t)stream>>>(x, y, n, (uint32_t)seed, (uint32_t)(seed >> 32),
                                                                         stream_id, mean, sigma, out_uniforms);
  return fplx_check_launch("add_noise_philox");
}

}  // extern "C"
