// Crop, bounding-box and label transforms on the GPU: the kernels behind CenterCrop / CropWithBoundingBox (and the
// inverse RandomCrop inherits), LabelConvert / LabelConvertNonzero and PartialLabelToProbability
// (PyMIC/pymic/transform/crop.py:13-167, label_convert.py:27-130, util/image_process.py:8-35,62-97,194-208).  The gathers of
// the forward crops are fplx_crop_flip (sample.hip); what is new here is
//   nonzero_bbox   numpy.nonzero's bounding box of a float32 volume: integer min / max / count only, so the result does
//                  not depend on the order in which blocks arrive;
//   label_lut      out = lut[in] on uint8 labels, the table in LDS;
//   partial_label  one-hot + pixel weight + largest label in one pass over the label;
//   paste_roi      the inverse of a crop: every output element written once, the block inside the box, zero outside.
// All of them are streams: a thread per 1-16 elements, grid-stride, at most 2048 blocks.
#include "common.h"

namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_WAVES = CL_THREADS / FPLX_WAVE;

inline int cl_grid(int64_t work) {
  int64_t g = (work + CL_THREADS - 1) / CL_THREADS;
  return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g));
}

// numpy.nonzero on float32: every bit pattern except +0.0 and -0.0 (a NaN and a denormal count)
__device__ __forceinline__ bool nonzero_bits(unsigned u) { return (u & 0x7fffffffu) != 0u; }

struct Box {
  int cnt, lo[4], hi[4];                                   // hi: largest index + 1
  __device__ __forceinline__ void clear() {
    cnt = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) { lo[a] = 0x7fffffff; hi[a] = 0; }
  }
  __device__ __forceinline__ void add(int c, int d, int h, int w) {
    ++cnt;
    lo[0] = min(lo[0], c); lo[1] = min(lo[1], d); lo[2] = min(lo[2], h); lo[3] = min(lo[3], w);
    hi[0] = max(hi[0], c + 1); hi[1] = max(hi[1], d + 1); hi[2] = max(hi[2], h + 1); hi[3] = max(hi[3], w + 1);
  }
};

__global__ void bbox_init_k(int* out) {
  if (threadIdx.x == 0) out[0] = 0;
  if (threadIdx.x >= 1 && threadIdx.x <= 4) out[threadIdx.x] = 0x7fffffff;
  if (threadIdx.x >= 5 && threadIdx.x <= 8) out[threadIdx.x] = 0;
}

// four consecutive elements starting at linear index 4 q: one index decomposition, then a carry chain
__device__ __forceinline__ void box_add_quad(Box& b, const uint4 v, unsigned q, unsigned D, unsigned H, unsigned W) {
  const unsigned u[4] = {v.x, v.y, v.z, v.w};
  if (!nonzero_bits(u[0] | u[1] | u[2] | u[3])) return;
  unsigned r = q << 2;
  unsigned w = r % W; r /= W;
  unsigned h = r % H; r /= H;
  unsigned d = r % D;
  unsigned c = r / D;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (nonzero_bits(u[k])) b.add((int)c, (int)d, (int)h, (int)w);
    if (++w == W) { w = 0; if (++h == H) { h = 0; if (++d == D) { d = 0; ++c; } } }
  }
}

// out = [count, min_c, min_d, min_h, min_w, max_c+1, max_d+1, max_h+1, max_w+1] (the layout of label_bbox_k).  total < 2^31.
// VEC: 16-byte loads over the first total / 4 * 4 elements (x 16-byte aligned), four of them in flight per lane; the tail
// (and everything, without VEC) element by element.  A block ends with at most nine integer atomics on out, and leaves
// out those that could not change anything: a minimum only falls and a maximum only rises, so a value that does not beat
// what out already holds never will.  (Measured on 48 x 160 x 272: 45 us with up to 2048 blocks, one quad per lane and nine
// unconditional atomics per block on one cache line; 17 us in this form.  DESIGN 1g.)
constexpr int BB_MAX_BLOCKS = 512;
template <bool VEC>
__global__ void __launch_bounds__(CL_THREADS)
nonzero_bbox_k(const unsigned* __restrict__ x, unsigned D, unsigned H, unsigned W, unsigned total, int* __restrict__ out) {
  __shared__ int red[CL_WAVES][9];
  Box b;
  b.clear();
  const unsigned tid = blockIdx.x * CL_THREADS + threadIdx.x, stride = gridDim.x * CL_THREADS;
  unsigned done = 0;
  if (VEC) {
    const unsigned quads = total >> 2;                     // < 2^29, stride <= 2^17: q + 3 stride cannot wrap
    const uint4* __restrict__ x4 = (const uint4*)x;
    for (unsigned q0 = tid; q0 < quads; q0 += 4 * stride) {
      uint4 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned q = q0 + k * stride;
        v[k] = q < quads ? x4[q] : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) box_add_quad(b, v[k], q0 + k * stride, D, H, W);
    }
    done = quads << 2;
  }
  for (unsigned i = done + tid; i < total; i += stride) {
    if (!nonzero_bits(x[i])) continue;
    unsigned r = i;
    const unsigned w = r % W; r /= W;
    const unsigned h = r % H; r /= H;
    b.add((int)(r / D), (int)(r % D), (int)h, (int)w);
  }
  // wave, then block, then the atomics of a block that saw anything
  int v[9] = {b.cnt, b.lo[0], b.lo[1], b.lo[2], b.lo[3], b.hi[0], b.hi[1], b.hi[2], b.hi[3]};
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    v[0] += __shfl_xor(v[0], o, 64);
#pragma unroll
    for (int k = 1; k < 5; ++k) v[k] = min(v[k], __shfl_xor(v[k], o, 64));
#pragma unroll
    for (int k = 5; k < 9; ++k) v[k] = max(v[k], __shfl_xor(v[k], o, 64));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const int k = threadIdx.x;
    int t = red[0][k];
    for (int wv = 1; wv < CL_WAVES; ++wv) t = k == 0 ? t + red[wv][k] : (k < 5 ? min(t, red[wv][k]) : max(t, red[wv][k]));
    int any = 0;
    for (int wv = 0; wv < CL_WAVES; ++wv) any += red[wv][0];
    if (any) {
      const int seen = k == 0 ? 0 : __hip_atomic_load(out + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (k == 0) atomicAdd(out, t);
      else if (k < 5) { if (t < seen) atomicMin(out + k, t); }
      else if (t > seen) atomicMax(out + k, t);
    }
  }
}

// out = lut[in]; in may be out.  VEC: 16 labels per lane over the first n / 16 * 16 (both pointers 16-byte aligned)
template <bool VEC>
__global__ void __launch_bounds__(CL_THREADS)
label_lut_k(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int64_t n,
            const unsigned char* __restrict__ lut256) {
  __shared__ unsigned char lut[256];
  lut[threadIdx.x] = lut256[threadIdx.x];                    // CL_THREADS == 256
  __syncthreads();
  const int64_t tid = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * CL_THREADS;
  int64_t done = 0;
  if (VEC) {
    const int64_t chunks = n >> 4;
    const uint4* in4 = (const uint4*)in;
    uint4* out4 = (uint4*)out;
    for (int64_t q = tid; q < chunks; q += stride) {
      const uint4 v = in4[q];
      unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        u[k] = (unsigned)lut[u[k] & 255u] | ((unsigned)lut[(u[k] >> 8) & 255u] << 8) | ((unsigned)lut[(u[k] >> 16) & 255u] << 16) |
               ((unsigned)lut[u[k] >> 24] << 24);
      out4[q] = make_uint4(u[0], u[1], u[2], u[3]);
    }
    done = chunks << 4;
  }
  for (int64_t i = done + tid; i < n; i += stride) out[i] = lut[in[i]];
}

// prob[k][v] = label[v] == k (k < classes), weight[v] = 1 - (label[v] == classes), *max_label = max(label).
// VEC = 4: four voxels per lane (voxels % 4 == 0 and aligned pointers: every class row then starts 16-byte aligned)
template <int VEC>
__global__ void __launch_bounds__(CL_THREADS)
partial_label_k(const unsigned char* __restrict__ lab, float* __restrict__ prob, float* __restrict__ weight, int classes,
                int64_t voxels, int* __restrict__ max_label) {
  __shared__ int red[CL_WAVES];
  int top = 0;
  const int64_t groups = voxels / VEC;
  for (int64_t g = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; g < groups; g += (int64_t)gridDim.x * CL_THREADS) {
    int l[VEC];
    if (VEC == 4) {
      const uchar4 v = ((const uchar4*)lab)[g];
      l[0] = v.x; l[1 % VEC] = v.y; l[2 % VEC] = v.z; l[3 % VEC] = v.w;
    } else {
      l[0] = lab[g];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) top = max(top, l[k]);
    for (int c = 0; c < classes; ++c) {
      float* row = prob + (int64_t)c * voxels;
      if (VEC == 4)
        ((float4*)row)[g] = make_float4(l[0] == c ? 1.f : 0.f, l[1 % VEC] == c ? 1.f : 0.f, l[2 % VEC] == c ? 1.f : 0.f,
                                        l[3 % VEC] == c ? 1.f : 0.f);
      else
        row[g] = l[0] == c ? 1.f : 0.f;
    }
    if (VEC == 4)
      ((float4*)weight)[g] = make_float4(l[0] == classes ? 0.f : 1.f, l[1 % VEC] == classes ? 0.f : 1.f,
                                         l[2 % VEC] == classes ? 0.f : 1.f, l[3 % VEC] == classes ? 0.f : 1.f);
    else
      weight[g] = l[0] == classes ? 0.f : 1.f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = top;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int wv = 1; wv < CL_WAVES; ++wv) top = max(top, red[wv]);
    // unconditional on purpose: reading the word first (to skip an atomic that cannot raise it) makes the wave wait for
    // its own stores and measured slower here (43 against 30 us on 48 x 160 x 272, four classes)
    if (top > 0) atomicMax(max_label, top);
  }
}

// out[c][d][h][w] = sub[c][d - ld][h - lh][w - lw] inside the box, 0 elsewhere: numpy.zeros + slice assignment in one pass
template <typename T>
__global__ void __launch_bounds__(CL_THREADS)
paste_roi_k(const T* __restrict__ sub, T* __restrict__ out, int C, int SD, int SH, int SW, int OD, int OH, int OW, int ld,
            int lh, int lw) {
  const int64_t total = (int64_t)C * OD * OH * OW;
  for (int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CL_THREADS) {
    int64_t r = i;
    const int w = (int)(r % OW) - lw; r /= OW;
    const int h = (int)(r % OH) - lh; r /= OH;
    const int d = (int)(r % OD) - ld; r /= OD;
    const int c = (int)r;
    const bool inside = (unsigned)d < (unsigned)SD && (unsigned)h < (unsigned)SH && (unsigned)w < (unsigned)SW;
    out[i] = inside ? sub[(((int64_t)c * SD + d) * SH + h) * SW + w] : (T)0;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// c * d * h * w of positive ints if it is below 2^bits (bits <= 52: the double product is exact there), else -1
inline int64_t cl_elems(int c, int d, int h, int w, int bits) {
  const double t = (double)c * (double)d * (double)h * (double)w;
  return t < (double)((int64_t)1 << bits) ? (int64_t)t : -1;
}

}  // namespace

extern "C" {

int fplx_nonzero_bbox(const float* x, int c, int d, int h, int w, int* out9, fplx_stream_t stream) {
  FPLX_REQUIRE(x && out9, FPLX_E_NULL, "nonzero_bbox: null pointer");
  FPLX_REQUIRE(c > 0 && d > 0 && h > 0 && w > 0, FPLX_E_BADSHAPE, "nonzero_bbox: bad shape %dx%dx%dx%d", c, d, h, w);
  const int64_t total = cl_elems(c, d, h, w, 31);
  FPLX_REQUIRE(total > 0, FPLX_E_BADSHAPE, "nonzero_bbox: %dx%dx%dx%d is 2^31 elements or more", c, d, h, w);
  hipStream_t st = (hipStream_t)stream;
  bbox_init_k<<<1, 64, 0, st>>>(out9);
  if (aligned16(x) && total >= 4)
    nonzero_bbox_k<true><<<min(cl_grid(total / 16), BB_MAX_BLOCKS), CL_THREADS, 0, st>>>((const unsigned*)x, d, h, w,
                                                                                         (unsigned)total, out9);
  else
    nonzero_bbox_k<false><<<min(cl_grid(total), BB_MAX_BLOCKS), CL_THREADS, 0, st>>>((const unsigned*)x, d, h, w,
                                                                                    (unsigned)total, out9);
  return fplx_check_launch("nonzero_bbox");
}

int fplx_label_lut(const uint8_t* in, uint8_t* out, int64_t n, const uint8_t* lut256, fplx_stream_t stream) {
  FPLX_REQUIRE(in && out && lut256, FPLX_E_NULL, "label_lut: null pointer");
  FPLX_REQUIRE(n > 0, FPLX_E_BADSHAPE, "label_lut: %lld labels", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  if (aligned16(in) && aligned16(out) && n >= 16)
    label_lut_k<true><<<cl_grid(n / 16), CL_THREADS, 0, st>>>(in, out, n, lut256);
  else
    label_lut_k<false><<<cl_grid(n), CL_THREADS, 0, st>>>(in, out, n, lut256);
  return fplx_check_launch("label_lut");
}

int fplx_partial_label_to_probability(const uint8_t* label, float* prob, float* weight, int class_num, int64_t voxels,
                                      int* max_label, fplx_stream_t stream) {
  FPLX_REQUIRE(label && prob && weight && max_label, FPLX_E_NULL, "partial_label_to_probability: null pointer");
  FPLX_REQUIRE(class_num > 0 && class_num <= 255 && voxels > 0, FPLX_E_BADSHAPE,
               "partial_label_to_probability: %d classes (1..255) over %lld voxels", class_num, (long long)voxels);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(max_label, 0, sizeof(int), st) != hipSuccess)
    return fplx_fail(FPLX_E_HIP, "partial_label_to_probability: memset failed");
  if (voxels % 4 == 0 && ((uintptr_t)label & 3u) == 0 && aligned16(prob) && aligned16(weight))
    partial_label_k<4><<<cl_grid(voxels / 4), CL_THREADS, 0, st>>>(label, prob, weight, class_num, voxels, max_label);
  else
    partial_label_k<1><<<cl_grid(voxels), CL_THREADS, 0, st>>>(label, prob, weight, class_num, voxels, max_label);
  return fplx_check_launch("partial_label_to_probability");
}

int fplx_paste_roi(const void* sub, void* out, int elem_bytes, int c, int sd, int sh, int sw, int od, int oh, int ow,
                   int lo_d, int lo_h, int lo_w, fplx_stream_t stream) {
  FPLX_REQUIRE(sub && out, FPLX_E_NULL, "paste_roi: null pointer");
  FPLX_REQUIRE(c > 0 && sd > 0 && sh > 0 && sw > 0 && lo_d >= 0 && lo_h >= 0 && lo_w >= 0 && sd <= od && sh <= oh && sw <= ow &&
                   lo_d <= od - sd && lo_h <= oh - sh && lo_w <= ow - sw,
               FPLX_E_BADSHAPE, "paste_roi: box outside the output volume");
  const int64_t total = cl_elems(c, od, oh, ow, 40);
  FPLX_REQUIRE(total > 0, FPLX_E_BADSHAPE, "paste_roi: %dx%dx%dx%d is 2^40 elements or more", c, od, oh, ow);
  hipStream_t st = (hipStream_t)stream;
  const int g = cl_grid(total);
  if (elem_bytes == 4)
    paste_roi_k<float><<<g, CL_THREADS, 0, st>>>((const float*)sub, (float*)out, c, sd, sh, sw, od, oh, ow, lo_d, lo_h, lo_w);
  else if (elem_bytes == 1)
    paste_roi_k<unsigned char><<<g, CL_THREADS, 0, st>>>((const unsigned char*)sub, (unsigned char*)out, c, sd, sh, sw, od,
                                                         oh, ow, lo_d, lo_h, lo_w);
  else
    return fplx_fail(FPLX_E_BADDTYPE, "paste_roi: element size %d", elem_bytes);
  return fplx_check_launch("paste_roi");
}

}  // extern "C"
