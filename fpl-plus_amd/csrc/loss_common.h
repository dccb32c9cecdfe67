// What the two segmentation-loss families (loss_filter.hip, loss_ext.hip) share: the class / block limits, the number of
// partial rows of a pass and the softmax of one voxel.  Kernels stay in their own files.
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

}  // namespace
