// Connected components and KeepLargestComponent (reference: PyMIC/pymic/util/post_process.py:19-49 on top of
// util/image_process.py:139-163, get_largest_k_components = scipy.ndimage.label with the 6-neighbour structure
// generate_binary_structure(3, 1), component sizes, keep the largest).
//
// Block-based union-find (Playne & Hawick 2018; Allegretti et al. 2019, BUF) on a uint8 volume [d][h][w]:
//  1. cc_local_k    one workgroup per box tile of at most CC_TILE voxels: union-find in LDS (LDS atomics), then every
//                   voxel's global parent = the global linear index of its tile-local root (-1: background) and, when
//                   sizes are wanted, lcount[root] = voxels of the tile-local component (0 at every other voxel).
//  2. cc_merge_k    one thread per voxel on a tile's low faces whose neighbour lies in the previous tile: the monotone
//                   merge loop (find both roots, hook the larger to the smaller by an agent-scope atomicMin, continue
//                   from the value the atomic returned).
//  3. cc_flatten_k  label[x] = root(x); a tile-local root that is not a final root adds its lcount to its final root's.
//  4. cc_max_k      the per-class maximum cmax[256] of the final roots' sizes (LDS per block, then global atomicMax).
//  5. cc_apply_k    out[x] = seg[x] where the size of x's component is its class's maximum, else 0.
// The root of every set is its minimum linear index, so a component's label is the C-order index of its first voxel:
// canonical (comparable with scipy after relabelling) and, every quantity being an integer, bitwise reproducible.
//
// Coherence.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's stores, so inside
// cc_merge_k a plain load of parent[] may return a value another workgroup has since lowered.  That is safe because:
//  - parent[] is written in cc_merge_k ONLY by agent-scope atomicMin, so every entry only ever decreases, and every value
//    it ever held is an ancestor of the entry's voxel (a hook points a root at a smaller member of the other set; path
//    halving points a voxel at its grandparent).  A stale value is therefore still an ancestor: `find` through stale
//    values ends at some ancestor that still is, or once was, a root - never in another set.
//  - the loop's exits do not depend on seeing another workgroup's plain store: "both finds reached the same index"
//    proves a common ancestor whatever was stale, and "the atomicMin returned b" is the atomic's own, current answer.
//    When the atomic returns b' != b, b' is a current ancestor of b and the loop continues from it; the larger of the two
//    indices under merge strictly decreases every round, so the loop ends without any other thread's store becoming
//    visible.
//  - the cross-workgroup results (final parents, sizes, maxima) are read only by later launches.
// Every loop is capped (CC_BUDGET steps per thread); a thread that reaches the cap sets the error word by a vector
// atomic and exits, and the host turns the word into an exception instead of a hang.
#include "common.h"

namespace {

constexpr int CC_THREADS = 256;          // cc_max_k relies on one thread per class value
constexpr int CC_TILE = 4096;            // voxels per tile (LDS: 4 + 4 + 1 bytes per voxel = 36 KB)
constexpr int CC_BUDGET = 1 << 20;       // find steps + merge rounds per thread before the error word is set
constexpr int CC_HEAD = 320;             // ints in front of the per-voxel workspace: [0] error word, [64, 320) cmax
constexpr int CC_CMAX = 64;

struct CcGeo {
  int d, h, w;          // volume
  int bd, bh, bw;       // tile box
  int nd, nh, nw;       // tiles per axis; tile t = (tz * nh + ty) * nw + tx
  int per_class;        // 0: binary (both nonzero), 1: per class (equal and nonzero)
};

__device__ __forceinline__ bool cc_join(int a, int b, int per_class) {
  return a != 0 && b != 0 && (!per_class || a == b);
}

__device__ __forceinline__ void cc_error(int* err, int code) {
  __hip_atomic_fetch_or(err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- LDS union-find of one tile (one workgroup: LDS is coherent inside it, the loads are atomic only to keep the
// compiler from reusing a value across iterations)
__device__ __forceinline__ int lds_ld(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int lds_find(int* par, int x, int& budget) {
  int p = lds_ld(&par[x]);
  while (p != x && budget > 0) {
    x = p;
    p = lds_ld(&par[x]);
    --budget;
  }
  return x;
}

__device__ __forceinline__ void lds_union(int* par, int a, int b, int& budget) {
  while (budget > 0) {
    a = lds_find(par, a, budget);
    b = lds_find(par, b, budget);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(&par[b], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == b) return;
    b = old;
    --budget;
  }
}

__global__ void __launch_bounds__(CC_THREADS) cc_local_k(const uint8_t* __restrict__ seg, int* __restrict__ label,
                                                         int* __restrict__ lcount, int* __restrict__ err, CcGeo g) {
  __shared__ int par[CC_TILE];
  __shared__ int cnt[CC_TILE];
  __shared__ uint8_t val[CC_TILE];
  const int t = blockIdx.x;
  const int tx = t % g.nw, ty = (t / g.nw) % g.nh, tz = t / (g.nw * g.nh);
  const int z0 = tz * g.bd, y0 = ty * g.bh, x0 = tx * g.bw;
  const int n = g.bd * g.bh * g.bw, plane = g.bh * g.bw;
  for (int l = threadIdx.x; l < n; l += CC_THREADS) {
    const int lx = l % g.bw, ly = (l / g.bw) % g.bh, lz = l / plane;
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    const bool in = z < g.d && y < g.h && x < g.w;
    val[l] = in ? seg[((int64_t)z * g.h + y) * g.w + x] : 0;        // outside the volume: background, joins nothing
    par[l] = l;
    cnt[l] = 0;
  }
  __syncthreads();
  int budget = CC_BUDGET;
  for (int l = threadIdx.x; l < n; l += CC_THREADS) {
    const int s = val[l];
    if (!s) continue;
    const int lx = l % g.bw, ly = (l / g.bw) % g.bh, lz = l / plane;
    if (lx > 0 && cc_join(s, val[l - 1], g.per_class)) lds_union(par, l, l - 1, budget);
    if (ly > 0 && cc_join(s, val[l - g.bw], g.per_class)) lds_union(par, l, l - g.bw, budget);
    if (lz > 0 && cc_join(s, val[l - plane], g.per_class)) lds_union(par, l, l - plane, budget);
  }
  __syncthreads();
  for (int l = threadIdx.x; l < n; l += CC_THREADS) {
    if (!val[l]) continue;
    const int r = lds_find(par, l, budget);
    par[l] = r;                                   // only this thread reads par[l] below; concurrent finds see l's root either way
    if (lcount) atomicAdd(&cnt[r], 1);
  }
  if (budget <= 0) cc_error(err, 1);
  __syncthreads();
  for (int l = threadIdx.x; l < n; l += CC_THREADS) {
    const int lx = l % g.bw, ly = (l / g.bw) % g.bh, lz = l / plane;
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    if (z >= g.d || y >= g.h || x >= g.w) continue;
    const int gi = (z * g.h + y) * g.w + x;
    int root = -1, c = 0;
    if (val[l]) {
      const int r = par[l];
      const int rx = r % g.bw, ry = (r / g.bw) % g.bh, rz = r / plane;
      root = ((z0 + rz) * g.h + (y0 + ry)) * g.w + (x0 + rx);       // box order = C order: the local minimum is the global one
      c = (r == l) ? cnt[l] : 0;
    }
    label[gi] = root;
    if (lcount) lcount[gi] = c;
  }
}

// ---- global union-find (see the coherence argument at the top of the file)
__device__ __forceinline__ int g_find(int* par, int x, int& budget) {
  int p = par[x];                                  // plain load: possibly stale, always an ancestor
  while (p != x) {
    if (--budget <= 0) return -1;
    const int gp = par[p];
    if (gp != p) __hip_atomic_fetch_min(&par[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // path halving, monotone
    x = p;
    p = gp;
  }
  return x;
}

// merges the sets of a and b; false when the budget ran out
__device__ __forceinline__ bool g_union(int* par, int a, int b, int& budget) {
  while (true) {
    a = g_find(par, a, budget);
    b = g_find(par, b, budget);
    if (a < 0 || b < 0) return false;
    if (a == b) return true;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(&par[b], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == b) return true;                     // b was a root and now hangs under a
    b = old;                                       // b had been hooked meanwhile: merge a with its current parent
    if (--budget <= 0) return false;
  }
}

__global__ void __launch_bounds__(CC_THREADS) cc_merge_k(const uint8_t* __restrict__ seg, int* par, int* __restrict__ err,
                                                         CcGeo g) {
  const int t = blockIdx.x;
  const int tx = t % g.nw, ty = (t / g.nw) % g.nh, tz = t / (g.nw * g.nh);
  const int z0 = tz * g.bd, y0 = ty * g.bh, x0 = tx * g.bw;
  const int ed = min(g.bd, g.d - z0), eh = min(g.bh, g.h - y0), ew = min(g.bw, g.w - x0);
  const int nz = z0 > 0 ? eh * ew : 0, ny = y0 > 0 ? ed * ew : 0, nx = x0 > 0 ? ed * eh : 0;
  const int hw = g.h * g.w;
  int budget = CC_BUDGET;
  bool ok = true;
  for (int i = threadIdx.x; i < nz + ny + nx; i += CC_THREADS) {
    int z, y, x, step, pstep;         // step: to the neighbour in the previous tile; pstep: to the previous voxel of the face
    bool has_prev;
    if (i < nz) {
      z = z0; y = y0 + i / ew; x = x0 + i % ew; step = hw; pstep = 1; has_prev = x > x0;
    } else if (i < nz + ny) {
      const int j = i - nz;
      z = z0 + j / ew; y = y0; x = x0 + j % ew; step = g.w; pstep = 1; has_prev = x > x0;
    } else {
      const int j = i - nz - ny;
      z = z0 + j / eh; y = y0 + j % eh; x = x0; step = 1; pstep = g.w; has_prev = y > y0;
    }
    const int a = (z * g.h + y) * g.w + x, b = a - step;
    const int s = seg[a];
    if (!cc_join(s, seg[b], g.per_class)) continue;
    // the previous face voxel already joins this pair's two tile-local components: nothing new to merge
    if (has_prev && cc_join(s, seg[a - pstep], g.per_class) && cc_join(seg[a - pstep], seg[b - pstep], g.per_class)) continue;
    if (!g_union(par, a, b, budget)) { ok = false; break; }
  }
  if (!ok) cc_error(err, 2);
}

__global__ void __launch_bounds__(CC_THREADS) cc_flatten_k(int* label, int* lcount, int64_t n, int* __restrict__ err) {
  bool ok = true;
  for (int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * CC_THREADS) {
    const int x = (int)i;
    int r = label[x];
    if (r < 0) continue;
    int budget = CC_BUDGET;
    for (int p = label[r]; p != r; p = label[r]) {     // after the merge launch: no writer but this kernel's own
      r = p;                                          // (which stores roots only: any value read is an ancestor)
      if (--budget <= 0) { ok = false; break; }
    }
    if (!ok) break;
    label[x] = r;
    if (lcount && r != x) {
      const int c = lcount[x];                        // a final root never adds, so no source is also a target
      if (c) atomicAdd(&lcount[r], c);
    }
  }
  if (!ok) cc_error(err, 4);
}

// per-class maxima of the root sizes: first per block in LDS, then one global atomicMax per block and class present (a
// noisy mask has hundreds of thousands of roots: one global atomic each on the same word serialised to 1.3 ms at 48x160x272)
__global__ void __launch_bounds__(CC_THREADS) cc_max_k(const uint8_t* __restrict__ seg, const int* __restrict__ label,
                                                       const int* __restrict__ lcount, int* __restrict__ cmax, int64_t n,
                                                       int per_class) {
  __shared__ int lmax[256];
  lmax[threadIdx.x] = 0;                                   // CC_THREADS == 256
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * CC_THREADS)
    if (label[i] == (int)i) atomicMax(&lmax[per_class ? seg[i] : 1], lcount[i]);
  __syncthreads();
  if (lmax[threadIdx.x] > 0) atomicMax(&cmax[threadIdx.x], lmax[threadIdx.x]);
}

__global__ void __launch_bounds__(CC_THREADS) cc_apply_k(const uint8_t* __restrict__ seg, const int* __restrict__ label,
                                                         const int* __restrict__ lcount, const int* __restrict__ cmax,
                                                         uint8_t* __restrict__ out, int64_t n, int per_class) {
  for (int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * CC_THREADS) {
    const int s = seg[i], r = label[i];
    out[i] = (r >= 0 && lcount[r] == cmax[per_class ? s : 1]) ? (uint8_t)s : (uint8_t)0;
  }
}

int cc_balanced(int n, int cap) {
  if (n <= cap) return n;
  const int k = (n + cap - 1) / cap;
  return (n + k - 1) / k;
}

CcGeo cc_geometry(int d, int h, int w, int per_class) {
  CcGeo g;
  g.d = d; g.h = h; g.w = w; g.per_class = per_class ? 1 : 0;
  g.bw = cc_balanced(w, 64);
  const int rest = CC_TILE / g.bw;                                  // >= 64
  g.bh = cc_balanced(h, d == 1 ? rest : (rest / 4 > 0 ? rest / 4 : 1));
  g.bd = cc_balanced(d, rest / g.bh);
  g.nd = (d + g.bd - 1) / g.bd;
  g.nh = (h + g.bh - 1) / g.bh;
  g.nw = (w + g.bw - 1) / g.bw;
  return g;
}

unsigned cc_grid(int64_t n) {
  const int64_t b = (n + CC_THREADS - 1) / CC_THREADS;
  return (unsigned)(b < 4096 ? b : 4096);
}

int cc_check_args(const char* what, const uint8_t* seg, const void* out, int d, int h, int w, const int* ws, size_t ws_bytes,
                  size_t need) {
  FPLX_REQUIRE(seg && out, FPLX_E_NULL, "%s: null pointer", what);
  FPLX_REQUIRE(d > 0 && h > 0 && w > 0 && (int64_t)d * h * w < ((int64_t)1 << 31), FPLX_E_BADSHAPE,
               "%s: bad shape %dx%dx%d (every dimension positive, fewer than 2^31 voxels)", what, d, h, w);
  FPLX_REQUIRE(ws, FPLX_E_NULL, "%s: no workspace", what);
  FPLX_REQUIRE(ws_bytes >= need, FPLX_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need);
  return FPLX_OK;
}

// local labelling + merge + flatten into `label`; lcount (may be NULL) receives the component sizes at the roots
int cc_run(const uint8_t* seg, const CcGeo& g, int* label, int* lcount, int* ws, hipStream_t st) {
  const int64_t n = (int64_t)g.d * g.h * g.w;
  const unsigned tiles = (unsigned)g.nd * g.nh * g.nw;
  if (hipMemsetAsync(ws, 0, sizeof(int) * CC_HEAD, st) != hipSuccess) return fplx_fail(FPLX_E_HIP, "cc: memset failed");
  cc_local_k<<<tiles, CC_THREADS, 0, st>>>(seg, label, lcount, ws, g);
  if (tiles > 1) cc_merge_k<<<tiles, CC_THREADS, 0, st>>>(seg, label, ws, g);
  cc_flatten_k<<<cc_grid(n), CC_THREADS, 0, st>>>(label, lcount, n, ws);
  return fplx_check_launch("cc_label");
}

}  // namespace

extern "C" {

int fplx_cc_label(const uint8_t* seg, int d, int h, int w, int per_class, int* labels, int* ws, size_t ws_bytes,
                  fplx_stream_t stream) {
  const int rc = cc_check_args("cc_label", seg, labels, d, h, w, ws, ws_bytes, FPLX_CC_LABEL_WS_BYTES((int64_t)d * h * w));
  if (rc) return rc;
  return cc_run(seg, cc_geometry(d, h, w, per_class), labels, nullptr, ws, (hipStream_t)stream);
}

int fplx_keep_largest_component(const uint8_t* seg, int d, int h, int w, int per_class, uint8_t* out, int* ws,
                                size_t ws_bytes, fplx_stream_t stream) {
  const int64_t n = (int64_t)d * h * w;
  const int rc = cc_check_args("keep_largest_component", seg, out, d, h, w, ws, ws_bytes, FPLX_KLC_WS_BYTES(n));
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const CcGeo g = cc_geometry(d, h, w, per_class);
  int* label = ws + CC_HEAD;
  int* lcount = label + n;
  const int r2 = cc_run(seg, g, label, lcount, ws, st);
  if (r2) return r2;
  const unsigned gmax = cc_grid(n) < 1024 ? cc_grid(n) : 1024;      // at most 1024 global atomics per class
  cc_max_k<<<gmax, CC_THREADS, 0, st>>>(seg, label, lcount, ws + CC_CMAX, n, g.per_class);
  cc_apply_k<<<cc_grid(n), CC_THREADS, 0, st>>>(seg, label, lcount, ws + CC_CMAX, out, n, g.per_class);
  return fplx_check_launch("keep_largest_component");
}

}  // extern "C"
