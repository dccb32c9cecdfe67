// Every function one .hip file of the library defines and another one calls, declared ONCE: the definers include this
// header as well as the users, so a definition that drifts from its declaration is a compile error (all of them are
// extern "C": a stale hand copy would still link, and read garbage).  None of them is exported (-fvisibility=hidden; the
// public ABI is include/fplx.h).
// Launchers return 1 if they launched, 0 if the layer / the operands are not theirs (the caller goes on to the next
// kernel), < 0 (FPLX_E_*) on error; the *_ok / *_rows / *_ws_bytes queries are pure host functions of the shape and the
// tuning table.  Operands are bf16 NDHWC with a leading dimension (elements per voxel) unless a comment says otherwise.
#pragma once
#include "common.h"

extern "C" {

// ---- conv_march.hip: depth-march forward of the 3x3x3 convolution (Cin 32 | 64 | 128)
int fplx_march_ok(int n, int d, int h, int w, int cin, int cout);
int fplx_march_rows(int n, int d, int h, int w, int cin, int cout);        // statistics rows = blocks along x
// Cin = 32: 2 = the one-wave-per-SIMD kernels, 0 = the 8-wave kernel; Cin >= 64: the footprint width (16 | 32)
int fplx_march_variant(int n, int d, int h, int w, int cin, int cout);
// x1 / y1: second half of a split input / output; twod: the pack is a Conv2d in the middle depth plane
int fplx_march_conv3d_fwd(const void* x, int64_t ldx, const void* wp, const float* bias, void* y, int64_t ldy, int n, int d,
                          int h, int w, int cin, int cout, float* stats, hipStream_t st, const void* x1, void* y1, int twod);
// slope != NULL (inference): PReLU in the write-out, no statistics; x read modulo nmod0 samples (0: all of them)
int fplx_march_conv3d_fwd_act(const void* x, int64_t ldx, const void* wp, const float* bias, void* y, int64_t ldy, int n,
                              int d, int h, int w, int cin, int cout, float* stats, hipStream_t st, const void* x1, void* y1,
                              int twod, const float* slope, int nmod0);

// ---- conv_brick.hip: brick forward of the 3x3x3 convolution (Cin >= 64, Cout % 64 == 0)
int fplx_brick_ok(int n, int d, int h, int w, int cin, int cout);
int fplx_brick_first(int n, int d, int h, int w, int cin, int cout);       // ... and ahead of the march kernels
// for a layer fplx_brick_ok accepts: geometry (0 = 4x8x8, 1 = 5x4x8), Cin split (1 = none), number of bricks; returns ok
int fplx_brick_plan(int n, int d, int h, int w, int cin, int cout, int* geo, int* ksplit, int* bricks);
// ksplit > 1: writes partial[ksplit][V][cout] fp32, the caller finishes; x1: second half of a split input (slope form only)
int fplx_brick_conv3d_fwd_act(const void* x, int64_t ldx, const void* wp, const float* bias, void* y, int64_t ldy, int n,
                              int d, int h, int w, int cin, int cout, float* stats, float* partial, int geo, int ksplit,
                              hipStream_t st, const float* slope, const void* x1, int nmod0);

// ---- conv_wgrad.hip: rolling-window weight gradient of the 3x3x3 convolution
// shape and knobs only (mid: the Conv2d-per-slice form, splitx: x given as two tensors of Cin / 2 channels)
int fplx_wgroll_ok(int n, int d, int h, int w, int cin, int cout, int mid, int splitx);
size_t fplx_wgroll_ws_bytes(int n, int d, int h, int w, int cin, int cout);                // the larger of the 3D and the 2D form's
// for a layer fplx_wgroll_ok accepts; dw fp32 [Cout][Cin][27] ([Cout][Cin][3][3] with mid)
int fplx_wgroll_conv3d_wgrad(const void* x, int64_t ldx, const void* dy, int64_t ldy, float* dw, int n, int d, int h, int w,
                             int cin, int cout, void* ws, size_t ws_bytes, hipStream_t st, const void* x1, int mid);

// ---- conv_mfma.hip: dispatch of the 3x3x3 bf16 convolution (mid: 27-tap pack of a Conv2d per depth slice) and the
// transposed convolutions
int fplx_mfma_conv3d_plan(int n, int d, int h, int w, int cin, int cout, int mid, int* kernel, int* geo, int* ksplit);
int fplx_mfma_conv3d_stats_rows(int n, int d, int h, int w, int cin, int cout, int mid);    // 0: not an MFMA layer
size_t fplx_mfma_conv3d_fwd_ws_bytes(int n, int d, int h, int w, int cin, int cout, int mid);
int fplx_mfma_conv3d_fwd(const void* x, int64_t ldx, const void* wp, const float* bias, void* y, int64_t ldy, int n, int d,
                         int h, int w, int cin, int cout, float* stats, void* ws, size_t ws_bytes, int mid, hipStream_t st);
int fplx_mfma_conv3d_act_ok(int n, int d, int h, int w, int cin, int cout, int mid);
int fplx_mfma_conv3d_act_cat2_ok(int n, int d, int h, int w, int cin, int cout, int mid);
int fplx_mfma_conv3d_fwd_act(const void* x, int64_t ldx, const void* wp, const float* bias, const float* slope, void* y,
                             int64_t ldy, int n, int d, int h, int w, int cin, int cout, void* ws, size_t ws_bytes, int mid,
                             hipStream_t st);
int fplx_mfma_conv3d_fwd_act_cat2(const void* x0, const void* x1, int64_t ldx, const void* wp, const float* bias,
                                  const float* slope, void* y, int64_t ldy, int n, int d, int h, int w, int cin, int cout,
                                  int nmod0, hipStream_t st);
int fplx_mfma_conv3d_wgrad_cit(int n, int d, int h, int w, int cin, int cout);             // ci tiles per block of the footprint march
size_t fplx_mfma_conv3d_wgrad_ws_bytes(int n, int d, int h, int w, int cin, int cout);
// x1: second half of a split Cin = 64 input; mid: only the middle-plane taps, dw fp32 [Cout][Cin][3][3]
int fplx_mfma_conv3d_wgrad(const void* x, int64_t ldx, const void* dy, int64_t ldy, float* dw, int n, int d, int h, int w,
                           int cin, int cout, void* ws, size_t ws_bytes, hipStream_t st, const void* x1, int mid);
// sums the per-block partial tiles [nblk][npairs][27][32][32] of a weight-gradient kernel into dw; FPLX_OK or < 0
int fplx_wgrad_reduce_launch(const float* part, int nblk, int npairs, int cin, int cout, float* dw, int mid, hipStream_t st);
// sd = 2: ConvTranspose3d(k=2,s=2); sd = 1: ConvTranspose2d(k=2,s=2) on every depth slice
int fplx_mfma_deconv2_fwd(const void* x, int64_t ldx, const void* wf, const float* bias, void* y, int64_t ldy, int n, int d,
                          int h, int w, int cin, int cout, int sd, hipStream_t st);
int fplx_mfma_deconv2_dgrad(const void* dy, int64_t ldy, const void* wb, void* dx, int64_t ldx, int n, int d, int h, int w,
                            int cin, int cout, int sd, hipStream_t st);
size_t fplx_mfma_deconv2_wgrad_ws_bytes(int n, int d, int h, int w, int cin, int cout);
int fplx_mfma_deconv2_wgrad(const void* x, int64_t ldx, const void* dy, int64_t ldy, float* dw, float* db, int n, int d,
                            int h, int w, int cin, int cout, void* ws, size_t ws_bytes, int sd, hipStream_t st);

// ---- conv_edge.hip: the stem (fp32 NCDHW in, in_chns <= 4) and the out_conv (classes <= 4, fp32 NCDHW out)
int fplx_edge_stem_rows(int n, int d, int h, int w, int cin, int cout);                    // 0: not a stem layer
int fplx_edge_stem_fwd(const float* x, const void* wf, const float* bias, void* y, int64_t ldy, int n, int d, int h, int w,
                       int cin, int cout, float* stats, hipStream_t st);
size_t fplx_edge_stem_wgrad_ws_bytes(int n, int d, int h, int w, int cin, int cout);
int fplx_edge_stem_wgrad(const float* x, const void* dy, int64_t ldy, float* dw, int n, int d, int h, int w, int cin,
                         int cout, void* ws, hipStream_t st);
int fplx_edge_stem_wgrad_bn(const float* x, const void* dy, int64_t ldy, float* dw, int n, int d, int h, int w, int cin,
                            int cout, void* ws, hipStream_t st, const void* y, int64_t ldyy, const float* mean,
                            const float* rstd, const float* scale, const float* shift, const float* slope, const float* coef);
int fplx_edge_outconv_fwd(const void* x, int64_t ldx, const float* wf, const float* bias, float* out, int n, int d, int h,
                          int w, int cin, int ncls, hipStream_t st);
int fplx_edge_outconv_dgrad(const float* dl, const void* wb, void* dx, int64_t ldx, int n, int d, int h, int w, int c0,
                            int ncls, hipStream_t st);
size_t fplx_edge_outconv_wgrad_ws_bytes(int n, int d, int h, int w, int c0, int ncls);
int fplx_edge_outconv_wgrad(const void* x, int64_t ldx, const float* dl, float* dw, int n, int d, int h, int w, int c0,
                            int ncls, void* ws, hipStream_t st);
// the forms fused with the last site's BatchNorm + PReLU (include/fplx.h: fplx_outconv_*_bn)
int fplx_edge_outconv_bn_ok(int n, int d, int h, int w, int c0, int ncls);
int fplx_edge_outconv_bn_rows(int n, int d, int h, int w, int ncls);
int fplx_edge_outconv_fwd_bn(const void* y, int64_t ldy, const float* scale, const float* shift, const float* slope, void* a,
                             int64_t lda, const float* wf, const float* bias, float* out, int n, int d, int h, int w, int c0,
                             int ncls, hipStream_t st);
int fplx_edge_outconv_dgrad_bn(int mode, const float* dl, const void* wb, const void* y, int64_t ldy, const float* mean,
                               const float* rstd, const float* scale, const float* shift, const float* slope,
                               const float* coef, float* part, void* dy, int64_t lddy, int n, int d, int h, int w, int c0,
                               int ncls, hipStream_t st);
size_t fplx_edge_outconv_wgrad_bn_ws_bytes(int n, int d, int h, int w, int c0, int ncls);
int fplx_edge_outconv_wgrad_bn(const void* y, int64_t ldy, const float* scale, const float* shift, const float* slope,
                               const float* dl, float* dw, float* db, int n, int d, int h, int w, int c0, int ncls, void* ws,
                               hipStream_t st);

}  // extern "C"
