// General-geometry kernels (conv_any.hip, norm_any.hip): the routes that conv.hip / norm.hip take for the shapes their
// specialised kernels refuse -- maps that are not square powers of two in [8, 128] (any H x W), GroupNorm rows whose
// H*W is not a power of two, float4 helpers on rows whose length is not a multiple of 4.
#pragma once
#include "common.h"

// Direct convolution at any H x W (runtime geometry; the same packed weights as conv_mfma_kernel).
// H, W = the grid the output tiles run over: the OUTPUT size for modes 0 / 1 / 2, the dY size for mode 4 (whose output is
// 2H x 2W).  x2 / C1: 1x1 input concatenation; y2 / C1o: 1x1 output split (dgrad of a conv on a concatenation).
int vfi_conv_any_fwd(const float* x, const float* x2, int C1, const float* w_packed, const float* bias,
                     const float* view_bias, const float* residual, float* y, float* y2, int C1o, float* ws, long ws_floats,
                     int S, int Cin, int Cout, int H, int W, int KS, int mode, hipStream_t st);
long vfi_conv_any_fwd_ws_floats(int S, int Cin, int Cout, int H, int W, int KS);
// the plan of that launch, host only: out = {npt (64-pixel units per tile), nblk (workgroups per K split), ks (K splits
// after the workspace clamp)}
void vfi_conv_any_fwd_plan(int S, int Cin, int Cout, int H, int W, int KS, int mode, bool split_out, bool has_ws,
                           long ws_floats, int out[3]);
// Weight gradient at any H x W (output size), modes 0 / 1 / 2.  desc9 != null: the slab sum is left to the caller's
// deferred vf_wino44_reduce_multi launch (desc9 receives the row, *nblocks its workgroup count).
int vfi_conv_any_wgrad(const float* x, const float* x2, int C1, const float* dy, float* dw, float* ws, long ws_floats, int S,
                       int Cin, int Cout, int H, int W, int KS, int mode, hipStream_t st, long long* desc9, int* nblocks);
long vfi_conv_any_wgrad_ws_floats(int S, int Cin, int Cout, int H, int W, int KS);

// GroupNorm(+Swish) forward / backward at any HW >= 1: one workgroup per (view, group), fixed-order reductions.
int vfi_gn_any_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int S, int C,
                   int HW, int groups, float eps, int silu, hipStream_t st);
int vfi_gn_any_bwd(const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                   const float* dy, const float* addend, const float* addend2, float* dx, float* dgamma_part,
                   float* dbeta_part, int S, int C, int HW, int groups, int silu, hipStream_t st);

// Scalar-row helpers (len / HW not a multiple of 4)
int vfi_rowsum_any(const float* x, float* out, int rows, int len, hipStream_t st);
int vfi_bias_grad_any(const float* dy, float* db, float* dvb, int S, int C, int HW, hipStream_t st);
