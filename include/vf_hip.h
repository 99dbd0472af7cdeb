/* vf_hip.h -- C ABI of libvf_hip.so, the MI355X (gfx950) kernels of the ViewFusion hot path.
 *
 * The reference (bronemos/view-fusion) has no FFI: its hot path is `model/unet.py` +
 * `model/view_fusion.py` calling stock torch ops.  Each entry point below replaces the torch
 * op(s) cited next to it.  Conventions:
 *   - raw DEVICE pointers to contiguous fp32 NCHW tensors, explicit sizes, explicit stream
 *     (`hipStream_t` passed as void*); no torch types;
 *   - every call only ENQUEUES work: no allocation, no synchronisation, no retained
 *     pointers, re-entrant, HIP-graph capturable; workspaces are passed in by the caller
 *     (the one exception: the five vf_xgmi_* MEMORY calls at the end of this file, which allocate / export / map the
 *     IPC-shared gradient arena once per process, outside any stream);
 *   - return value is a hipError_t as int (0 = success; hipErrorInvalidValue for an
 *     unsupported shape -- there is no fallback path).
 */
#ifndef VF_HIP_H
#define VF_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- GroupNorm (+Swish) : nn.GroupNorm(32,C,eps) -> Swish, unet.py:211-212,254,180-182 ----
 * Any HW >= 1 with C % groups == 0: HW a power of two >= 4 runs the register-resident kernels (norm.hip), any other
 * HW -- or a group too large for registers -- the general one-workgroup-per-(view, group) kernels (norm_any.hip). */
int vf_gn_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean /*[S*G]*/,
              float* rstd /*[S*G]*/, int S, int C, int HW, int groups, float eps, int silu, void* stream);
/* dgamma_part/dbeta_part: [S][C] per-view partials; reduce over S with vf_colsum.
 * addend (like x, or NULL) is added to dx: gradient of a second consumer of x (residual branch).
 * dx_rowsum ([S][C] or NULL): sum of dx over the map per (view, channel), excluding addend -- the gradient of
 * the conv bias / embedding bias added in front of this GroupNorm (unet.py:160-177); only filled where
 * vf_gn_bwd_emits_rowsum() says so. */
int vf_gn_bwd_emits_rowsum(int C, int HW, int groups);
/* The plan vf_gn_cat_fwd / vf_gn_cat_bwd (vf_gn_fwd / vf_gn_bwd: cat = 0) take for these arguments: host only, touches no
 * device, launches nothing; the launchers run the function that fills it.  cat: the input is the concatenation
 * [C1 | C - C1]; has_addend / has_addend2 / has_dx2: which optional pointers the backward gets (the forward's fields do
 * not depend on them).  out[12] = {
 *   [0] forward route: 0 rejected (hipErrorInvalidValue), 1 gn_fwd_kernel<NV, NT>, 2 gn_any_fwd_kernel;
 *   [1] [2] the forward's NV, NT (route 1, else 0);
 *   [3] backward route: 0 rejected, 1 gn_bwd_fused_kernel<NV, 256, 16>, 2 gn_bwd_fused_kernel<NV, NT, 64>,
 *       3 gn_bwd_rows_kernel + gn_bwd_dx_kernel (+ add_inplace_kernel per addend), 4 gn_any_bwd_kernel;
 *   [4] [5] [6] the backward's NV, NT, SEG and [7] its dynamic LDS bytes (routes 1, 2, else 0);
 *   [8] chunks, the second grid dimension of gn_bwd_dx_kernel, and [9] add_inplace_kernel launches (route 3, else 0);
 *   [10] dx_rowsum is written where one is passed (= vf_gn_bwd_emits_rowsum for a plain input);
 *   [11] channels per group (0 where groups does not divide C) }.
 * Returns hipErrorInvalidValue only for out == NULL: a refused call is a plan with route 0. */
int vf_gn_plan(int C, int HW, int groups, int cat, int C1, int has_addend, int has_addend2, int has_dx2, int* out /*[12]*/);
int vf_gn_bwd(const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
              const float* dy, const float* addend, float* dx, float* dgamma_part, float* dbeta_part,
              float* dx_rowsum, int S, int C, int HW, int groups, int silu, void* stream);
/* same on the never-materialised channel concatenation [x (C1 channels) | x2 (C - C1)] of two NCHW tensors
 * (decoder skip connections, unet.py:134); the second-consumer gradients and dx are split the same way.
 * x2 == NULL: plain input; then addend2 (or NULL) is a second full-size tensor added to dx (gradient of a third
 * consumer of x).  x2 != NULL: HW a power of two >= 4; backward with x2: single-pass shapes only
 * (vf_gn_bwd_emits_rowsum, which answers 0 wherever HW is not a power of two). */
int vf_gn_cat_fwd(const float* x, const float* x2, int C1, const float* gamma, const float* beta, float* y, float* mean,
                  float* rstd, int S, int C, int HW, int groups, float eps, int silu, void* stream);
int vf_gn_cat_bwd(const float* x, const float* x2, int C1, const float* gamma, const float* beta, const float* mean,
                  const float* rstd, const float* dy, const float* addend, const float* addend2, float* dx, float* dx2,
                  float* dgamma_part, float* dbeta_part, float* dx_rowsum, int S, int C, int HW, int groups, int silu,
                  void* stream);
/* any len / HW: rows whose length is a multiple of 4 take the float4 kernels, others a scalar kernel */
int vf_rowsum(const float* x, float* out /*[rows]*/, int rows, int len, void* stream);
/* conv epilogue gradients in one launch: db[C] (|NULL) and dvb[S][C] (|NULL) from dy[S][C][HW] */
int vf_bias_grad(const float* dy, float* db, float* dvb, int S, int C, int HW, void* stream);
int vf_colsum(const float* part /*[batch][S][C]*/, float* out /*[batch][C]*/, int batch, int S, int C,
              void* stream);
/* many column sums in one launch: desc = device int64 [n][6] rows {part, out, S, C, batch, first 64-column block};
 * total_blocks = sum over the rows of ceil(C/64) * batch.  Same arithmetic as vf_colsum per row. */
int vf_colsum_multi(const void* desc, int n, long total_blocks, void* stream);

/* ---- convolution : nn.Conv2d 3x3 / 1x1, nn.Upsample+conv, stride-2 conv,
 *      unet.py:42,189,198,214,238,255,256 (+ FeatureWiseAffine add :160-177, residual add :245,277) ---- */
int vf_conv_pack_sizes(int Cout, int Cin, int KS, long* fwd_floats, long* bwd_floats);
int vf_conv_pack_weights(const float* w_oihw, float* w_fwd, float* w_bwd /*or NULL*/, int Cout, int Cin, int KS,
                         void* stream);
/* every layer of a network in one launch; desc = device int64 [nlayers][9] rows
 * {w, w_fwd, w_bwd, Cout, Cin, KS, fwd_floats, bwd_floats, first_block}, block = 256 elements */
int vf_conv_pack_weights_multi(const void* desc, int nlayers, long total_blocks, void* stream);
/* mode 0 stride-1 | 1 stride-2 (x is 2Hx2W) | 2 nearest-x2 upsampled x (x is H/2xW/2) |
 * 4 sub-pixel dgrad of mode 1: x = dY (HxW), y = dX (2Hx2W), every
 * output parity gets its own taps (no zeros multiplied; w_packed = the dgrad pack; no epilogue operands but the
 * residual, which has dX's layout).  Mode 4 never splits K: it ignores ws / ws_floats.
 * H,W = OUTPUT size (mode 4: the dY size), any size (mode 2: both even).  The shapes the specialised kernels are
 * compiled for (square power of two in [8,128]; mode 1 / 4 up to 64, mode 2 from 16) run them (conv.hip); every other
 * geometry runs the general runtime-H,W kernels (conv_any.hip) from the same packed weights.  The same holds for
 * vf_conv_fwd_gn (general geometry: conv, then a GroupNorm launch), the 1x1 cat forms and the weight gradients. */
int vf_conv_fwd(const float* x, const float* w_packed, const float* bias /*[Cout]|NULL*/,
                const float* view_bias /*[S][Cout]|NULL*/, const float* residual /*like y|NULL*/, float* y,
                float* ws /*|NULL*/, long ws_floats, int S, int Cin, int Cout, int H, int W, int KS, int mode,
                void* stream);
/* inference fusion: a_out = [Swish](GroupNorm(groups, eps)(conv output)), the GroupNorm evaluated inside the conv's
 * split-K reduce launch where the conv runs split-K (small S: the sampler), by a GroupNorm launch behind it otherwise.
 * y: a valid output buffer; it holds the conv output afterwards if store_y != 0 (or the unfused route ran).
 * gn_stats: scratch, 2*S*groups floats. */
int vf_conv_fwd_gn(const float* x, const float* w_packed, const float* bias, const float* view_bias, const float* residual,
                   float* y, int store_y, const float* gn_gamma, const float* gn_beta, float* a_out, float* gn_stats,
                   int groups, float eps, int silu, float* ws, long ws_floats, int S, int Cin, int Cout, int H, int W,
                   int KS, int mode, void* stream);
/* The sampler's convolutions at few stacked views (model/view_fusion.py:179-214 driving model/unet.py:42,189,198,214,
 * 238,255,256 with S = 1 ... a dozen): ONE launch per layer, K split over the waves of a workgroup and summed in LDS in a
 * fixed order; reads the UNPACKED OIHW parameter.  x2 != NULL (1x1 only): input channels [C1, Cin) come from x2.
 * H = W = the output map, stride 1: mode 0, or mode 2 for 3x3 (x stored at half size, nearest-x2 upsampled on read: the
 * Upsample conv of unet.py:185-190; round 5) (vf_conv_small_supported says which layers are taken:
 * 1x1 with Cin % 4 == 0, 3x3 with Cin % 32 == 0, power-of-two maps of at least 4x4). */
int vf_conv_small_supported(int Cin, int Cout, int H, int W, int KS, int mode);
int vf_conv_small(const float* x, const float* x2 /*|NULL*/, int C1, const float* w_oihw, const float* bias /*|NULL*/,
                  const float* view_bias /*|NULL*/, const float* residual /*|NULL*/, float* y, int S, int Cin, int Cout,
                  int H, int W, int KS, int mode, void* stream);
/* The same 3x3 launch with the residual block's 1x1 convolution folded in as extra K (unet.py:238,245:
 * block2(h) + res_conv(x)):  y = conv3x3(x, w) + bias + view_bias + conv1x1([rx | rx2], rw_oihw) + rbias.
 * rC = channels of [rx | rx2] (a multiple of 4), the first rC1 of them from rx; rx2 == NULL: all from rx. */
int vf_conv_small_res(const float* x, const float* w_oihw, const float* bias /*|NULL*/, const float* view_bias /*|NULL*/,
                      float* y, int S, int Cin, int Cout, int H, int W, const float* rx, const float* rx2 /*|NULL*/,
                      int rC1, int rC, const float* rw_oihw, const float* rbias /*|NULL*/, void* stream);
/* The general one-launch form (round 5): GroupNorm(+Swish) around the conv without a GroupNorm launch (unet.py:207-218,
 * 254: GroupNorm -> Swish -> conv).  in_stats != NULL: x is the RAW GroupNorm input and in_stats the [S][Cin][2] 64-bit
 * integer sums (x, x^2 in 2^-24 units) left by the launch that produced x; the normalisation is applied while x is
 * staged (not with x2).  out_stats != NULL ([S][Cout][2] uint64, ZERO before the launch): the launch adds the sums of
 * y and y^2 per (view, channel) with integer atomics -- order-independent, bit-reproducible.  rx != NULL: as
 * vf_conv_small_res.  w_packed != NULL (3x3): weights from vf_conv_small_pack.  mode 0, or 2 for a plain 3x3 conv. */
int vf_conv_small_gn(const float* x, const float* x2 /*|NULL*/, int C1, const float* w_oihw, const float* bias /*|NULL*/,
                     const float* view_bias /*|NULL*/, const float* residual /*|NULL*/, float* y, int S, int Cin,
                     int Cout, int H, int W, int KS, const unsigned long long* in_stats /*|NULL*/,
                     const float* in_gamma, const float* in_beta, int in_groups, float eps, int silu,
                     unsigned long long* out_stats /*|NULL*/, const float* rx /*|NULL*/, const float* rx2 /*|NULL*/,
                     int rC1, int rC, const float* rw_oihw, const float* rbias /*|NULL*/, const float* w_packed /*|NULL*/,
                     int mode, void* stream);
/* Host only, launches nothing: the plan the launcher behind the three entries above executes for a vf_conv_small_gn
 * call of these sizes and operands (has_*: the pointer is not NULL; has_in_affine: in_gamma and in_beta both), as
 * out = { [0] 0 if taken, else the refusal branch in the order the launcher tests them: 1 unsupported layer, 2 x2 (not
 *         1x1 / C1 outside (0, Cin)), in_stats with 3 x2, 4 no affine, 5 in_groups <= 0, 6 Cin % in_groups, 7 1x1 Cin > 1024,
 *         8 3x3 Cin / 8 > 64, 9 mode 2 with rx or in_stats, rx with 10 KS != 3, 11 residual, 12 no rw, 13 rC < 4,
 *         14 rC % 4, 15 rC1 outside (0, rC);
 *   [1] kernel: 0 none (refused, or S <= 0), 1 conv1_small_kernel<false>, 2 conv1_small_kernel<true>, 3 conv3_small_kernel;
 *   [2] LOGTC, [3] RS (16 RS output channels per workgroup; 2 for 1x1), [4] PACKED, [5] workgroups,
 *   [6] n: products per wave of the 1x1 kernel, [7] rn: the same of the folded residual conv (0 without rx),
 *   [8] rounds per wave (3x3), [9] channels of the last round (8 or 4), [10] x upsampled on read,
 *   [11] GroupNorm on load, [12] output statistics, [13] residual conv folded in, [14] log2 W, [15] channels per group }.
 * Fields that do not apply are 0.  Returns hipErrorInvalidValue only for out == NULL. */
int vf_conv_small_plan(int S, int Cin, int Cout, int H, int W, int KS, int mode, int has_x2, int C1, int has_in_stats,
                       int has_in_affine, int in_groups, int has_out_stats, int has_rx, int has_rx2, int rC1, int rC,
                       int has_rw, int has_residual, int has_w_packed, int* out /*[16]*/);
/* 3x3 weights in the load order of the one-launch kernel (every weight load of a wave = 1 KB of consecutive memory instead
 * of 16 pieces of 16 OIHW rows); static weights (the sampler) are packed once.  Cin % 32 == 0. */
long vf_conv_small_pack_floats(int Cout, int Cin);
int vf_conv_small_pack(const float* w_oihw, float* w_packed, int Cout, int Cin, void* stream);
/* split-K workspace the call above wants at this shape (0 when the natural grid fills the chip) */
long vf_conv_fwd_ws_floats(int S, int Cin, int Cout, int H, int W, int KS);
/* Host-only query (touches no device, launches nothing): the plan vf_conv_fwd takes for these arguments -- also
 * vf_conv_fwd_gn (gn_groups > 0, else 0), vf_conv1x1_cat_fwd (0 < C1 < Cin, else 0 or Cin) and vf_conv1x1_cat_dgrad
 * (0 < C1o < Cout, else 0 or Cout); has_ws: a workspace of ws_floats floats is passed.  The launchers execute the
 * function that answers.  out[8] = { route: 0 conv_mfma_kernel, 1 conv1x1_kernel<1>, 2 conv1x1_kernel<2>,
 * 3 conv_any_kernel;  npt: 64-pixel units per workgroup tile;  nblk: workgroups per K split;  ks: K splits after the
 * clamp by the workspace (the launch has nblk * ks workgroups and writes ks slabs of S*Cout*H*W floats);  safe: the
 * instantiation with unconditional loads;  what follows the conv: 0 nothing, 1 the split-K reduce, 2 the reduce that also
 * evaluates the GroupNorm, 3 a GroupNorm launch (ks = 1), 4 the split-K reduce and then a GroupNorm launch (group above
 * 8192 float4);  NV, NT: the variant of 2, else 0 }.  Mode 4 ignores the workspace: ks = 1 whatever is passed.
 * Returns hipErrorInvalidValue for arguments the entries refuse. */
int vf_conv_fwd_plan(int S, int Cin, int Cout, int H, int W, int KS, int mode, int C1, int C1o, int gn_groups, int has_ws,
                     long ws_floats, int* out /*[8]*/);
/* 1x1 conv on the channel concatenation [x1 (C1 channels, multiple of 64) | x2] (residual conv of the decoder
 * blocks, unet.py:134,238): forward, dgrad into two tensors, wgrad */
int vf_conv1x1_cat_fwd(const float* x1, const float* x2, int C1, const float* w_packed, const float* bias, float* y,
                       float* ws, long ws_floats, int S, int Cin, int Cout, int H, int W, void* stream);
int vf_conv1x1_cat_dgrad(const float* dy, const float* w_packed_bwd, float* dx1, float* dx2, int C1, int S, int Cin,
                         int Cout, int H, int W, void* stream);
int vf_conv1x1_cat_wgrad(const float* x1, const float* x2, int C1, const float* dy, float* dw_oihw, float* ws,
                         long ws_floats, int S, int Cin, int Cout, int H, int W, void* stream);
/* EXPERIMENT (hosts select it with VF_BF16X3=1; default off): the same 1x1 convolutions with fp32-accurate products on
 * the bf16 matrix path -- every operand split into three bf16 pieces, six MFMAs per K=16 block, fp32 accumulation
 * (csrc/conv1x1_bf16x3.hip).  pack: w_oihw [Cout][Cin] -> split + packed forward operand (and the transposed dgrad
 * operand if w3_bwd != NULL); sizes in 32-bit words from vf_conv1x1_bf16x3_pack_dwords(M, K) with (M, K) = (Cout, Cin) /
 * (Cin, Cout).  conv: x may be the concatenation [x | x2] (x2 != NULL: C1in channels in x), y may be split into
 * [y | y2] (y2 != NULL: C1out channels in y); HW a power of two >= 64. */
long vf_conv1x1_bf16x3_pack_dwords(int M, int K);
int vf_conv1x1_bf16x3_pack(const float* w_oihw, void* w3_fwd, void* w3_bwd, int Cout, int Cin, void* stream);
int vf_conv1x1_bf16x3(const float* x, const float* x2, int C1in, const void* w3, const float* bias,
                      const float* view_bias, const float* residual, float* y, float* y2, int C1out, int S, int Cin,
                      int Cout, int HW, void* stream);
long vf_conv_wgrad_ws_floats(int S, int Cin, int Cout, int H, int W, int KS);
int vf_conv_wgrad(const float* x, const float* dy, float* dw_oihw, float* ws, long ws_floats, int S, int Cin,
                  int Cout, int H, int W, int KS, int mode, void* stream);
/* vf_conv_wgrad / vf_conv1x1_cat_wgrad without their follow-up launch (round 6): the main kernel only; desc9 (HOST memory,
 * 9 x int64) receives the row vf_wino44_reduce_multi needs for this layer, *nblocks its workgroup count; ws must stay
 * untouched until that launch (hosts that can postpone the weight gradients to the end of the backward pass). */
int vf_conv_wgrad_main(const float* x, const float* dy, float* dw_oihw, float* ws, long ws_floats, int S, int Cin,
                       int Cout, int H, int W, int KS, int mode, long long* desc9, int* nblocks, void* stream);
int vf_conv1x1_cat_wgrad_main(const float* x1, const float* x2, int C1, const float* dy, float* dw_oihw, float* ws,
                              long ws_floats, int S, int Cin, int Cout, int H, int W, long long* desc9, int* nblocks,
                              void* stream);
int vf_sumpool2(const float* x, float* y, long n_out, int Wo, void* stream);

/* fused Winograd F(2x2,3x3) path for stride-1 3x3 convs on 8x8 / 16x16 / 32x32 / 64x64 maps (forward and
 * dgrad); modes 0 and 2 as above.  Pack layout differs from the direct kernel's. */
int vf_wino_supported(int H, int W, int mode);
int vf_wino_pack_sizes(int Cout, int Cin, long* fwd_floats, long* bwd_floats);
int vf_wino_pack_weights(const float* w_oihw, float* u_fwd, float* u_bwd /*or NULL*/, int Cout, int Cin,
                         void* stream);
/* desc = device int64 [nlayers][8] rows {w, u_fwd, u_bwd, Cout, Cin, fwd_floats, bwd_floats, first_block} */
int vf_wino_pack_weights_multi(const void* desc, int nlayers, long total_blocks, void* stream);
/* ws: room for the K-split partial tiles of a grid that does not divide the 256 CUs (vf_wino_conv_ws_floats;
 * NULL / too small = plain grid) */
long vf_wino_conv_ws_floats(int S, int Cin, int Cout, int H, int W);
/* expected CU fill in percent under the tail plan (+ the workgroup-tile count): policy input for hosts */
int vf_wino_conv_fill_pct(int S, int Cin, int Cout, int H, int W, int* tiles_out);
int vf_wino_conv_fwd(const float* x, const float* u_packed, const float* bias, const float* view_bias,
                     const float* residual, float* y, float* ws, long ws_floats, int S, int Cin, int Cout, int H,
                     int W, int mode, void* stream);
/* The same conv with the GroupNorm(+Swish) BEHIND it (unet.py:207-218: the next Block's norm) evaluated by the conv's
 * fix-up launch -- possible where every tile of the launch is a K-split tail tile (the sampler at a few stacked views,
 * 16x16 ... 64x64 maps): vf_wino_conv_gn_fusable() says where.  a_out = [Swish](GroupNorm(groups, eps)(y)); y itself is
 * written only if store_y.  One graph node less than conv + fix-up + GroupNorm. */
int vf_wino_conv_gn_fusable(int S, int Cin, int Cout, int H, int W, int mode, int groups);
int vf_wino_conv_fwd_gn(const float* x, const float* u_packed, const float* bias /*|NULL*/, const float* view_bias /*|NULL*/,
                        const float* residual /*|NULL*/, float* y, int store_y, const float* gn_gamma, const float* gn_beta,
                        float* a_out, int groups, float eps, int silu, float* ws, long ws_floats, int S, int Cin, int Cout,
                        int H, int W, int mode, void* stream);
/* fused Winograd F(4x4,3x3) path (36 products per 4x4 outputs: 2.25 multiplies per output instead of the nested
 * kernel's 3) for the stride-1 3x3 convs on the 32x32 / 64x64 maps, forward and dgrad -- replaces nn.Conv2d 3x3
 * at reference model/unet.py:42,189,214 on those maps; same calling convention as the vf_wino_* entries above, its own
 * pack layout (U = G4 w G4^T, 36 slices in wave order). */
int vf_wino44_supported(int H, int W, int mode);
int vf_wino44_pack_sizes(int Cout, int Cin, long* fwd_floats, long* bwd_floats);
int vf_wino44_pack_weights(const float* w_oihw, float* u_fwd, float* u_bwd /*or NULL*/, int Cout, int Cin,
                           void* stream);
int vf_wino44_pack_weights_multi(const void* desc, int nlayers, long total_blocks, void* stream);
long vf_wino44_conv_ws_floats(int S, int Cin, int Cout, int H, int W);
int vf_wino44_conv_fill_pct(int S, int Cin, int Cout, int H, int W, int* tiles_out);
int vf_wino44_conv_fwd(const float* x, const float* u_packed, const float* bias, const float* view_bias,
                       const float* residual, float* y, float* ws, long ws_floats, int S, int Cin, int Cout, int H,
                       int W, int mode, void* stream);
/* Host-only query (touches no device, launches nothing): the plan vf_wino_conv_fwd (kind 1) / vf_wino44_conv_fwd
 * (kind 2; ops.wino_kind's codes) takes for these arguments; has_ws: a workspace of ws_floats floats is passed.  The
 * launchers execute the function that answers.  out[8] = { T: workgroup tiles of the launch (tile groups x 64-channel
 * tiles);  nch: 8-channel K chunks;  nfull: tiles [0, nfull) are computed whole;  split: K ranges per tail tile AFTER the
 * clamp by the workspace (parts that do not fit, or no workspace: nfull = T, split = 1, the plain grid);  per: chunks per
 * K range (the last may be shorter);  npers: persistent workgroups = min(nfull, 256);  workgroups of the conv launch
 * = npers + (T - nfull) * split;  workgroups of the fix-up launch, 0: none }.  vf_wino_conv_fwd_gn runs the same conv
 * launch and chooses its GroupNorm fix-up's grid itself.  Returns hipErrorInvalidValue for S <= 0, out == NULL and a
 * size / mode the kind does not support. */
int vf_wino_conv_plan(int kind, int S, int Cin, int Cout, int H, int W, int mode, int has_ws, long ws_floats,
                      int* out /*[8]*/);
/* weight gradient of a stride-1 3x3 conv (modes 0 and 2, output H = W in {8,16,32,64}) through the same
 * transform: dU = sum over tiles of (A dY A^T) (B^T d B)^T per Winograd slice, split over tile ranges into `ws`
 * slabs that are summed in a fixed order, then dW = G^T dU G */
int vf_wino_wgrad_supported(int H, int W, int mode);
long vf_wino_wgrad_ws_floats(int S, int Cin, int Cout, int H, int W);
/* db (or NULL): also the bias gradient sum_{s,p} dY -- the kernel reads every dY tile anyway; db2 (or NULL) is a
 * second [Cout] destination for the same sums (a layer sharing this dY, the residual 1x1 conv, gets its own tensor) */
int vf_wino_wgrad(const float* x, const float* dy, float* dw_oihw, float* db, float* db2, float* ws, long ws_floats,
                  int S, int Cin, int Cout, int H, int W, int mode, void* stream);
/* the same without the follow-up slab-sum launch (round 5): only the main kernel runs; desc9 (HOST memory, 9 x int64)
 * receives this layer's row for vf_wino44_reduce_multi, *nblocks its workgroup count; ws must stay untouched until then.
 * vf_wino44_reduce_multi sums the slabs of many layers in one launch: table = DEVICE copy of the rows, each row's `first`
 * field (the int32 at byte 64) set to the sum of the preceding rows' workgroup counts, nblocks = the total. */
int vf_wino_wgrad_main(const float* x, const float* dy, float* dw_oihw, float* db, float* db2, float* ws, long ws_floats,
                       int S, int Cin, int Cout, int H, int W, int mode, long long* desc9, int* nblocks, void* stream);
int vf_wino44_reduce_multi(const void* table, int nrows, int nblocks, void* stream);

/* ---- grouped time-embedding affine: all FeatureWiseAffine Linear(K->C_g) layers of the UNet on the same
 *      (S,K) embedding in one launch, unet.py:160-177.  desc = device int64 [ngroups][5] rows
 *      {W_g, b_g, C_g, out_off_g (floats), c_off_g}; out/de = flat buffers of the (S,C_g) matrices; CT = sum C_g ---- */
int vf_time_affine_fwd(const void* desc, int ngroups, const float* emb, float* out, int S, int K, int CT,
                       void* stream);
long vf_time_affine_ws_floats(int S, int K);
/* gdst (or NULL): device array of ngroups rows {float* dW_g, float* db_g}: one destination per layer (the slots of
 * a data-parallel gradient buffer) instead of the flat dw / db */
int vf_time_affine_bwd(const void* desc, int ngroups, const float* emb, const float* de, float* dw /*[CT][K]*/,
                       float* db /*[CT]*/, const void* gdst, float* demb /*[S][K] or NULL*/, float* ws, int S, int K,
                       int CT, void* stream);

/* ---- batched GEMM + softmax : torch.einsum / torch.softmax / nn.Linear,
 *      unet.py:267-274 (attention), :29-31,165 (linears) ---- */
int vf_bgemm(const float* A, const float* B, float* C, const float* bias /*[N]|NULL*/, int batch, int M, int N,
             int K, long sAb, long sAm, long sAk, long sBb, long sBk, long sBn, long sCb, long sCm, long sCn,
             float alpha, float beta, void* stream);
/* fused attention forward (unet.py:258-277 core): qkv [S][3C][L] -> out [S][C][L]; optionally
 * P [S][L][L] (softmax probabilities, saved for backward).  L in {64,256}, C % 32 == 0.  Other L <= 4096 run
 * vf_bgemm + vf_softmax_fwd / _bwd on materialised S x L x L scores (cols <= 4096); L > 4096 vf_attn_stream_*. */
int vf_attention_fwd(const float* qkv, float* out, float* P /*|NULL*/, int S, int C, int L, void* stream);
/* the forward kernel vf_attention_fwd launches at this shape (the launcher switches on it): 1 16-query, 2 32-query,
 * 3 key-split, 4 128-query; 0 where the shape is refused */
int vf_attention_fwd_kernel(int S, int C, int L);
/* attention backward (autograd of unet.py:267-274), L = 256, C % 32 == 0, first of three launches:
 * dS = P o (dP - rowsum(P o dP)) with dP = dO^T V computed in the kernel, and dQ = K dS^T / sqrt(C) -> q third of dqkv;
 * qkv, dqkv [S][3C][L], dO [S][C][L], P, dS [S][L][L] (dS must not alias P).  dV and dK stay vf_bgemm calls. */
int vf_attention_dscore(const float* qkv, const float* dO, const float* P, float* dS, float* dqkv, int S, int C, int L,
                        void* stream);
/* ... second launch (C % 64 == 0): dV = dO P and dK = q dS / sqrt(C) -> the v and k thirds of dqkv */
int vf_attention_dvdk(const float* qkv, const float* dO, const float* P, const float* dS, float* dqkv, int S, int C, int L,
                      void* stream);
/* streaming attention (unet.py:248-277 core, csrc/attention_stream.hip), any L >= 1, 1 <= C <= 512, no L x L buffer:
 * online softmax over key blocks.  qkv [S][3C][L] -> out [S][C][L]; rowstat [S][2][L] = per-query softmax statistics
 * (log2 e / sqrt(C) x the largest score, 1 / sum; training) or NULL.  ops.attention takes this route for L > 4096. */
int vf_attn_stream_fwd(const float* qkv, float* out, float* rowstat /*|NULL*/, int S, int C, int L, void* stream);
/* ... its backward (FlashAttention-2, deterministic, no float atomics): the probabilities recomputed from rowstat;
 * delta [S][L] workspace (rowsum(dO o out)); writes all of dqkv [S][3C][L].  Three launches: delta, dK + dV, dQ. */
int vf_attn_stream_bwd(const float* qkv, const float* out, const float* dO, const float* rowstat, float* delta,
                       float* dqkv, int S, int C, int L, void* stream);
/* ... their launch plan, host only (nothing is launched; the two launchers execute the function that answers; qkv and dO
 * count by their alignment alone): out[10] = {state (0 empty: S <= 0 or L <= 0, the launchers return 0; 1 runs; 2 refused:
 * C <= 0 or C > 512, hipErrorInvalidValue), NT of the <NT> kernels (1..4), 16-byte loads in the forward (L % 4 == 0 and
 * qkv aligned), in the backward (and dO aligned), grid x = ceil(L / 32) and y = S of the forward, dK / dV and dQ kernels,
 * grid x of the delta kernel, 128-wide blocks per workgroup, floats of rowstat (2 S L) and of delta (S L), saturating at
 * INT_MAX}; every field but state is 0 where nothing runs.  Returns hipErrorInvalidValue only for out == NULL. */
int vf_attn_stream_plan(const void* qkv, const void* dO, int S, int C, int L, int* out /*[10]*/);
int vf_softmax_fwd(const float* x, float* y, int rows, int cols, void* stream);
int vf_softmax_bwd(const float* y, const float* dy, float* dx, int rows, int cols, void* stream);
/* The launch plans of this family, host only (nothing is launched); the launchers execute the functions that answer.
 * vf_bgemm_plan: out[7] = {launches (0: batch, M or N <= 0), variant (0 bgemm_kernel, 1..4 bgemm_v2_kernel<A_KC, B_KC> =
 *   <1,1> <1,0> <0,1> <0,0>), grid x, y, z, xcd_batches (whole groups of eight batch items dealt one per XCD), refused};
 *   refused = the failed terms of the fast kernels' predicate as bits: 1 A has no unit stride, 2 B has none, 4 sCn != 1,
 *   8 K % 4, 16 sAb % 4, 32 sBb % 4, 64 sAm % 4 (A k-contiguous), 128 sAk % 4 and 256 M % 4 (A m-contiguous), 512 sBn % 4
 *   (B k-contiguous), 1024 sBk % 4 and 2048 N % 4 (B n-contiguous), 4096 A | B not 16-byte aligned.  A and B count by their
 *   alignment alone.
 * vf_softmax_plan: out[2] = {MAXV of softmax_fwd_kernel / softmax_bwd_kernel (1, 4, 16, 64; 0 above 4096 columns:
 *   refused), workgroups}.
 * vf_attention_bwd_plan: what the backward of the attention core runs (ops/attention.py), use_dscore / use_dvdk being its
 *   two switches: out[6] = {route (1 dscore + dvdk, 2 dscore + the dV and dK products, 3 four products + softmax backward
 *   on the materialised scores, 0 nothing: a size <= 0 or L > 4096), workgroups of vf_attention_dscore, of
 *   vf_attention_dvdk, the vf_bgemm products as bits (1 dP, 2 dV, 4 dQ, 8 dK), rows and columns of vf_softmax_bwd}.
 * Each returns hipErrorInvalidValue only for out == NULL. */
int vf_bgemm_plan(const void* A, const void* B, int batch, int M, int N, int K, long sAb, long sAm, long sAk, long sBb,
                  long sBk, long sBn, long sCn, int* out /*[7]*/);
int vf_softmax_plan(int rows, int cols, int* out /*[2]*/);
int vf_attention_bwd_plan(int S, int C, int L, int use_dscore, int use_dvdk, int* out /*[6]*/);

/* ---- small elementwise : PositionalEncoding unet.py:142-157, Swish :180-182, torch.cat :134 ---- */
int vf_sincos_embed(const float* level /*[S]*/, const float* angle /*[S]*/, float* out /*[S][dim]*/, int S, int dim,
                    void* stream);
int vf_swish_fwd(const float* x, float* y, long n, void* stream);
int vf_swish_bwd(const float* x, const float* dy, float* dx, long n, void* stream);
int vf_concat_channels(float* a, float* b, float* out, int S, long na, long nb, int split, void* stream);
/* nn.Dropout(p) inside Block, unet.py:207-216 (training mode): y = x * (u >= p) / (1-p), u = caller's uniform draws;
 * applied to dy it is the backward */
int vf_dropout(const float* x, const float* u, float* y, long n, float p, void* stream);
/* The same with the mask drawn in the kernel (csrc/rng.h, kind 5): element e of row v (view v - off[b] of sample b) is
 * kept iff (word e % 4 of block e / 4) >> 8 >= thr, thr = ceil(float32(p) * 2^24); y = keep ? x * scale : 0 with
 * scale = 1.0f / (1.0f - p): bit-identical to vf_dropout fed u = (word >> 8) * 2^-24.  Applied to dy it is the backward.
 * x, y [S][n]; ids DEVICE int64 [B]; off DEVICE int32 [B + 1] (every sample at most 4095 views: the caller's check).
 * hipErrorInvalidValue for n % 4, thr > 2^24, layer outside [0, 2^16), n / 4 >= 2^32. */
int vf_dropout_seeded(const float* x, float* y, unsigned long long seed, const long long* ids, const int* off, int B,
                      int S, long n, unsigned thr, float scale, int layer, void* stream);
/* Host mirror (HOST pointers, no stream, no GPU needed): keep [S][n], 1 = kept */
int vf_dropout_mask_host(unsigned long long seed, const long long* ids, const int* off, int B, int S, long n,
                         unsigned thr, int layer, unsigned char* keep /*[S][n]*/);

/* ---- ViewFusion : view_fusion.py:162-164 (q_sample), :244-263/:95-115 (stack), :265-298/:116-150
 *      (compose, mean ablation, MSE), :70-84,152-177 (posterior + p_sample), :314-317 (extract) ---- */
int vf_gather_level(const float* gammas, const long long* t, const float* u /*[B]|NULL*/, float* level, int B,
                    void* stream);
int vf_stack_views(const float* y_cond /*[B][Nmax][Cc][HW]*/, const float* y_t /*[B][3][HW]*/,
                   const float* noise /*|NULL*/, const float* level, const float* angle, const int* off /*[B+1]*/,
                   float* x /*[S][Cc+3][HW]*/, float* level_s, float* angle_s, int B, int Nmax,
                   int Cc /* conditioning channels: 3, or 6 for the `relative` configs */, int HW, int S,
                   int copy_cond, void* stream);
int vf_compose_fwd(const float* unet_out, const int* off, const float* target /*|NULL*/, float* noise_hat,
                   float* weights /*[B][maxV][3][HW]|NULL*/, float* loss_part /*[B*64]*/, float* loss, int B,
                   int Cout, int HW, int maxV, int weighting, void* stream);
int vf_compose_mse_bwd(const float* unet_out, const int* off, const float* target, const float* noise_hat,
                       const float* gloss, float* dout, int B, int Cout, int HW, int weighting, void* stream);
/* Loss options (csrc/loss_weight.h holds the specification): the two calls above with a target, generalised.
 * penalty 0 mse | 1 l1 | 2 huber(delta > 0) of d = noise_hat - target;  weight_kind 0 none | 1 min_snr(a) | 2 p2(k = a,
 * p = b) | 3 trunc_snr of level[b] (DEVICE float [B], the sample's gamma).  Writes noise_hat, sample_loss[b] = mean_i rho(d_bi),
 * sample_w[b] and loss = sum_b w_b s_b / B; bin_sum (float [K]) / bin_cnt (int [K]) (both or neither): persistent
 * accumulators, bin min(K-1, (int)(level K)) += the UNWEIGHTED s_b / 1.  Two launches, no atomics. */
int vf_compose_loss_fwd(const float* unet_out, const int* off, const float* target, const float* level,
                        float* noise_hat, float* loss_part /*[B*64]*/, float* sample_loss /*[B]*/,
                        float* sample_w /*[B]*/, float* loss, float* bin_sum /*[K]|NULL*/, int* bin_cnt /*[K]|NULL*/,
                        int B, int Cout, int HW, int weighting, int penalty, float delta, int weight_kind, float a,
                        float b, int K, void* stream);
/* d unet_out for gloss * loss: g = gloss w_b rho'(d) / (3 HW B) through the softmax / mean; one launch */
int vf_compose_loss_bwd(const float* unet_out, const int* off, const float* target, const float* noise_hat,
                        const float* gloss, const float* sample_w, float* dout, int B, int Cout, int HW, int weighting,
                        int penalty, float delta, void* stream);
/* vf_compose_loss_fwd with a per-sample scale (DEVICE float [B]; csrc/level_sampler.h's importance weight).  With a
 * scale, sample_w holds 2 B floats: w_b scale_b (what loss and vf_compose_loss_bwd use), then w_b alone; sample_loss and
 * the histogram stay unweighted.  scale == NULL: vf_compose_loss_fwd itself. */
int vf_compose_loss_fwd_scaled(const float* unet_out, const int* off, const float* target, const float* level,
                               const float* scale /*[B]|NULL*/, float* noise_hat, float* loss_part /*[B*64]*/,
                               float* sample_loss /*[B]*/, float* sample_w /*[2B] ([B] without scale)*/, float* loss,
                               float* bin_sum /*[K]|NULL*/, int* bin_cnt /*[K]|NULL*/, int B, int Cout, int HW,
                               int weighting, int penalty, float delta, int weight_kind, float a, float b, int K,
                               void* stream);
/* ---- loss-aware noise-level sampling (csrc/level_sampler.h holds the specification): K bins over the timesteps
 *      1..T-1, a fixed-point proposal table c [K+1] (64-bit cut points, c[0] = 0, c[K] = 2^32), iw [K] and ready [1],
 *      all in DEVICE memory; 1 <= K <= min(T-1, 1024). ---- */
/* vf_draw_train's sibling.  Exactly one of ids (with seed: word 0 of the training-scalars call) and words (int64 [B],
 * values in [0, 2^32)).  *ready == 0: the uniform draw and iw_out = 1.  u / level: seeded path only, each |NULL. */
int vf_draw_level(unsigned long long seed, const long long* ids /*|NULL*/, const long long* words /*|NULL*/,
                  const float* gammas, int T, int K, const unsigned long long* c, const float* iw, const int* ready,
                  long long* t, float* u /*|NULL*/, float* level /*|NULL*/, float* iw_out /*[B]*/, int B, void* stream);
/* r_b = (sample_w[b] sample_loss[b])^2 (sample_w NULL: 1; non-finite r_b skipped) into bin(t[b]): m / seen [K] updated
 * with the EMA factor beta in [0, 1); then ready = min seen >= warmup && sum n_k sqrt(m_k) finite and positive, and,
 * when ready, c / iw rebuilt with the uniform share eps (eps 2^32 >= 2 (T-1)).  One workgroup, no atomics. */
int vf_level_stats(const float* sample_loss, const float* sample_w /*|NULL*/, const long long* t, int B, int T, int K,
                   float beta, int warmup, double eps, float* m, int* seen, unsigned long long* c, float* iw,
                   int* ready, void* stream);
/* Host mirrors: HOST pointers, no stream, no GPU needed.  masses q [K] -> c [K+1], lo [K+1], iw [K];
 * words x [n] + table -> t [n], iw_out [n]. */
int vf_level_table_host(const double* q, int T, int K, double eps, unsigned long long* c, int* lo, float* iw);
int vf_level_draw_host(const unsigned* x, int n, int T, int K, const unsigned long long* c, const float* iw,
                       long long* t, float* iw_out);
/* Host mirror of the weight function: HOST pointers, no stream, no GPU needed. */
int vf_loss_weights_host(const float* level, int B, int kind, float a, float b, float* out /*[B]*/);
/* Prediction (the head of csrc/diffusion.hip holds the definition): vf_compose_loss_fwd_scaled / vf_compose_loss_bwd for
 * pred 1 (v: target = sqrt(g) noise - sqrt(1 - g) y_0) | 2 (x0: target = y_0; noise may be NULL), g = level[b], the target
 * formed inside the kernels; the weight is the prediction's native one (csrc/loss_weight.h).  noise_hat receives the
 * composed output in the network's own parameterisation.  pred 0 (eps) is refused: that is the calls above.  Two launches
 * forward, one backward, no atomics. */
int vf_compose_loss_pred_fwd(const float* unet_out, const int* off, const float* noise /*|NULL for x0*/,
                             const float* y_0, const float* level, const float* scale /*[B]|NULL*/, float* noise_hat,
                             float* loss_part /*[B*64]*/, float* sample_loss /*[B]*/,
                             float* sample_w /*[2B] ([B] without scale)*/, float* loss, float* bin_sum /*[K]|NULL*/,
                             int* bin_cnt /*[K]|NULL*/, int B, int Cout, int HW, int weighting, int penalty, float delta,
                             int weight_kind, float a, float b, int K, int pred, void* stream);
int vf_compose_loss_pred_bwd(const float* unet_out, const int* off, const float* noise /*|NULL for x0*/,
                             const float* y_0, const float* level, const float* noise_hat, const float* gloss,
                             const float* sample_w, float* dout, int B, int Cout, int HW, int weighting, int penalty,
                             float delta, int pred, void* stream);
/* Host mirror of the native weight (pred 0 eps | 1 v | 2 x0): HOST pointers, no stream, no GPU needed. */
int vf_loss_weights_pred_host(const float* level, int B, int pred, int kind, float a, float b, float* out /*[B]*/);
int vf_p_sample_tail(const float* unet_out, const int* off, const float* y_t, const float* z /*|NULL*/,
                     const long long* t, const float* sqrt_recip_gammas, const float* sqrt_recipm1_gammas,
                     const float* posterior_log_variance, const float* posterior_mean_coef1,
                     const float* posterior_mean_coef2, float* y_next /*|NULL*/, float* mean_out /*|NULL*/,
                     float* weights /*|NULL*/, int B, int Cout, int HW, int maxV, int weighting, int clip,
                     void* stream);

/* ---- seeded counter-based draws (csrc/rng.h holds the specification: Philox4x32-10, key = seed, counter =
 *      (float4 block, id lo, id hi, kind << 28 | step)).  ids: DEVICE int64 [B], one identifier per sample; a draw
 *      depends on (seed, id, kind, step, element) only, never on the sample's row or on the rest of the batch.
 *      kinds: 0 training scalars, 1 training noise, 2 sampler start noise, 3 reverse-step noise (step = t[b]). ---- */
/* t[b] = 1 + mulhi32(w0, T-1) (int64, the reference's randint(1, T)), u[b] = (w1 >> 8) 2^-24 (|NULL),
 * level[b] = (g[t] - g[t-1]) u + g[t-1]; gammas [T], 2 <= T <= 2^28 */
int vf_draw_train(unsigned long long seed, const long long* ids, const float* gammas, int T, long long* t,
                  float* u /*[B]|NULL*/, float* level /*[B]*/, int B, void* stream);
/* out [B][n] standard normals (Box-Muller, cut at 6.76 sigma), n % 4 == 0, 0 <= step < 2^28 */
int vf_randn_ids(unsigned long long seed, const long long* ids, int kind, int step, float* out, int B, int n,
                 void* stream);
/* out [B][n] the raw 32-bit words of the same counters (four per float4 block) */
int vf_philox_ids(unsigned long long seed, const long long* ids, int kind, int step, unsigned* out, int B, int n,
                  void* stream);
/* vf_p_sample_tail with z computed in the kernel from (seed, ids[b], kind 3, t[b], float4 index) instead of loaded;
 * z = 0 where t[b] == 0.  No step-dependent argument: a captured launch replays for every step. */
int vf_p_sample_tail_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                         const long long* ids, const long long* t, const float* sqrt_recip_gammas,
                         const float* sqrt_recipm1_gammas, const float* posterior_log_variance,
                         const float* posterior_mean_coef1, const float* posterior_mean_coef2,
                         float* y_next /*|NULL*/, float* mean_out /*|NULL*/, float* weights /*|NULL*/, int B, int Cout,
                         int HW, int maxV, int weighting, int clip, void* stream);
/* ---- few-step samplers (strided DDIM, DPM-Solver++ 2M): the reverse-step tail with a table-driven update.
 *      k = kidx[b] (DEVICE int64 [B]) indexes the K-entry fp32 DEVICE tables of schedule.sampler_tables:
 *        y0 = clamp(a[k] y - b[k] eps, -1, 1);  y_next = cy[k] y + c0[k] y0 + c1[k] y0_prev + sigma[k] z;
 *        y0_prev <- y0 (when given).
 *      sigma[k] == 0: z is neither loaded nor drawn; c1[k] == 0: y0_prev is not read.  y_next may be y_t. ---- */
int vf_sampler_step(const float* unet_out, const int* off, const float* y_t, const float* z /*|NULL*/,
                    const long long* kidx, const float* a, const float* b, const float* cy, const float* c0,
                    const float* c1, const float* sigma, float* y0_prev /*[B][3][HW]|NULL*/, float* y_next,
                    float* weights /*|NULL*/, int B, int Cout, int HW, int maxV, int weighting, void* stream);
/* ... with z drawn in the kernel from (seed, ids[b], kind 3, tau[k], float4 index): tau (DEVICE int64 [K]) holds the
 * model timestep of every entry, so the draw at one noise level is the same for every K. */
int vf_sampler_step_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                        const long long* ids, const long long* kidx, const long long* tau, const float* a,
                        const float* b, const float* cy, const float* c0, const float* c1, const float* sigma,
                        float* y0_prev /*|NULL*/, float* y_next, float* weights /*|NULL*/, int B, int Cout, int HW,
                        int maxV, int weighting, void* stream);
/* ---- classifier-free guidance (csrc/diffusion.hip holds the definition): conditioning dropout in training, an
 *      unconditional ("null") row per sample and a guided noise eps = g eps_c + (1 - g) eps_u in sampling. ---- */
/* vf_stack_views with drop (DEVICE uint8 [B] | NULL: the conditioning half of every row of a sample with drop[b] != 0
 * is zeros, y_cond is not read for it) and null_rows (!= 0: S + B rows are written; row S + b = [ 0 | y_t[b] ] with
 * level[b], angle[b]).  x [S (+ B)][Cc+3][HW], level_s / angle_s [S (+ B)].  copy_cond == 0 touches no conditioning half.
 * With null_rows every sample must have a real row (S >= B, else hipErrorInvalidValue); without, any S as above. */
int vf_stack_views_cfg(const float* y_cond, const float* y_t, const float* noise /*|NULL*/, const float* level,
                       const float* angle, const int* off /*[B+1]*/, const unsigned char* drop /*[B]|NULL*/, float* x,
                       float* level_s, float* angle_s, int B, int Nmax, int Cc, int HW, int S, int copy_cond,
                       int null_rows, void* stream);
/* drop[b] = (w2 >> 8) < thr: word 2 of the training-scalar call (kind 0) of sample ids[b]; thr = ceil(p 2^24) <= 2^24 */
int vf_draw_cond_drop(unsigned long long seed, const long long* ids, unsigned thr, unsigned char* drop /*[B]*/, int B,
                      void* stream);
/* The guided reverse-step tails: the sibling's arguments plus g (DEVICE fp32 [B], the guidance scales); unet_out is
 * [S + B][Cout][HW] with S = off[B], row S + b the null row of sample b.  weights stay the conditional ones. */
int vf_p_sample_tail_cfg(const float* unet_out, const int* off, const float* y_t, const float* z /*|NULL*/,
                         const long long* t, const float* sqrt_recip_gammas, const float* sqrt_recipm1_gammas,
                         const float* posterior_log_variance, const float* posterior_mean_coef1,
                         const float* posterior_mean_coef2, float* y_next /*|NULL*/, float* mean_out /*|NULL*/,
                         float* weights /*|NULL*/, int B, int Cout, int HW, int maxV, int weighting, int clip,
                         const float* g /*[B]*/, void* stream);
int vf_p_sample_tail_cfg_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                             const long long* ids, const long long* t, const float* sqrt_recip_gammas,
                             const float* sqrt_recipm1_gammas, const float* posterior_log_variance,
                             const float* posterior_mean_coef1, const float* posterior_mean_coef2,
                             float* y_next /*|NULL*/, float* mean_out /*|NULL*/, float* weights /*|NULL*/, int B,
                             int Cout, int HW, int maxV, int weighting, int clip, const float* g /*[B]*/,
                             void* stream);
int vf_sampler_step_cfg(const float* unet_out, const int* off, const float* y_t, const float* z /*|NULL*/,
                        const long long* kidx, const float* a, const float* b, const float* cy, const float* c0,
                        const float* c1, const float* sigma, float* y0_prev /*[B][3][HW]|NULL*/, float* y_next,
                        float* weights /*|NULL*/, int B, int Cout, int HW, int maxV, int weighting,
                        const float* g /*[B]*/, void* stream);
int vf_sampler_step_cfg_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                            const long long* ids, const long long* kidx, const long long* tau, const float* a,
                            const float* b, const float* cy, const float* c0, const float* c1, const float* sigma,
                            float* y0_prev /*|NULL*/, float* y_next, float* weights /*|NULL*/, int B, int Cout, int HW,
                            int maxV, int weighting, const float* g /*[B]*/, void* stream);
/* ---- dynamic thresholding and guidance rescaling of the reverse step (csrc/diffusion.hip holds the definition): three
 *      launches in place of one tail.  eps [B][3][HW] and stat [B][2] = {r_b, s_b} are the caller's scratch. ---- */
/* The composed (g != NULL: and guided, unet_out [off[B] + B][Cout][HW]) noise into eps, the conditional weights as
 * vf_compose_fwd writes them, and per-workgroup sums of eps_c, eps_c^2, eps_g, eps_g^2 into part (DEVICE double
 * [B * 64 * 4]), reduced in a fixed order.  fused: which tail follows, as in vf_sample_stat (the guided combination is
 * rounded as that tail's composing sibling rounds it). */
int vf_compose_eps(const float* unet_out, const int* off, const float* g /*[B]|NULL*/, float* eps,
                   float* weights /*|NULL*/, double* part, int B, int Cout, int HW, int maxV, int weighting, int fused,
                   void* stream);
/* One workgroup per sample: r_b = phi sigma(eps_c) / sigma(eps_g) + 1 - phi from `part` (phi <= 0: r_b = 1, part not
 * read) and s_b = min(max(1, quantile), cmax), the (k, frac) quantile of |ta[idx[b]] y - tb[idx[b]] r_b eps| by exact radix
 * selection (k < 0: s_b = 1, nothing selected).  k = floor(q (n - 1)), frac = q (n - 1) - k in [0, 1), n = 3 HW; frac != 0
 * needs k + 1 < n.  cmax >= 1 (+inf: no cap).  fused: how the tail that follows rounds y0_hat -- 1 in front of
 * vf_p_sample_tail_eps(_rng) (fma(a, y, -(b eps))), 0 in front of vf_sampler_step_eps(_rng) (a y and b eps rounded, then
 * subtracted) -- so that the selection sees the very values the tail bounds. */
int vf_sample_stat(const float* eps, const double* part /*|NULL*/, const float* y, const long long* idx, const float* ta,
                   const float* tb, float* stat, int B, int HW, float phi, int k, float frac, float cmax, int fused,
                   void* stream);
/* out[b] = x_s[k] + frac (x_s[k+1] - x_s[k]) with x_s = sort(|x[b][0..n)|): the same selection on a plain [B][n] buffer,
 * any n >= 1.  x_s[k+1] is not read when frac == 0. */
int vf_abs_quantile(const float* x, int B, int n, int k, float frac, float* out /*[B]*/, void* stream);
/* The tails on the eps buffer: eps is multiplied by stat[b][0] when rescale != 0; thr != 0 bounds y0_hat by
 * clamp(., -s, s) / s with s = stat[b][1], else the static clamp (under `clip` in the ancestral tail).  Everything else
 * as vf_p_sample_tail(_rng) / vf_sampler_step(_rng); the weights come from vf_compose_eps. */
int vf_p_sample_tail_eps(const float* eps, const float* stat, const float* y_t, const float* z /*|NULL*/,
                         const long long* t, const float* sqrt_recip_gammas, const float* sqrt_recipm1_gammas,
                         const float* posterior_log_variance, const float* posterior_mean_coef1,
                         const float* posterior_mean_coef2, float* y_next /*|NULL*/, float* mean_out /*|NULL*/, int B,
                         int HW, int clip, int rescale, int thr, void* stream);
int vf_p_sample_tail_eps_rng(const float* eps, const float* stat, const float* y_t, unsigned long long seed,
                             const long long* ids, const long long* t, const float* sqrt_recip_gammas,
                             const float* sqrt_recipm1_gammas, const float* posterior_log_variance,
                             const float* posterior_mean_coef1, const float* posterior_mean_coef2,
                             float* y_next /*|NULL*/, float* mean_out /*|NULL*/, int B, int HW, int clip, int rescale,
                             int thr, void* stream);
int vf_sampler_step_eps(const float* eps, const float* stat, const float* y_t, const float* z /*|NULL*/,
                        const long long* kidx, const float* a, const float* b, const float* cy, const float* c0,
                        const float* c1, const float* sigma, float* y0_prev /*[B][3][HW]|NULL*/, float* y_next, int B,
                        int HW, int rescale, int thr, void* stream);
int vf_sampler_step_eps_rng(const float* eps, const float* stat, const float* y_t, unsigned long long seed,
                            const long long* ids, const long long* kidx, const long long* tau, const float* a,
                            const float* b, const float* cy, const float* c0, const float* c1, const float* sigma,
                            float* y0_prev /*|NULL*/, float* y_next, int B, int HW, int rescale, int thr, void* stream);
/* ---- progressive distillation (csrc/diffusion.hip holds the definition): the target of a student that does in one
 *      DDIM step what its teacher does in two.  Two launches around the teacher's two forwards; the first teacher step is
 *      vf_sampler_step(_cfg) with a history buffer. ---- */
/* i[b] = i_in[b] clamped to 0..K-1, or mulhi32(word 0 of the kind-0 call of ids[b], K) (exactly one of i_in / ids);
 * k1 = 2 i + 1, k0 = 2 i (int64 [B] each); level_s[b] = gammas[tau_s[i]]; z_t = sqrt(level_s) y_0 + sqrt(1 - level_s) noise
 * ([B][n], n % 4 == 0).  tau_s: DEVICE int64 [K], 1 <= K <= 2^27. */
int vf_distill_begin(unsigned long long seed, const long long* ids /*|NULL*/, const long long* i_in /*|NULL*/,
                     const long long* tau_s, const float* gammas, int K, const float* y_0, const float* noise,
                     long long* i_out, long long* k1, long long* k0, float* level_s, float* z_t, int B, int n,
                     void* stream);
/* The second teacher step's tail: x2 = clamp(a[k0] y - b[k0] out2, -1, 1) with out2 composed (g != NULL: and guided,
 * unet_out [off[B] + B][Cout][HW]) from unet_out; x_tilde = clamp(w1[i] x1 + w2[i] x2, -1, 1);
 * eps_tilde = (z_t - sqrt(level_s) x_tilde) / sqrt(1 - level_s).  y = z', x1 = the history buffer of the first step. */
int vf_distill_target(const float* unet_out, const int* off, const float* y, const float* x1, const float* z_t,
                      const float* level_s, const long long* idx, const long long* kidx, const float* a, const float* b,
                      const float* w1, const float* w2, float* x_tilde, float* eps_tilde, int B, int Cout, int HW,
                      int weighting, const float* g /*[B]|NULL*/, void* stream);
/* Host mirrors: the same inline functions run on the CPU.  HOST pointers, no stream, no GPU needed. */
int vf_distill_step_host(unsigned long long seed, const long long* ids, int K, long long* i_out /*[B]*/, int B);
/* the truncated-SNR weight max(SNR, 1) / SNR in its native form for pred 0 eps | 1 v | 2 x0 (csrc/loss_weight.h, kind 3) */
int vf_loss_weights_trunc_snr_host(const float* level, int B, int pred, float* out /*[B]*/);
int vf_rng_host_philox(const unsigned* counter /*[4]*/, const unsigned* key /*[2]*/, unsigned* out /*[4]*/);
int vf_rng_host_normal(unsigned long long seed, const long long* ids, int kind, int step, float* out /*[B][n]*/,
                       int B, int n);
int vf_rng_host_train_scalars(unsigned long long seed, const long long* ids, int T, long long* t, float* u, int B);
/* vf_draw_cond_drop on the CPU */
int vf_cond_drop_host(unsigned long long seed, const long long* ids, unsigned thr, unsigned char* drop /*[B]*/, int B);
/* ---- self-conditioning (csrc/diffusion.hip holds the definition): the network also sees its own previous estimate of
 *      the clean image, as three more input channels.  The stacking is the guided kernel's SC instantiation; the other two
 *      are siblings of the kernels above. ---- */
/* vf_stack_views_cfg plus the third part: x [S (+ B)][Cc+6][HW], row v = [ cond | target | sc[b] ]; sc (DEVICE
 * [B][3][HW] | NULL: zeros).  drop / null_rows / copy_cond as there; copy_cond == 0 rewrites the target and sc parts only. */
int vf_stack_views_sc(const float* y_cond, const float* y_t, const float* noise /*|NULL*/, const float* level,
                      const float* angle, const int* off /*[B+1]*/, const unsigned char* drop /*[B]|NULL*/,
                      const float* sc /*[B][3][HW]|NULL*/, float* x, float* level_s, float* angle_s, int B, int Nmax,
                      int Cc, int HW, int S, int copy_cond, int null_rows, void* stream);
/* keep[b] = (w3 >> 8) < thr: word 3 of the training-scalar call (kind 0) of sample ids[b]; thr = ceil(p 2^24) <= 2^24 */
int vf_draw_self_cond(unsigned long long seed, const long long* ids, unsigned thr, unsigned char* keep /*[B]*/, int B,
                      void* stream);
/* x_hat[b] = keep[b] clamp(a(g) y_t - b(g) out_b, -1, 1), g = level[b], out_b composed over the sample's rows of unet_out
 * ([off[B]][Cout][HW]; weighting: softmax of channels 3..5, else the mean); pred 0 eps | 1 v | 2 x0 (x_hat = clamp(out_b),
 * y and level not read).  y_t of sample b is read at y + row * y_stride + y_off floats (both multiples of 4), row = off[b]
 * when y_by_view != 0 (the stacked input: y_stride = (Cc + 6) HW, y_off = Cc HW), else b.  keep (DEVICE uint8 [B] | NULL:
 * all kept); keep[b] == 0 writes zeros. */
int vf_self_cond_estimate(const float* unet_out, const int* off, const float* level, const float* y /*|NULL for x0*/,
                          long y_stride, long y_off, int y_by_view, const unsigned char* keep /*[B]|NULL*/,
                          float* x_hat /*[B][3][HW]*/, int B, int Cout, int HW, int weighting, int pred, void* stream);
/* Host mirrors (HOST pointers, no stream): vf_draw_self_cond on the CPU, and the (a, b) of the estimate at levels [n] */
int vf_self_cond_draw_host(unsigned long long seed, const long long* ids, unsigned thr, unsigned char* out /*[B]*/, int B);
int vf_self_cond_coeffs_host(const float* level, int pred, float* a /*[n]*/, float* b /*[n]*/, int n);
/* ---- learned variance (csrc/diffusion.hip holds the definition, csrc/vlb.h the arithmetic): unet_out has nine channels,
 *      0..2 the prediction, 3..5 the view logits, 6..8 the raw variance output.  The loss entries run the LV instantiations
 *      of the loss family's kernels, the tail entries a sibling of the few-step tail. ---- */
/* The hybrid loss L_simple + lambda L_vlb: vf_compose_loss_pred_fwd / _bwd for pred 0 | 1 | 2 (0: noise is the ready-made
 * target, y_0 not read) plus t (DEVICE int64 [B], clamped into [0, T - 1]), the fp32 tables c1 (posterior_mean_coef1), hi,
 * lo [T], var_hat [B][3][HW] (the composed channels 6..8), vlb_part [B * 64], sample_vlb [B] (bits per dimension).  No
 * per-sample scale.  The backward writes all nine channels of dout. */
int vf_compose_loss_lv_fwd(const float* unet_out, const int* off, const float* noise /*|NULL for x0*/,
                           const float* y_0 /*|NULL for eps*/, const float* level, const long long* t, const float* c1,
                           const float* hi, const float* lo, float* noise_hat, float* var_hat, float* loss_part,
                           float* vlb_part, float* sample_loss, float* sample_w, float* sample_vlb, float* loss,
                           float* bin_sum /*|NULL*/, int* bin_cnt /*|NULL*/, int B, int Cout, int HW, int weighting,
                           int penalty, float delta, int weight_kind, float a, float b, int K, int pred, int T,
                           float lambda, void* stream);
int vf_compose_loss_lv_bwd(const float* unet_out, const int* off, const float* noise, const float* y_0,
                           const float* level, const long long* t, const float* c1, const float* hi, const float* lo,
                           const float* noise_hat, const float* var_hat, const float* gloss, const float* sample_w,
                           float* dout, int B, int Cout, int HW, int weighting, int penalty, float delta, int pred, int T,
                           float lambda, void* stream);
/* The learned-variance reverse step: vf_sampler_step{, _rng, _cfg, _cfg_rng} on the "ddim", eta = 1 tables without c1,
 * with hi, lo [K] behind sigma -- where sigma[k] != 0 the noise scale is expf(0.5 lp) per element, lp between lo[k] and
 * hi[k] by the composed channels 6..8 of the conditional rows -- and lp_out ([B][3][HW] | NULL: lp itself). */
int vf_sampler_step_lv(const float* unet_out, const int* off, const float* y_t, const float* z /*|NULL*/,
                       const long long* kidx, const float* a, const float* b, const float* cy, const float* c0,
                       const float* sigma, const float* hi, const float* lo, float* y0_prev /*|NULL*/, float* y_next,
                       float* weights /*|NULL*/, float* lp_out /*|NULL*/, int B, int Cout, int HW, int maxV,
                       int weighting, void* stream);
int vf_sampler_step_lv_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                           const long long* ids, const long long* kidx, const long long* tau, const float* a,
                           const float* b, const float* cy, const float* c0, const float* sigma, const float* hi,
                           const float* lo, float* y0_prev, float* y_next, float* weights, float* lp_out, int B, int Cout,
                           int HW, int maxV, int weighting, void* stream);
int vf_sampler_step_lv_cfg(const float* unet_out, const int* off, const float* y_t, const float* z,
                           const long long* kidx, const float* a, const float* b, const float* cy, const float* c0,
                           const float* sigma, const float* hi, const float* lo, float* y0_prev, float* y_next,
                           float* weights, float* lp_out, int B, int Cout, int HW, int maxV, int weighting, const float* g,
                           void* stream);
int vf_sampler_step_lv_cfg_rng(const float* unet_out, const int* off, const float* y_t, unsigned long long seed,
                               const long long* ids, const long long* kidx, const long long* tau, const float* a,
                               const float* b, const float* cy, const float* c0, const float* sigma, const float* hi,
                               const float* lo, float* y0_prev, float* y_next, float* weights, float* lp_out, int B,
                               int Cout, int HW, int maxV, int weighting, const float* g, void* stream);
/* Host mirror of csrc/vlb.h (HOST pointers, no stream): per element lp, KL in bits and dKL/dlp */
int vf_vlb_terms_host(const float* o, const float* hi, const float* lo, const float* c1, const float* level,
                      const float* r, int pred, float* lp, float* kl, float* dkl, int n);
/* ---- the variational bound in bits per dimension (csrc/diffusion.hip holds the definition, csrc/vlb.h the arithmetic):
 *      evaluation only, new kernels only.  kidx: DEVICE int64 [B], the step of every sample, clamped into [0, K - 1];
 *      the fp32 tables a, b, c0, hi, lo [K] are schedule.nll_tables'. ---- */
/* y_k [B][3][HW] = sqrt(g) y_0 + sqrt(1 - g) n, g = gammas[tau[k]]: n from noise [B][K][3][HW] at (b, k), or, with noise
 * NULL, drawn from (seed, ids[b], kind 6, tau[k], float4 index) */
int vf_nll_noisy(const float* y_0, const float* noise /*|NULL*/, unsigned long long seed, const long long* ids /*|NULL*/,
                 const long long* kidx, const long long* tau /*[K]*/, const float* gammas /*[T]*/, float* y_k, int B,
                 int HW, int K, int T, void* stream);
/* column k of vb [B][K] (the term in bits, the mean over 3 HW elements) and of x0_mse [B][K] (the mean of (y0 - y_0)^2);
 * lv: nine channels, lp by the composed channels 6..8; else lp = hi[k] where large, lo[k] otherwise; dec: the decoder
 * likelihood (k == 0) instead of the KL; vb_part, sq_part: [B * 64] scratch.  Two launches, no atomics. */
int vf_nll_terms(const float* unet_out, const int* off, const float* y_k, const float* y_0, const long long* kidx,
                 const float* a, const float* b, const float* c0, const float* hi, const float* lo, float* vb_part,
                 float* sq_part, float* vb, float* x0_mse, int B, int Cout, int HW, int K, int weighting, int clip, int lv,
                 int dec, int large, void* stream);
/* prior [B]: L_T from y_0 and gammas[T - 1]; part: [B * 64] scratch */
int vf_nll_prior(const float* y_0, const float* gammas, float* part, float* prior, int B, int HW, int T, void* stream);
/* Host mirror of one term (HOST pointers, no stream): per element i of n its own composed out, raw variance o (lv alone,
 * else NULL), y_k, y_0 and table row -> term[i] in bits and sq[i] = (y0 - y_0)^2 */
int vf_nll_terms_host(const float* out, const float* o, const float* y_k, const float* y_0, const float* a,
                      const float* b, const float* c0, const float* hi, const float* lo, int lv, int dec, int large,
                      int clip, float* term, float* sq, int n);
/* ---- the analytic variance (csrc/diffusion.hip holds the definition): estimation only, one new kernel.  kidx: DEVICE
 *      int64 [B], clamped into [0, K - 1]; the fp32 tables ea, eb [K] are schedule.eps_tables'. ---- */
/* column k of m2 [B][K]: the mean over 3 HW elements of (ea[k] y_k + eb[k] out_b)^2, out_b the composition of channels
 * 0..2 over the sample's views; part: [B * 64] scratch.  Two launches, no atomics. */
int vf_eps_moments(const float* unet_out, const int* off, const float* y_k, const long long* kidx, const float* ea,
                   const float* eb, float* part, float* m2, int B, int Cout, int HW, int K, int weighting,
                   void* stream);
/* Host mirror of one element (HOST pointers, no stream): eps[i] = ea[i] y_k[i] + eb[i] out[i], sq[i] = eps[i]^2 */
int vf_eps_moment_host(const float* out, const float* y_k, const float* ea, const float* eb, float* eps, float* sq,
                       int n);

/* ---- batch assembly from a device-resident view store (csrc/batch.hip; data.ViewStore): the reference loader's
 *      process_sample + collate + H2D, data/nmr_dataset.py:10-52, as one launch.  store: planar uint8 [N][24][3][H][W],
 *      H * W % 4 == 0.  The views of sample b are a function of (seed, ids[b]) alone: the data draws of csrc/rng.h (kind 4)
 *      through csrc/batch_plan.h.  objects (DEVICE int64 [B] | NULL): the object of every sample, else drawn from
 *      [0, N); an object outside [0, N) fills that sample's outputs with NaN and reads nothing.
 *      y_0 [B][3][H][W], y_cond [B][23][3 (relative: 6)][H][W], angle [B] (relative: the relative angle), objects_out
 *      (|NULL) [B] the objects used.  all != 0: the identity plan -- y_cond [B][24][3][H][W] = the 24 views of
 *      objects[b] (required) as floats; seed, ids, y_0, angle unused.  Grid (24, B), no atomics, no workspace. ---- */
int vf_batch_assemble(const unsigned char* store, long N, int H, int W, unsigned long long seed, const long long* ids,
                      const long long* objects, int B, int train, int relative, int all, float* y_0, float* y_cond,
                      float* angle, long long* objects_out, void* stream);
/* Host mirror (HOST pointers, no stream, no GPU): per sample src [B][24] (cond[k] = views[src[k + 1]]), target [B]
 * (the target view p[0]), q01 [B][2] (q[0], q[1] of the relative angle), second [B], view_count [B] in [lo, hi]
 * (1 <= lo <= hi <= 23) and the object [B] (objects[b] when given, checked against N) */
int vf_batch_host_plan(unsigned long long seed, const long long* ids, int B, int train, int lo, int hi, long N,
                       const long long* objects, int* src, int* target, int* q01, int* second, long long* view_count,
                       long long* object);

/* eval metric next to the path: utils/metrics.py:6-8; out[b] = PSNR of image b (n floats each) */
int vf_psnr(const float* generated, const float* target, float* out /*[B]*/, int B, int n, void* stream);
/* ... and utils/metrics.py:11-12 (csrc/ssim.hip): out[b] = SSIM of image b, [B][C][H][W] inputs, any H, W >= 11 and
 * C >= 1 -- pytorch_msssim.ssim(X, Y, data_range, size_average=False) with its defaults (11-tap Gaussian sigma 1.5,
 * separable "valid" filtering, K = (0.01, 0.03), no clamp).  window11: DEVICE [11], the normalised fp32 window the
 * host computed.  workspace: vf_ssim_workspace_floats(B, C, H, W) floats (one partial per 32 x 32 tile), 0 when the
 * geometry is refused.  Two launches, no atomics: bit-reproducible. */
long vf_ssim_workspace_floats(int B, int C, int H, int W);
int vf_ssim(const float* generated, const float* target, float* out /*[B]*/, float* workspace, int B, int C, int H,
            int W, const float* window11, float data_range, void* stream);
/* ... and utils/compute_metrics.py (csrc/lpips.hip): what LPIPS (vgg, version 0.1) needs around the 3x3 convolutions of
 * its VGG16 trunk, which run through vf_conv_fwd / the Winograd entries like any other layer.
 * vf_lpips_prep: out [2B][3][HW] = ((2 x - 1) - shift_c) / scale_c of [generated | target], each [B][3][HW].
 * vf_relu: in place.  vf_relu_maxpool2: y [planes][H][W] (H, W even) is ReLU'd in place and pooled [planes][H/2][W/2]
 * receives its 2x2 maxima, in one read.
 * vf_lpips_layer: one tap; feat [2B][C][HW] (image b against image B + b), lin [C]; per pixel
 * sum_c lin_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2, one partial sum / HW per workgroup at
 * workspace[b * slots + slot0 + tile], tile < vf_lpips_layer_tiles(C, HW).  vf_lpips_finish: out[b] = the sum of the
 * image's `slots` partials in index order (in double).  vf_lpips_workspace_floats: B * the slots of the five VGG16 taps
 * (64, 128, 256, 512, 512 channels at H x W ... H/16 x W/16); 0 unless H and W are multiples of 16.
 * No atomics, fixed summation order: bit-reproducible. */
int vf_lpips_prep(const float* generated, const float* target, float* out, int B, int HW, void* stream);
int vf_relu(float* x, long n, void* stream);
int vf_relu_maxpool2(float* y, float* pooled, long planes, int H, int W, void* stream);
int vf_lpips_layer_tiles(int C, int HW);
long vf_lpips_workspace_floats(int B, int H, int W);
int vf_lpips_layer(const float* feat, const float* lin, float* workspace, int B, int C, int HW, int slot0, int slots,
                   void* stream);
int vf_lpips_finish(const float* workspace, float* out /*[B]*/, int B, int slots, void* stream);

/* ---- optimizer step next to the path: torch.optim.Adam, experiment.py:118-120,293 ----
 * desc = device int64 [ntensors][6] rows {p, g, exp_avg, exp_avg_sq, numel, first_block}, block = 1024 elems */
int vf_adam_multi(const void* desc, int ntensors, long total_blocks, float lr, float beta1, float beta2, float eps,
                  float bias_correction1, float bias_correction2, void* stream);
/* the same update with {lr, 1-beta1^t, 1-beta2^t} read from device memory (float[3]) at run time: the form a HIP-graph
 * capture of the training step uses */
int vf_adam_multi_dev(const void* desc, int ntensors, long total_blocks, const float* scalars, float beta1, float beta2,
                      float eps, void* stream);
/* scalars[0..2] = {lr, bc1, bc2}, enqueued on `stream` (values carried as launch arguments) */
int vf_adam_set_scalars(float* scalars, float lr, float bc1, float bc2, void* stream);

/* ---- opt-in extras of the fused step (optim.FusedAdam(ema_decay=, max_grad_norm=)): global-norm gradient clipping and an
 *      exponential moving average of the weights; the three entry points above are what runs when both are off ----
 * partial[b] = sum of squares, in double, of the gradient elements of block b (b < total_blocks) of one descriptor table */
int vf_grad_sumsq_multi(const void* desc, int ntensors, long total_blocks, double* partial, void* stream);
/* one workgroup, fixed order, double: out[0] = norm = sqrt(sum of partial[0..n)), out[1] = scale =
 * min(1, max_norm[0] / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_); max_norm: DEVICE float, or NULL for scale = 1 */
int vf_grad_norm_finish(const double* partial, long n, const float* max_norm, float* out, void* stream);
/* vf_adam_multi with gscale (device float or NULL): the update reads g * gscale[0], the stored gradient stays raw; and
 * ema_tab (device float*[ntensors], one EMA tensor per descriptor row, or NULL) + ema_scal (device {d, 1 - d}):
 * ema = fma(d, ema, (1 - d) p_new) after the parameter update */
int vf_adam_multi_ex(const void* desc, const void* ema_tab, int ntensors, long total_blocks, float lr, float beta1,
                     float beta2, float eps, float bias_correction1, float bias_correction2, const float* gscale,
                     const float* ema_scal, void* stream);
/* the same with {lr, 1-beta1^t, 1-beta2^t} read from device memory, as vf_adam_multi_dev */
int vf_adam_multi_ex_dev(const void* desc, const void* ema_tab, int ntensors, long total_blocks, const float* scalars,
                         float beta1, float beta2, float eps, const float* gscale, const float* ema_scal, void* stream);
/* scalars[0..2] = {lr, bc1, bc2} (skipped when scalars is NULL) and xs[0..2] = {ema decay d, 1 - d, max_norm} */
int vf_adam_set_scalars_ex(float* scalars, float lr, float bc1, float bc2, float* xs, float ema_d, float ema_omd,
                           float max_norm, void* stream);
/* exchange p <-> ema in place for every row (desc: only p, numel, first_block are read) */
int vf_swap_multi(const void* desc, const void* ema_tab, int ntensors, long total_blocks, void* stream);

/* ---- opt-in gradient accumulation over micro-batches (optim.FusedAdam.accumulate, train.Trainer(accum_steps=)) ----
 * acc = beta * acc + w * g per element: both products and the sum rounded to float, no fma (csrc/adam_update.h).  desc rows
 * as vf_adam_multi with p = the accumulator, g = the gradient to add (exp_avg / exp_avg_sq unused); scalars: DEVICE
 * float[2] {beta, w} read when the kernel runs (vf_adam_set_scalars writes them), so a captured launch serves every
 * micro-batch; beta == 0 never reads the accumulator (it may hold NaN).  No atomics: bit-reproducible */
int vf_grad_accum_multi(const void* desc, int ntensors, long total_blocks, const float* scalars, void* stream);

/* ---- gradient exchange next to the path: replaces DistributedDataParallel's bucketed NCCL
 *      all-reduce + optimizer.step(), experiment.py:104-107, 118-120, 292-293 -- a one-shot all-reduce over IPC-mapped
 *      peer gradient arenas fused with the Adam update (csrc/xgmi.hip; host side reducer.XgmiArena, VF_REDUCER=xgmi).
 *      The five memory calls below are the only entry points of the library that allocate / map memory; they run once
 *      per process, outside any stream. ---- */
int vf_xgmi_alloc(void** ptr, long bytes);                 /* zero-filled, IPC-exportable device memory */
int vf_xgmi_free(void* ptr);
int vf_xgmi_export(void* ptr, void* handle64 /*64 bytes out*/);
int vf_xgmi_open(const void* handle64, void** ptr);        /* a peer's allocation mapped into this process */
int vf_xgmi_close(void* ptr);
/* flag[slot][rank] = epoch in every rank's flag block (unsigned [nslots][world]); peer_flags: HOST array of `world`
 * device pointers.  Ordered behind everything `stream` has executed before, released at system scope. */
int vf_xgmi_signal(const void* const* peer_flags, int world, int rank, int slot, unsigned epoch, void* stream);
/* one wave waits until flag[slot][p] >= epoch for every p and slot in [slot_lo, slot_hi) of this rank's block; gives
 * up after timeout_us and stores 1 + slot_lo to *status (device unsigned) instead of hanging the queue */
int vf_xgmi_wait(const void* my_flags, int world, int slot_lo, int slot_hi, unsigned epoch, void* status,
                 long timeout_us, void* stream);
/* g = (arena_0 + ... + arena_{W-1}) / W in rank order -> gavg, then vf_adam_multi_dev's update of this rank's own
 * parameters; desc rows as vf_adam_multi with g = the slot in the LOCAL arena (p == 0: average only);
 * peer_bases: HOST array of `world` arena base pointers (own rank: my_base) */
int vf_xgmi_reduce_adam(const void* desc, int ntensors, long total_blocks, const void* const* peer_bases,
                        const float* my_base, float* gavg_base, int world, const float* scalars, float beta1,
                        float beta2, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_H */
