/*
 * pswin.h -- C ABI of libpswin_hip.so: the MI355X (gfx950) kernels behind the PanoSwin windowed-attention
 * hot path.
 *
 * The reference (1069066484/PanoSwinTransformerObjectDetection) has no native code and no FFI: every
 * step of the path is eager PyTorch inside mmdet/models/backbones/simple_panoswin_transformer.py ("HOT").
 * Each entry point below therefore names the reference *Python* function(s) it replaces (file:line
 * relative to the reference root); INTEGRATION.md shows the ctypes binding a reference maintainer adds.
 *
 * Conventions
 *   - plain C: raw device pointers, explicit sizes, no torch types.  `stream` is a hipStream_t passed as
 *     void* (NULL = the default stream).  The caller owns every buffer including workspaces; the library
 *     allocates nothing, keeps no global state and is thread-safe (the caller sets the device).
 *   - every function returns 0 on success, a negative PSWIN_ERR_* for a rejected argument, or a positive
 *     hipError_t from the launch.  Nothing aborts or throws.
 *   - launches are asynchronous on `stream`; no function synchronises.
 *   - "rows" are feature vectors of C contiguous elements; tensors are dense row-major.
 *   - dtype codes: PSWIN_F32 = 0, PSWIN_BF16 = 1 (bf16 = upper 16 bits of an IEEE f32, RNE conversion).
 *   - window size is 7 (49 tokens) and head_dim is 32 in every attention entry point, as in every
 *     configuration the reference ships (the swin model configs under configs/_base_/models: window_size=7, C/heads=32).
 */
#ifndef PSWIN_H_
#define PSWIN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSWIN_ABI_VERSION 11

#define PSWIN_F32 0
#define PSWIN_BF16 1

#define PSWIN_MODE_PLANAR 0
#define PSWIN_MODE_PANO 1

#define PSWIN_OK 0
#define PSWIN_ERR_ARG (-1)         /* null pointer, non-positive size, misaligned or inconsistent sizes */
#define PSWIN_ERR_UNSUPPORTED (-2) /* valid request outside what the kernels are specialised for */

#define PSWIN_WS 7        /* window size */
#define PSWIN_WTOK 49     /* tokens per window */
#define PSWIN_WPAD 64     /* tokens per window padded to the MFMA tile */
#define PSWIN_HEAD_DIM 32

int pswin_version(void);

/* ------------------------------------------------------------------------------------------------
 * Index maps (bit-exact integer work)
 * ---------------------------------------------------------------------------------------------- */

/* Host helper: padded grid of the window layout.
 * pano  : the north-south layout [2H, ceil(W/2)] padded to multiples of 7 (HOT:337-353, 486-491)
 * planar: [H, W] padded to multiples of 7 (HOT:486-491).
 * Writes Hp, Wp and the number of windows per image.  Pure host arithmetic, no launch. */
int pswin_window_grid(int mode, int H, int W, int* Hp, int* Wp, int* n_windows);

/* Window map and its inverse, on the device.
 * Replaces the chain WindowTransition.forward -> pad_x -> window_partition (HOT:376-409, 486-491, 64-75)
 * and, for `inv`, crop -> WindowTransition.forward(reverse=True) after window_reverse (HOT:78-92, 516-528).
 *   map[slot] , slot = window*49 + token : flat source token h*W+w, or -1 for a zero (padding) slot
 *   inv[h*W+w]                            : the slot that holds this token (every token has exactly one)
 * pano  : roll W by +shift, east-west -> north-south fold, roll H by +shift   (closed form)
 * planar: pad, then roll by (-shift, -shift)                                  (closed form)
 * map: int32 [n_windows*49]; inv: int32 [H*W]. */
int pswin_window_map(int mode, int H, int W, int shift, int32_t* map, int32_t* inv, void* stream);

/* Planar shifted-window attention mask, BasicLayer._get_attention_mask (HOT:664-688):
 * mask[w][i][j] = 0 if tokens i, j of window w lie in the same of the 9 shift regions else -100.0.
 * mask: f32 [n_windows, 49, 49] for the planar grid of (H, W). */
int pswin_planar_mask(int H, int W, int shift, float* mask, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Geometry (fp32)
 * ---------------------------------------------------------------------------------------------- */

/* make_uv_hw2 (HOT:153-189): uv[(y*W+x)*2 + {0,1}] = (u, v), u = x*gap - pi + gap/2, v = y*gap - pi/2 + gap/2,
 * gap = pi/H, evaluated in fp32 in exactly that order (no FMA contraction) -> bit-identical to the reference. */
int pswin_uv_grid(int H, int W, float* uv, void* stream);

/* SimplePanoSwinTransformer._pano_abs_position input features (HOT:926-932):
 * feat[t*5 + 0..4] = (sin u sin v, cos u sin v, cos v, u, v) for n tokens. */
int pswin_abs_pos_features(const float* uv, int n, float* feat, void* stream);

/* uv of every window slot: uv_win[slot] = uv[map[slot]] or (0, 0) in padding slots (the reference carries
 * uv as two feature channels, so zero padding zeroes them: HOT:504-513). */
int pswin_gather_uv(const float* uv, const int32_t* map, int n_slots, float* uv_win, void* stream);

/* haversine22 (lzx/models/great_circle.py:71-86) per window:
 * dist[w][i][j] = 2 asin(sqrt(sin^2(|v2_j - v1_i|/2) + cos v2_j cos v1_i sin^2((u2_j - u1_i)/2))).
 * uv1, uv2: f32 [n_windows, 49, 2]; dist: f32 [n_windows, 49, 49]. */
int pswin_haversine_windows(const float* uv1, const float* uv2, int n_windows, float* dist, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row movers (HBM-bound gathers; the copies of window_partition / window_reverse / roll / flip / cat /
 * pad that the reference materialises one by one: SURVEY appendix B)
 * ---------------------------------------------------------------------------------------------- */

/* win[b][slot][:] = map[slot] >= 0 ? (scale ? scale[b] : 1) * x[b][map[slot]][:] : 0
 * Forward of window partition (x = LayerNorm-ed features) and, with map = the forward map and scale = the
 * per-sample DropPath factor, backward of pswin_window_scatter_add.
 * x: [B, S, C] of x_dtype; win: [B, n_slots, C] of win_dtype; C % 8 == 0. */
int pswin_window_gather(const void* x, int x_dtype, const int32_t* map, const float* scale, void* win,
                        int win_dtype, int B, int S, int n_slots, int C, void* stream);

/* out[b][t][:] = (resid ? resid[b][t][:] : 0) + (scale ? scale[b] : 1) * (win[b][inv[t]][:] + (bias ? bias[:] : 0))
 * window_reverse + crop + reverse transition + residual add + DropPath scaling (HOT:483, 516-533), and,
 * with resid = NULL, backward of pswin_window_gather.  bias (f32 [C], may be NULL): the bias of the Linear that
 * produced win (proj, HOT:309; fc2, HOT:58), added here so that the GEMM runs without an epilogue and the bias
 * gradient comes out of pswin_ln_gather_bwd (dres_sum) instead of a column-sum pass over the GEMM's output gradient.
 * win: [B, n_slots, C] win_dtype; resid, out: [B, S, C] of x_dtype. */
int pswin_window_scatter_add(const void* win, int win_dtype, const int32_t* inv, const void* resid,
                             const float* scale, const float* bias, void* out, int x_dtype, int B, int S, int n_slots,
                             int C, void* stream);

/* LayerNorm fused into the window gather: y[b][slot][:] = LN(x[b][map[slot]][:]) * gamma + beta, zero rows in the
 * padding slots (the reference pads AFTER norm1: HOT:504, 512).  Replaces norm1 + WindowTransition + pad_x +
 * window_partition (HOT:503-513).  With map == NULL (then n_out must equal S) it is a plain row LayerNorm: norm2
 * (HOT:534), PatchEmbed.norm (HOT:771), the output norms (HOT:975-976).
 * Statistics (biased variance, eps inside the sqrt, as nn.LayerNorm) are fp32 and stored per SOURCE token:
 * mean, rstd: f32 [B, S].  x: [B, S, C] x_dtype; y: [B, n_out, C] y_dtype; gamma, beta: f32 [C]; 8 <= C <= 2048, C % 8 == 0. */
int pswin_ln_gather_fwd(const void* x, int x_dtype, const int32_t* map, const float* gamma, const float* beta, float eps,
                        void* y, int y_dtype, float* mean, float* rstd, int B, int S, int n_out, int C, void* stream);

/* The same with one more f32 row added to every normalised row: y[b][t][:] = LN(x[b][t][:]) * gamma + beta + add_rows[t][:].
 * add_rows: f32 [S, C] (NULL: nothing added) -- the absolute position encoding of HOT:926-934 (abs_encoder(xyzuv), the same for
 * every image) added to the PatchEmbed.norm output (HOT:771, 934) in the pass that writes it; map must be NULL with add_rows. */
int pswin_ln_gather_fwd_add(const void* x, int x_dtype, const int32_t* map, const float* gamma, const float* beta, float eps,
                            const float* add_rows, void* y, int y_dtype, float* mean, float* rstd, int B, int S, int n_out, int C,
                            void* stream);

/* Its backward: for every token (b, t), dy row = dy[b][inv ? inv[t] : t] and
 *   dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma, xhat = (x - mean) * rstd;
 *   dgamma = sum dy * xhat, dbeta = sum dy (block partials in `workspace`, reduced in a fixed order).
 * dres (may be NULL; f32 [B, S, C], needs x_dtype f32): the gradient reaching x along the residual shortcut
 * (x + DropPath(f(norm(x))), HOT:533-536); it is added into dx here, which replaces autograd's separate accumulation pass.
 * dres_sum (may be NULL; f32 [C]) = sum_{b,t} res_scale[b] * dres[b][t][:] (res_scale: f32 [B] DropPath factors or NULL = 1):
 * the gradient of a bias that pswin_window_scatter_add added on the branch whose shortcut dres came along (the proj /
 * fc2 bias of the block, HOT:309, 58), obtained from the pass that reads dres anyway.
 * dy: [B, n_out, C] dy_dtype; dx: [B, S, C] x_dtype; workspace: f32, pswin_ln_workspace(B * S, C) elements. */
int pswin_ln_gather_bwd(const void* dy, int dy_dtype, const int32_t* inv, const void* x, int x_dtype, const float* mean,
                        const float* rstd, const float* gamma, const float* dres, const float* res_scale,
                        float* dres_sum, void* dx, float* dgamma, float* dbeta, float* workspace, int B, int S, int n_out,
                        int C, void* stream);

/* pswin_ln_gather_bwd with a second output (round 4): ex[b][ex_map ? ex_map[t] : t] = bf16(ex_scale[b] * dx[b][t]) for every token, zero
 * rows at the ex_pads slots of every image -- the backward of the pswin_window_scatter_add that fed this LayerNorm's input (gather of the
 * residual-stream gradient into window order, or the plain bf16 cast of the Mlp branch), written while dx is in registers instead of by
 * pswin_window_gather re-reading it.  ex: bf16 [B, ex_rows, C]; ex_map: int32 [S] (token -> slot) or NULL (identity, ex_rows == S);
 * ex_pads: int32 [n_ex_pads = ex_rows - S] the slots no token maps to; ex_scale: f32 [B] or NULL.  x_dtype f32, C <= 1024.
 * ex == NULL: pswin_ln_gather_bwd. */
int pswin_ln_gather_bwd_ex(const void* dy, int dy_dtype, const int32_t* inv, const void* x, int x_dtype, const float* mean,
                           const float* rstd, const float* gamma, const float* dres, const float* res_scale, float* dres_sum, void* dx,
                           float* dgamma, float* dbeta, float* workspace, int B, int S, int n_out, int C, void* ex, const int32_t* ex_map,
                           int ex_rows, const float* ex_scale, const int32_t* ex_pads, int n_ex_pads, void* stream);

/* window_scatter_add followed at once by a token-order LayerNorm (the attention half of a block, HOT:516-536:
 * x1 = shortcut + DropPath(window_reverse(proj out) + proj bias), then norm2(x1)) in ONE pass:
 *   x1[b][t] = resid[b][t] + scale[b] * (win[b][inv[t]] + bias);   y[b][t] = LN(x1[b][t]) * gamma + beta
 * win: [B, n_slots, C] win_dtype; inv: int32 [S] or NULL (identity, n_slots == S); resid, x1: f32 [B, S, C]; scale: f32 [B]
 * or NULL; bias: f32 [C] or NULL; y: [B, S, C] y_dtype; mean, rstd: f32 [B, S].  Bitwise the result of
 * pswin_window_scatter_add + pswin_ln_gather_fwd; the backward pass is pswin_ln_gather_bwd + pswin_window_gather.
 * C % 8 == 0, C <= 1024. */
int pswin_scatter_add_ln_fwd(const void* win, int win_dtype, const int32_t* inv, const float* resid, const float* scale,
                             const float* bias, float* x1, const float* gamma, const float* beta, float eps, void* y,
                             int y_dtype, float* mean, float* rstd, int B, int S, int n_slots, int C, void* stream);

/* The same pass with the normalised rows written through a token -> slot map (round 4): y[b][out_map[t]] = LN(x1[b][t]) ..., zero rows at
 * the out_pads slots -- the residual add that ends a block (x + DropPath(mlp)) fused with the NEXT block's norm1 + shift + pad + window
 * partition (HOT:534-536 then HOT:503-513 of the following block): the new residual stream is written once and not re-read by a
 * LayerNorm + gather kernel.  y: [B, n_out, C]; out_map: int32 [S] or NULL (then n_out == S: pswin_scatter_add_ln_fwd);
 * out_pads: int32 [n_out_pads = n_out - S]. */
int pswin_scatter_add_ln_fwd_map(const void* win, int win_dtype, const int32_t* inv, const float* resid, const float* scale,
                                 const float* bias, float* x1, const float* gamma, const float* beta, float eps, void* y, int y_dtype,
                                 float* mean, float* rstd, int B, int S, int n_slots, int C, const int32_t* out_map, int n_out,
                                 const int32_t* out_pads, int n_out_pads, void* stream);

/* Output norms: y = LayerNorm(x) written channel-major, i.e. norm{i}(x).view(B, H, W, C).permute(0, 3, 1, 2).contiguous()
 * of HOT:975-977 in one pass (x: f32 [B, S, C]; y: f32 [B, C, S]; mean, rstd: f32 [B, S]), and its backward from the
 * NCHW gradient dy f32 [B, C, S] (dres as in pswin_ln_gather_bwd; workspace: pswin_ln_workspace(B * S, C) elements).
 * pswin_ln_nchw_supported(S, C) != 0 when the token count per image fits the kernels' tiling (S % (256 / lanes(C)) == 0). */
int pswin_ln_nchw_supported(int S, int C);
int pswin_ln_nchw_fwd(const float* x, const float* gamma, const float* beta, float eps, float* y, float* mean, float* rstd,
                      int B, int S, int C, void* stream);
/* The same with the residual add that closes the stage in front of it (HOT:536 followed by 975-977):
 *   x1[b][t] = x[b][t] + scale[b] * (win[b][t] + bias)   (win: bf16 [B, S, C] in token order, scale: f32 [B] or NULL, bias: f32 [C] or NULL),
 * written to x1 and normalised in the same pass; bitwise pswin_window_scatter_add followed by pswin_ln_nchw_fwd.  win == NULL: plain. */
int pswin_scatter_add_ln_nchw_fwd(const void* win_bf16, const float* x, const float* scale, const float* bias, float* x1,
                                  const float* gamma, const float* beta, float eps, float* y, float* mean, float* rstd, int B, int S,
                                  int C, void* stream);
int pswin_ln_nchw_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                      const float* dres, float* dx, float* dgamma, float* dbeta, float* workspace, int B, int S, int C,
                      void* stream);
/* The same with a second output: ex_bf16 [B, S, C] = bf16(ex_scale[b] * dx[b]) (ex_scale: f32 [B] DropPath factors or NULL = 1) -- the
 * gradient that flows into the MLP branch which closes the stage (x + DropPath(mlp(norm2(x))), HOT:536, followed by norm{i}, HOT:975):
 * the backward of pswin_window_scatter_add's cast, written in the pass that produces dx. */
int pswin_ln_nchw_bwd_ex(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                         const float* dres, float* dx, float* dgamma, float* dbeta, float* workspace, void* ex_bf16,
                         const float* ex_scale, int B, int S, int C, void* stream);

/* Workspace elements for the LayerNorm backward kernels over `rows` walked rows of width C. */
int pswin_ln_workspace(long long rows, int C);

/* The three LayerNorm backward entry points accept dgamma == dbeta == NULL ("partial rows only"): the kernel leaves
 * pswin_ln_partial_rows(rows, C) rows of [dgamma(C) | dbeta(C)] (or [dgamma | dbeta | dres_sum] when dres_sum != NULL;
 * dres_sum is then only a flag and is not written) in `workspace`, and the caller sums them later, typically together
 * with every other parameter-gradient reduction of the backward pass through pswin_reduce_jobs. */
int pswin_ln_partial_rows(long long rows, int C);
/* Process-wide tuning hook of the LayerNorm family.  Rows of C == 96, 192, 384 or 768 elements whose operands lie within 32-bit byte
 * offsets run on exact-row kernels (no chunk test, all loads of a row in flight together); the results are bitwise those of the generic
 * kernels.  mode 0 = automatic (default), 1 = always the generic kernels (for tests and A/B measurements). */
int pswin_ln_rows_tune(int mode);

/* PatchMerging gather fused with its LayerNorm(4C) (HOT:563-574): y[b][i*W2+j] = LN(concat of the 4 tokens).
 * x: [B, H*W, C]; y: [B, H2*W2, 4C]; gamma, beta: f32 [4C]; mean, rstd: f32 [B, H2*W2]; C % 16 == 0, 4C <= 2048. */
int pswin_ln_patch_merge_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, float eps, void* y,
                             int y_dtype, float* mean, float* rstd, int B, int H, int W, int C, void* stream);

/* Its backward; dx: [B, H*W, C] (every token belongs to exactly one merged row);
 * workspace: pswin_ln_workspace(B * H2 * W2, 4 * C) elements. */
int pswin_ln_patch_merge_bwd(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* mean,
                             const float* rstd, const float* gamma, void* dx, float* dgamma, float* dbeta,
                             float* workspace, int B, int H, int W, int C, void* stream);

/* PatchMerging gather (HOT:560-573): out[b][i*W2+j][k*C + c] = x[b][(2i+dy_k)*W + 2j+dx_k][c] or 0 outside,
 * (dy,dx)_k = (0,0),(1,0),(0,1),(1,1); H2 = ceil(H/2), W2 = ceil(W/2).  x: [B, H*W, C], out: [B, H2*W2, 4C]. */
int pswin_patch_merge_gather(const void* x, int x_dtype, void* out, int out_dtype, int B, int H, int W, int C,
                             void* stream);

/* Its adjoint: dx[b][h*W+w][c] = dout[b][(h/2)*W2 + w/2][((h&1) + 2*(w&1))*C + c]. */
int pswin_patch_merge_scatter(const void* dout, int out_dtype, void* dx, int x_dtype, int B, int H, int W, int C,
                              void* stream);

/* BatchNorm2d + ReLU of the PatchEmbed stem (nn.BatchNorm2d + nn.ReLU after each 3x3 convolution, HOT:742-748) on a
 * channels-last activation viewed as rows y[M = N*H*W, C]:  z = relu((y - mean) * rstd * gamma + beta).
 * train != 0: mean / biased variance of the batch (nn.BatchNorm2d training semantics), running_mean / running_var
 * (may be NULL) updated in place with `momentum` and the unbiased variance; train == 0: the running statistics.
 * mean_offset (may be NULL): a per-channel constant the caller has NOT added to y although the reference adds it in
 * front of the BatchNorm (the convolution bias, HOT:743/746): it cancels in z and only shifts the tracked mean, so it is
 * folded into running_mean (train) / subtracted from it (eval) instead of costing a pass over the activation.
 * save_mean, save_rstd: f32 [C], kept for the backward pass.  y, z: dtype f32 or bf16, C % 8 == 0, C <= 1024.
 * workspace: f32, pswin_bn_workspace(C) elements. */
int pswin_bn_workspace(int C);
int pswin_bn_relu_fwd(const void* y, int dtype, const float* gamma, const float* beta, const float* mean_offset,
                      float eps, float momentum, int train, float* running_mean, float* running_var, void* z, float* save_mean, float* save_rstd,
                      float* workspace, long long M, int C, void* stream);

/* Its backward: g = dz * [z > 0];  dy = gamma * rstd * (g - mean(g) - xhat * mean(g * xhat)) (train) or
 * gamma * rstd * g (eval);  dgamma = sum g * xhat, dbeta = sum g (fixed summation order). */
int pswin_bn_relu_bwd(const void* dz, const void* y, int dtype, const float* gamma, const float* beta,
                      const float* save_mean, const float* save_rstd, int train, void* dy, float* dgamma, float* dbeta,
                      float* workspace, long long M, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused PatchEmbed stem (HOT:742-750: Conv3x3(3->32) BN ReLU Conv3x3(32->64) BN ReLU Conv4x4/s4(64->96)), bf16
 * operands / f32 accumulation, specialised for embed_dim 96, in_chans 3, patch_size 4.  Only y2 (the second
 * convolution's output) is ever stored at full resolution; see csrc/pswin_stem.hip for the data flow.
 * Packed operands (bf16): x4 [B][H][W][4] (channel 3 = 1), w1p [32][12][4] (tap-major, taps 9..11 / channel 3 zero),
 * w2p [9][64 out][32 in], w2t [9][32 in][64 out], w3p [16][96 out][64 in], w3t [16][64 in][96 out].
 * scale / shift: the BatchNorm folded to z = scale * y + shift per channel (f32).  workspace: f32,
 * pswin_stem_workspace(B, H, W) elements.
 * ---------------------------------------------------------------------------------------------- */
int pswin_stem_workspace(int B, int H, int W);
/* [B,3,H,W] f32 -> x4 */
int pswin_stem_pack_input(const float* x, int B, int H, int W, void* x4, void* stream);
/* sums: f32 [64 + 48*48]: per-channel sum / sum of squares of y1 = conv1(x) over all pixels (y1 is not stored), then
 * (want_xx) the input autocorrelation XX[k][k'] = sum_p xp[p][k] xp[p][k'] over the 48 tap-channel slots (slot
 * 4*4+3, the centre tap's ones channel, yields the plain sums and the pixel count) used by the backward pass. */
int pswin_stem_conv1_stats(const void* x4, const void* w1p, int B, int H, int W, int want_xx, float* sums,
                           float* workspace, void* stream);
/* y2 = conv2(relu(scale1 * conv1(x) + shift1)) (no bias), [B][H][W][64] bf16; sums2 (may be NULL): f32 [128] per-channel
 * sum / sum of squares of y2. */
int pswin_stem_conv2_fwd(const void* x4, const void* w1p, const float* scale1, const float* shift1, const void* w2p, int B,
                         int H, int W, void* y2, float* sums2, float* workspace, void* stream);
/* tokens[B*H/4*W/4][96] bf16 = conv3(relu(scale2 * y2 + shift2)) + bias3 */
int pswin_stem_conv3_fwd(const void* y2, const float* scale2, const float* shift2, const void* w3p, const float* bias3,
                         int B, int H, int W, void* tokens, void* stream);

/* Backward of the stem.  dtok: [M][96] bf16 gradient of the tokens.
 * conv3_bwd_stats: g2 = (dtok . W3)[pixel] * [scale2 y2 + shift2 > 0]; sums f32 [128] = per-channel sum g2 (= dbeta2),
 *   sum g2 * yhat2 (= dgamma2), yhat2 = a y2 + b.  prm: f32 [4][64] = scale2, shift2, a = rstd2, b = -mean2 rstd2.
 * conv3_bwd_data: dy2 = k1 g2 - P y2 - Q, [B][H][W][64] bf16.  prm: f32 [5][64] = scale2, shift2, k1, P, Q
 *   (training-mode BatchNorm backward: k1 = gamma rstd, P = k1 a mean(g2 yhat2), Q = k1 (mean g2 + b mean(g2 yhat2))).
 * conv3_wgrad: dw3 f32 [4 ky][8 waves][12][256] accumulator tiles (decoded by the host: stem.decode_dw3) of
 *   sum_tokens dtok (x) relu(scale2 y2 + shift2) patches.
 * conv2_wgrad: dw2 f32 [2][36][256] accumulator tiles (stem.decode_dw2) of sum_p dy2[p] (x) a1[p + tap], a1 recomputed.
 * perm (both; int32, may be NULL): where each accumulator element goes in the parameter layout ([96][64][4][4] /
 *   [64][32][3][3]); with it the final column sum writes the gradient directly in nn.Conv2d's weight layout.
 * conv2_bwd: out f32 [64 + 32*48]: sum g1 (= dbeta1), sum g1 * yhat1 (= dgamma1), G[ch][slot] = sum_p g1[p][ch] xp[p][slot]
 *   with g1 = conv2 data gradient of dy2 masked by relu(bn1 y1) > 0, never stored.  prm: f32 [4][32] = scale1, shift1,
 *   a = rstd1, b = -mean1 rstd1. */
int pswin_stem_conv3_bwd_stats(const void* dtok, const void* y2, const float* prm, const void* w3t, int B, int H, int W,
                               float* sums, float* workspace, void* stream);
int pswin_stem_conv3_bwd_data(const void* dtok, const void* y2, const float* prm, const void* w3t, int B, int H, int W,
                              void* dy2, void* stream);
int pswin_stem_conv3_wgrad(const void* dtok, const void* y2, const float* scale2, const float* shift2, int B, int H, int W,
                           const int32_t* perm, float* dw3, float* workspace, void* stream);
int pswin_stem_conv2_wgrad(const void* x4, const void* w1p, const float* scale1, const float* shift1, const void* dy2, int B,
                           int H, int W, const int32_t* perm, float* dw2, float* workspace, void* stream);
int pswin_stem_conv2_bwd(const void* x4, const void* w1p, const float* prm, const void* dy2, const void* w2t, int B, int H,
                         int W, float* out, float* workspace, void* stream);

/* Bias + exact GELU between fc1 and fc2 of Mlp (HOT:44-61).  y: [M, N] pre-activation WITHOUT the bias (the GEMM runs
 * without an epilogue), bias: f32 [N] or NULL, dtype f32 or bf16, N % 8 == 0.
 *   fwd: h = gelu(y + bias)      bwd: dy = dh * gelu'(y + bias), dbias[n] = sum_m dy[m][n] (f32, fixed order)
 * workspace: f32, pswin_bias_gelu_workspace(M, N) elements. */
int pswin_bias_gelu_fwd(const void* y, int dtype, const float* bias, void* h, long long M, int N, void* stream);
int pswin_bias_gelu_workspace(long long M, int N);
int pswin_bias_gelu_tune(int unr_fwd, int unr_bwd);   /* rows steps per block of the two kernels: 1, 2 or 4 (default 2, 4) */
int pswin_bias_gelu_partial_rows(long long M, int N, int dtype);   /* rows of N sums left in workspace when dbias == NULL */
int pswin_bias_gelu_bwd(const void* dh, const void* y, int dtype, const float* bias, void* dy, float* dbias,
                        float* workspace, long long M, int N, void* stream);

/* Small parameter kernels of the stem (one launch each).
 * pack_weights: nn.Conv2d weights f32 ([32,3,3,3], [64,32,3,3], [96,64,4,4]) -> w1p, w2p, w2t, w3p, w3t (bf16).
 * bn_fold: per-channel sum / sum of squares over `count` values of a bias-free convolution output -> prm f32 [4][C] =
 *   scale, shift, rstd, -mean * rstd (z = scale y + shift, yhat = rstd y - mean rstd); training != 0: batch statistics
 *   and nn.BatchNorm2d's running-statistics update (conv_bias, which cancels in z, is added to the tracked mean);
 *   training == 0: running statistics (conv_bias subtracted from the mean).
 * bn2_coefs: sums f32 [2][64] of conv3_bwd_stats + prm [4][64] -> prm5 f32 [5][64] = scale, shift, k1, P, Q for
 *   conv3_bwd_data (P = Q = 0 when training == 0).
 * conv1_wgrad: out5 of conv2_bwd, XX of conv1_stats (training), w1p, prm1 [4][32] -> dw1 f32 [32][3][3][3] and db1
 *   (zero in training: a bias in front of a BatchNorm has no gradient). */
int pswin_stem_pack_weights(const float* w1, const float* w2, const float* w3, void* w1p, void* w2p, void* w2t, void* w3p,
                            void* w3t, void* stream);
int pswin_stem_bn_fold(const float* sum, const float* sumsq, double count, const float* gamma, const float* beta,
                       const float* conv_bias, float eps, float momentum, int training, float* running_mean,
                       float* running_var, int C, float* prm, long long* num_batches_tracked, void* stream);
/* (num_batches_tracked: nn.BatchNorm2d's int64 counter, incremented by one on the device, or NULL) */
int pswin_stem_bn2_coefs(const float* sums, const float* prm, double count, int training, float* prm5, void* stream);
int pswin_stem_conv1_wgrad(const float* out5, const float* xx, const void* w1p, const float* prm1, double count, int training,
                           float* dw1, float* db1, void* stream);

/* Tiled bf16 GEMM for the Linear layers of stages 1-3 (qkv / proj / fc1 / fc2 / reduction, HOT:287, 309, 50-58, 575) and,
 * through a transposed copy of the weight, their data gradients:  y[M, N] = x[M, K] . w[N, K]^T (+ bias), bf16 in / out,
 * f32 accumulation, bias f32 [N] or NULL.  128 (or 64 / 96) x 192 macro tiles, both operands by LDS-DMA into XOR-swizzled
 * LDS tiles: double buffered with two workgroups per CU, or -- launches of at most 256 tiles -- four stages with three k-steps in
 * flight and one workgroup per CU (csrc/pswin_gemm_nt.hip).  Needs N % 192 == 0, K % 64 == 0, M >= 64 (pswin_gemm_nt_supported).
 * tile_m: 0 = choose, or 64 / 96 / 128 (96: plain epilogue only). */
/* The same product with a three-stage LDS ring (counted waits, one raw barrier per 64-row slab, one 8-wave workgroup per CU):
 * csrc/pswin_gemm_tn.hip, "Round 3".  One macro tile of 192 x 192 serves every Linear of the model (N % 192 == 0, K % 192 == 0).
 * partial: [splits, N, K] in `partial_dtype` (PSWIN_F32, or PSWIN_BF16 = each split's tile rounded once, as the library's batched GEMM
 * does for its row chunks); 1 <= splits <= M / 64; pswin_gemm_tn_ring_splits(M, N, K, target_wgs) suggests a split count for about
 * target_wgs workgroups (0 = 256: one per CU). */
int pswin_gemm_tn_ring_supported(long long M, int N, int K);
int pswin_gemm_tn_ring_splits(long long M, int N, int K, int target_wgs);
int pswin_gemm_tn_ring(const void* dy, const void* x, void* partial, int partial_dtype, long long M, int N, int K, int splits, void* stream);
/* The same launch with the bias gradient of the Linear riding along (autograd of HOT:287: db = column sums of dy): dbias_partial
 * f32 [splits][N] receives, per row split, the column sums of dy over the split's rows (summed by pswin_reduce_jobs like the
 * weight partials); columns zero_lo <= n < zero_hi are written as exact zeros (the K third of the qkv bias gradient sums to
 * zero analytically: ops.linear's zero_bias_cols).  dbias_partial = NULL: pswin_gemm_tn_ring. */
int pswin_gemm_tn_ring_bias(const void* dy, const void* x, void* partial, int partial_dtype, float* dbias_partial, int zero_lo, int zero_hi,
                            long long M, int N, int K, int splits, void* stream);

/* Several weight gradients in ONE launch per tile geometry (round 4).  A weight gradient is not needed before the backward pass ends,
 * so the host can queue them (ops.py: deferred weight gradients) and issue them together: with ~50 products in flight at once no
 * product needs a 256-way row split to fill the chip, so every workgroup contracts a few thousand rows and the partial-slab traffic
 * (256 x 192 x 192 x 2 B = 18.9 MB per product when each is launched alone) falls with the split count; per-launch ramps disappear.
 * Jobs are independent; each is the argument list of pswin_gemm_tn_ring_bias.  `jobs` is a HOST array (copied into the kernel
 * arguments, <= 48 jobs per launch and geometry; list the longest row ranges first).  splits == 1 with partial_dtype == PSWIN_F32 writes
 * the finished [N, K] gradient (no reduction needed). */
typedef struct pswin_tn_job {
    const void* dy;       /* bf16 [M, N] */
    const void* x;        /* bf16 [M, K] */
    void* partial;        /* [splits, N, K] in partial_dtype */
    float* dbias_partial; /* f32 [splits, N] or NULL */
    long long M;
    int N, K, splits, partial_dtype, zero_lo, zero_hi;
    /* Sample liveness (optional; NULL = every row is contracted): the rows are sample-major, sample b owns rows [b * rows_per_sample,
     * (b + 1) * rows_per_sample), M = B * rows_per_sample with B <= 64, and sample_scale is the f32 [B] per-sample DropPath factor
     * vector on the device.  sample_scale[b] == 0 declares sample b dead: its rows of dy are exact zeros, and the 64-row slabs that
     * lie entirely inside dead samples are not read (neither operand); slabs that straddle a live sample are contracted as always. */
    const float* sample_scale;
    int rows_per_sample;
} pswin_tn_job;
int pswin_gemm_tn_ring_jobs(const pswin_tn_job* jobs, int n_jobs, void* stream);
/* bytes of the job table one launch carries in its kernel arguments (<= 4,000: the 4 KB segment) */
int pswin_gemm_tn_ring_table_bytes(void);

typedef struct pswin_transpose_job {
    const void* src; /* bf16 [rows][cols] */
    void* dst;       /* bf16 [cols][rows] */
    int rows;
    int cols;
} pswin_transpose_job;
/* dst = src^T for every job in one launch (rows, cols multiples of 64): the per-step [K][N] bf16 copies of the Linear
 * weights with which pswin_gemm_nt computes data gradients.  `jobs` is a HOST array, copied into the kernel arguments. */
int pswin_transpose_jobs(const pswin_transpose_job* jobs, int n_jobs, void* stream);

/* AdamW over the one flat fp32 parameter buffer of a model: the update that ends every training step of the path (the reference runs
 * torch.optim.AdamW through mmcv's OptimizerHook, mmdet/apis/train.py:91-112 with the configs/swin files: lr 1e-4, betas (0.9, 0.999),
 * weight_decay 0.05), fused with the bf16 copy of the updated parameters that the next step's kernels read.  p, g, m, v: f32 [n]
 * (n a multiple of 4, 16-byte aligned); p_bf16: bf16 [n] or NULL; step: DEVICE pointer to the number (>= 1, as a float) of the step being
 * taken.  Same arithmetic, element by element, as torch.optim.AdamW. */
int pswin_adamw_flat(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, double lr, double beta1, double beta2, double eps,
                     double weight_decay, const float* step, void* stream);
/* The same update with PARAMETER GROUPS, as the reference's optimizer is configured
 * (configs/swin/mask_rcnn_swin_tiny_patch4_window7_mstrain_480-800_adamw_1x_coco.py:64-67: paramwise_cfg.custom_keys give every parameter
 * whose name contains 'norm' / 'relative_position_bias_table' / 'absolute_pos_embed' decay_mult = 0; mmcv's optimizer constructor turns that
 * into per-parameter groups).  group_of: DEVICE array of n / 4 bytes, the group (< n_groups <= PSWIN_ADAMW_MAX_GROUPS) of elements
 * 4 i .. 4 i + 3 (parameters start on 64-element boundaries of the flat buffer, so a granule never straddles two); lr_mult / decay_mult:
 * HOST arrays of n_groups multipliers (copied into the kernel arguments).  Group k is updated exactly as torch.optim.AdamW updates a
 * group with lr * lr_mult[k] and weight_decay * decay_mult[k].  group_of == NULL (n_groups 0): one group, = pswin_adamw_flat. */
#define PSWIN_ADAMW_MAX_GROUPS 8
int pswin_adamw_flat_groups(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, const unsigned char* group_of,
                            int n_groups, const float* lr_mult, const float* decay_mult, double lr, double beta1, double beta2, double eps,
                            double weight_decay, const float* step, void* stream);

/* ---- the training recipe on the device: lr schedule, gradient-norm clipping, non-finite guard -----------------------------------
 * mmcv's LrUpdaterHook (configs/_base_/schedules/schedule_1x.py:5-10: policy 'step', linear warmup) and OptimizerHook(grad_clip)
 * (mmdet/utils/optimizer.py:30-32 -> clip_grad_norm_) evaluated on the device, so that a captured step (hipGraph replay) follows
 * them without a host synchronisation.  One step is up to three launches on `stream`:
 *   pswin_grad_sumsq      (only with clipping or the guard)  gradient -> PSWIN_GRADSQ_PARTIALS f64 partial sums of squares
 *   pswin_adamw_record    (one workgroup)                    partials + schedule + counters -> pswin_step_record
 *   pswin_adamw_flat_sched                                   the AdamW update of pswin_adamw_flat_groups with the record's
 *                                                            lr per group, step number t and clip coefficient
 * Schedule, with i = the 0-based iteration about to run (`*iteration` before the record's increment), e = i / iters_per_epoch
 * when by_epoch, base_k = lr * lr_mult[k]:
 *   policy STEP:  progress = by_epoch ? e : i; exp = #{milestones s : progress >= s} (or progress / step_every when
 *                 n_milestones = 0); regular_k = base_k * gamma^exp, then max(regular_k, min_lr) when has_min_lr
 *   policy FIXED: regular_k = base_k
 *   warmup, while i < warmup_iters: CONSTANT regular_k * ratio; LINEAR regular_k * (1 - (1 - i / warmup_iters) * (1 - ratio));
 *                 EXP regular_k * ratio^(1 - i / warmup_iters)
 * All of it in double.  The struct is a HOST pointer, copied into the kernel arguments. */
#define PSWIN_LR_FIXED 0
#define PSWIN_LR_STEP 1
#define PSWIN_WARMUP_NONE 0
#define PSWIN_WARMUP_CONSTANT 1
#define PSWIN_WARMUP_LINEAR 2
#define PSWIN_WARMUP_EXP 3
#define PSWIN_LR_MAX_MILESTONES 8
#define PSWIN_GRADSQ_PARTIALS 1024
typedef struct pswin_lr_schedule {
    int policy;                                 /* PSWIN_LR_FIXED / PSWIN_LR_STEP */
    int warmup;                                 /* PSWIN_WARMUP_* */
    int warmup_iters;                           /* in iterations (warmup_by_epoch already multiplied out); >= 1 with a warmup */
    int by_epoch;                               /* the step policy counts epochs of iters_per_epoch iterations */
    int iters_per_epoch;                        /* >= 1 when by_epoch */
    int n_milestones;                           /* 0 .. PSWIN_LR_MAX_MILESTONES, ascending */
    int step_every;                             /* n_milestones == 0: exp = progress / step_every (mmcv's int `step`); 0 = never */
    int has_min_lr;
    int milestones[PSWIN_LR_MAX_MILESTONES];
    double warmup_ratio;
    double gamma;
    double min_lr;
} pswin_lr_schedule;
/* What one step applies, written by pswin_adamw_record into DEVICE memory (96 bytes, 8-byte aligned). */
typedef struct pswin_step_record {
    double lr[PSWIN_ADAMW_MAX_GROUPS];          /* scheduled lr of every parameter group (lr_mult included) */
    double norm;                                /* 2-norm of the whole gradient before clipping; 0 when it was not computed */
    float lr_base;                              /* (float)lr[0]: group 0 is the base group (lr_mult 1) */
    float norm_f;                               /* (float)norm */
    float coef;                                 /* clip coefficient min(1, max_norm / (norm + 1e-6)); 1 without clipping */
    float t;                                    /* Adam step number the update uses (*step after the record) */
    int applied;                                /* 0: the guard saw a non-finite norm and the update leaves everything alone */
    int iteration;                              /* i of this step */
} pswin_step_record;
/* partials: DEVICE f64 [PSWIN_GRADSQ_PARTIALS]; partial b = sum of g[j]^2 over a fixed contiguous range of j, in a fixed order
 * (bit-identical from run to run).  g: f32 [n], n a multiple of 4, 16-byte aligned. */
int pswin_grad_sumsq(const float* g, long long n, double* partials, void* stream);
/* One workgroup.  partials: the output of pswin_grad_sumsq, or NULL (then norm = 0, coef = 1, every step applied; max_norm must be
 * <= 0 and skip_nonfinite 0).  max_norm > 0: clip; <= 0: no clipping.  Counters (DEVICE f32 scalars, exact up to 2^24):
 * *iteration += 1 always; *step += 1 when the step is applied (always without skip_nonfinite, finite norm with it);
 * *skipped += 1 otherwise.  lr: the base lr; lr_mult: HOST array of n_groups (1 .. PSWIN_ADAMW_MAX_GROUPS) multipliers, NULL = one
 * group.  record: DEVICE. */
int pswin_adamw_record(const double* partials, const pswin_lr_schedule* sched, double lr, int n_groups, const float* lr_mult,
                       double max_norm, int skip_nonfinite, float* step, float* iteration, float* skipped, pswin_step_record* record,
                       void* stream);
/* The update of pswin_adamw_flat_groups (same arithmetic, same bf16 shadow write) with lr per group, t and the clip coefficient read
 * from `record` (DEVICE): the gradient enters as g * coef in f32 and is not written back (the buffer keeps the unclipped gradient);
 * record->applied == 0 leaves p, m, v and p_bf16 untouched.  decay_mult: HOST array of n_groups multipliers (NULL with group_of
 * NULL, n_groups 0 = one group). */
int pswin_adamw_flat_sched(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, const unsigned char* group_of,
                           int n_groups, const float* decay_mult, double beta1, double beta2, double eps, double weight_decay,
                           const pswin_step_record* record, void* stream);
/* ---- the caller's side of the path: RoIAlign over an FPN pyramid ------------------------------------------------
 * configs/_base_/models/mask_rcnn_swin_fpn.py:44-48, 63-67 (SingleRoIExtractor, RoIAlign output 7 / 14, sampling_ratio = 0, strides
 * 4..32) and mmdet/models/roi_heads/roi_extractors/single_level_roi_extractor.py:78-108.  RoIAlign itself is mmcv.ops (not in the
 * reference tree): the published operator is implemented (csrc/pswin_roi.hip states it); parity with the reference is unpinned.
 * Feature maps are NHWC [B, H, W, C] (`dtype`), rois f32 [R, 5] = (batch index, x1, y1, x2, y2) in image pixels, roi_level int32 [R]
 * = the pyramid level of every RoI (map_roi_levels, :55-60, computed by the caller), out / dout [R, P, P, C] (`dtype`).
 * Backward ACCUMULATES (f32 atomics) into the f32 NHWC maps levels->dfeat, which the caller zeroes. */
#define PSWIN_ROI_MAX_LEVELS 4
typedef struct pswin_roi_levels {
    const void* feat[PSWIN_ROI_MAX_LEVELS]; /* forward: feature maps (NULL in backward) */
    float* dfeat[PSWIN_ROI_MAX_LEVELS];     /* backward: gradient maps (NULL in forward) */
    int H[PSWIN_ROI_MAX_LEVELS];
    int W[PSWIN_ROI_MAX_LEVELS];
    float spatial_scale[PSWIN_ROI_MAX_LEVELS]; /* 1 / stride */
    int n_levels;
} pswin_roi_levels;
int pswin_roi_align_supported(int C, int dtype);
int pswin_roi_align_fwd(const pswin_roi_levels* levels, const float* rois, const int32_t* roi_level, int R, int C, int P, int sampling_ratio,
                        int aligned, int dtype, void* out, void* stream);
int pswin_roi_align_bwd(const pswin_roi_levels* levels, const float* rois, const int32_t* roi_level, int R, int C, int P, int sampling_ratio,
                        int aligned, int dtype, const void* dout, void* stream);

/* Greedy NMS over `groups` independent lists of boxes sorted by descending score -- the proposal stage of RPNHead (mmcv.ops.nms inside
 * mmdet/models/dense_heads/rpn_head.py: one list per image and pyramid level): keep[i] = no kept j < i with IoU(i, j) > iou_threshold.
 * boxes f32 [groups][nmax][4] (x1, y1, x2, y2), counts int32 [groups] (valid boxes per group) or NULL (= nmax everywhere), keep uint8
 * [groups][nmax] (1 = kept, 0 = suppressed or past the group's count).  nmax <= 2048, a multiple of 64.  Unpinned like RoIAlign (mmcv.ops is not in
 * the reference tree): tests check it against the sequential rule. */
int pswin_nms_workspace(int groups, int nmax);                 /* bytes of workspace for pswin_nms_groups (the suppression bit masks); groups <= 2048 */
int pswin_nms_groups(const float* boxes, const int32_t* counts, int groups, int nmax, float iou_threshold, unsigned char* keep, void* workspace,
                     void* stream);

/* MaxIoUAssigner.assign for a padded batch (mmdet/core/bbox/assigners/max_iou_assigner.py:85-212; gt_max_assign_all = True, no
 * gt_bboxes_ignore): the target assignment of the RPN and of the RoI head, with the per-image box count read from DEVICE memory, so that
 * a captured step takes the next batch's annotations by copying them into the same buffers.
 *   cand      f32 [N][4] shared by every image (cand_per_image = 0: the RPN's anchors) or [B][N][4] (cand_per_image = 1: the RoI stage)
 *   gt        f32 [B][Gmax][4], gt_count int32 [B] on the device: rows at index >= gt_count[b] are padding and are never read as boxes
 *   lead_gt   0, or the number of leading candidates of image b that are its own gt rows (add_gt_as_proposals: Gmax); a candidate
 *             i < lead_gt with i >= gt_count[b] is padding: gt_inds = -1, max_iou = -1, and it takes no part in any maximum
 *   gt_inds   int64 [B][N]: -1 ignore, 0 negative, g + 1 matched to gt g;  max_iou f32 [B][N] or NULL
 * For image b with G = gt_count[b]: G == 0 -> every other candidate gets gt_inds = 0 and max_iou = 0 (:147-153); otherwise IoU as
 * detector.box_iou (clamped widths, union (area_gt + area_cand) - inter floored at 1e-6), best = max over g, arg = the lowest g that
 * reaches it; 0 <= best < neg_iou_thr -> 0; best >= pos_iou_thr -> arg + 1; with match_low_quality every candidate whose IoU with gt g
 * EQUALS that gt's maximum over the valid candidates is reassigned to g + 1 when that maximum is >= min_pos_iou (the largest such g: the
 * reference's sequential loop).  Inputs are finite; the result with a NaN is unspecified.
 * Two launches, no atomics, nothing to clear between calls: per-workgroup partial maxima go to `workspace` with plain stores and are
 * folded in index order, so the outputs are bit-identical from call to call and from graph replay to graph replay.
 * 1 <= Gmax <= 256, N >= 1, B >= 1, 0 <= lead_gt <= N, 16-byte aligned cand / gt / workspace; anything else is PSWIN_ERR_ARG. */
int pswin_max_iou_assign_rows_per_workgroup(void);              /* candidates one workgroup of the first launch covers */
int pswin_max_iou_assign_workspace(int B, int N, int Gmax);     /* bytes of workspace for pswin_max_iou_assign, or PSWIN_ERR_ARG */
int pswin_max_iou_assign(const float* cand, int cand_per_image, const float* gt, const int32_t* gt_count, int B, int N, int Gmax, int lead_gt,
                         float pos_iou_thr, float neg_iou_thr, float min_pos_iou, int match_low_quality, long long* gt_inds, float* max_iou,
                         void* workspace, void* stream);

int pswin_gemm_nt_supported(long long M, int K, int N);
int pswin_gemm_nt(const void* x, const void* w, const float* bias, void* y, long long M, int K, int N, int tile_m, void* stream);
/* The same product with an f32 result (y: f32 [M, N], M * N * 4 < 4 GiB): PatchMerging.reduction (HOT:575), whose output is the fp32
 * residual stream of the next stage -- written once instead of as bf16 plus a cast. */
int pswin_gemm_nt_f32(const void* x, const void* w, const float* bias, float* y, long long M, int K, int N, int tile_m, void* stream);
/* The data gradient of the Mlp's fc2 fused with the backward of fc1's bias + nn.GELU (HOT:50-58):
 *   dpre[M, N] = (dy[M, K] . w_t[N, K]^T) * gelu'(pre + bias),   partial[t][n] = sum over the rows of row tile t of dpre[., n]
 * with w_t = fc2.weight^T ([hidden N, K]), pre = the pre-activation fc1(x) without bias, bias = fc1.bias (f32 [N] or NULL).
 * dL/dh is never written.  partial: f32 [pswin_gemm_nt_partial_rows(M, tile_m), N]; its column sums are the fc1 bias
 * gradient (pswin_reduce_jobs).  tile_m: 64 or 128. */
/* fc1 of the Mlp with its bias + nn.GELU in the GEMM epilogue (HOT:50-57):  pre = x . w^T (no bias; kept for the backward pass),
 * h = gelu(pre + bias), both bf16 [M, N], bias f32 [N].  h is computed from the bf16-rounded pre: bit-identical to
 * pswin_gemm_nt followed by pswin_bias_gelu_fwd, one pass over [M, N] less.  tile_m: 64 or 128. */
int pswin_gemm_nt_gelu_fwd(const void* x, const void* w, const float* bias, void* pre, void* h, long long M, int K, int N, int tile_m,
                           void* stream);
int pswin_gemm_nt_partial_rows(long long M, int tile_m);
int pswin_gemm_nt_gelu_bwd(const void* dy, const void* w_t, const void* pre, const float* bias, void* dpre, float* partial, long long M,
                           int K, int N, int tile_m, void* stream);
/* The three products above with SAMPLE LIVENESS (the Mlp under per-sample DropPath): rows are sample-major, sample b owns rows
 * [b * rows_per_sample, (b + 1) * rows_per_sample), M = B * rows_per_sample, B <= 64, rows_per_sample a multiple of the row tile;
 * sample_scale: the f32 [B] DropPath factor vector on the device, sample b is DEAD iff sample_scale[b] == 0.  The tiles of the live
 * samples are compacted into the first workgroups of the (unchanged) grid and computed as always; a dead sample's rows are neither read
 * nor multiplied: pswin_gemm_nt_live writes zeros to its rows of y, pswin_gemm_nt_gelu_bwd_live writes zero rows of `partial` and
 * leaves its rows of dpre UNWRITTEN, pswin_gemm_nt_gelu_fwd_live leaves its rows of pre and h UNWRITTEN -- whoever reads those must
 * skip the same rows.  sample_scale = NULL: the entry point without the suffix. */
int pswin_gemm_nt_live(const void* x, const void* w, const float* bias, void* y, long long M, int K, int N, int tile_m,
                       const float* sample_scale, int rows_per_sample, void* stream);
int pswin_gemm_nt_gelu_fwd_live(const void* x, const void* w, const float* bias, void* pre, void* h, long long M, int K, int N, int tile_m,
                                const float* sample_scale, int rows_per_sample, void* stream);
int pswin_gemm_nt_gelu_bwd_live(const void* dy, const void* w_t, const void* pre, const float* bias, void* dpre, float* partial, long long M,
                                int K, int N, int tile_m, const float* sample_scale, int rows_per_sample, void* stream);

/* Streaming GEMM for the Linear layers of the high-resolution stages (qkv / proj / fc1 / fc2 of stage 0, HOT:287, 309,
 * 50-58; proj of stage 1):  y[M, N] = x[M, K] . W^T (+ bias), bf16 in / out, f32 accumulation, the whole weight resident
 * in LDS.  transpose_w == 0: w is [N, K] (nn.Linear layout, forward pass); transpose_w != 0: w is [K, N], i.e. the
 * data gradient dx[M, K'] = dy[M, N'] . W with w = the same nn.Linear weight [N', K'] passed as K = N', N = K'.
 * bias: f32 [N] or NULL.  pswin_gemm_skinny_supported(K, N) != 0 for the (K, N) pairs the kernel is instantiated for. */
int pswin_gemm_skinny_supported(int K, int N);
int pswin_gemm_skinny(const void* x, const void* w, const float* bias, void* y, long long M, int K, int N, int transpose_w,
                      void* stream);

/* fc1 + bias + GELU of Mlp (HOT:50-57) fused into the streaming GEMM for the stage-0 shape (K = 96, N = 384):
 *   fwd: h[M, N] = gelu(x[M, K] . W^T + bias)                        -- the pre-activation is never stored
 *   bwd: dy = dh * gelu'(x . W^T + bias) with the pre-activation RECOMPUTED, dbias[n] = sum_m dy[m][n]
 * (dy is then the output gradient of the fc1 GEMM: dx = dy . W and dW = dy^T x follow as for any Linear).
 * x, w, h, dh, dy: bf16; bias, dbias: f32; workspace: f32, pswin_fc1_gelu_workspace(N) elements. */
int pswin_fc1_gelu_supported(int K, int N);
int pswin_fc1_gelu_fwd(const void* x, const void* w, const float* bias, void* h, long long M, int K, int N, void* stream);
int pswin_fc1_gelu_workspace(int N);
int pswin_fc1_gelu_partial_rows(long long M);                      /* rows of N sums left in workspace when dbias == NULL */
int pswin_fc1_gelu_bwd(const void* x, const void* w, const float* bias, const void* dh, void* dy, float* dbias,
                       float* workspace, long long M, int K, int N, void* stream);

/* Stage-0 Mlp backward, first half, as ONE pass (round 3): g = (dy . W2) * gelu'(x . W1^T + b1) -- fc2's data gradient (HOT:58), the
 * backward of nn.GELU (HOT:57) on the recomputed fc1 pre-activation (HOT:56) and the fc1 bias gradient's partial sums; dh = dy . W2
 * (201 MB per block at batch 8) is never written.  x, dy [M, C] bf16 rows; w1 = fc1.weight [hidden, C], w2 = fc2.weight [C, hidden]
 * bf16; b1 f32 [hidden] or NULL; g [M, hidden] bf16; workspace f32 [pswin_mlp0_bwd_partial_rows(M)][hidden] receives the
 * per-workgroup column sums of g; dbias1 f32 [hidden] their fixed-order sum, or NULL (partial rows only); workspace = NULL: no column
 * sums (a caller that runs fc1's weight gradient on pswin_gemm_tn_ring_bias gets them from that launch).  C = 96, hidden = 384. */
/* Stage-0 Mlp forward in one pass (HOT:50-58 without fc2's bias, which the caller adds with the residual): h[M, hidden] = gelu(x W1^T +
 * b1) is written once for the backward pass and y[M, C] = h W2^T is formed from the first product's accumulators (h is not read
 * back).  Same shapes and dtypes as pswin_mlp0_bwd; pswin_mlp0_bwd_supported(C, hidden) says whether both exist. */
int pswin_mlp0_fwd(const void* x, const void* w1, const float* b1, const void* w2, void* h, void* y, long long M, int C, int hidden, void* stream);
int pswin_mlp0_bwd_supported(int C, int hidden);
int pswin_mlp0_bwd_partial_rows(long long M);
int pswin_mlp0_bwd(const void* x, const void* w1, const float* b1, const void* dy, const void* w2, void* g, float* dbias1, float* workspace,
                   long long M, int C, int hidden, void* stream);

/* Column sums of a row-major [M, N] matrix in fp32: out[n] = sum_m x[m][n] (fixed summation order).  The bias
 * gradient of every Linear on the path (autograd of nn.Linear, HOT:50-52, 236, 323) and the reduction of split-K
 * weight-gradient partials.  N % 8 == 0; workspace: f32, pswin_colsum_workspace(M, N, dtype) elements. */
int pswin_colsum_workspace(long long M, int N, int dtype);
int pswin_colsum(const void* x, int dtype, long long M, int N, float* out, float* workspace, void* stream);
/* out == NULL: first stage only; pswin_colsum_workspace(M, N, dtype) / N partial rows of N sums stay in workspace. */
/* First stage only, for a matrix whose columns [skip_lo, skip_hi) are known to sum to zero: they are not read and their
 * partial sums are zeros.  Used for the qkv bias gradient (autograd of HOT:236, 287): the K third of d(qkv) sums to zero
 * over the window tokens analytically (dK = dS^T Q and every row of dS sums to 0 because softmax rows sum to 1), so a
 * third of the largest gradient tensor of each block is not re-read.  skip_lo, skip_hi: multiples of 8 (bf16) / 4 (f32). */
int pswin_colsum_skip(const void* x, int dtype, long long M, int N, int skip_lo, int skip_hi, float* workspace, void* stream);

/* Grouped column sums: dst[c] = sum_{r < rows} src[r * ld + c], c < cols, for up to a few hundred independent jobs in
 * ONE launch per 96 jobs (fixed summation order, bitwise reproducible).  The autograd of the path produces ~120 small
 * parameter-gradient reductions per backward pass (split-K partials of dW = dY^T X, bias-gradient partial rows, the
 * LayerNorm dgamma / dbeta rows; reference: torch autograd of HOT:50-58, 236, 323, 503, 512); none of them is needed
 * before the pass ends, so the host queues them and issues them here together.  `jobs` is a HOST array (it is copied
 * into the kernel arguments, so it may be freed on return and a captured hipGraph keeps its own copy).
 * src: f32 or bf16 (dtype), 16-byte aligned, ld % 8 == 0 (bf16) / % 4 == 0 (f32); cols likewise; dst: f32, aligned. */
typedef struct pswin_reduce_job {
    const void* src;
    float* dst;
    int dtype;
    int rows;
    int cols;
    int ld;
} pswin_reduce_job;
int pswin_reduce_jobs(const pswin_reduce_job* jobs, int n_jobs, void* stream);

/* Static 4-tap row interpolation (the two F.grid_sample calls of PitchAttentionModule.get_rotated,
 * HOT:1038, 1090, with input-independent grids; lzx/pano_rotate.py:169-187):
 * out[b][p][:] = sum_k wgt[p][k] * x[b][idx[p][k]][:]   x: [B, S, C] f32, out: [B, P, C] f32,
 * idx: int32 [P, 4], wgt: f32 [P, 4]. */
int pswin_interp_rows(const float* x, const int32_t* idx, const float* wgt, float* out, int B, int S, int P, int C,
                      void* stream);

/* Its adjoint (atomic f32 adds): dx[b][idx[p][k]][:] += wgt[p][k] * dout[b][p][:]; dx must be zeroed by the
 * caller. */
int pswin_interp_rows_adjoint(const float* dout, const int32_t* idx, const float* wgt, float* dx, int B, int S,
                              int P, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Window attention (the hot kernel): BasicWindowAttention.forward (HOT:274-311) between the qkv and
 * proj Linear layers, and PitchAttentionModule._attention (HOT:1206-1237) between q/k/v_linear and proj.
 * ---------------------------------------------------------------------------------------------- */

/* Score bias of window n, head h (BasicWindowAttention._sphere_bias, HOT:241-272, plus the shifted-window mask add
 * of HOT:295-303), evaluated inside the attention kernels once per (bias window, head) and shared by every image
 * of the batch (window n uses bias window n % n_bias_windows):
 *   bias(i,j) = (dist ? dist[wb % n_dist](i,j) * alpha[idx(i,j)][h] : 0) + beta[idx(i,j)][h]
 *               + (mask ? mask[wb % n_mask](i,j) : 0)
 *   idx(i,j)  = (i/7 - j/7 + 6) * 13 + (i%7 - j%7 + 6)         (make_relative_position_index, HOT:95-129)
 * dist / mask are passed as zero-padded 64 x 64 TILES (pswin_attn_pad_tiles): the forward kernel reads tile[i][j],
 * the backward kernel reads the TRANSPOSED tile[j][i] (for the symmetric self-attention tables both are the same
 * buffer).  alpha (ignored when dist is NULL: planar mode, HOT:257-258), beta: f32 [169, heads].
 * n_bias_windows must be a multiple of n_dist and of n_mask. */

/* [n, 49, 49] -> zero-padded [n, 64, 64] tiles, transposed when `transpose` != 0. */
int pswin_attn_pad_tiles(const float* src, int n, int transpose, float* dst, void* stream);

/* out[n][i][h*32 + d] = sum_j softmax_j(scale * q[n][i][h][:] . k[n][j][h][:] + bias(i, j)) v[n][j][h][d]
 * q, k, v: element pointers to head 0 of token 0 of window 0; token rows are ld_qkv elements apart, heads 32
 * elements apart (one fused [n*49, 3C] qkv buffer: q = base, k = base + C, v = base + 2C, ld_qkv = 3C).
 * out: [n_windows*49, ld_out]; lse: f32 [n_windows, heads, 64] = log-sum-exp of every score row (+inf in rows
 * >= 49), kept for the backward pass.  n_windows % n_bias_windows == 0.
 * n_chunks: how many work items share one bias window's batch loop (0 = pswin_attn_suggest_chunks; otherwise a
 * divisor of n_windows / n_bias_windows).
 * dtype: q, k, v, out all PSWIN_F32 (exact-f32 MFMA) or all PSWIN_BF16 (bf16 MFMA, f32 softmax/accumulate).
 * Pointers 16-byte aligned, ld_qkv % 8 == 0, ld_out % 8 == 0. */
int pswin_attn_fwd(const void* q, const void* k, const void* v, int ld_qkv, const float* dist_tiles, int n_dist,
                   const float* alpha, const float* beta, const float* mask_tiles, int n_mask, void* out, int ld_out,
                   float* lse, int n_chunks, int n_windows, int n_bias_windows, int heads, float scale, int dtype,
                   void* stream);

/* Host helper: the number of batch-loop chunks the library would pick for this geometry (enough independent
 * waves to fill the chip while keeping the per-work-item bias reuse long), for the forward (backward = 0) or the
 * backward (backward = 1) kernel.  Returns the chunk count (>= 1) or PSWIN_ERR_ARG. */
int pswin_attn_suggest_chunks(int n_windows, int n_bias_windows, int heads, int backward);

/* The whole WindowAttention module per window in ONE kernel (HOT:274-323: self.qkv, the attention core above, self.proj):
 *   y = softmax(scale * q k^T + bias) v @ Wproj^T   with [q | k | v] = x @ Wqkv^T + b_qkv,
 * x: [n_windows*49, C] window rows (the output of pswin_ln_gather_fwd), y: [n_windows*49, C] WITHOUT the proj bias (the
 * residual scatter kernel adds it, as on the unfused path).  The qkv tensor never exists in HBM: both weight matrices
 * are resident in LDS as MFMA operand fragments and every product of a window runs out of registers
 * (csrc/pswin_fused.hip).  w_qkv: [3C, C], w_proj: [C, C] (nn.Linear layout), b_qkv: f32 [3C] or NULL; dist / mask tiles,
 * tables, n_bias_windows and scale as pswin_attn_fwd (forward tiles, not transposed).
 * Training: pass qkv_out (bf16 [n, heads, 3, 49, 32]: q, k, v of a head as contiguous blocks, the packing pswin_attn_bwd_ex
 * reads), att_out [n*49, C] (the attention output before proj, row-major: the proj weight-gradient GEMM reads it) and
 * lse_out f32 [n, heads, 64] (all three or none).
 * Specialised for C = 96, heads = 3, PSWIN_BF16 (PanoSwin-T / -S stage 0); pswin_win_attn_fused_supported says so,
 * anything else returns PSWIN_ERR_UNSUPPORTED.  Rounding points are those of the unfused bf16 path (qkv and the attention
 * output rounded to bf16, f32 scores / softmax / accumulation). */
int pswin_win_attn_fused_supported(int C, int heads, int dtype);
int pswin_win_attn_fused_fwd(const void* x, const void* w_qkv, const float* b_qkv, const void* w_proj, const float* dist_tiles,
                             int n_dist, const float* alpha, const float* beta, const float* mask_tiles, int n_mask, void* y,
                             void* qkv_out, void* att_out, float* lse_out, long long n_windows, int n_bias_windows, int C,
                             int heads, float scale, int dtype, void* stream);

/* The same fusion WITHOUT the proj Linear for the stages behind the first one (csrc/pswin_qkvattn.hip, round 3): qkv Linear (HOT:287) +
 * attention core (HOT:288-308) of one (window, head) per wave, C = 192 (6 heads) or 384 (12); the head's 96 weight rows stay in LDS for
 * the lifetime of a workgroup.  y: attention output rows [n_windows * 49, C] (the input of the proj GEMM).  qkv_out / lse_out: both or
 * neither (training): q, k, v as packed [n][heads][3][49][32] blocks and the log-sum-exp rows [n][heads][64], what pswin_attn_bwd_ex
 * (ld_in 32, win_stride heads * 3 * 49 * 32, head_stride 3 * 49 * 32) reads.  Other arguments as pswin_win_attn_fused_fwd. */
int pswin_qkv_attn_fused_supported(int C, int heads, int dtype);
int pswin_qkv_attn_fused_fwd(const void* x, const void* w_qkv, const float* b_qkv, const float* dist_tiles, int n_dist, const float* alpha,
                             const float* beta, const float* mask_tiles, int n_mask, void* y, void* qkv_out, float* lse_out, long long n_windows,
                             int n_bias_windows, int C, int heads, float scale, int dtype, void* stream);

/* Gradients of pswin_attn_fwd.  dq, dk, dv use the q/k/v addressing (ld_dqkv), dout the out addressing.
 * dist_tiles_t / mask_tiles_t: the TRANSPOSED tiles.  n_chunks splits the batch loop (1 <= n_chunks <=
 * n_windows / n_bias_windows, must divide it).
 * dscore_sum: f32 [n_chunks * n_bias_windows, heads, 64(j), 64(i)] or NULL: per work item, the sum over its images
 * of dScore (= the gradient w.r.t. the bias), transposed like the backward tiles; input of pswin_attn_table_grads. */
int pswin_attn_bwd(const void* q, const void* k, const void* v, int ld_qkv, const float* dist_tiles_t, int n_dist,
                   const float* alpha, const float* beta, const float* mask_tiles_t, int n_mask, const void* dout,
                   int ld_out, const float* lse, void* dq, void* dk, void* dv, int ld_dqkv, float* dscore_sum,
                   int n_chunks, int n_windows, int n_bias_windows, int heads, float scale, int dtype, void* stream);
/* The same with q / k / v in any packing: window w, head h starts w * qkv_window_stride + h * qkv_head_stride elements behind the
 * q / k / v pointer, token rows ld_qkv elements apart.  pswin_win_attn_fused_fwd saves q, k, v as contiguous [49][32] blocks
 * ([n][heads][3][49][32]: ld_qkv = 32, head stride 3 * 49 * 32, window stride heads * 3 * 49 * 32; k = q + 49 * 32 elements,
 * v = q + 2 * 49 * 32), which it can write -- and this kernel read -- as whole 1 KB runs instead of 64-byte row segments. */
int pswin_attn_bwd_ex(const void* q, const void* k, const void* v, int ld_qkv, long long qkv_window_stride, int qkv_head_stride,
                      const float* dist_tiles_t, int n_dist, const float* alpha, const float* beta, const float* mask_tiles_t,
                      int n_mask, const void* dout, int ld_out, const float* lse, void* dq, void* dk, void* dv, int ld_dqkv,
                      float* dscore_sum, int n_chunks, int n_windows, int n_bias_windows, int heads, float scale, int dtype,
                      void* stream);


/* Table gradients (adjoint of the bias w.r.t. alpha, beta), in a fixed summation order:
 *   dbeta[t][h] = sum over tiles and (i,j) with idx(i,j) = t of g ;  dalpha[t][h] = the same sum of g * dist(i,j).
 * dscore_sum: the n_tiles = n_chunks * n_bias_windows tiles written by pswin_attn_bwd; dist_tiles_t as there (NULL in
 * planar mode: dalpha untouched); dalpha, dbeta: f32 [169, heads], overwritten.
 * workspace: f32, pswin_attn_table_grads_workspace(heads) elements. */
int pswin_attn_table_grads_workspace(int heads);
int pswin_attn_table_grads_partial_rows(int n_tiles, int heads);
int pswin_attn_table_grads(const float* dscore_sum, int n_tiles, int n_bias_windows, const float* dist_tiles_t,
                           int n_dist, int heads, float* dalpha, float* dbeta, float* workspace, void* stream);

/* The same for several attention modules at once.  stages: 1 = only the partial sums over the dScore tiles (best issued
 * right after pswin_attn_bwd while the tiles are still in the last-level cache), 2 = only the sum of those partials
 * and the per-bin sums (one binning launch for all jobs), 3 = both, 4 = only the per-bin sums: the caller has summed
 * the partial rows itself, e.g. as pswin_reduce_jobs jobs together with the other parameter-gradient reductions of
 * the backward pass.  Workspace layout for that: pswin_attn_table_grads_partial_rows(n_tiles, heads) rows of
 * ld = pswin_attn_table_grads_workspace(heads) / 129 floats from the start, their sum (ld floats) at offset 128 * ld.  `jobs` is a HOST array; it is copied into the kernel
 * arguments (32 jobs per launch).  Field meaning as the arguments of pswin_attn_table_grads. */
typedef struct pswin_table_grad_job {
    const float* dscore_sum;
    const float* dist_tiles_t;
    float* dalpha;
    float* dbeta;
    float* workspace;
    int n_tiles;
    int n_bias_windows;
    int n_dist;
    int heads;
} pswin_table_grad_job;
int pswin_attn_table_grads_batch(const pswin_table_grad_job* jobs, int n_jobs, int stages, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Panorama training augmentation (the image side of the PanoSwin data pipeline; the boxes stay on the host:
 * panoswintransformerobjectdetection_amd/pano_aug.py)
 * ---------------------------------------------------------------------------------------------- */

/* PanoStretch + RollAug + RandomFlip of mmdet/datasets/pipelines/transforms.py:992-1068 and the recipe's RandomFlip in one gather:
 *   dst[b][y][x][:] = S_b[y][xs][:],  xs = ((flip ? W-1-x : x) - shift) mod W,
 * S_b = the stretch of src[b] by (kx, ky) (lzx/yolo/extensions/xzaug.py getAug: float64 coordinates, order-1 map_coordinates with
 * scipy's 'wrap' boundary of period n-1, rounded half-up) or src[b] itself when the stretch is off.
 * params: f64 [B, 4] on the DEVICE, per image (kx, ky, shift, flags), flags bit 0 = stretch, bit 1 = flip; shift is taken modulo W
 * (a captured graph replays with whatever the buffer holds).  src, dst: uint8 [B, H, W, C], distinct; H >= 2, W even, 1 <= C <= 4. */
int pswin_pano_warp_u8(const uint8_t* src, const double* params, uint8_t* dst, int B, int H, int W, int C, void* stream);

/* Resize(keep_ratio) + Normalize + Pad + collate of the recipe, into the backbone's input:
 *   dst[b][c][y][x] = (u - norm[c]) * norm[3 + c] for y < out_hw[b][0], x < out_hw[b][1], else 0 (the pad, written here),
 *   u = floor(bilinear(src[b], channel to_rgb ? 2-c : c) + 0.5), the bilinear resize from H x W to out_hw[b] in float32 with
 *   src = (dst + 0.5) * (in / out) - 0.5 clamped at 0 and the last row / column replicated (cv2 INTER_LINEAR geometry).
 * src: uint8 [B, H, W, 3]; out_hw: int32 [B, 2] on the DEVICE (clamped to [0, Hp] x [0, Wp]); norm: f32 [6] on the device = the
 * mean and 1/std of each OUTPUT channel; dst: f32 [B, 3, Hp, Wp]. */
int pswin_pano_resize_normalize_pad(const uint8_t* src, const int32_t* out_hw, const float* norm, int to_rgb, float* dst, int B, int H,
                                    int W, int Hp, int Wp, void* stream);

/* The recipe's AutoAugment (configs/swin/faster_rcnn_panoswin_tiny_patch4_window7_mstrain_480800_adamw_1x_streetwin.py:65-89) with
 * Normalize + Pad + collate, in one launch without a scratch buffer: per image either policy 0, Resize (mmdet/datasets/pipelines/
 * transforms.py:212-242, 289-330), or policy 1, Resize -> RandomCrop (transforms.py:840-876, 960-975) -> Resize(override=True).
 * plan: int32 [B, 8] on the DEVICE, per image (h1, w1, cy, cx, ch, cw, oh, ow).  "resize" is the float32 resize of
 * pswin_pano_resize_normalize_pad, rounded half-up to uint8.
 *   h1 <= 0: dst[b] is what pswin_pano_resize_normalize_pad writes for out_hw[b] = (oh, ow), bit for bit;
 *   h1 >  0: I = resize(src[b], h1 x w1) as uint8, K = I[cy:cy+ch, cx:cx+cw], u = resize(K, oh x ow) -- the replicated border is the
 *            crop's border -- then (u - norm[c]) * norm[3 + c] with the channel swap of to_rgb, and 0 outside oh x ow up to Hp x Wp.
 * I and K are never stored: a workgroup computes the pixels of I its output tile reads into LDS, or, where the second resize shrinks
 * by more than about 2, each thread computes its own; both give the same bits.  The plan is clamped on the device (a captured graph
 * replays with whatever the buffer holds): oh, ow to [0, Hp] x [0, Wp], w1 to >= 1, cy to [0, h1-1], ch to [1, h1-cy], cx to
 * [0, w1-1], cw to [1, w1-cx].  src, norm, dst, to_rgb: as pswin_pano_resize_normalize_pad. */
int pswin_pano_resize_crop_resize_normalize_pad(const uint8_t* src, const int32_t* plan, const float* norm, int to_rgb, float* dst, int B,
                                                int H, int W, int Hp, int Wp, void* stream);

/* The instance masks of a batch through the geometry of the two launches above, into PaddedTargets.masks, in one launch:
 *   dst[b][r][y][x] = 0 for r >= count[b] (clamped to [0, Gmax]), for y >= oh and for x >= ow; otherwise
 *   dst[b][r][y][x] = max over k in {0, 1} with 0 <= a = rows[b][r][k] < Gin of Wm[b][a][sy][sx]    (no such k: 0), where
 *   nn(d, n_in, n_out) = min((int)floor(d * (1.0 / ((double)n_out / (double)n_in))), n_in - 1) in float64, uncontracted: the index rule
 *     of cv2.resize(INTER_NEAREST), which mmdet's BitmapMasks.rescale / resize reach through mmcv.imrescale(interpolation='nearest').
 *     PARITY: unpinned -- neither cv2 nor mmcv is at hand to compare with;
 *   h1 <= 0: sy = nn(y, H, oh), sx = nn(x, W, ow);
 *   h1 >  0: iy = cy + nn(y, ch, oh), ix = cx + nn(x, cw, ow), sy = nn(iy, H, h1), sx = nn(ix, W, w1);
 *   Wm[b][a] = the plane (src[b][a] != 0), values 0 / 1, through pswin_pano_warp_u8 with params[b] as a one-channel image: on such a
 *     plane the half-up rounding of the stretch's blend is "blend + 0.5 >= 1" and the result is again 0 / 1.  The reference has no
 *     mask path for PanoStretch and RollAug; the mask goes where the image goes, by the same expression.
 * rows[b][r] names the one or two source rows output row r came from (second entry -1: one source; RollAug's seam merge joins two):
 * pano_aug.py, "Row provenance".  Entries outside [0, Gin) read nothing.
 * src: uint8 [B, Gin, H, W]; params: f64 [B, 4] as pswin_pano_warp_u8; plan: int32 [B, 8] as
 * pswin_pano_resize_crop_resize_normalize_pad and clamped alike; rows: int32 [B, Gmax, 2]; count: int32 [B]; dst: uint8
 * [B, Gmax, Hp, Wp], distinct from src.  All on the DEVICE (a captured graph replays with whatever the buffers hold).  EVERY byte of dst
 * is written, by vector stores (16 bytes per lane where Wp % 16 == 0 and dst is 16-byte aligned, 4 where Wp % 4 == 0, bytes
 * otherwise): no memset, no atomics, no dependence on what dst held.  No intermediate mask is stored; the geometry of a pixel is worked
 * out once and reused for the Gmax rows, and without the stretch flag no trigonometric function runs.  H >= 2, W even, any positive
 * Hp, Wp; H * W and Hp * Wp below 2^31 (offsets inside a plane are 32-bit, plane bases 64-bit), B <= 65535, Hp <= 16 * 65535. */
int pswin_pano_masks(const uint8_t* src, const double* params, const int32_t* plan, const int32_t* rows, const int32_t* count, uint8_t* dst,
                     int B, int Gin, int Gmax, int H, int W, int Hp, int Wp, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Detector inference behind the heads (csrc/pswin_detect.hip; panoswintransformerobjectdetection_amd/detector.py:
 * multiclass_nms, paste_masks, MiniMaskRCNN.heads_predict)
 * ---------------------------------------------------------------------------------------------- */

/* Class-wise NMS of a batch (BBoxHead.get_bboxes -> multiclass_nms, mmdet/models/roi_heads/bbox_heads/bbox_head.py:270-371,
 * mmdet/core/post_processing/bbox_nms.py:7-93) in three calls with two stable sorts of the caller between them.  Limits, checked:
 * R <= 1024 proposals per image, C <= 128 classes, K <= 1024 detections per image.  Nothing is read back: the proposal count of an
 * image is read from device memory, every output entry is written by every call.
 *
 * (1) keys f32 [B][C][R]: softmax(cls[b][r])[c] over the C + 1 logits (background last) where it is > score_thr and r < roi_count[b],
 *     else -1.  cls: [B][R][C + 1], f32 or bf16.  The caller sorts keys along r, descending and STABLE (equal scores in ascending r). */
int pswin_multiclass_nms_scores(const void* cls, int cls_dtype, const int32_t* roi_count, int B, int R, int C, float score_thr, float* keys,
                                void* stream);
/* (2) sorted_keys f32 / sorted_index int64 [B][C][R]: the sorted keys and the r they came from (a permutation per list).  Decodes the
 *     candidates (detector.decode_deltas with stds, clipped to img_h x img_w, divided by scale[b] = (w, h, w, h) unless scale is NULL;
 *     rois f32 [B][R][4], deltas [B][R][4 C] f32 or bf16; stds: HOST array of 4 floats), runs the greedy rule of pswin_nms_groups on every (image, class) list and
 *     writes final_keys f32 [B][R * C]: the score of a surviving (r, c) at r * C + c, else -1.  The caller sorts final_keys along its
 *     row, descending and STABLE (equal scores in ascending r * C + c), and keeps the first min(K, R * C) columns.
 *     workspace: pswin_multiclass_nms_workspace(B, R, C) bytes, 16-byte aligned. */
int pswin_multiclass_nms_workspace(int B, int R, int C);
int pswin_multiclass_nms(const float* sorted_keys, const long long* sorted_index, const float* rois, const void* deltas, int deltas_dtype,
                         const float* stds, int img_h, int img_w, const float* scale, int B, int R, int C, float iou_thr, float* final_keys,
                         void* workspace, void* stream);
/* (3) top_keys f32 / top_index int64: the first n_sorted columns of that order, rows row_stride elements apart.  Writes boxes f32
 *     [B][K][4], scores f32 [B][K], labels int64 [B][K], source int32 [B][K] (r * C + c) and count int32 [B]; rows past count[b] are
 *     zeros.  rois ... scale: as in (2); the boxes are decoded again by the same function.  stds: HOST array of 4 floats. */
int pswin_multiclass_nms_select(const float* top_keys, const long long* top_index, long long row_stride, int n_sorted, const float* rois,
                                const void* deltas, int deltas_dtype, const float* stds, int img_h, int img_w, const float* scale, int B, int R,
                                int C, int K, float* boxes, float* scores, long long* labels, int32_t* source, int32_t* count, void* stream);

/* FCNMaskHead.get_seg_masks / _do_paste_mask(skip_empty=False) (mmdet/models/roi_heads/mask_heads/fcn_mask_head.py:169-377) for a batch:
 *   out[b][k][y][x] = bilinear(sigmoid(logits[b K + k][labels[b][k]]), grid_sample geometry of box[b][k], align_corners=False, zero
 *   padding) >= thr  for k < count[b], else 0.
 * logits: [B K][C][28][28], f32 or bf16, element strides given (NCHW or channels-last); labels int64 [B][K]; boxes f32 [B][K][4] in the
 * output image's pixels; count int32 [B] on the device; out uint8 [B][K][H][W], every byte written.  K <= 1024, C <= 128. */
int pswin_paste_masks(const void* logits, int dtype, long long stride_n, long long stride_c, long long stride_y, long long stride_x,
                      const long long* labels, const float* boxes, const int32_t* count, int B, int K, int C, int H, int W, float thr,
                      unsigned char* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Test-time augmentation behind the heads (csrc/pswin_augtest.hip; panoswintransformerobjectdetection_amd/tta.py:
 * map_to_view, map_back, merge_aug_proposals, merge_aug_bboxes, merge_aug_masks, aug_heads_predict)
 * ---------------------------------------------------------------------------------------------- */

#define PSWIN_AUG_VIEWS_MAX 8
#define PSWIN_AUG_MASK_SOURCES_MAX 24

/* The geometry of one test view, the same for every image of the batch: the unpadded size of the view's image, its scale factor
 * (w, h, w, h) and whether it is flipped horizontally.  HOST data: an entry point copies the views into its launches. */
typedef struct pswin_aug_view {
    int img_h, img_w;
    float scale[4];
    int flip;
} pswin_aug_view;

/* The mask heads' outputs that one paste merges: `count` <= 24 tensors [B K][C][28][28] of one dtype on the device, each with its own
 * element strides (NCHW or channels-last, as pswin_paste_masks takes them) and the flip flag of the view it was computed on.  HOST data. */
typedef struct pswin_aug_mask_sources {
    const void* logits[PSWIN_AUG_MASK_SOURCES_MAX];
    long long stride_n[PSWIN_AUG_MASK_SOURCES_MAX], stride_c[PSWIN_AUG_MASK_SOURCES_MAX], stride_y[PSWIN_AUG_MASK_SOURCES_MAX],
        stride_x[PSWIN_AUG_MASK_SOURCES_MAX];
    int flip[PSWIN_AUG_MASK_SOURCES_MAX];
    int count;
} pswin_aug_mask_sources;

/* merge_aug_proposals (mmdet/core/post_processing/merge_augs.py:12-80) for a batch: tta.merge_aug_proposals, bit for bit.
 *   props f32 [V][B][P][4] and scores f32 [V][B][P]: the proposals of every view in the view's pixels; count int32 [V][B] on the DEVICE:
 *   the first count[v][b] rows take part.  They are mapped back (un-flipped with the view's img_w, divided by its scale; float32,
 *   operation by operation), concatenated view-major, visited in the order of (descending score, ascending concatenated position), a
 *   candidate dropped when a kept one before it has IoU > iou_thr with it (the IoU of pswin_nms_groups), and the first
 *   Pm = min(max_per_img, V P) survivors written to rois f32 [B][Pm][4], out_scores f32 [B][Pm], out_count int32 [B]; rows past the
 *   count are zeros.  Three launches (pswin_aug_merge_proposals_launches), no atomics, nothing read back, every output row and every
 *   workspace word that is read written by the call.  V <= 8, V P <= 8192, B <= 65535; workspace: pswin_aug_merge_proposals_workspace
 *   bytes (the suppression masks: B * ceil64(V P)^2 / 8), 16-byte aligned.  NaN scores are outside the contract (the order is then
 *   unspecified; nothing is read out of bounds). */
int pswin_aug_merge_proposals_launches(int V, int P, int max_per_img);
int pswin_aug_merge_proposals_workspace(int V, int B, int P, int max_per_img);
int pswin_aug_merge_proposals(const float* props, const float* scores, const int32_t* count, const pswin_aug_view* views, int V, int B, int P,
                              float iou_thr, int max_per_img, float* rois, float* out_scores, int32_t* out_count, void* workspace, void* stream);

/* bbox_mapping (mmdet/core/bbox/transforms.py:34-43) of boxes f32 [B][N][4] into every view: out f32 [V][B][N][4] = box * scale, then
 * x0' = img_w - x2, x2' = img_w - x0 where the view is flipped.  One launch; float32, operation by operation. */
int pswin_aug_map_rois(const float* boxes, const pswin_aug_view* views, int V, int B, int N, float* out, void* stream);

/* merge_aug_bboxes (merge_augs.py:83-109) behind the box heads of V views: rois / cls / deltas are HOST arrays of V device pointers to
 * f32 [B][R][4], [B][R][C + 1] and [B][R][4 C] (cls and deltas f32 or bf16, read in place).  Per view softmax(cls) and
 * detector.decode_deltas(rois, deltas, stds) clipped to the view's img_h x img_w and mapped back as above; over the views summed in view
 * order and divided by V, in float32: boxes f32 [B][R][4 C], scores f32 [B][R][C + 1].  stds: HOST array of 4 floats.  One launch.
 * R <= 1024, C <= 128. */
int pswin_aug_merge_bboxes(const float* const* rois, const void* const* cls, const void* const* deltas, int cls_dtype, int deltas_dtype,
                           const float* stds, const pswin_aug_view* views, int V, int B, int R, int C, float* boxes, float* scores, void* stream);

/* The class-wise NMS chain above on GIVEN boxes and probabilities (merged_boxes f32 [B][R][4 C], scores f32 [B][R][C + 1]) instead of
 * logits and deltas: the same three calls with the same two sorts of the caller between them, the same rule (strict > score_thr, ties by
 * ascending r * C + c), the same outputs and limits; workspace: pswin_multiclass_nms_workspace(B, R, C). */
int pswin_multiclass_nms_scores_boxes(const float* scores, const int32_t* roi_count, int B, int R, int C, float score_thr, float* keys,
                                      void* stream);
int pswin_multiclass_nms_boxes(const float* sorted_keys, const long long* sorted_index, const float* merged_boxes, int B, int R, int C,
                               float iou_thr, float* final_keys, void* workspace, void* stream);
int pswin_multiclass_nms_select_boxes(const float* top_keys, const long long* top_index, long long row_stride, int n_sorted,
                                      const float* merged_boxes, int B, int R, int C, int K, float* boxes, float* scores, long long* labels,
                                      int32_t* source, int32_t* count, void* stream);

/* pswin_paste_masks whose pasted 28 x 28 probability is merge_aug_masks (merge_augs.py:120-150) of the sources: the mean, in source order
 * and float32, of sigmoid(logits_s[b K + k][labels[b][k]]) with the column index reversed where flip[s].  The mean lives in LDS only.
 * Everything else as pswin_paste_masks. */
int pswin_paste_masks_aug(const pswin_aug_mask_sources* sources, int dtype, const long long* labels, const float* boxes, const int32_t* count,
                          int B, int K, int C, int H, int W, float thr, unsigned char* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * COCO run-length encoding of instance masks (csrc/pswin_rle.hip; panoswintransformerobjectdetection_amd/rle.py states the
 * format: rle_encode, RleMasks, encode_masks, paste_masks_rle)
 * ---------------------------------------------------------------------------------------------- */

/* The runs of N masks of H x W pixels, each scanned column by column (linear position x H + y): mask n owns
 * runs[offsets[n] .. offsets[n + 1]), the lengths of its alternating runs starting with the run of zeros (0 when pixel 0 is set); they
 * sum to H W.  offsets int64 [N + 1] is always written whole and exact, offsets[N] being what the batch needs; runs uint32 [capacity]:
 * no index >= capacity is written, and a mask whose range lies below capacity is written whole.  With count (int32 [N / K] on the
 * device; may be NULL, K is then ignored) mask n = b K + k is read only when k < count[b] clamped to [0, K]; the others own no runs.
 * Four launches for any N and any data; no atomics; the contents are a function of the inputs alone.
 * Limits: H, W <= 65536, H W < 2^32, N < 2^31.  workspace: pswin_rle_workspace bytes, 16-byte aligned; every part of it is written
 * by a call before the call reads it.
 *
 * pswin_rle_encode: masks uint8 [N][H][W], a non-zero byte is foreground. */
int pswin_rle_workspace(long long N, int H, int W, long long* bytes);
int pswin_rle_encode(const unsigned char* masks, const int32_t* count, long long N, int K, int H, int W, long long* offsets, uint32_t* runs,
                     long long capacity, void* workspace, void* stream);

/* pswin_rle_encode of what pswin_paste_masks would write for the same arguments (N = B K), without the bitmap: the column bits come from
 * the paste's own sample, the same float32 expression compared with thr, so the runs are those of the bitmap route bit for bit. */
int pswin_paste_masks_rle(const void* logits, int dtype, long long stride_n, long long stride_c, long long stride_y, long long stride_x,
                          const long long* labels, const float* boxes, const int32_t* count, int B, int K, int C, int H, int W, float thr,
                          long long* offsets, uint32_t* runs, long long capacity, void* workspace, void* stream);

/* Intersections, areas and IoU of a padded batch's masks from their runs (csrc/pswin_rle_iou.hip; rle.py states the rule: rle_inter,
 * inter_pairs_definition): the counterpart of pycocotools' rleArea / rleIou, and of pswin_mask_inter_pairs / pswin_mask_iou_pairs below,
 * without bitmaps.  det_offsets int64 [B K + 1] / det_runs uint32 [det_capacity] and gt_offsets int64 [B G + 1] / gt_runs uint32
 * [gt_capacity] as pswin_rle_encode lays them out (masks of H x W pixels, mask b K + k the detection k of image b); labels int64 and
 * counts int32 as pswin_box_iou_pairs takes them.
 * pswin_rle_inter_pairs writes every element of inter int32 [B][K][G] and areas int32 [B][K + G] exactly as pswin_mask_inter_pairs
 * documents them; pswin_rle_iou_pairs stores what pswin_mask_iou_pairs stores: iou f32 [B][K][G] = float32(double(inter) / double(union)),
 * 0 when the union is 0, -1 outside the pairs, and the areas as f32 [B][K] and [B][G], 0 past a count.  One device code for both.
 * Overflow: a mask inside its count is whole when 0 <= offsets[n] <= offsets[n + 1] <= capacity; a mask that is not whole has area 0 and
 * intersection 0 in its pairs, and overflow[0] = 1 is stored (overflow int32 [1]: the caller clears it; nothing else is written to it).
 * No index >= capacity of runs is read, and every search stays inside the mask's own range, whatever the runs hold.
 * Two launches for any batch and any data (the tables of both sides; the pairs), no atomics, no host synchronisation: the results are a
 * function of the inputs alone.  A detection's tables of up to pswin_rle_inter_stage() entries are searched in LDS, longer ones in the
 * workspace.  Limits: H W < 2^31, 1 <= B <= 65535, K <= 1024, G <= 512 (pswin_coco_supported), 1 <= capacity <= 2^40, at most 2^31 - 1
 * runs per mask.  workspace: pswin_rle_inter_workspace bytes (8 bytes per unit of both capacities + 4 B (K + G)), 16-byte aligned; every
 * part of it is written by a call before the call reads it.  Anything else is PSWIN_ERR_ARG, checked before the device is touched. */
int pswin_rle_inter_stage(void);
int pswin_rle_inter_workspace(int B, int K, int G, long long det_capacity, long long gt_capacity, long long* bytes);
int pswin_rle_inter_pairs(const long long* det_offsets, const uint32_t* det_runs, long long det_capacity, const long long* det_labels,
                          const int* det_count, const long long* gt_offsets, const uint32_t* gt_runs, long long gt_capacity,
                          const long long* gt_labels, const int* gt_count, int B, int K, int G, int H, int W, int* inter, int* areas,
                          int* overflow, void* workspace, void* stream);
int pswin_rle_iou_pairs(const long long* det_offsets, const uint32_t* det_runs, long long det_capacity, const long long* det_labels,
                        const int* det_count, const long long* gt_offsets, const uint32_t* gt_runs, long long gt_capacity,
                        const long long* gt_labels, const int* gt_count, int B, int K, int G, int H, int W, float* iou, float* det_area,
                        float* gt_area, int* overflow, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Detector training between "assigned" and "loss" for a padded batch (csrc/pswin_targets.hip;
 * panoswintransformerobjectdetection_amd/detector.py: sample_ranks, rpn_targets, roi_targets, mask_targets)
 * ---------------------------------------------------------------------------------------------- */

/* RandomSampler with static shapes (detector.sample_ranks): for every image the first n_pos candidates of the positive order and the
 * first n_neg of the negative order.
 *   gt_inds int64 [B][N] (pswin_max_iou_assign's result), key f32 [B][N]: finite and >= 0
 *   composed key of candidate i in a list: key[i] if it is a member (positives: gt_inds > 0; negatives: gt_inds == 0), else
 *   key[i] + 2, or key[i] + 4 where gt_inds < 0 -- float32 additions
 *   pos_rank int64 [B][n_pos], neg_rank int64 [B][n_neg]: the candidates in ascending (composed key, index)
 * The order is that of the 64-bit value (bits of the composed key) << 32 | index, unique per candidate, taken through a reduction tree
 * of LDS sorts over chunks of pswin_sample_rows_per_workgroup() candidates: the result does not depend on the order of execution, no
 * atomics, nothing to clear between calls, a fixed number of launches for given (N, k).  A key outside the contract (negative, NaN)
 * leaves the order unspecified, but every index written lies in [0, N).
 * B >= 1, 1 <= n_pos, n_neg <= N, k = max(n_pos, n_neg) <= rows_per_workgroup / 2, B * N < 2^31; 8-byte aligned int64 arrays, 16-byte
 * aligned workspace of pswin_sample_workspace(B, N, k) bytes; anything else is PSWIN_ERR_ARG. */
int pswin_sample_rows_per_workgroup(void);                       /* candidates one workgroup sorts (the chunk of the tree) */
int pswin_sample_workspace(int B, int N, int k);                 /* bytes of workspace for pswin_sample_ranks, or PSWIN_ERR_ARG */
int pswin_sample_ranks(const long long* gt_inds, const float* key, int B, int N, int n_pos, int n_neg, long long* pos_rank, long long* neg_rank,
                       void* workspace, void* stream);

/* The RPN's sampled targets (detector.rpn_targets) from the ranks: pos_rank int64 [B][n_pos_max], neg_rank int64 [B][n_tot].
 *   anchors f32 [N][4] shared by the images, gt f32 [B][Gmax][4]
 *   idx int64 [B][n_pos_max + n_tot] = (pos_rank, neg_rank); valid f32 of that shape: 1 for a positive slot holding a positive and for
 *   a negative slot j < n_tot - (valid positives) holding a negative, else 0; pos_valid uint8 [B][n_pos_max];
 *   reg_t f32 [B][n_pos_max][4] = detector.encode_deltas(anchor, gt[gt_inds - 1], stds 1) in a valid positive slot, zeros elsewhere.
 * Ranks are clamped to [0, N) and gt rows to [0, Gmax) on the device.  1 <= Gmax <= 256, 1 <= n_pos_max <= n_tot <= N,
 * n_tot <= rows_per_workgroup / 2; 16-byte aligned anchors / gt / reg_t; anything else is PSWIN_ERR_ARG. */
int pswin_rpn_targets(const long long* gt_inds, const long long* pos_rank, const long long* neg_rank, const float* anchors, const float* gt, int B,
                      int N, int Gmax, int n_pos_max, int n_tot, long long* idx, float* valid, unsigned char* pos_valid, float* reg_t,
                      void* stream);

/* The RoI head's sampled RoIs and targets (detector.roi_targets) from the ranks: pos_rank int64 [B][n_pos_max], neg_order int64
 * [B][n_tot] (the first n_tot of the negative order).
 *   cand f32 [B][N][4], gt f32 [B][Gmax][4], gt_labels int64 [B][Gmax], stds: HOST array of 4 positive floats
 *   rois f32 [B][n_tot][4]: cand[pos_rank], then cand[neg_order[j + filler]] with filler = n_pos_max - (valid positives);
 *   labels int64 [B][n_tot]: the matched gt's label in a valid positive slot, num_classes elsewhere; pos_valid uint8 [B][n_pos_max];
 *   gt_idx int64 [B][n_pos_max] = max(gt_inds - 1, 0) of the slot; reg_t f32 [B][n_pos_max][4] = encode_deltas(roi, gt[gt_idx], stds)
 *   in a valid slot, zeros elsewhere.
 * Limits as pswin_rpn_targets; 16-byte aligned cand / gt / rois / reg_t. */
int pswin_roi_targets(const long long* gt_inds, const long long* pos_rank, const long long* neg_order, const float* cand, const float* gt,
                      const long long* gt_labels, int B, int N, int Gmax, int n_pos_max, int n_tot, int num_classes, const float* stds,
                      float* rois, long long* labels, float* reg_t, unsigned char* pos_valid, long long* gt_idx, void* stream);

/* The mask head's targets (detector.mask_targets): out f32 [B P][size][size], 1 where the bilinear sample (grid_sample geometry,
 * align_corners=False, zero padding) of the bitmap masks[b][gt_idx[b][p]] at point (i, j) of RoI p -- ((j + 0.5) / size along x,
 * (i + 0.5) / size along y) -- is >= 0.5, else 0; rows whose pos_valid is 0 are zeros and read nothing.
 *   masks uint8 [B][Gmax][H][W], rois f32 [B][P][4] in image pixels, gt_idx int64 [B][P] (clamped to [0, Gmax) on the device),
 *   pos_valid uint8 [B][P].  Nothing outside [0, H) x [0, W) of the one plane is read.
 * 1 <= Gmax <= 256, 1 <= size <= 64, H * W < 2^31, B * P < 2^31, 16-byte aligned rois; anything else is PSWIN_ERR_ARG. */
int pswin_mask_targets(const unsigned char* masks, const float* rois, const long long* gt_idx, const unsigned char* pos_valid, int B, int P,
                       int Gmax, int H, int W, int size, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The RPN's proposals of a batch (csrc/pswin_proposals.hip; panoswintransformerobjectdetection_amd/detector.py:
 * proposals_batch, the stacked MiniMaskRCNN._proposals)
 * ---------------------------------------------------------------------------------------------- */

/* RPNHead.get_bboxes for a whole batch (detector.proposals_batch):
 *   scores f32 [B][A] raw logits of either sign, deltas f32 [B][A][4], anchors f32 [A][4] shared by the images; the A anchors are the L
 *   pyramid levels one after the other, level_sizes: HOST array of their L sizes n_l.
 *   Per (image, level): the first k_l = min(nms_pre, n_l) candidates in descending score, equal scores (+0.0 and -0.0 are equal) in
 *   ascending anchor index; decoded as detector.decode_deltas(anchor, delta, stds 1, (img_h, img_w)) in float32 operation by operation
 *   (only expf may differ from the host); the greedy rule of pswin_nms_groups on all B L lists in one call.  Per image the candidates of
 *   all levels are concatenated level-major in rank order, a suppressed one's score becomes -1e4, and the first
 *   P = min(max_per_img, sum_l k_l) in descending score, equal scores in ascending concatenated position, are the result:
 *   rois f32 [B][P][4], out_scores f32 [B][P], count int32 [B] (the rows whose score is > -1e4: the survivors, which lead).
 * The orders are those of 64-bit values (order bits of the score) << 32 | index, unique per candidate, taken through reduction trees of
 * LDS sorts over chunks of pswin_rpn_proposals_rows_per_workgroup() candidates: the result does not depend on the order of execution.  No
 * atomics, no host synchronisation, nothing to clear between calls: everything the call reads from the workspace it has written before.
 * pswin_rpn_proposals_launches(level_sizes, L, nms_pre, max_per_img) kernel launches, whatever B.  NaN scores and scores <= -1e4 leave the
 * order unspecified, but every index used lies in range.
 * Limits: 1 <= L <= 8, n_l >= 1, 1 <= nms_pre <= 2048, max_per_img >= 1 and P <= 2048, B L <= 2048, B A < 2^31; 16-byte aligned deltas /
 * anchors / rois and workspace of pswin_rpn_proposals_workspace(level_sizes, L, B, nms_pre, max_per_img) bytes (PSWIN_ERR_ARG beyond
 * the limits or 2^31 - 1 bytes); anything else is PSWIN_ERR_ARG. */
int pswin_rpn_proposals_rows_per_workgroup(void);                /* candidates one workgroup sorts (the chunk of the trees) */
int pswin_rpn_proposals_launches(const int* level_sizes, int L, int nms_pre, int max_per_img);
int pswin_rpn_proposals_workspace(const int* level_sizes, int L, int B, int nms_pre, int max_per_img);
int pswin_rpn_proposals(const float* scores, const float* deltas, const float* anchors, const int* level_sizes, int L, int B, int nms_pre,
                        float iou_thr, int max_per_img, int img_h, int img_w, float* rois, float* out_scores, int32_t* count, void* workspace,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cascade R-CNN: stage refinement and the GIoU loss on decoded boxes (csrc/pswin_cascade.hip;
 * panoswintransformerobjectdetection_amd/cascade.py: refine_rois, giou_rows)
 * ---------------------------------------------------------------------------------------------- */

int pswin_cascade_rows_per_workgroup(void);                      /* rows one workgroup of the three kernels below takes */

/* BBoxHead.regress_by_class for a batch in one launch (cascade.refine_rois): the class of every RoI, the RoI regressed by that class's
 * deltas and clipped to the image.
 *   rois f32 [B][R][4]; cls [B][R][C + 1] and deltas [B][R][4 C], each f32 or bf16 and read in place; labels int64 [B][R] or NULL;
 *   stds: HOST array of 4 positive floats
 *   used int64 [B][R]: labels where labels < C (negative labels count as 0), else the FIRST maximum of cls[..][0 .. C) (a NaN counts as
 *   the maximum): torch.argmax's answer on the same values, ties included.  labels = NULL: every row takes the argmax.
 *   new_rois f32 [B][R][4] = detector.decode_deltas(roi, the four deltas of used, stds, (img_h, img_w)), evaluated in double and rounded
 *   once.
 * 1 <= C <= 128, B R 4 C < 2^31; 16-byte aligned rois / new_rois, deltas aligned to four of its elements; anything else is PSWIN_ERR_ARG. */
int pswin_cascade_refine(const float* rois, const void* cls, int cls_dtype, const void* deltas, int deltas_dtype, const long long* labels, int B,
                         int R, int C, const float* stds, int img_h, int img_w, float* new_rois, long long* used, void* stream);

/* GIoULoss on decoded boxes, row by row (cascade.giou_rows): out f32 [N] = weight * (1 - GIoU(box, target)) with
 *   box = the decode of rois f32 [N][4] by the four deltas of class labels[n] (clamped to [0, C)) of deltas [N][4 C] (f32 or bf16, read in
 *   place) with stds (HOST array of 4 positive floats), dw / dh clamped to +-|log(16 / 1000)|, NOT clipped to an image;
 *   GIoU as mmdet's bbox_overlaps(mode='giou', is_aligned=True) orders its operations, union and enclosing area each max(., eps);
 *   evaluated in double and rounded once.  A row whose weight is 0 reads nothing else and gives 0.
 * pswin_giou_rows_bwd recomputes the forward from the same inputs and writes EVERY element of grad_deltas [N][4 C] (the dtype of deltas,
 * bf16 rounded to nearest even): grad_rows[n] * d out[n] / d deltas in the four columns of the label's class of a row whose weight is
 * not 0, zeros everywhere else -- plain stores, no memset, no atomics.  Gradients of max / min / clamp as torch has them: half to each
 * side on a tie of max / min, passed on a clamp's bounds.
 * N >= 1, 1 <= C <= 128, N 4 C < 2^31, eps > 0; 16-byte aligned rois / target, deltas and grad_deltas aligned to four of their elements;
 * anything else is PSWIN_ERR_ARG. */
int pswin_giou_rows_fwd(const float* rois, const void* deltas, int deltas_dtype, const long long* labels, const float* weight, const float* target,
                        int N, int C, const float* stds, double eps, float* out, void* stream);
int pswin_giou_rows_bwd(const float* rois, const void* deltas, int deltas_dtype, const long long* labels, const float* weight, const float* target,
                        const float* grad_rows, int N, int C, const float* stds, double eps, void* grad_deltas, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The detector's training losses, row by row (csrc/pswin_losses.hip; panoswintransformerobjectdetection_amd/losses.py:
 * ce_rows, l1_rows, mask_bce_rows, rpn_losses)
 * ---------------------------------------------------------------------------------------------- */

/* Common to the eight entry points below: the heads' outputs are read in place as f32 or bf16; every value is evaluated in double and
 * rounded once; every sum has a fixed order, so two calls on the same inputs return the same bits; a backward recomputes its forward from
 * the same inputs (the mask loss: from the label's channel the forward left) and writes EVERY element of its gradient (the dtype of the prediction, bf16 rounded to nearest even) by plain stores --
 * no memset, no atomics, no workspace, no host synchronisation.  Arguments are checked before the device is touched. */
int pswin_losses_rows_per_workgroup(void);                       /* rows one workgroup of the ce_rows / l1_rows kernels takes */
int pswin_rpn_losses_chunk(void);                                /* anchors one workgroup of pswin_rpn_losses_bwd owns */

/* Softmax cross-entropy per row (losses.ce_rows): out f32 [N] = logsumexp(cls[n]) - cls[n][labels[n]] over the C + 1 logits of cls
 * [N][C + 1], the row's maximum subtracted first.  A label outside [0, C] gives 0 and an all-zero gradient row; nothing outside the row is
 * read.  grad [N][C + 1] = (softmax - onehot) * grad_rows[n].
 * N >= 1, 1 <= C <= 128, N (C + 1) < 2^31; anything else is PSWIN_ERR_ARG. */
int pswin_ce_rows_fwd(const void* cls, int dtype, const long long* labels, int N, int C, float* out, void* stream);
int pswin_ce_rows_bwd(const void* cls, int dtype, const long long* labels, const float* grad_rows, int N, int C, void* grad, void* stream);

/* Class-selected L1 per row (losses.l1_rows): out f32 [N] = weight[n] * sum_4 |reg[n][4 lab .. 4 lab + 4) - target[n]| with lab =
 * labels[n] clamped to [0, C); reg [N][4 C], target f32 [N][4].  A row whose weight is 0 reads nothing else and gives 0.
 * grad [N][4 C]: sign(reg - target) * fl(weight * grad_rows[n]) (float32 product, sign(0) = 0) in the label's four columns of a row whose
 * weight is not 0, zeros everywhere else.
 * N >= 1, 1 <= C <= 128, N 4 C < 2^31; 16-byte aligned target, reg and grad aligned to four of their elements; else PSWIN_ERR_ARG. */
int pswin_l1_rows_fwd(const void* reg, int dtype, const long long* labels, const float* weight, const float* target, int N, int C, float* out,
                      void* stream);
int pswin_l1_rows_bwd(const void* reg, int dtype, const long long* labels, const float* weight, const float* target, const float* grad_rows, int N,
                      int C, void* grad, void* stream);

/* BCE-with-logits on the label's channel (losses.mask_bce_rows): out f32 [M] = weight[m] * mean over the S x S map of
 * max(x, 0) - x t + log1p(exp(-|x|)), x = logits[m][lab][y][x] (lab = labels[m] clamped to [0, C)), t = target[m][y][x] (f32 [M][S][S]).
 * logits: [M][C][S][S] with element strides given, as pswin_paste_masks takes them; only the label's channel is read.  A row whose weight
 * is 0 reads nothing else and gives 0.  picked (may be NULL): f32 [M][S][S], the label's channel as it was read (zeros in a weight-0 row)
 * -- all the backward needs of the logits, 1 / C of their size: the caller need not keep them between the passes.
 * pswin_mask_bce_rows_bwd takes `picked` and writes grad [M][C][S][S] in `dtype` with the element strides given, which must be one of the
 * two dense layouts (NCHW: S S, S, 1 or channels-last: 1, S C, C; stride_n = C S S): (sigmoid(x) - t) * weight * grad_rows[m] / S^2 in the
 * label's channel, zeros in every other channel; walked in memory order, 16 bytes per lane where C S S is a multiple of the group and the
 * buffer is 16-byte aligned.
 * M >= 1, 1 <= C <= 128, 1 <= S <= 56, M C S S < 2^31; anything else is PSWIN_ERR_ARG. */
int pswin_mask_bce_rows_fwd(const void* logits, int dtype, long long stride_n, long long stride_c, long long stride_y, long long stride_x,
                            const long long* labels, const float* target, const float* weight, int M, int C, int S, float* out, float* picked,
                            void* stream);
int pswin_mask_bce_rows_bwd(const float* picked, int dtype, long long stride_n, long long stride_c, long long stride_y, long long stride_x,
                            const long long* labels, const float* target, const float* weight, const float* grad_rows, int M, int C, int S,
                            void* grad, void* stream);

/* The RPN's two losses per image (losses.rpn_losses) on what pswin_rpn_targets returns: cls_all f32 [B][A], reg_all f32 [B][A][4], idx
 * int64 [B][S], valid f32 [B][S], pos_valid uint8 [B][P], reg_t f32 [B][P][4], P <= S.
 *   out[b][0] = sum_s valid * BCE(cls_all[b][idx[b][s]], s < P ? 1 : 0) / avg_b
 *   out[b][1] = sum_{p < P} pos_valid * sum_4 |reg_all[b][idx[b][p]] - reg_t[b][p]| / avg_b,   avg_b = max(sum_s valid, 1)
 * A slot whose valid (pos_valid for the second loss) is 0 or whose index is outside [0, A) is skipped: nothing is read for it and it does
 * not count in avg_b.  CONTRACT: the counted slots of an image name distinct anchors (sample_ranks gives that).
 * pswin_rpn_losses_bwd takes grad_out f32 [B][2] and writes every element of grad_cls f32 [B][A] and grad_reg f32 [B][A][4]: the counted
 * slots' values at their anchors, zeros everywhere else (a skipped slot never overwrites a counted one's anchor).
 * 1 <= B <= 65535, A >= 1, 1 <= P <= S, B A 4 < 2^31; 16-byte aligned reg_all / reg_t / grad_reg; anything else is PSWIN_ERR_ARG. */
int pswin_rpn_losses_fwd(const float* cls_all, const float* reg_all, const long long* idx, const float* valid, const unsigned char* pos_valid,
                         const float* reg_t, int B, int A, int S, int P, float* out, void* stream);
int pswin_rpn_losses_bwd(const float* cls_all, const float* reg_all, const long long* idx, const float* valid, const unsigned char* pos_valid,
                         const float* reg_t, const float* grad_out, int B, int A, int S, int P, float* grad_cls, float* grad_reg, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mean average precision of a padded batch's detections (csrc/pswin_eval.hip; panoswintransformerobjectdetection_amd/evaluation.py:
 * box_iou_pairs, mask_iou_pairs, match_pairs, average_precision_sorted, MapAccumulator)
 * ---------------------------------------------------------------------------------------------- */

/* Common to the entry points below: a batch is a Detections (boxes f32 [B][K][4], scores f32 [B][K], labels int64 [B][K], count int32 [B])
 * and a PaddedTargets (boxes f32 [B][G][4], labels int64 [B][G], count int32 [B]), read in place with both counts from the device; no host
 * synchronisation, no data-dependent shape, every output element written by plain stores (the ground-truth histogram: integer atomic
 * adds, whose result has no order).  1 <= B <= 65535, 1 <= K <= 1024, G >= 1, B K G < 2^31; anything else is PSWIN_ERR_ARG, checked
 * before the device is touched. */
int pswin_ap_segments_chunk(void);                               /* records one workgroup of pswin_ap_segments takes per trip */

/* iou f32 [B][K][G]: bbox_overlaps' float32 expression, overlap / max(area_d + area_g - overlap, 1e-6) in that order of operations, for
 * the pairs with k < det_count[b], g < gt_count[b] and equal labels; -1 for every other pair.  det_area f32 [B][K] and gt_area f32 [B][G]
 * (either may be NULL): (x2 - x1) (y2 - y1) in float32 of EVERY row.  16-byte aligned boxes. */
int pswin_box_iou_pairs(const float* det_boxes, const long long* det_labels, const int* det_count, const float* gt_boxes,
                        const long long* gt_labels, const int* gt_count, int B, int K, int G, float* iou, float* det_area, float* gt_area,
                        void* stream);

/* The same for bitmaps: det_masks uint8 [B][K][H][W], gt_masks uint8 [B][G][H][W], a pixel counts where its byte is not zero.
 * iou = float(double(inter) / double(area_d + area_g - inter)), 0 when the union is 0, for the pairs as above, -1 elsewhere; det_area /
 * gt_area (required): the pixel counts as f32, 0 for a row past its count.  Areas are counted once per counted mask and intersections only
 * for the pairs as above: H W bytes per counted mask plus 2 H W per pair are read, nothing else of the masks.  workspace:
 * pswin_mask_iou_workspace(B, K, G) bytes.  H W must be a multiple of 16 (16-byte loads) and the masks 16-byte aligned. */
int pswin_mask_iou_workspace(int B, int K, int G);
int pswin_mask_iou_pairs(const unsigned char* det_masks, const long long* det_labels, const int* det_count, const unsigned char* gt_masks,
                         const long long* gt_labels, const int* gt_count, int B, int K, int G, int H, int W, float* iou, float* det_area,
                         float* gt_area, void* workspace, void* stream);

/* tpfp_default for a batch (evaluation.match_pairs).  iou as above (a negative entry is no candidate); ignore uint8 [B][G] or NULL;
 * iou_thrs: T floats in (0, 1] and area_ranges: S pairs (min_area, max_area) or NULL with S = 1, both HOST arrays read during the call;
 * T <= 16, S <= 8.  marks uint8 [T][S][B][K]: 0 ignored or past the count, 1 true positive, 2 false positive.  A detection can only
 * match the box of its best IoU (ties: regular before ignored, then the lower index); below the threshold it is a false positive if its
 * own area is in the range; on an ignored box or one outside the range it is ignored; else it is a true positive exactly when no
 * detection in front of it in (descending score, ascending row) chose the same box with an IoU at or above the threshold.
 * The accumulator: image b goes to slot cursor[0] + b (cursor: device int32, read only).  rec_score f32 / rec_label int32 [capacity][K]
 * (label C for a row past the count or outside [0, C)) and rec_marks uint8 [T][S][capacity][K] get the slot's rows; num_gts int32 [S][C]
 * gains the image's regular boxes per (range, class).  A slot outside [0, capacity) writes nothing but overflow[0] = 1. */
int pswin_eval_match(const float* iou, const float* det_scores, const long long* det_labels, const int* det_count, const long long* gt_labels,
                     const int* gt_count, const unsigned char* ignore, const float* det_area, const float* gt_area, const float* iou_thrs, int T,
                     const float* area_ranges, int S, int B, int K, int G, int C, int capacity, const int* cursor, unsigned char* marks,
                     float* rec_score, int* rec_label, unsigned char* rec_marks, int* num_gts, int* overflow, void* stream);

/* average_precision(mode='area') per (threshold, range, class): marks_sorted uint8 [T S][N], the records' marks in the order (class,
 * descending score); bounds int32 [C + 1], class c owning records bounds[c] .. bounds[c + 1] - 1; num_gts int32 [S][C] -> ap f32 [T][S][C].
 * Integer counts, precision float32(tp / max(tp + fp, eps)), recall and the sum in double in a fixed order; 0 where num_gts is 0.
 * N <= 2^24 (the counts stay exact in float32). */
int pswin_ap_segments(const unsigned char* marks_sorted, const int* bounds, const int* num_gts, int T, int S, int C, long long N, float* ap,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Proposal recall of a padded batch (csrc/pswin_recall.hip; evaluation.py: proposal_round_ious, recall_hits, RecallAccumulator)
 * ---------------------------------------------------------------------------------------------- */

/* The reference's eval_recalls on a Proposals (prop_boxes f32 [B][R][4], prop_count int32 [B]) and a PaddedTargets (gt_boxes f32 [B][G][4],
 * gt_count int32 [B]; ignore uint8 [B][G] or NULL), read in place with both counts from the device, clamped into [0, R] / [0, G]; rows past
 * a count are never read.  proposal_nums: Kn ints >= 1 and iou_thrs: T DOUBLES in (0, 1], both HOST arrays read during the call.
 * Per (k, image): the rows are the image's boxes inside its count that are not ignored, the columns its first min(count, proposal_nums[k])
 * proposals; the IoU is bbox_overlaps' float32 expression (pswin_box_iou_pairs').  Round j takes the largest IoU among the live rows and
 * columns (ties: the lowest row, inside it the lowest column), stores it in rounds[k][b][j] and deletes that row and that column; rounds
 * after the columns ran out store -1, an image without columns stores 0 in all its rounds, slots past the number of rows hold -2.
 * Every element of rounds f32 [Kn][B][G] is written by plain stores.  hits int64 [Kn][T] GAINS the number of rounds with double(value) >=
 * iou_thrs[t], num_gts int64 [1] the number of rows of the batch (integer atomic adds: no order); the caller clears both.
 * One workgroup per (k, image), one launch, no host synchronisation.  1 <= B <= 65535, 1 <= R <= 2048, 1 <= G <= 512, 1 <= Kn <= 8,
 * 1 <= T <= 16, 16-byte aligned boxes, 8-byte aligned hits / num_gts; anything else is PSWIN_ERR_ARG, checked before the device is touched. */
int pswin_recall_match(const float* prop_boxes, const int* prop_count, const float* gt_boxes, const int* gt_count,
                       const unsigned char* ignore, const int* proposal_nums, int Kn, const double* iou_thrs, int T, int B, int R, int G,
                       float* rounds, long long* hits, long long* num_gts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The COCO protocol: bbox / segm mAP and AR of a padded batch (csrc/pswin_coco.hip, csrc/pswin_eval.hip; evaluation.py: coco_pair_iou,
 * coco_match, coco_accumulate, CocoAccumulator).  Built from the published algorithm; the rules are evaluation.py's docstring.
 * ---------------------------------------------------------------------------------------------- */

/* The integer parts of the bitmaps' IoU, for pswin_coco_match: inter int32 [B][K][G], the number of pixels that are non-zero in both
 * masks for the pairs with k < det_count[b], g < gt_count[b] and equal labels, -1 for every other pair; areas int32 [B][K + G], the
 * pixel counts of image b's detections (first K) and boxes (last G), 0 past a count.  Shares its device code with pswin_mask_iou_pairs,
 * and reads what that reads.  Any H, W >= 1: a size that is no multiple of 16 bytes (or masks that are not 16-byte aligned) is read
 * byte by byte.  Shapes as pswin_box_iou_pairs. */
int pswin_mask_inter_pairs(const unsigned char* det_masks, const long long* det_labels, const int* det_count, const unsigned char* gt_masks,
                           const long long* gt_labels, const int* gt_count, int B, int K, int G, int H, int W, int* inter, int* areas,
                           void* stream);

/* 1 if pswin_coco_match / pswin_coco_accumulate take the shape: 1 <= B <= 65535, 1 <= K <= 1024, 1 <= G <= 512 (an image's detections and
 * boxes stay in one workgroup's LDS, a lane keeps the "taken" bits of its G / 64 columns in a register), 1 <= T <= 16, 1 <= A <= 8,
 * 1 <= M <= 4; else 0. */
int pswin_coco_supported(int B, int K, int G, int T, int A, int M);
int pswin_coco_accumulate_chunk(void);                           /* records one workgroup of pswin_coco_accumulate takes per trip */

/* COCOeval's evaluateImg for a batch, ONE launch: a workgroup per (image, range), a wavefront per threshold.  The batch as above, with
 * crowd uint8 [B][G] or NULL and gt_area f64 [B][G] or NULL (the annotations' area field; NULL: the box's w h in double, or the mask's
 * pixel count).  mask_inter / mask_areas: both NULL for boxes (IoU of the boxes as x, y, w, h in double), or pswin_mask_inter_pairs'
 * results (then det_boxes and gt_boxes are not read and may be NULL).  iou_thrs: T doubles in (0, 1], compared as min(t, 1 - 1e-10);
 * area_ranges: A pairs (lo, hi) of doubles, closed; both HOST arrays read during the call.
 * A box is ignored in range a if it is crowd or its area is < lo or > hi.  The detections of an image are taken in (descending score
 * bits, ascending row); a detection's rank is its position among those of its class.  Each takes, among the boxes of its class with
 * IoU >= threshold that are unmatched or crowd, the greatest under (not ignored before ignored, higher IoU, higher index); a matched box
 * that is not crowd is taken for the rest.  flags uint8 [T][A][B][K]: bit 0 matched, bit 1 ignored (matched: its box is ignored;
 * unmatched: its own area is outside the range); 0 for a row past the count or with a label outside [0, C).
 * The accumulator: image b goes to slot cursor[0] + b.  rec_score f32 / rec_label int32 (C for "no record") / rec_rank uint16
 * [capacity][K] and rec_flags uint8 [T][A][capacity][K] get the slot's rows, every byte of them; num_gts int32 [A][C] gains the image's
 * boxes that are not ignored (integer atomic adds).  A slot outside [0, capacity) writes nothing but overflow[0] = 1.
 * Shapes inside pswin_coco_supported, C <= 65535, 16-byte aligned boxes; anything else is PSWIN_ERR_ARG, checked before the device is
 * touched. */
int pswin_coco_match(const float* det_boxes, const float* det_scores, const long long* det_labels, const int* det_count, const float* gt_boxes,
                     const long long* gt_labels, const int* gt_count, const unsigned char* crowd, const double* gt_area, const int* mask_inter,
                     const int* mask_areas, const double* iou_thrs, int T, const double* area_ranges, int A, int B, int K, int G, int C,
                     int capacity, const int* cursor, unsigned char* flags, float* rec_score, int* rec_label, unsigned short* rec_rank,
                     unsigned char* rec_flags, int* num_gts, int* overflow, void* stream);

/* COCOeval's accumulate: flags_sorted uint8 [T A][N] and rank_sorted uint16 [N], the records in the order (class, descending score,
 * slot, row); bounds int32 [C + 1]; num_gts int32 [A][C]; max_dets: M ascending ints >= 1 and rec_thrs: R <= 128 ascending doubles in
 * [0, 1], both HOST arrays read during the call.  Per (t, class, a, m) over the records with rank < max_dets[m]: tp / fp the cumulative
 * counts of (matched, not ignored) / (unmatched, not ignored); recall = tp / num_gts and precision = tp / (fp + tp + 2.220446049250313e-16)
 * in double; precision made non-increasing from the right; precision f64 [T][R][C][A][M] gets, per threshold r, the precision at the
 * first record with recall >= r, or 0; recall f64 [T][C][A][M] the last recall (0 without records).  Every entry of a (class, a) with
 * num_gts == 0 is -1.  One workgroup per (t, a, m, class); every operation's order is fixed.  N <= 2^24. */
int pswin_coco_accumulate(const unsigned char* flags_sorted, const unsigned short* rank_sorted, const int* bounds, const int* num_gts,
                          const int* max_dets, int M, const double* rec_thrs, int R, int T, int A, int C, long long N, double* precision,
                          double* recall, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PSWIN_H_ */
