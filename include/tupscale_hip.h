/* C ABI of libtupscale_hip.so -- the MI355X (gfx950) kernels behind the FastTransformer
 * plugin surface (models/FastTransformer/model.py: TransformerModel).
 *
 * The reference has no native layer: its hot path is a chain of PyTorch aten calls inside
 * nn.Module.forward.  Each entry point below replaces the aten call site(s) cited next to it
 * (reference file:line, relative to the reference repo root).  A binding needs only plain
 * pointers to device memory, ints and a hipStream_t (passed as void*); no torch types.
 *
 * Conventions
 *   - every function returns 0 on success or a hipError_t value; launches are asynchronous on
 *     `stream` (pass the caller's current stream, never assume the null stream);
 *   - bf16 tensors are raw uint16 storage; NHWC = [B][H][W][C] with C = 64;
 *   - "window layout" = token rows ordered [B][window_y][window_x][8*8 tokens], 192 features,
 *     the order window_partition (model.py:31-45) produces, including zero rows for the
 *     tokens added by the bottom/right padding (model.py:273-280);
 *   - packed weights are produced by transformerupscaler_amd/packing.py (layouts documented
 *     at each function).
 */
#ifndef TUPSCALE_HIP_H
#define TUPSCALE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* library / ABI version, bumped when a signature changes or an entry is removed (16: seven entries removed, none changed).
 * This header is compiled into every translation unit of the library (a definition that drifts from its prototype fails the
 * build) and the Python binding parses it at import: it is the one place where an entry or the version number is written. */
#define TUP_ABI_VERSION 16
int tup_abi_version(void);

/* conv1: Conv2d(3,64,k3,p1)+ReLU. model.py:202-203,251.
 * x fp32 [B][3][H][W]; wp bf16 [64][32] (row ct*16+4g+e = channel g*16+ct*4+e, k = tap*3+cin,
 * zero pad 27..31); bias fp32 [64] or NULL; out bf16 NHWC.
 * Also the input-gradient conv of the 64->3 convs (transposed/flipped weight as wp): in_mask fp32
 * (shape of x; input *= in_mask > 0) and out_mask bf16 NHWC (out *= out_mask > 0) fuse the ReLU backward. */
int tup_conv3x3_c3_fwd(const float* x, const void* wp, const float* bias, const float* in_mask,
                       const void* out_mask, void* out, int B, int H, int W, int relu, void* stream);

/* Conv2d(64*in_r^2, Cout, k3, p1) on NHWC bf16:
 *   conv2 model.py:204,252 | decoder_conv1 model.py:228,312 | Upsampler convs + PixelShuffle(r)
 *   utils.py:62-63,74-75,83-84 (out_mode 0, ntiles = r*r, the cout tile index is the sub-pixel
 *   i*r+j) | up1_conv utils.py:32-40 and decoder_conv2 model.py:229,313 (out_mode 1).
 * x bf16 [B][H*in_r][W*in_r][64]: in_r = 1 is a plain map; in_r > 1 reads 64*in_r^2 logical channels
 * through PixelShuffle^-1 (the input-gradient conv of an Upsampler stage).
 * wp bf16 [ntiles][in_r^2][9][rows][64]; out_mode 0: rows = 64, bias fp32 [ntiles][64] or NULL,
 * out bf16 [B][H*r][W*r][64], optional add / mask (bf16, shape of out):
 * out = (conv + bias [relu] + add) * (mask > 0); out_mode 1: rows = 16 (cout_valid real), bias fp32
 * [cout_valid] or NULL, out fp32 [B][cout_valid][H][W]. */
int tup_conv3x3_c64_fwd(const void* x, const void* wp, const float* bias, const void* add,
                        const void* mask, void* out, int B, int H, int W, int ntiles, int r,
                        int cout_valid, int relu, int out_mode, int in_r, void* stream);

/* Inference decoder (decoder_conv1 64->64 +bias ReLU, then decoder_conv2 64->3 +bias; model.py:228-229,312-313) with the
 * 64-channel map between them kept in registers: decoder_conv2 is evaluated in scatter form inside decoder_conv1's epilogue,
 * and a finishing launch adds the terms that cross a wave boundary in a fixed order (csrc/decoder_fused.hip).
 * x bf16 NHWC [B][H][W][64]; w1 bf16 [1][1][9][64][64] + b1 fp32 [64] (tup_conv3x3_c64_fwd's out_mode 0 packing);
 * wz bf16 [48][64] (decoder_conv2 with permuted columns, packing.pack_dec2_scatter); b2 fp32 [3];
 * seamv fp32 [B][3][H][W] and cseam fp32 [B][H][ceil(W/32)][32] workspaces (no initialisation needed);
 * out fp32 [B][3][H][W].  Requires 12*H*W < 2^31. */
int tup_decoder_fused_fwd(const void* x, const void* w1, const float* b1, const void* wz, const float* b2,
                          float* seamv, float* cseam, float* out, int B, int H, int W, void* stream);

/* The same without the finishing launch: part and seamv fp32 [B][3][H][W] and cseam fp32 [B][H][ceil(W/32)][32] are left unfinished
 * (the wave's own sums, the row-seam terms, the raw tile-edge columns; the rows of seamv without a seam partner and cseam's pad
 * words are not written).  The finished plane is b2 + part [+ seamv] [+ three cseam terms], in that order
 * (decoder_finish_kernel): tup_tail_stream_r2_parts_fwd / tup_tail_stream_r2_resize_parts_fwd form it where they read it. */
int tup_decoder_fused_parts_fwd(const void* x, const void* w1, const float* b1, const void* wz,
                                float* part, float* seamv, float* cseam, int B, int H, int W, void* stream);

/* Inference conv1 + conv2 (model.py:202-204,251-252: Conv2d(3,64)+ReLU, Conv2d(64,64)+ReLU) without the 64-channel map between
 * them in HBM (csrc/conv12_fused.hip).  tup_conv1_compact_fwd: x fp32 [B][3][H][W] -> xc bf16 [B][Hp][Wp][4], Hp = 8 ceil(H/8) + 4,
 * Wp = 32 ceil(W/32) + 4 (image at (+2, +2), zero border, channel 3 = 0).  tup_conv12_fused_fwd: xc -> out bf16 NHWC [B][H][W][64]
 * = ReLU(conv2(ReLU(conv1(x)))), conv1 recomputed per conv2 tile; w1 bf16 [64][32] + b1 fp32 [64] (tup_conv3x3_c3_fwd's packing),
 * w2 bf16 [1][1][9][64][64] + b2 fp32 [1][64] (tup_conv3x3_c64_fwd's out_mode 0 packing).  Bit-identical to the two kernels.
 * Requires 8*Hp*Wp < 2^31. */
int tup_conv1_compact_fwd(const float* x, void* xc, int B, int H, int W, void* stream);
int tup_conv12_fused_fwd(const void* xc, const void* w1, const float* b1, const void* w2, const float* b2, void* out,
                         int B, int H, int W, void* stream);

/* Inference-only composition of branch A: the LAST Upsampler conv (64->64rr, +bias) + PixelShuffle(r)
 * (utils.py:62-63,74-75,83-84) and up1_conv (64->3, no bias, ReLU; utils.py:32-40), called back to back at
 * model.py:264-265 with no non-linearity between them, evaluated as one 5x5-tap conv with 3rr outputs
 * (exact algebra; the outermost HR pixel ring uses per-border weight variants because the reference
 * zero-pads the HR intermediate).  x bf16 NHWC [B][H][W][64]; wp bf16 [25][rows][64] (rows 16/32/112 for
 * r 2/3/6); bias fp32 [3rr]; wv bf16 [9][3rr][25][64]; bv fp32 [9][3rr]; out fp32 [B][3][H*r][W*r].
 * wp / wv must come from a composition (packing.pack_branch_a, tup_bra_compose): output (si, sj)'s 5x5 kernel is then supported
 * on a block of at most 4 x 4 taps.  At r = 2 (tap row 4 / 0 dead for si = 0 / 1, tap column 4 / 0 for sj = 0 / 1) and on the
 * border ring of every r the kernels read only the taps inside each output's support and ignore anything in the other taps.
 * At r = 2 out must be 8-byte aligned. */
int tup_conv5x5_c64_planar_fwd(const void* x, const void* wp, const float* bias, const void* wv,
                               const float* bv, float* out, int B, int H, int W, int r, int relu, void* stream);

/* Planar fp32 Conv2d(3, 3*r*r, k3, p1) + PixelShuffle(r) [+ add] [+ clamp(0,1)]:
 *   final_upscale utils.py:62-63,74-75,83-84 (n_feats=3) | final_upscale_conv model.py:212,317
 *   fused with "out = upscaled_input + residual_up" model.py:320 and torch.clamp model.py:327.
 * x fp32 [B][3][H][W]; w28 fp32 [3*r*r][28] (27 taps (cin,ky,kx) + pad); out/add fp32 [B][3][H*r][W*r].
 * clamp01 = 2 (training): out is [2][B][3][H*r][W*r]: the unclamped sum (the clamp's backward gate), then the clamped output. */
int tup_conv3x3_planar_fwd(const float* x, const float* w28, const float* bias, const float* add,
                           float* out, int B, int H, int W, int r, int clamp01, void* stream);

/* transforms.Resize on a tensor = antialiased bilinear (model.py:323-325, train.py:127-130)
 * [+ clamp(0,1) model.py:327].  Tap tables as aten's _compute_indices_weights_aa (float32).
 * clamp01: 0 = out is the resized tensor; 1 = clamped; 2 (training) = out is [2][planes][Ho][Wo]: first the unclamped values
 * (the gate of the clamp's backward), then the clamped ones (the model output), written in the same pass. */
int tup_resize_aa_fwd(const float* in, float* out, const int* ymin, const int* ysize, const float* yw,
                      int KY, const int* xmin, const int* xsize, const float* xw, int KX, int planes,
                      int Hi, int Wi, int Ho, int Wo, int clamp01, void* stream);

/* The same output tail for a last stage of r = 2 (scales 2 and 4) WITHOUT the Resize, as a register-streaming stencil (no LDS):
 * final_upscale's last Conv2d(3,12,3)+PixelShuffle(2) utils.py:62-63,74-75, final_upscale_conv + "+ upscaled_input"
 * model.py:316-320 [+ clamp model.py:327].  x fp32 [B][3][H][W]; wfu_t fp32 [27][12], wfc_t fp32 [27][4] tap-major
 * (k = cin*9 + ky*3 + kx; packing.pack_planar_t); bfu [12], bfc [3]; ui / out fp32 [B][3][2H][2W].
 * The four tup_tail_stream_r2_* entries take their 420 wave-uniform weights by scalar loads straight from wfu_t / bfu / wfc_t / bfc
 * into scalar operands of the packed FMAs: these four pointers must be 16-byte aligned, or the entries return hipErrorInvalidValue. */
int tup_tail_stream_r2_fwd(const float* x, const float* wfu_t, const float* bfu, const float* wfc_t, const float* bfc,
                           const float* ui, float* out, int B, int H, int W, int clamp01, void* stream);

/* ... followed by the antialiased Resize to Ho x Wo (model.py:323-325; tap tables as tup_resize_aa_fwd, at most 4 taps per output)
 * and the clamp, in the same kernel: out fp32 [B][3][Ho][Wo].  sc = LR columns a wave strip advances by
 * (<= 60 - ceil((max taps - 1) / 2)), band_h = LR rows per band (multiple of 3), ext = LR rows a band runs past its end
 * (ceil((max taps - 1) / 2)); oxb int [ceil(W / sc) + 1] / oyb int [ceil(H / band_h) + 1]: first output column / row whose
 * first tap lies in strip s's HR columns [2 s sc, ...) / band k's HR rows [2 k band_h, ...). */
int tup_tail_stream_r2_resize_fwd(const float* x, const float* wfu_t, const float* bfu, const float* wfc_t, const float* bfc,
                                  const float* ui, float* out, const int* ymin, const int* ysize, const float* yw, int KY,
                                  const int* xmin, const int* xsize, const float* xw, int KX, const int* oxb, const int* oyb,
                                  int B, int H, int W, int Ho, int Wo, int sc, int band_h, int ext, int clamp01, void* stream);

/* The two entries above on the unfinished output of tup_decoder_fused_parts_fwd in place of x (part, seamv, cseam as left by it,
 * b2 fp32 [3] = decoder_conv2's bias, tilesX = ceil(W / 32)): every LR value is formed in decoder_finish_kernel's order of fp32
 * additions where the kernel would have loaded it, so out equals, bit for bit, what the finished plane gives.
 * Requires B*H*tilesX*32 < 2^29 beside the limits of the entries above. */
int tup_tail_stream_r2_parts_fwd(const float* part, const float* seamv, const float* cseam, const float* b2, int tilesX,
                                 const float* wfu_t, const float* bfu, const float* wfc_t, const float* bfc,
                                 const float* ui, float* out, int B, int H, int W, int clamp01, void* stream);
int tup_tail_stream_r2_resize_parts_fwd(const float* part, const float* seamv, const float* cseam, const float* b2, int tilesX,
                                        const float* wfu_t, const float* bfu, const float* wfc_t, const float* bfc,
                                        const float* ui, float* out, const int* ymin, const int* ysize, const float* yw, int KY,
                                        const int* xmin, const int* xsize, const float* xw, int KX, const int* oxb, const int* oyb,
                                        int B, int H, int W, int Ho, int Wo, int sc, int band_h, int ext, int clamp01, void* stream);

/* Inference fusion of the output tail (model.py:316-327): last final_upscale stage (Conv2d(3,3rr,3)+PixelShuffle),
 * final_upscale_conv, "+ upscaled_input", Resize (tap tables; identity tables when sizes match) and clamp.
 * x fp32 [B][3][H][W]; ui fp32 [B][3][H*r][W*r]; out fp32 [B][3][Ho][Wo]; EH/EW = largest HR window a 16x64
 * output tile's taps touch. */
int tup_tail_fused_fwd(const float* x, const float* wfu, const float* bfu, const float* wfc, const float* bfc,
                       const float* ui, float* out, const int* ymin, const int* ysize, const float* yw, int KY,
                       const int* xmin, const int* xsize, const float* xw, int KX, int B, int H, int W, int r,
                       int Ho, int Wo, int EH, int EW, int clamp01, void* stream);

/* torch.clamp(out, 0, 1) model.py:327 when no resize precedes it. */
int tup_clamp01_fwd(const float* in, float* out, long long n, void* stream);

/* nn.LayerNorm(192) model.py:142,144,163,169.  x fp32 [M][192] -> y bf16 [M][192];
 * mean/rstd fp32 [M] optional (saved for backward). */
int tup_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y,
                      float* mean, float* rstd, int M, void* stream);

/* relative_position_bias_table[relative_position_index] model.py:120-123 -> dense per-head bias
 * in the attention kernel's fragment order, fp32 [12][4][4][64][4]. */
int tup_relpos_bias_expand(const float* table, float* frag, void* stream);

/* WindowAttention core model.py:114-130 (q*scale, qk^T + bias, softmax, @v, head concat).
 * qkv bf16 [nwin][64][576]; out bf16 [nwin][64][192].  drop_p > 0: attn_drop (model.py:80,127) with a
 * stateless hash mask keyed by drop_seed (csrc/common.h); the backward re-derives the same mask.
 * lse: NULL (inference) or fp32 [nwin][12][64] <- log-sum-exp of every score row, saved for tup_window_attn_bwd. */
int tup_window_attn_fwd(const void* qkv, const float* bias_frag, void* out, float* lse, int nwin, float drop_p,
                        unsigned int drop_seed, void* stream);

/* nn.Linear family model.py:79,81,146-151 with fused epilogues (forward AND the input-gradient
 * GEMMs of the backward, which are the same product with the transposed weight packed as Wt).
 * Wt bf16 [N][K] (rows permuted per 64-group: row ct*16+4g+e = feature g*16+ct*4+e), bias fp32 [N].
 * a_dtype 0: A bf16 [M][lda]; 1: A fp32.  epilogue 0: (+bias) -> bf16 | 1: +bias, erf-GELU -> bf16
 * (model.py:148) | 2: +bias + res -> fp32 (residual adds model.py:164,171) | 3: * gelu'(aux) -> bf16
 * (aux bf16 [M][ldo] = saved pre-activation; backward of model.py:148).  With epilogue 1 a non-NULL
 * aux is an OUTPUT that receives the bf16 pre-activation (saved for the backward).  drop_p > 0 (epilogue 2):
 * out = dropout(acc + bias) + res -- proj_drop / the MLP's Dropout (model.py:82,132,150). */
int tup_gemm_tokens_fwd(const void* A, int a_dtype, int lda, const void* Wt, const float* bias,
                        const float* res, const void* aux, void* out, int ldo, int M, int N, int K,
                        int epilogue, float drop_p, unsigned int drop_seed, void* stream);

/* reflect pad + patch_embed Conv2d(64,192,k8,s8) + NHWC permute + zero token pad +
 * window_partition: model.py:256-261,268-285.  feat bf16 NHWC; Wt bf16 [192][4096],
 * k = (i*8+j)*64+c; x_out fp32 window layout. */
int tup_patch_embed_fwd(const void* feat, const void* Wt, const float* bias, float* x_out,
                        int B, int H, int W, void* stream);

/* window_reverse + crop + patch_unembed ConvTranspose2d(192,64,k8,s8) + crop + skip add:
 * model.py:292-309.  x window layout, fp32 (x_bf16 = 0) or bf16 (x_bf16 = 1: tup_blocks_stream_fwd's out_bf16 -- the GEMM rounds an
 * fp32 x to the same bf16 values on load); Wt bf16 [4096][192], n = (i*8+j)*64+o; bias fp32 [64];
 * skip/out bf16 NHWC [B][H][W][64]. */
int tup_patch_unembed_fwd(const void* x, int x_bf16, const void* Wt, const float* bias, const void* skip,
                          void* out, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ResidualTransformer path (reference models/ResidualTransformer/model.py; forward / inference).
 * Reuses conv1/conv2/decoder kernels above; the stride-2 `downsample` conv (model.py:89,132) runs on
 * tup_conv3x3_c64_fwd with in_r = 2 (space-to-depth read) and a zero-padded 3x3x4 weight pack.
 * ------------------------------------------------------------------------------------------- */

/* patch_embed Conv2d(64,128,k8,s8) + flatten/transpose + pos_embed (model.py:135-140): feat bf16 NHWC
 * [B][H][W][64]; Wt bf16 [128][4096]; pos fp32 [T][128]; x_out fp32 [B*T][128], T = (H/8)*(W/8). */
int tup_rt_patch_embed_fwd(const void* feat, const void* Wt, const float* bias, const float* pos, float* x_out,
                           int B, int H, int W, void* stream);

/* transpose/view + patch_unembed ConvTranspose2d(128,64,k8,s8) + skip add (model.py:147-153). */
int tup_rt_patch_unembed_fwd(const float* x, const void* Wt, const float* bias, const void* skip, void* out,
                             int B, int H, int W, void* stream);

/* nn.MultiheadAttention(128, 8 heads) core, eval mode (model.py:31,43): qkv bf16 [B][N][384] -> out bf16 [B][N][128];
 * flash-style (online softmax), any N; lse (optional) receives the per-query log-sum-exp for the backward.
 * drop_p > 0: nn.MultiheadAttention's dropout on the attention probabilities, stateless hash mask on (image, head, q, k). */
int tup_rt_attention_fwd(const void* qkv, void* out, float* lse, int B, int N, float drop_p, unsigned int drop_seed,
                         void* stream);

/* Its backward (P recomputed from the saved log-sum-exp `lse` fp32 [B][8][N]; two passes, no atomics):
 * out/gout bf16 [B][N][128], work fp32 [B][8][N] scratch, gqkv bf16 [B][N][384]. */
int tup_rt_attention_bwd(const void* qkv, const void* out, const void* gout, const float* lse, float* work,
                         void* gqkv, int B, int N, float drop_p, unsigned int drop_seed, void* stream);

/* nn.LayerNorm(128) (model.py:30,32): x fp32 [M][128] -> y bf16. */
int tup_layernorm128_fwd(const float* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                         int M, void* stream);

/* out = clamp(F.interpolate(a, bicubic) + F.interpolate(b, bicubic)) (model.py:125,160-164); tables [Ho][4]/[Wo][4]
 * of clamped source indices and weights per source (align_corners=False, A=-0.75). */
int tup_rt_bicubic_sum_fwd(const float* a, const float* b, float* out, const int* ayi, const float* ayw,
                           const int* axi, const float* axw, const int* byi, const float* byw, const int* bxi,
                           const float* bxw, int planes, int Ha, int Wa, int Hb, int Wb, int Ho, int Wo,
                           int clamp01, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward (what torch autograd executes for the same call sites under train.py:138).
 * Accumulating outputs (documented per function) must be zeroed by the caller.
 * ------------------------------------------------------------------------------------------- */

/* Weight gradient of a Linear: out[NI][NJ] (fp32, ldo) += P^T Q, P [M][NI], Q [M][NJ]; dtypes 0 = bf16,
 * 1 = fp32.  For nn.Linear: P = grad_output, Q = input -> out = weight.grad layout [out][in]. */
int tup_gemm_wgrad(const void* P, int p_dtype, int ldp, const void* Q, int q_dtype, int ldq,
                   float* out, int ldo, int M, int NI, int NJ, void* stream);
/* The same with the layer's bias gradient in the same pass (model.py:79,81,146-151 under train.py:138):
 * colsum_out[NI] (fp32, zeroed by the caller) += column sums of P. */
int tup_gemm_wgrad_bias(const void* P, int p_dtype, int ldp, const void* Q, int q_dtype, int ldq,
                        float* out, int ldo, float* colsum_out, int M, int NI, int NJ, void* stream);

/* Weight gradient of patch_embed (reflect=1: P = grad tokens, map = feat) and of patch_unembed
 * (reflect=0: P = tokens, map = grad of its output).  out fp32 [192][4096] +=, column (i*8+j)*64+c. */
int tup_patch_wgrad(const float* P, const void* map, float* out, int B, int H, int W, int reflect, void* stream);
/* The same from bf16 token rows P [M][192] (the rounding tup_patch_wgrad applies on load, done by the caller) on the wide-tile
 * kernel: one workgroup per CU owns 192 x 128 of the output, both operands by LDS-DMA, the map is read once instead of three
 * times and the token rows 32 instead of 64 times.  B * H * W * 128 < 2^31. */
int tup_patch_wgrad_bf16(const void* P, const void* map, float* out, int B, int H, int W, int reflect, void* stream);

/* Bias gradients: out[N] += column sums of G [M][N] (dtype 0 bf16 / 1 fp32) over the rows with
 * rowmask[m] != 0 (uint8 [M]; NULL = all rows). */
int tup_colsum(const void* G, int dtype, int ld, float* out, int M, int N, const void* rowmask, void* stream);

/* LayerNorm backward: dx = LN'(gy) (+ gres), dgamma/dbeta fp32 [192] +=.  gdrop: NULL, or bf16 [M][192] <- dx * dropout mask /
 * (1 - drop_p) for the site keyed by drop_seed (tup_dropout_bwd of dx fused in: the gradient's next stop is the Dropout behind
 * attn.proj / mlp.2, model.py:82,132,150). */
int tup_layernorm_bwd(const void* gy, const float* x, const float* mean, const float* rstd,
                      const float* gamma, const float* gres, float* dx, float* dgamma, float* dbeta,
                      int M, void* gdrop, float drop_p, unsigned int drop_seed, void* stream);

/* Dense relative-position bias in the second (query-row) fragment order used by the backward. */
int tup_relpos_bias_expand_n(const float* table, float* frag, void* stream);

/* Attention-core backward: P is rebuilt from q, k, the dense bias (bias_n, tup_relpos_bias_expand_n) and the forward's lse;
 * rowsum(P dP) = gout . att with att bf16 [nwin][64][192] the forward's output.  gqkv bf16 [nwin][64][576]; dbias_n fp32
 * [12][4][4][64][4] overwritten (the dense gradient of the relative-position bias, in bias_n's layout).  scratch: fp32
 * [tup_window_attn_bwd_scratch(nwin, heads)], uninitialised -- each persistent wave writes its own partial sum there and a
 * second kernel adds the slots up (no float atomics). */
int tup_window_attn_bwd(const void* qkv, const void* gout, const void* att, const float* lse, const float* bias_n,
                        void* gqkv, float* dbias_n, float* scratch, int nwin, float drop_p, unsigned int drop_seed, void* stream);
long long tup_window_attn_bwd_scratch(int nwin, int heads);

/* Backward of nn.Dropout after proj / mlp.2: gout bf16 = gin fp32 * mask / (1 - p), element index m*192+n. */
int tup_dropout_bwd(const float* gin, void* gout, long long n, float drop_p, unsigned int drop_seed, void* stream);

/* dense bias gradient -> relative_position_bias_table.grad fp32 [225][12] (overwritten). */
int tup_relpos_bias_reduce(const float* dbias_n, float* dtable, void* stream);

/* Input gradients of patch_unembed (gx fp32 window layout, overwritten) and patch_embed (gmap_pad bf16
 * NHWC [B][ceil8(H)][ceil8(W)][64], the reflect-PADDED map, overwritten). */
int tup_patch_unembed_bwd(const void* gmap, const void* Wt, float* gx, int B, int H, int W, void* stream);
int tup_patch_embed_bwd(const float* gx, const void* Wt, void* gmap_pad, int B, int H, int W, void* stream);

/* ... with the gradient merge at `feat` in the epilogue (H, W multiples of 8): out bf16 NHWC [B][H][W][64] = (gx Wt^T + add1 + add2)
 * * (relu_src > 0) -- tup_patch_embed_bwd followed by tup_feat_grad_combine without the padded map in between.  add2 may be NULL.
 * add1_colsum: NULL, or fp32 [16][64] (zeroed by the caller) += per-channel sums of add1 in 16 replicas (tup_colsum of add1 for free). */
int tup_patch_embed_bwd_merge(const float* gx, const void* Wt, const void* add1, const void* add2, const void* relu_src,
                              void* out, float* add1_colsum, int B, int H, int W, void* stream);

/* Weight/bias gradients of the 3x3 convs (accumulating).
 *   c64:    x bf16 NHWC, gmap bf16 NHWC [B][H*gr][W*gr][64] sub-pixel plane sp -> dwp fp32 [64][9][64]
 *           (co, tap, ci) for couts {c*gr*gr + sp}, dbias fp32 [64] or NULL
 *   thin:   gpl fp32 [B][3][H][W] -> dwp fp32 [3][9][64], dbias [3] or NULL   (up1_conv, decoder_conv2)
 *   c3:     x fp32 [B][3][H][W], gmap bf16 NHWC -> dw fp32 [64][3][3][3], dbias [64]   (conv1)
 *   planar: x fp32 [B][3][H][W], gpl fp32 [B][3][H*r][W*r] -> dw fp32 [3rr][3][3][3], dbias [3rr] */
int tup_conv3x3_c64_wgrad(const void* x, const void* gmap, float* dwp, float* dbias,
                          int B, int H, int W, int gr, int sp, void* stream);
int tup_conv3x3_thin_wgrad(const void* x, const float* gpl, float* dwp, float* dbias, int B, int H, int W, void* stream);
int tup_conv3x3_c3_wgrad(const float* x, const void* gmap, float* dw, float* dbias, int B, int H, int W, void* stream);
int tup_conv3x3_planar_wgrad(const float* x, const float* gpl, float* dw, float* dbias,
                             int B, int H, int W, int r, void* stream);

/* Deterministic forms.  The forms above add per-workgroup partial sums with float atomics, so their result bits depend on the
 * order the adds arrive in.  The *_det forms take the same arguments plus `slab`, an fp32 workspace of tup_conv_wgrad_slab(...)
 * floats provided by the caller (contents ignored, no allocation inside): every persistent workgroup stores its partial sums into
 * its own slice, and tup_slab_reduce adds the slices onto the outputs in a fixed order.  The grids
 * depend on the shapes only, so the result is bitwise reproducible for a given build and device model.
 *   tup_conv_wgrad_slab: kind 0 = c64 (and c64 s2d; H, W of gmap's plane), 1 = thin, 2 = planar with factor r.  Host only: returns
 *   a float count (0 for invalid arguments), not a hipError_t.
 *   tup_slab_reduce: out[i] (accumulate ? += : =) sum over s < nslab of slab[s * ld + i], i < n: group y (0..3) adds slices
 *   y, y + 4, ... left to right, then ((group 0 + group 2) + (group 1 + group 3)) is written or added to out[i]. */
long long tup_conv_wgrad_slab(int kind, int B, int H, int W, int r);
int tup_slab_reduce(const float* slab, long long ld, int nslab, float* out, long long n, int accumulate, void* stream);
int tup_conv3x3_c64_wgrad_det(const void* x, const void* gmap, float* dwp, float* dbias,
                              int B, int H, int W, int gr, int sp, float* slab, void* stream);
int tup_conv3x3_c64_wgrad_s2d_det(const void* x, const void* gmap, float* dwp, float* dbias,
                                  int B, int H, int W, int xr, int xsp, float* slab, void* stream);
int tup_conv3x3_thin_wgrad_det(const void* x, const float* gpl, float* dwp, float* dbias, int B, int H, int W, float* slab, void* stream);
int tup_conv3x3_planar_wgrad_det(const float* x, const float* gpl, float* dw, float* dbias,
                                 int B, int H, int W, int r, float* slab, void* stream);

/* Deterministic forms of the token-path reductions (the weight-gradient GEMMs, the column sums, the LayerNorm backward): the
 * arguments of the atomic twin plus `slab`, an fp32 workspace of tup_wgrad_slab(...) floats (contents ignored, no allocation
 * inside).  Every static work item -- an M slice of a 64 x 64 tile, a wide-kernel workgroup's M slice, a column-sum row chunk, a
 * LayerNorm workgroup -- stores its partial result into its own slab slice, and tup_slab_reduce adds the slices onto the outputs
 * (accumulating: the caller zeroes them, as for the atomic forms).  The split of M depends on the shapes only.
 *   tup_wgrad_slab(kind, M, NI, NJ): kind 0 = the 64 x 64-tile GEMM (tup_gemm_wgrad_bias_det and the three fp32 patch forms; M
 *   token rows, output NI x NJ; a slice is NI x NJ with NI column sums behind it), 1 = the wide patch GEMM
 *   (tup_patch_wgrad_bf16_det; NI = 192, NJ = 4096), 2 = tup_colsum_det (M rows, NI columns, NJ ignored), 3 = the LayerNorm
 *   backward (M rows, NI = 192 or 128, NJ ignored; at most 256 slices of 2 x NI).  For the patch forms M is the token-row count
 *   of the twin's P operand (B * windows * 64, or B * H/8 * W/8 for tup_rt_patch_wgrad_det).  Host only: returns a float count
 *   (0 for an invalid request), not a hipError_t.
 *   tup_gemm_wgrad_bias_det: colsum_out == NULL gives the deterministic tup_gemm_wgrad.  When colsum_out == out + NI * NJ (and
 *   ldo == NJ) one reduce launch serves both; an output with ldo > NJ is reduced row by row.
 *   tup_layernorm_bwd_det / tup_layernorm128_bwd_det: dbeta == dgamma + C likewise takes one reduce launch. */
long long tup_wgrad_slab(int kind, long long M, int NI, int NJ);
int tup_gemm_wgrad_bias_det(const void* P, int p_dtype, int ldp, const void* Q, int q_dtype, int ldq,
                            float* out, int ldo, float* colsum_out, int M, int NI, int NJ, float* slab, void* stream);
int tup_patch_wgrad_det(const float* P, const void* map, float* out, int B, int H, int W, int reflect, float* slab, void* stream);
int tup_patch_wgrad_bf16_det(const void* P, const void* map, float* out, int B, int H, int W, int reflect, float* slab, void* stream);
int tup_rt_patch_wgrad_det(const float* P, const void* map, float* out, int B, int H, int W, float* slab, void* stream);
int tup_wt_patch_wgrad_det(const float* P, const void* map, float* out, int B, int H, int W, int NI, float* slab, void* stream);
int tup_colsum_det(const void* G, int dtype, int ld, float* out, int M, int N, const void* rowmask, float* slab, void* stream);
int tup_layernorm_bwd_det(const void* gy, const float* x, const float* mean, const float* rstd,
                          const float* gamma, const float* gres, float* dx, float* dgamma, float* dbeta,
                          int M, void* gdrop, float drop_p, unsigned int drop_seed, float* slab, void* stream);
int tup_layernorm128_bwd_det(const void* gy, const float* x, const float* mean, const float* rstd,
                             const float* gamma, const float* gres, float* dx, float* dgamma, float* dbeta,
                             int M, void* gdrop, float drop_p, unsigned int drop_seed, float* slab, void* stream);

/* Input gradient of Conv2d(3,3rr,k3)+PixelShuffle(r) on planar fp32 (final_upscale): w fp32 [3rr][3][3][3]. */
int tup_conv3x3_planar_dgrad(const float* gpl, const float* w, float* gx, int B, int H, int W, int r, void* stream);

/* Backward of Resize(antialias) [+ clamp]: gin fp32 [planes][Hi][Wi]; pre = pre-clamp output or NULL;
 * oy0/oyn/ox0/oxn: per input row/col the range of outputs that reference it.
 * l1_scale: NULL, or device float[2] = {d loss / numel, plain} -- then `gout` is the TARGET of nn.L1Loss (train.py:103,132) and the
 * gradient is formed in the kernel (pre required): plain = 0: sign(clamp(pre) - target) * l1_scale[0], gated by the clamp (pre = the
 * pre-clamp output); plain != 0: sign(pre - target) * l1_scale[0] with pre = the Resize output itself (train.py:127-130 resizes the
 * clamped model output, nothing clamps after it).  The loss's backward pass and its 100 MB gradient tensor do not exist. */
int tup_resize_aa_bwd(const float* gout, const float* pre, float* gin, const int* ymin, const float* yw, int KY,
                      const int* xmin, const float* xw, int KX, const int* oy0, const int* oyn,
                      const int* ox0, const int* oxn, int planes, int Hi, int Wi, int Ho, int Wo,
                      const float* l1_scale, void* stream);

/* gin = gout * [0 <= pre <= 1] * [relu_src > 0] (clamp / ReLU backward; either source may be NULL); l1_scale as above. */
int tup_mask_bwd(const float* gout, const float* pre, const float* relu_src, float* gin, long long n,
                 const float* l1_scale, void* stream);

/* Gradient merge at `feat` (model.py:264,268,308 fan-out) + conv2's ReLU backward:
 * out = (a + b + fold_reflect(gpe)) * (feat > 0), NHWC bf16; gpe = padded map from tup_patch_embed_bwd. */
int tup_feat_grad_combine(const void* a, const void* b, const void* gpe, const void* feat, void* out,
                          int B, int H, int W, void* stream);

/* ---- ResidualTransformer backward (autograd through models/ResidualTransformer/model.py:121-165 in train.py:138) ---- */

/* LayerNorm(128) backward; same contract as tup_layernorm_bwd (dgamma / dbeta fp32 [128] accumulated). */
int tup_layernorm128_bwd(const void* gy, const float* x, const float* mean, const float* rstd, const float* gamma,
                         const float* gres, float* dx, float* dgamma, float* dbeta, int M, void* gdrop, float drop_p,
                         unsigned int drop_seed, void* stream);

/* patch_embed / patch_unembed weight gradients on the plain token grid: out fp32 [128][4096] += P^T patches(map);
 * P fp32 [B*T][128], map NHWC bf16 [B][H][W][64], column (i*8+j)*64 + c. */
int tup_rt_patch_wgrad(const float* P, const void* map, float* out, int B, int H, int W, void* stream);

/* Weight gradient of the stride-2 `downsample` conv (model.py:132) as a conv over the space-to-depth input:
 * x NHWC bf16 [B][H*xr][W*xr][64] plane xsp, gmap NHWC bf16 [B][H][W][64]; dwp fp32 [64][9][64] +=, dbias [64] += or NULL. */
int tup_conv3x3_c64_wgrad_s2d(const void* x, const void* gmap, float* dwp, float* dbias, int B, int H, int W,
                              int xr, int xsp, void* stream);

/* Backward of tup_rt_bicubic_sum_fwd w.r.t. source a (F.interpolate bicubic + clamp, model.py:160-164): gout / out fp32
 * [planes][Ho][Wo] (out = saved forward output, gate 0 < out < 1; NULL = no clamp), ga fp32 [planes][Ha][Wa], tmp fp32
 * [planes][Ha][Wo]; (ystart [Ha+1], yo, yw) / (xstart [Wa+1], xo, xw) = transposed tap lists. */
int tup_rt_bicubic_bwd(const float* gout, const float* out, float* ga, float* tmp, const int* ystart, const int* yo,
                       const float* yw, const int* xstart, const int* xo, const float* xw, int planes, int Ha, int Wa,
                       int Ho, int Wo, void* stream);
/* The same with the row pass in bands of 16 source rows (every output row is read once per band instead of once per source row it
 * touches) and dense column tables: band_r0 / band_n int [ceil(Ha/16)] = first output row / row count of band b, band_w fp32
 * [nbands][nr_max][16] = weight of output row band_r0[b] + i for source row 16 b + k (zero where none); xoT int / xwT fp32
 * [kmax][Wa] = entry k of source column x's transposed tap list (padding: weight 0); blk_c0 / blk_n int [ceil(Wa/256)] = the
 * stretch (<= 4096 columns) of a tmp row that source columns 256 j .. 256 j + 255 read.  l1_scale (device scalar, or NULL): when
 * given, `gout` is the TARGET of nn.L1Loss (train.py:103,132) applied to the forward output and the upstream gradient
 * sign(out - target) * l1_scale[0] is formed inside the row pass instead of being read. */
int tup_rt_bicubic_bwd_banded(const float* gout, const float* out, float* ga, float* tmp, const int* band_r0, const int* band_n,
                              const float* band_w, int nr_max, const int* xoT, const float* xwT, int kmax, const int* blk_c0,
                              const int* blk_n, int planes, int Ha, int Wa, int Ho, int Wo, const float* l1_scale, void* stream);

/* ---- frame pre/post-processing either side of the model ---- */

/* torchvision ToTensor on a uint8 frame (reference data_handling/data_class.py:61-71, inference.py:65-75,
 * app_overlay.py preproc): src u8 [B][H][W][3] -> dst fp32 [B][3][H][W] = src / 255.  swap_rb = 1: BGR source. */
int tup_u8hwc_to_f32chw(const void* src, float* dst, int B, int H, int W, int swap_rb, void* stream);

/* (x * 255).clamp(0, 255).to(uint8).permute(1, 2, 0)[..., [2, 1, 0]] (reference app_overlay.py:381-388; ToPILImage
 * in inference.py:123-124): src fp32 [B][3][H][W] -> dst u8 [B][H][W][3], truncating.  swap_rb = 1: BGR output. */
int tup_f32chw_to_u8hwc(const float* src, void* dst, int B, int H, int W, int swap_rb, void* stream);

/* NV12 video frames (YUV 4:2:0, 8 bit; no counterpart in the reference, which reads RGB files and screen grabs).
 * Layout: y u8 [B][H][W]; uv u8 [B][H/2][W/2][2] = (Cb, Cr) pairs.  Each plane has its own row pitch and batch stride IN BYTES
 * (pitch >= W), so a pitched decoder surface, or the usual single allocation [B][3H/2][pitch] with Y on top and UV below, is
 * passed as it is.  matrix: 0 = BT.601, 1 = BT.709; full_range: 0 = Y 16..235 / chroma 16..240, 1 = 0..255.
 * Chroma siting "left" (the H.264 / HEVC default): sample (j, i) sits at luma column 2i, halfway between luma rows 2j and 2j+1.
 * Both directions are integer arithmetic on bytes and bit-exact with the definition in DESIGN.md section 3 ("NV12 frames"):
 *   decode  chroma upsampled without intermediate rounding (vertical C[j-1] + 3 C[j] | 3 C[j] + C[j+1], horizontal 2 v[i] |
 *           v[i] + v[i+1], indices clamped to the plane), 16.16 matrix, R = clip8((cy (Y - yoff) + 32768 + rv cr) >> 16), ...;
 *           dst fp32 [B][3][H][W] = byte / 255, i.e. exactly "convert to RGB24, then tup_u8hwc_to_f32chw";
 *   encode  src fp32 [B][3][H][W] -> bytes as tup_f32chw_to_u8hwc makes them (truncating, NaN -> 0),
 *           Y = clip8((ry R + gy G + by B + (yoff << 16) + 32768) >> 16), chroma from the [1 2 1] x [1 1] filter around
 *           column 2i of rows 2j, 2j+1 (columns clamped to the image).  Bytes between W and the pitch are left untouched.
 * One launch each, no allocation, synchronisation or host read (capturable into a hipGraph).  B <= 65535; an empty shape
 * returns 0; odd H or W, a pitch below W, a null pointer, or an unknown matrix / full_range returns hipErrorInvalidValue before any
 * launch. */
int tup_nv12_to_f32chw(const void* y, const void* uv, long long y_batch_stride, int y_pitch,
                       long long uv_batch_stride, int uv_pitch, float* dst,
                       int B, int H, int W, int matrix, int full_range, void* stream);
int tup_f32chw_to_nv12(const float* src, void* y, void* uv, long long y_batch_stride, int y_pitch,
                       long long uv_batch_stride, int uv_pitch,
                       int B, int H, int W, int matrix, int full_range, void* stream);

/* P010 video frames (YUV 4:2:0, 10 bit: HEVC Main10, AV1 10-bit, UHD / HDR sources): the NV12 pair above carried to 10 bits
 * (csrc/p010.hip; definition in DESIGN.md section 3, "P010 frames").
 * Layout: y u16 [B][H][W]; uv u16 [B][H/2][W/2][2] = (Cb, Cr) pairs; samples little-endian with the 10-bit code in the HIGH bits:
 * a reader takes code = sample >> 6 and ignores the low six bits, a writer stores code << 6.  The plane pointers are void*.  Each
 * plane has its own row pitch and batch stride IN BYTES, both even (pitch >= 2 W).  matrix: 0 = BT.601, 1 = BT.709, 2 = BT.2020
 * (non-constant luminance); full_range: 0 = Y 64..940 / chroma 64..960, 1 = 0..1023.  Chroma sited left, as for NV12.  The transfer
 * function is not touched: PQ / HLG code values pass through as they are.
 *   decode  the NV12 upsampling taps, cb = c8(Cb) - 4096, cr = c8(Cr) - 4096, R = clip10((cy (Y - yoff) + 32768 + rv cr) >> 16), ...;
 *           dst fp32 [B][3][H][W] = code / 1023 (the IEEE quotient; never through 8 bits);
 *   encode  src fp32 [B][3][H][W] -> codes q_10(x): t = x * 1023, NaN -> 0, clamp to [0, 1023], (int)(t + 0.5f) -- round to nearest,
 *           where the 8-bit entries truncate -- then Y = clip10((ry R + gy G + by B + (yoff << 16) + 32768) >> 16) and chroma
 *           clip10((ur sR + ug sG + ub sB + (512 << 19) + (1 << 18)) >> 19) from the [1 2 1] x [1 1] filter.  Samples between W and
 *           the pitch are left untouched.
 * One launch each, no allocation, synchronisation or host read (capturable into a hipGraph).  B <= 65535; an empty shape
 * returns 0; odd H or W, a pitch below 2 W, a null or odd pointer, an odd pitch or batch stride, or an unknown matrix / full_range returns
 * hipErrorInvalidValue before any launch. */
int tup_p010_to_f32chw(const void* y, const void* uv, long long y_batch_stride, int y_pitch,
                       long long uv_batch_stride, int uv_pitch, float* dst,
                       int B, int H, int W, int matrix, int full_range, void* stream);
int tup_f32chw_to_p010(const float* src, void* y, void* uv, long long y_batch_stride, int y_pitch,
                       long long uv_batch_stride, int uv_pitch,
                       int B, int H, int W, int matrix, int full_range, void* stream);

/* ---- WindowTransformer plugin (models/WindowTransformer/model.py): the FastTransformer window
 * block at embedding width 128 / 8 heads ---- */

/* relative_position_bias_table [225][heads] -> dense S^T-fragment bias [heads*16*256] (heads = 8 or 12). */
int tup_relpos_bias_expand_h(const float* table, float* frag, int heads, void* stream);

/* WindowAttention core (model.py:125-143) for heads x 16 channels: qkv bf16 [nwin][64][48*heads] -> out bf16
 * [nwin][64][16*heads]; lse NULL or fp32 [nwin][heads][64] as tup_window_attn_fwd. */
int tup_window_attn_fwd_h(const void* qkv, const float* bias_frag, void* out, float* lse, int nwin, int heads, float drop_p,
                          unsigned int drop_seed, void* stream);

/* patch_embed (stride-8 conv, no padding: floor(H/8) x floor(W/8) tokens) + permute + zero token pad + window_partition
 * (model.py:247-268): feat bf16 NHWC [B][H][W][64], Wt bf16 [N][4096], x_out fp32 window layout [B*nWy*nWx*64][N]. */
int tup_wt_patch_embed_fwd(const void* feat, const void* Wt, const float* bias, float* x_out, int B, int H, int W, int N,
                           void* stream);

/* window_reverse + crop + patch_unembed + cropped skip add (model.py:272-291): x fp32 window layout [M][K], Wt bf16
 * [4096][K], skip / out bf16 NHWC [B][Hs][Ws][64] (Hs, Ws multiples of 8 = the token grid times 8). */
int tup_wt_patch_unembed_fwd(const float* x, const void* Wt, const float* bias, const void* skip, void* out,
                             int B, int Hs, int Ws, int K, void* stream);

/* nn.L1Loss() of the training step (reference train.py:103,132) and its backward.  a, b fp32 [n] (n % 4 == 0):
 * partial[nblocks] receives per-workgroup sums of |a - b| (the caller adds them and divides by n);
 * ga = sign(a - b) * gout[0] / n. */
int tup_l1_loss_partial(const float* a, const float* b, float* partial, long long n, int nblocks, void* stream);
int tup_l1_loss_bwd(const float* a, const float* b, const float* gout, float* ga, long long n, void* stream);

/* Measurement aid (bench.py `sustained.clock_GHz`; no reference counterpart): writes s_memtime (shader cycles) and s_memrealtime
 * (100 MHz ticks) of one wave to out2[0], out2[1] (two uint64 on the device), in stream order. */
int tup_clock_probe(void* out2, void* stream);

/* WindowTransformer backward pieces: the FastTransformer entries for `heads` = 8 or 12 and the window-layout patch weight
 * gradient on the floor(H/8) x floor(W/8) token grid (out fp32 [NI][4096] += P^T patches(map), no reflect padding). */
int tup_relpos_bias_expand_n_h(const float* table, float* frag, int heads, void* stream);
int tup_window_attn_bwd_h(const void* qkv, const void* gout, const void* att, const float* lse, const float* bias_n, void* gqkv,
                          float* dbias_n, float* scratch, int nwin, int heads, float drop_p, unsigned int drop_seed, void* stream);
int tup_relpos_bias_reduce_h(const float* dbias_n, float* dtable, int heads, void* stream);
int tup_wt_patch_wgrad(const float* P, const void* map, float* out, int B, int H, int W, int NI, void* stream);

/* Branch A in TRAINING through its exact composition (r = 2): replaces autograd through `self.up1(feat)` + `self.up1_conv(...)`,
 * model.py:264-265 (Upsampler utils.py:62-63 + BasicConv utils.py:32-40; no non-linearity between the two convs, utils.py:50).
 * compose: wu fp32 [256][64][3][3], bu fp32 [256], w3 fp32 [3][64][3][3] -> the composed 5x5 conv's weights in every layout the
 * kernels use: wv bf16 [9 border variants][12 n][25 taps][64] + bv fp32 [9][12]; wp bf16 [25][16][64] (forward main kernel,
 * zero-initialised by the caller); wd bf16 [13][64][32] (input-gradient kernel, zero-initialised by the caller). */
int tup_bra_compose(const float* wu, const float* bu, const float* w3, void* wv, float* bv, void* wp, void* wd, void* stream);
/* backward: g fp32 [B][3][2H][2W] (gradient w.r.t. upscaled_input, before its ReLU mask), ui fp32 [B][3][2H][2W], feat bf16
 * [B][H][W][64] -> dfeat bf16 [B][H][W][64] (written); G fp32 [16][9][12][25][64], Gb fp32 [16][9][12] = gradient w.r.t. the
 * composed weights / biases per variant, spread over 16 replicas against atomic contention (ACCUMULATED: zero first; the
 * gradient is the sum over the replicas); g12 bf16 [B][H][W][16] workspace.  H, W >= 6. */
int tup_bra_backward(const float* g, const float* ui, const void* feat, const void* wd, const void* wv,
                     void* g12, void* dfeat, float* G, float* Gb, int B, int H, int W, void* stream);
/* chain rule through the composition: G, Gb (16 replicas each, summed here) -> dwu fp32 [256][64][3][3], dbu fp32 [256], dw3 fp32 [3][64][3][3] (written);
 * dM fp32 [62208] and dMb fp32 [108] workspaces. */
int tup_bra_chain(const float* G, const float* Gb, const float* wu, const float* bu, const float* w3,
                  float* dM, float* dMb, float* dwu, float* dbu, float* dw3, void* stream);

/* transforms.Resize on a uint8 PIL image (reference data_handling/data_class.py:61-71, inference.py:65-75) = Pillow's two-pass
 * 8-bit BILINEAR resampler (third-party Pillow libImaging/Resample.c: triangle filter widened by the down-scale factor,
 * weights normalised in double and rounded to 22 fractional bits, out = clip8((2^21 + sum(pixel * k)) >> 22), horizontal pass
 * into a uint8 image first).  Bit-exact with Pillow.  Tables (device, int32) from resize_taps.pil_bilinear_coeffs:
 * min / size [out], k [out][ksize].
 * rows: src u8 [B][H][W][3] -> dst u8 [B][H][Wo][3]. */
int tup_resize_u8_rows(const void* src, void* dst, const int* xmin, const int* xsize, const int* k, int ksize,
                       int B, int H, int W, int Wo, void* stream);
/* cols: src u8 [B][H][W][3] -> dst_u8 u8 [B][Ho][W][3] (or NULL) and / or dst_f32 fp32 [B][3][Ho][W] = value / 255 (or NULL;
 * ToTensor fused, swap_rb = 1 for BGR frames). */
int tup_resize_u8_cols(const void* src, void* dst_u8, float* dst_f32, const int* ymin, const int* ysize, const int* k,
                       int ksize, int B, int H, int W, int Ho, int swap_rb, void* stream);

/* ---- image-quality metrics (reference inference.py:128-145 skimage SSIM / PSNR, ab_test.py:96-124 MSE; csrc/metrics.hip) ---- */

/* skimage.metrics.structural_similarity(a, b, data_range, channel_axis=-1) with its defaults (7x7 uniform window,
 * use_sample_covariance, K1 = 0.01, K2 = 0.03, mean over [3:H-3, 3:W-3]) and the sum of squared errors, in one pass, as
 * per-workgroup partials: partial fp64 [B][3][nparts][2] = {sum of SSIM, sum of squared errors} per image, channel and workgroup,
 * nparts = ceil((W - 6) / 250) * ceil((H - 6) / 96) (any other value, or H / W < 7, returns hipErrorInvalidValue).
 * f32: a, b fp32 planar [B][3][H][W]; window moments of data shifted by one constant per workgroup.
 * u8hwc: a, b uint8 [B][H][W][3]; integer window moments, fp64 formula; squared errors in the input's units. */
int tup_quality_f32_partial(const float* a, const float* b, double* partial, int B, int H, int W, int nparts,
                            float data_range, void* stream);
int tup_quality_u8hwc_partial(const void* a, const void* b, double* partial, int B, int H, int W, int nparts,
                              float data_range, void* stream);
/* The partials of either launcher -> out fp64 [6][B] = {mse, psnr = 10 log10(data_range^2 / mse) (+inf when mse == 0), ssim
 * (mean of the channels), ssim of channels 0, 1, 2}; each image's slots are added in index order in fp64 (no atomics), so an
 * image's result does not depend on the run or on the other images of the batch. */
int tup_quality_reduce(const double* partial, double* out, int B, int H, int W, int nparts, float data_range, void* stream);

/* ---- training loss on the scored quantities (transformerupscaler_amd/losses.py; csrc/quality_loss.hip) ----
 * loss = w_l1 * mean|x - y| + w_mse * mean (x - y)^2 + w_ssim * (1 - mean_b SSIM(x[b], y[b])), x, y fp32 planar [B][3][H][W],
 * SSIM as tup_quality_f32_partial defines it. */

/* out[0] (fp32, device) = the loss, from qpartial = the partials of tup_quality_f32_partial (read when w_mse or w_ssim != 0, else
 * may be NULL) and l1partial = the nl1 partials of tup_l1_loss_partial over the whole batch (read when w_l1 != 0, else may be NULL).
 * One workgroup: an image's slots are added as tup_quality_reduce adds them, then the images in index order, in fp64; no atomics. */
int tup_quality_loss_reduce(const double* qpartial, const float* l1partial, float* out, int B, int H, int W, int nparts, int nl1,
                            float w_l1, float w_mse, float w_ssim, void* stream);
/* grad (fp32 [B][3][H][W]) = gscalar[0] * d loss / d x  (gscalar: the upstream scalar gradient, on the device).  One streaming
 * pass (x and y read ~1.18 times, grad written once), no workspace, no atomics: a pixel's gradient depends on its own plane only.
 * With w_ssim == 0 an elementwise kernel runs instead.  H, W >= 7. */
int tup_quality_loss_f32_bwd(const float* x, const float* y, const float* gscalar, float* grad, int B, int H, int W,
                             float w_l1, float w_mse, float w_ssim, float data_range, void* stream);

/* nblk (<= 8) consecutive WindowTransformerBlocks in ONE launch (the loop `for block in self.window_blocks`, model.py:288-289; a block,
 * model.py:153-172, is x += proj(attention(qkv(norm1(x)))) followed by x += mlp.2(GELU(mlp.0(norm2(x))))), two waves per window (one
 * window per workgroup at <= 512 windows), two workgroups per CU.  The residual stream of a token tile stays in registers through a block;
 * between blocks it passes through memory as each wave's own stores followed by its own loads (L2), so the launch boundaries and their
 * chip-wide load / store bursts disappear.  x fp32 [64*nwin][192] (window layout) in place; table: HOST array [nblk][9] of device
 * pointers, per block (wh, bh, bias_frag, wproj, bproj, w1, b1, w2, b2).  norm1 / norm2's scale and shift arrive folded into attn.qkv /
 * mlp.0 (packing.fold_layernorm: W diag(gamma), b + W beta): wh bf16 [12][64][192] / bh fp32 [12][48] = pack_qkv_heads of the folded qkv
 * (per head the q, k, v weight rows, 16 each, + 16 zero rows); bias_frag from tup_relpos_bias_expand; wproj bf16 [192][192] from
 * packing.pack_proj_pairs (rows permuted per 64-group, columns in head-pair K order); w1 bf16 [768][192] / b1 = pack_fc1_fused_q of the
 * folded mlp.0 (x 1/4, exact powers of two; rows permuted per 64-group AND columns in the kernel's K order); w2 FP16 [192][768] =
 * 4 mlp.2.weight (pack_fc2_h4): erf-GELU (nn.GELU(), model.py:148) is evaluated in packed fp16 on x / 4 and FC2 runs on the fp16 MFMA,
 * the factors of 4 cancel. */
int tup_fused_blocks32_fwd(float* x, const void* const* table, int nblk, int nwin, void* stream);

/* The same loop (model.py:288-289; blocks :153-172) as the streamed 32x32x16-MFMA kernel (csrc/block_stream.hip): one workgroup of
 * eight waves carries four windows through all nblk blocks; LayerNorm / softmax / GELU instructions sit between the matrix
 * instructions of the same wave.  x fp32 [64*nwin][192]; out_bf16 = NULL: in place; out_bf16 != NULL: the result goes there as bf16
 * [64*nwin][192] (round to nearest even) and x is left holding the kernel's parked intermediate -- for tup_patch_unembed_fwd with
 * x_bf16 = 1, which then reads half the bytes for the same operand.  table: HOST array [nblk][7] of device pointers, per block the
 * tensors of packing.pack_stream_block: wqk bf16 [12][3][32][64], wv bf16 [6][3][32][64], wproj bf16 [6][3][32][64],
 * w1 bf16 [24][3][32][64], w2 fp16 [24][6][32][32], tab fp32 [1536], sbias fp32 [12][2][2][64][16]. */
int tup_blocks_stream_fwd(float* x, void* out_bf16, const void* const* table, int nblk, int nwin, void* stream);

/* Re-packing the weights after an optimizer step (training; replaces the torch index / permute / cat / cast calls of
 * packing.py that follow reference train.py:139 `optimizer.step()`): dst[i] = map[i] < 0 ? 0 : concat(src[0..nparam-1])[map[i]].
 * src: device array of nparam device pointers to the fp32 parameters; offs: device int [nparam + 1] prefix sum of their sizes;
 * map: device int [n] (built once by pack_plan.py from packing.py itself); dst: bf16 (to_bf16 != 0, round to nearest even) or fp32 [n]. */
int tup_pack_gather(const void* src, const int* offs, int nparam, const int* map, void* dst, long long n, int to_bf16, void* stream);

/* torch.optim.Adam's step (reference train.py:104,139; default betas / eps, no weight decay, no amsgrad) for all parameters in one
 * launch.  segs: device array [nseg] of 64-byte records {float* p; const float* g; float* m; float* v; long long n; float step_size
 * (= lr / bias_correction1), inv_sqrt_bc2 (= 1 / sqrt(bias_correction2)), beta2, 1 - beta1, 1 - beta2, eps}; chunks: device int [nchunks][2] =
 * (segment index, first element), one workgroup per 4096 elements.  p, m, v are updated in place. */
int tup_adam_step(const void* segs, const int* chunks, int nchunks, void* stream);

/* Gradient accumulation of a mixed-scale step (reference train.py:119-138: several samples, one optimizer step) for all parameters of
 * one backward in one launch.  segs: device array [nseg] of 32-byte records {float* dst; const float* src; long long n; float alpha;
 * int mode}; mode 0: dst = alpha * src, 1: dst = dst + alpha * src (alpha * src rounded first: with alpha == 1 a plain fp32 add),
 * 2: dst = 0 (src ignored, may be NULL); chunks: device int [nchunks][2] = (segment index, first element), one workgroup per 4096
 * elements.  16-byte accesses where dst and src are 16-byte aligned, scalar otherwise.  Segments must not overlap; no atomics. */
int tup_grad_accumulate(const void* segs, const int* chunks, int nchunks, void* stream);

/* The guarded optimizer step (csrc/step_guard.hip): GradScaler's skipping of steps with non-finite gradients (reference
 * train.py:136-139) and torch.nn.utils.clip_grad_norm_, decided on the device; at most three launches, no host synchronisation.
 *
 * tup_grad_sumsq_partial: segs: device array [nseg] of 16-byte records {const float* g; long long n}; chunks: device int [nchunks][2] =
 * (segment index, first element), one workgroup per 4096 elements; partials: device double [nchunks], partials[w] = the sum of
 * (double)g * (double)g over workgroup w's elements.  16-byte loads where g is 16-byte aligned, scalar otherwise.
 *
 * tup_grad_guard_finish: one workgroup sums partials[0 .. npartials) in a fixed order and writes the 64-byte guard record
 * {double sumsq, norm; float coef; int apply; float norm_f32; int clipped; unsigned long long steps, applied, clipped, skipped}:
 * coef = min(1, max_norm / (norm + 1e-6)) computed in double and rounded (1 when max_norm < 0: no clipping), apply = isfinite(sumsq)
 * || !skip_nonfinite, clipped = apply && coef < 1; the four running counters are incremented in place (zero the record once).
 * No floating-point atomics: the record is bitwise reproducible.
 *
 * tup_adam_step_guarded: tup_adam_step with weight decay, reading the guard record (NULL: apply, coef = 1).  segs: device array [nseg]
 * of 72-byte records {float* p; const float* g; float* m; float* v; long long n; float step_size (= lr / bias_correction1), bc2_sqrt
 * (= sqrt(bias_correction2)), beta2, 1 - beta1, 1 - beta2, eps, wd_l2 (g += wd_l2 * p, torch.optim.Adam; 0: none), decay (p *= decay,
 * = 1 - lr * weight_decay, torch.optim.AdamW; 1: none)}; chunks as for tup_adam_step.  apply == 0: p, m, v are not written; otherwise
 * the gradient is coef * g.  g itself is never written. */
int tup_grad_sumsq_partial(const void* segs, const int* chunks, int nchunks, double* partials, void* stream);
int tup_grad_guard_finish(const double* partials, int npartials, double max_norm, int skip_nonfinite, void* guard, void* stream);
int tup_adam_step_guarded(const void* segs, const int* chunks, int nchunks, const void* guard, void* stream);

/* The optimizer step with an exponential moving average of the weights in the same launch (csrc/step_guard.hip).  segs: device array
 * [nseg] of 88-byte records {float* p; const float* g; float* m; float* v; long long n; float step_size, bc2, beta2, 1 - beta1,
 * 1 - beta2, eps, wd_l2, decay; float* e; float ema_w; int form}.  form 0: p, m, v are updated with tup_adam_step's arithmetic (bc2 =
 * 1 / sqrt(bias_correction2); wd_l2 and decay are not read), form 1: with tup_adam_step_guarded's (bc2 = sqrt(bias_correction2)); in
 * both they come out bit-equal to that entry's.  Then e = e + ema_w * (p - e) on the new p, as three separately rounded fp32
 * operations (sub, mul, add).  g == NULL: the parameter has no gradient in this step; e alone is updated, p is only read, m and v
 * are not touched.  chunks as for tup_adam_step; guard as for tup_adam_step_guarded (NULL: apply, coef = 1); apply == 0: p, m, v
 * and e are not written.  e must not overlap p, g, m or v. */
int tup_adam_step_ema(const void* segs, const int* chunks, int nchunks, const void* guard, void* stream);

/* Patch training samples of a whole batch in one launch (data.PatchSampler; csrc/patch_pairs.hip).  recs: device array [B] of 32-byte
 * records {const uint8_t* frame; int H; int W; int y0; int x0; int op; int reserved}, frame a contiguous uint8 [H][W][3] RGB image.
 * Per record, bit-exact: t = frame[y0:y0+P, x0:x0+P]; op & 1: t = t[:, ::-1]; op & 2: t = t[::-1]; op & 4: t = t.transpose(1, 0, 2)
 * (in that order); hr = ToTensor(t) = (float)v / 255.0f; lr = ToTensor(Image.resize((p, p), BILINEAR)(t)), Pillow's 8-bit two-pass
 * resampler as tup_resize_u8_rows / _cols state it, the horizontal pass over the TRANSFORMED image rounded to uint8 first.
 * P = p * s is the HR and p the LR patch side; xmin / xsize int32 [p], k int32 [p][ksize] = resize_taps.pil_bilinear_coeffs(P, p)
 * serve both passes; hr fp32 [B][3][P][P], lr fp32 [B][3][p][p], both in [0, 1].  One workgroup per 16 x 16 LR tile and sample; the
 * uint8 intermediate stays in LDS; one writer per output element, no atomics, no workspace.  A record whose box leaves its frame
 * or whose op is outside [0, 8) is skipped (its outputs are not written): validate on the host.  B <= 0: no-op.  B > 65535,
 * ksize < 1, P < p, p < 1, P not a multiple of p, or a window beyond 64 KiB of LDS (s > 8): hipErrorInvalidValue. */
int tup_patch_pairs(const void* recs, int B, int P, int p, const int* xmin, const int* xsize, const int* k, int ksize,
                    float* hr, float* lr, void* stream);

/* Training degradations of a whole batch in one launch (data.PatchSampler(degrade=...); csrc/degrade.hip).  in / out fp32
 * [B][3][H][W], any H, W >= 1; recs: device array [B] of 32-byte records {int taps[4]; int noise_amp; uint32_t noise_seed; int quality;
 * int flags}.  Per record, in integers, bit-exact against tests/_degrade_ref.py:
 *   u = clip(floor(v * 255.0f + 0.5f), 0, 255), both operations rounded to fp32;
 *   blur: 7 symmetric taps {k3 k2 k1 k0 k1 k2 k3} in 22-bit fixed point (k0 + 2 (k1 + k2 + k3) == 1 << 22), the horizontal pass and
 *     then the vertical pass, each clip8((sum k u + (1 << 21)) >> 22), indices clamped to the image; {1 << 22, 0, 0, 0} is the identity;
 *   noise: h = drop_hash(noise_seed, e), e = (y W + x) 3 + c, or y W + x with flags & 1; n = the sum of h's four bytes - 510;
 *     u = clip(u + ((n noise_amp + (1 << 15)) >> 16), 0, 255); noise_amp = 0 is off;
 *   JPEG round trip, quality in 1..100 (0 is off): baseline 4:4:4, Annex K tables scaled as jpeg_set_quality does, the image padded
 *     to multiples of 8 by replication, libjpeg's 16-bit RGB <-> YCbCr and its slow integer DCT (jfdctint / jidctint) both ways,
 *     quantised as sign(c) ((|c| + 4 t) / (8 t)); what Pillow's save(quality=q, subsampling=0) and open().convert("RGB") return;
 *   out = (float)u / 255.0f.
 * One workgroup per 32 x 32 tile and sample, everything between the load and the store in LDS; one writer per output element, no
 * atomics, no workspace.  A quality outside 0..100 is treated as 0 and other flag bits are ignored: validate on the host.
 * A null pointer, B, H or W <= 0, B > 65535, or out overlapping in (a tile reads its neighbours): hipErrorInvalidValue. */
int tup_degrade_lr(const float* in, const void* recs, int B, int H, int W, float* out, void* stream);

/* tup_degrade_lr for records of which some carry flags & 4 (ops.DEGRADE_JPEG_420; csrc/degrade420.hip): the JPEG round trip
 * of such a sample is baseline 4:2:0, what Pillow's save(quality=q, subsampling=2) and open().convert("RGB") return, bit-exact against
 * tests/_degrade420_ref.py:
 *   luma as at 4:4:4; Cb and Cr averaged over 2 x 2 pixels, d = (p00 + p01 + p10 + p11 + 1 + (downsampled column & 1)) >> 2, the last
 *     pixel column replicated up to the 16-pixel MCU width, pixel rows only from H to H + (H & 1), the downsampled plane then
 *     replicated downwards to a multiple of 8 (libjpeg's asymmetry); DCT, chroma table and inverse DCT per 8 x 8 block of samples;
 *   the ceil(H/2) x ceil(W/2) real samples upsampled by the decoder's triangle filter: rows 3 : 1 with the nearer row, then columns
 *     (3 s + before + 8) >> 4 and (3 s + after + 7) >> 4, neighbours clamped to the real samples; W <= 4: each sample replicated 2 x 2.
 * Blur and noise are unchanged and come first; the noise index stays the absolute pixel index.  All samples go through ONE launch, a
 * workgroup per 32 x 32 tile and sample: with the flag it works on the 64 x 64 pixels around its tile (the MCUs the filter reaches into),
 * without it it runs tup_degrade_lr's stages and writes what tup_degrade_lr writes, bit for bit.  The flag with a quality outside
 * 1..100 is ignored: validate on the host.  Capturable; one writer per output element, no atomics, no workspace.  Refusals as
 * tup_degrade_lr: a null pointer, B, H or W <= 0, B > 65535, or out overlapping in: hipErrorInvalidValue. */
int tup_degrade_lr_sub(const float* in, const void* recs, int B, int H, int W, float* out, void* stream);

/* Baseline JPEG (SOF0) of a whole batch on the GPU (ops.jpeg_encode; csrc/jpeg_encode.hip).  The file of image b is byte
 * for byte what Pillow's save(format="JPEG", quality, subsampling, restart_marker_rows=restart_rows) writes: standard Huffman tables,
 * a restart interval of restart_rows MCU rows; tests/_jpeg_ref.py states it in numpy.  subsampling: 0 = 4:4:4, 2 = 4:2:0.  Exactly
 * one of frames_u8 (uint8 [B][H][W][3], RGB) and frames_f32 (fp32 [B][3][H][W], quantised as tup_f32chw_to_u8hwc does) is given.
 * Three launches, each with a workgroup per (restart segment, image) or per image, all capturable, no host synchronisation:
 *   tup_jpeg_sizes    sizes int32 [B][S] <- the bytes of every restart segment, stuffed zeros and closing marker included;
 *   tup_jpeg_offsets  offsets int32 [B][S] <- header_len + the sizes before; lengths int32 [B] <- the file's length, or -1 where it
 *                     exceeds `capacity`, the bytes of one image's row of `data`;
 *   tup_jpeg_write    data uint8 [B][capacity] <- header (header_len bytes on the device, SOI .. SOS, built by the caller from the
 *                     same parameters), scan and EOI of every image whose length is not -1; nothing is written past a row.
 * S = tup_jpeg_segments(H, W, subsampling, restart_rows) (returns a count, not an error code), or -1 for what the encoder refuses:
 * H or W outside 1..65535, another subsampling, restart_rows < 1, a restart interval above 65535 MCUs.  Those, a null pointer, both or
 * neither frame pointers, B outside 1..65535, quality outside 1..100, S not the count above, capacity outside 0..2^31-1:
 * hipErrorInvalidValue. */
int tup_jpeg_segments(int H, int W, int subsampling, int restart_rows);
int tup_jpeg_sizes(const void* frames_u8, const float* frames_f32, int B, int H, int W, int quality, int subsampling, int restart_rows,
                   int* sizes, void* stream);
int tup_jpeg_offsets(const int* sizes, int B, int S, int header_len, long long capacity, int* offsets, int* lengths, void* stream);
int tup_jpeg_write(const void* frames_u8, const float* frames_f32, int B, int H, int W, int quality, int subsampling, int restart_rows,
                   const void* header, int header_len, const int* offsets, const int* lengths, void* data, long long capacity, void* stream);

/* Baseline JPEG (SOF0) files of a whole batch decoded on the GPU (ops.jpeg_decode; csrc/jpeg_decode.hip).  The pixels of
 * image b are what Pillow's Image.open(file).convert("RGB") returns; tests/_jpeg_decode_ref.py states it in numpy.  The caller parses
 * the marker segments and uploads
 *   records  B x 1488 bytes, per image {int32 scan_off (a multiple of 16, into `scans`), int32 scan_len (the bytes between SOS and
 *            EOI), uint8 td[4], ta[4] (each component's DC / AC Huffman table, 0 or 1), uint16 qt[3][64] (each component's
 *            quantisation table, natural order), uint8 huff[4][272] (DC 0, DC 1, AC 0, AC 1 as DHT carries them: 16 counts, then
 *            the symbols, zero filled)};
 *   scans    scans_bytes bytes (at most 0x7fff0000), 16-byte aligned, each scan padded to a multiple of 16 bytes.
 * All images share H, W, layout (0 = 4:4:4, 2 = 4:2:0, 4 = one component) and restart_interval in MCUs (0 = none).  Three launches,
 * all capturable, no host synchronisation:
 *   tup_jpeg_decode_index   segs int32 [B][S][8] <- the walker's state at the start of every segment (a restart interval, or an MCU
 *                           row where the file has none: found by one serial walk per image, or in parallel by
 *                           tup_jpeg_decode_index_sync in its place); status int32 [B] <- 0, or non-zero for a scan that does not
 *                           decode completely;
 *   tup_jpeg_decode_blocks  workspace uint8 [B][ws_bytes] <- the Y (Cb, Cr) sample planes padded to whole MCUs, ws_bytes = their
 *                           bytes for one image; status[b] <- non-zero where a segment's walk stops early;
 *   tup_jpeg_decode_finish  exactly one of out_u8 (uint8 [B][H][W][3], RGB) and out_f32 (fp32 [B][3][H][W] = byte / 255) <- the
 *                           pixels: fancy upsampling where 4:2:0, colour conversion, crop.
 * Any bytes are safe: nothing is read outside an image's scan or written outside its workspace and output; the pixels of an image
 * with a non-zero status are unspecified.  S = tup_jpeg_decode_segments(H, W, layout, restart_interval) (returns a count, not an
 * error code), or -1 for what the decoder refuses: H or W outside 1..65535, another layout, an interval outside 0..65535.  Those, a
 * null or misaligned pointer, both or neither outputs, B outside 1..65535, S or ws_bytes other than the geometry's:
 * hipErrorInvalidValue. */
int tup_jpeg_decode_segments(int H, int W, int layout, int restart_interval);
int tup_jpeg_decode_index(const void* records, const void* scans, long long scans_bytes, int B, int H, int W, int layout,
                          int restart_interval, int S, int* segs, int* status, void* stream);
/* tup_jpeg_decode_index for images without a restart interval as a parallel pass (csrc/jpeg_sync.hip): self-synchronising Huffman
 * decoding over subsequences of 132 raw bytes, a workgroup per image, one launch whatever the data.  segs int32 [B][S][8] with
 * S = tup_jpeg_decode_segments(H, W, layout, 0) and status are what tup_jpeg_decode_index(restart_interval = 0) gives, except that a
 * record of an image that decodes completely may hold another reader state (byte, bits, their number) for the same bit of the scan; a
 * damaged or short scan is walked serially in the same launch and its records are word for word the serial index's.  rounds int32 [B],
 * or null: the sync rounds each image took, at most its number of subsequences. */
int tup_jpeg_decode_index_sync(const void* records, const void* scans, long long scans_bytes, int B, int H, int W, int layout, int* segs,
                               int* status, int* rounds, void* stream);
int tup_jpeg_decode_blocks(const void* records, const void* scans, long long scans_bytes, int B, int H, int W, int layout,
                           int restart_interval, int S, const int* segs, int* status, void* workspace, long long ws_bytes, void* stream);
int tup_jpeg_decode_finish(const void* workspace, long long ws_bytes, int B, int H, int W, int layout, void* out_u8, float* out_f32,
                           void* stream);

/* PNG files (8-bit RGB, colour type 2, no interlace) of a whole batch made on the GPU (ops.png_encode; csrc/png_encode.hip).
 * The filtered stream of an image, H * (1 + 3 W) bytes, is cut every block_bytes bytes (256..32768); each range is one deflate block
 * on a byte boundary in an IDAT chunk of its own, which is what a workgroup codes.  Exactly one of frames_u8 (uint8 [B][H][W][3], RGB)
 * and frames_f32 (fp32 [B][3][H][W], quantised as tup_f32chw_to_u8hwc does) is given.  filter: 0 none, 1 sub, 2 up, 3 average,
 * 4 paeth for every row, 5 adaptive (the smallest sum of |residual| per row; `filters` is then tup_png_filters' output, otherwise unused).
 *   tup_png_filters   filters uint8 [B][H] <- the filter of every row;
 *   tup_png_sizes     sizes int32 [B][N] <- the bytes every block adds to the file (chunk framing included; the last block's count
 *                     includes the Adler-32 chunk and IEND); partials int32 [B][N] <- the block's Adler-32 partial;
 *   tup_png_offsets   offsets int32 [B][N] <- 33 + the sizes before; lengths int32 [B] <- the file's length, or -1 where it exceeds
 *                     `capacity`, the bytes of one image's row of `data`; adlers int32 [B] <- the Adler-32 of the filtered stream;
 *   tup_png_write     data uint8 [B][capacity] <- the whole file of every image whose length is not -1; nothing is written past a row.
 * N = tup_png_blocks(H, W, block_bytes) (returns a count, not an error code), or -1 for what the encoder refuses: H or W below 1,
 * H * (1 + 3 W) from 2^31, block_bytes outside 256..32768.  Those, a null pointer, both or neither of the inputs, B outside 1..65535, a
 * filter outside 0..5 or a capacity outside 0..2^31 - 1 are hipErrorInvalidValue before any launch. */
int tup_png_blocks(int H, int W, int block_bytes);
int tup_png_filters(const void* frames_u8, const float* frames_f32, int B, int H, int W, void* filters, void* stream);
int tup_png_sizes(const void* frames_u8, const float* frames_f32, int B, int H, int W, int filter, int block_bytes, const void* filters,
                  int* sizes, int* partials, void* stream);
int tup_png_offsets(const int* sizes, const int* partials, int B, int H, int W, int block_bytes, long long capacity, int* offsets,
                    int* lengths, int* adlers, void* stream);
int tup_png_write(const void* frames_u8, const float* frames_f32, int B, int H, int W, int filter, int block_bytes, const void* filters,
                  const int* offsets, const int* lengths, const int* adlers, void* data, long long capacity, void* stream);

/* The same encoder for 16-bit files: IHDR bit depth 16, colour type 2, samples big-endian, bpp = 6, a row of 1 + 6 W filtered bytes
 * (filters work on bytes, the left neighbour is 6 bytes back), refused from H * (1 + 6 W) = 2^31.  frames_u16 is uint16 [B][H][W][3]
 * in the machine's byte order (an even address); frames_f32 fp32 [B][3][H][W] is quantised inside the kernels, with no intermediate
 * frame, by q_16: t = x * 65535, NaN -> 0, clamp to [0, 65535], (int)(t + 0.5f) -- round to nearest, where the 8-bit entries
 * truncate.  Ranges, tokens, code lengths, block forms, chunks, CRC and Adler are those of the 8-bit file; every other argument,
 * workspace and refusal is as for its tup_png_* twin (same kernels, instantiated for two-byte samples).  tests/_png16_ref.py states
 * the file. */
int tup_png16_blocks(int H, int W, int block_bytes);
int tup_png16_filters(const void* frames_u16, const float* frames_f32, int B, int H, int W, void* filters, void* stream);
int tup_png16_sizes(const void* frames_u16, const float* frames_f32, int B, int H, int W, int filter, int block_bytes, const void* filters,
                    int* sizes, int* partials, void* stream);
int tup_png16_offsets(const int* sizes, const int* partials, int B, int H, int W, int block_bytes, long long capacity, int* offsets,
                      int* lengths, int* adlers, void* stream);
int tup_png16_write(const void* frames_u16, const float* frames_f32, int B, int H, int W, int filter, int block_bytes, const void* filters,
                    const int* offsets, const int* lengths, const int* adlers, void* data, long long capacity, void* stream);

/* PNG files (8 bits a sample, colour types 0, 2, 3, 4, 6, no interlace) of a whole batch decoded on the GPU (ops.png_decode;
 * csrc/png_decode.hip).  The pixels of image b are what Pillow's Image.open(file).convert("RGB") returns: grey R = G = B,
 * alpha dropped, palette looked up (an index past PLTE is black); tests/_png_decode_ref.py states it.  The caller walks the chunks
 * (ops.png_parse) and passes `records`, B records of 784 bytes {int32 offset of the image's zlib stream in `streams` (a multiple of
 * 16), int32 its length, int32 colour type, int32 bytes per pixel of the filtered stream (1, 3, 1, 2, 4 for the five types), the
 * palette as 256 x 3 bytes, zero-filled}, and `streams`, streams_bytes bytes: every image's IDAT payloads joined without chunk
 * framing, each image's area padded to a multiple of 16.  All images share H and W; `channels` is the most bytes per pixel of any of
 * them and sizes the workspace.
 *   tup_png_decode_inflate  workspace uint8 [B][ws_bytes] <- the filtered stream, H rows of 1 + bytes-per-pixel W bytes; status int32
 *                           [B] <- 0 for a stream that inflates to exactly that many bytes with the right Adler-32, otherwise the
 *                           first error in stream order: 1 block type 3, 2 stored LEN / NLEN, 3 a code RFC 1951 forbids, 4 bits that are
 *                           no symbol's code, 5 a distance before the start, 6 input exhausted (or a record that points outside
 *                           `streams`), 7 output too long, 8 output too short, 10 Adler-32 mismatch.  walk: 0 one token a round, 1 a
 *                           wave of token candidates a round; frames and status are the same bits;
 *   tup_png_decode_finish   exactly one of out_u8 (uint8 [B][H][W][3], RGB) and out_f32 (fp32 [B][3][H][W] = byte / 255) <- the
 *                           pixels, filters undone; status <- 9 where it was 0 or 10 and a row's filter byte is above 4.
 * The pixels of an image with a non-zero status are unspecified; nothing is read outside its stream or written outside its
 * workspace and frame.  ws_bytes = tup_png_decode_workspace(H, W, channels) (returns a byte count, not an error code), or -1 for what
 * the decoder refuses: H or W below 1, channels outside 1..4, H * (1 + 4 W) or ws_bytes from 2^31.  Those, another ws_bytes, B outside 1..65535,
 * a walk outside 0..1, and both or neither of the outputs are hipErrorInvalidValue before any launch. */
int tup_png_decode_workspace(int H, int W, int channels);
int tup_png_decode_inflate(const void* records, const void* streams, long long streams_bytes, int B, int H, int W, int channels, int walk,
                           void* workspace, long long ws_bytes, int* status, void* stream);
int tup_png_decode_finish(const void* records, void* workspace, long long ws_bytes, int B, int H, int W, int channels, void* out_u8,
                          float* out_f32, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TUPSCALE_HIP_H */
