/* vpt_hip.h -- C ABI of libvpt_hip.so: the MI355X (gfx950) kernels behind the VPT policy hot path.
 *
 * The reference (openai/Video-Pre-Training) has no FFI of its own: its hot path is PyTorch ATen calls made
 * from lib/policy.py, lib/impala_cnn.py, lib/util.py, lib/xf.py, lib/masked_attention.py and
 * lib/action_head.py.  Each entry point below replaces one such group of calls (cited per function); the
 * Python host side (video-pre-training_amd/lib/policy.py) binds them with ctypes and keeps the reference's
 * MinecraftAgentPolicy API on top.  See INTEGRATION.md for the binding a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (inputs, outputs, KV memory, workspaces);
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*; NULL = default stream):
 *     no allocation, no synchronisation, no global state besides the last-error string;
 *   - return 0 on success, <0 on a rejected argument or a launch failure (vpt_last_error() explains);
 *   - "blocked" activations are bf16 [frames][C/32][H][W][32]; "stats" are double[frames][2] holding the
 *     running (sum, sum of squares) of a frame, accumulated with atomics -- the caller zeroes them;
 *   - packed weight formats are produced by the vpt_pack_* / vpt_chw_to_blocked entry points below from the
 *     reference's fp32 tensors: a host without torch can prepare a model (video-pre-training_amd/packing.py is the CPU restatement
 *     the tests compare them with, bit for bit).
 */
#ifndef VPT_HIP_H
#define VPT_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Library / build identification: returns "vpt_hip <version> gfx950". */
const char* vpt_version(void);
/* Binary-interface number of THIS header (VPT_HIP_ABI).  It is raised whenever an existing entry point changes its argument
 * list or a symbol is renamed or removed (adding entry points does not raise it); a caller compares it with the VPT_HIP_ABI it
 * was built against before the first call -- _native.py does -- instead of finding out through a mis-typed argument.
 * History: 3 = round 3 (vpt_adam_step_multi + skip_flag, vpt_heads_logprob_backward + grad_scale, vpt_gate_cast renamed);
 * 4 = round 4 (vpt_conv3x3_forward_tiled rejects tiling 0; vpt_action_head_forward takes a counter-based noise source).
 * Entry points added under 5 without a change of number, by the rule above: vpt_grad_accumulate_multi, vpt_augment_*, vpt_rollout_record / _reward (a
 * binding that requires one of them refuses a library that lacks it by name, _native.py). */
#define VPT_HIP_ABI 5
int vpt_abi_version(void);
/* "bf16" (libvpt_hip.so, the default) or "fp16" (libvpt_hip_f16.so: the same sources built with -DVPT_OPERAND_F16): the format
 * of every 16-bit buffer this library reads or writes -- activations, packed weights, MFMA operands.  Same ABI, same
 * MFMA rate; the fp16 build is the parity mode (8x finer operand rounding; lib/policy.py: precision="fp16"). */
const char* vpt_operand_format(void);
/* Human-readable reason for the most recent non-zero return on this thread. */
const char* vpt_last_error(void);

/* ---- weight re-packing (the `.weights` state_dict, fp32, reference shapes -> what the kernels stream) ------------------
 * A host needs nothing else to prepare a model: sizes from the queries, then one launch per layer.
 *   vpt_pack_conv3x3: Conv2d weight [Cout][Cin][3][3] of a FanInInitReLULayer with GroupNorm(1, Cin) (lib/util.py:58-82,
 *     lib/impala_cnn.py:30-52,86-97) -> wpk (16-bit, vpt_conv3x3_packed_elems elements: round(W * gain) in the swizzled LDS
 *     image of vpt_conv3x3_forward) and, when edge_sa / edge_sg are given (forward use; both or neither), the tables of the
 *     GroupNorm fold (vpt_conv3x3_table_floats floats each).  For vpt_conv3x3_dgrad pass the transposed, spatially flipped
 *     weight, gain = ones, no tables.
 *   vpt_pack_linear: nn.Linear weight [N][K] (row stride ldw) -> [ceil(N/128)][K/32][128][32] 16-bit, rows >= N zero,
 *     K % 64 == 0.  With transposed = 1 the packed matrix is the TRANSPOSE of a [src_rows][ldw] source (element (n, k) =
 *     source[k][n], zero for k >= src_rows): the operand of the input-gradient GEMM dx = dy W, with the reduction dimension
 *     (the layer's output width) padded to K.
 *   vpt_pack_conv_first: stack-0 firstconv weight [Cout][3][3][3] + bias [Cout] (lib/impala_cnn.py:86-97 with lib/util.py:64-65: no
 *     norm => bias) -> the MFMA A-operand fragments vpt_conv_first_forward / _backward read (16-bit, vpt_conv_first_packed_elems):
 *     W / 255 (the pixel operand is the raw byte; ImgPreprocessing's x / 255, lib/policy.py:39-45, is folded in here) and the bias
 *     as two 16-bit halves in the spare K slots.
 *   vpt_pack_conv3d_t5: IDM Conv3d weight [O][3][5][1][1] + bias [O] (lib/policy.py:364-372) -> fragments (16-bit,
 *     vpt_conv3d_t5_packed_elems) + the bias zero-padded to ceil(O/128)*128 floats.
 *   vpt_chw_to_blocked: fp32 [rows][C*H*W] in the reference's C,H,W flatten order (lib/impala_cnn.py:192-193) -> the blocked
 *     activation order [rows][C/32][H][W][32]: the dense layer's weight columns (rows = 256) and its LayerNorm gain / bias
 *     (rows = 1) before vpt_pack_linear / vpt_frame_affine_forward.  Out of place. */
long vpt_conv3x3_packed_elems(int Cout, int Cin);
long vpt_conv3x3_table_floats(int Cout);
long vpt_linear_packed_elems(int N, int K);
long vpt_conv_first_packed_elems(int Cout);
long vpt_conv3d_t5_packed_elems(int O);
int vpt_pack_conv_first(const float* weight, const float* bias, void* wfrag, int Cout, void* stream);
int vpt_pack_conv3d_t5(const float* weight, const float* bias, void* wfrag, float* bias_padded, int O, void* stream);
int vpt_chw_to_blocked(const float* src, float* dst, int64_t rows, int C, int H, int W, void* stream);

/* Workspace query: bytes of caller-owned scratch for the entry points that take a `scratch` / partial-sum buffer.
 *   VPT_WS_CONV3X3_WGRAD         (frames, -, -, Cin, Cout)   vpt_conv3x3_wgrad's scratch
 *   VPT_WS_CONV_BACKWARD_PREPARE (frames, -, -, -, Cout)     scratch of vpt_conv_backward_prepare / _prepare_pooled / _reduce
 *   VPT_WS_LINEAR_SPLITK         (splitk, M, N, -, -)        the [splitk][M][N] fp32 slices vpt_linear_forward writes when splitk > 1
 *   VPT_WS_LAYERNORM_BACKWARD    (M, D, -, -, -)             vpt_layernorm_backward's partials
 *   VPT_WS_COLUMN_SUM            (M, N, -, -, -)             vpt_column_sum's partials (0: none needed)
 *   VPT_WS_ATTENTION_BACKWARD_DKV  (B, t, hid, -, -)         vpt_masked_attention_backward's dkv_slab
 *   VPT_WS_ATTENTION_BACKWARD_DBND (B, t, heads, maxlen, -)  ... and its dbnd_slab
 *   VPT_WS_FRAME_AFFINE_BACKWARD (frames, HW, per_element, pass, C)   vpt_frame_affine_backward's partials for that pass
 *   VPT_WS_CONV_FIRST_BACKWARD   (frames, H, W, -, Cout)     vpt_conv_first_backward's partials (depends on the device's CU count)
 *   VPT_WS_BC_LOSS               (M, -, -, -, -)             vpt_bc_loss's / vpt_idm_loss's workspace (the record slab + its reduction scratch)
 *   VPT_WS_FULL_ATTENTION_BACKWARD (B, t, hid, -, -)         vpt_full_attention_backward's dkv_slab (one slot per 32-query tile)
 *   VPT_WS_CONV3D_T5_BACKWARD    (frames, H, W, -, Cout)     vpt_conv3d_t5_backward's partials (one slab row per workgroup + the reduction's scratch)
 *   VPT_WS_RL_LOSS               (M, -, -, -, -)             vpt_rl_loss's workspace (the [M][16] record slab + its reduction scratch)
 *   VPT_WS_PPG_AUX_LOSS          (M, -, -, -, -)             vpt_ppg_aux_loss's workspace (the [M][8] record slab + its reduction scratch)
 * Returns -1 for an unknown op. */
enum { VPT_WS_CONV3X3_WGRAD = 1, VPT_WS_CONV_BACKWARD_PREPARE = 2, VPT_WS_LINEAR_SPLITK = 3, VPT_WS_LAYERNORM_BACKWARD = 4, VPT_WS_COLUMN_SUM = 5,
       VPT_WS_ATTENTION_BACKWARD_DKV = 6, VPT_WS_ATTENTION_BACKWARD_DBND = 7, VPT_WS_FRAME_AFFINE_BACKWARD = 8, VPT_WS_CONV_FIRST_BACKWARD = 9,
       VPT_WS_BC_LOSS = 10, VPT_WS_FULL_ATTENTION_BACKWARD = 11, VPT_WS_CONV3D_T5_BACKWARD = 12, VPT_WS_RL_LOSS = 13,
       VPT_WS_PPG_AUX_LOSS = 14 };
int64_t vpt_workspace_bytes(int op, int frames, int H, int W, int Cin, int Cout);
int vpt_pack_conv3x3(const float* weight, const float* gain, const float* bias, void* wpk, float* edge_sa, float* edge_sg,
                     int Cout, int Cin, void* stream);
int vpt_pack_linear(const float* weight, void* wpk, int N, int K, int transposed, int ldw, int src_rows, void* stream);

/* Stack-0 firstconv + ingest + ReLU + max-pool.
 * Replaces ImgPreprocessing.forward (lib/policy.py:39-45), the permute at lib/impala_cnn.py:190,
 * CnnDownStack.firstconv of stack 0 (lib/impala_cnn.py:86-97,115) and F.max_pool2d (lib/impala_cnn.py:117).
 * img: uint8 [frames][H][W][3]; wfrag: bf16 [NT][4][2][64][8]; y: blocked [frames][Cout/32][H/2][W/2][32].
 * out_gain (optional, [Cout], Cout <= 256): y is stored multiplied by it per channel -- the gain of the stack's GroupNorm `n` when that norm is
 * folded into the first block (vpt_nfold_coef); stats_out always holds the statistics of the UNscaled pooled tensor.
 * chs_out (optional, [frames][Cout][2] fp64, ACCUMULATED, Cout <= 128): per-channel (sum, sum of squares) of y as stored -- what
 * vpt_channel_stats would compute in a pass of its own; here the sums run in registers across the tiles of a frame. */
int vpt_conv_first_forward(const uint8_t* img, const void* wfrag, void* y, double* stats_out, const float* out_gain, double* chs_out,
                           int frames, int H, int W, int Cout, void* stream);

/* IDM temporal conv + ingest + bias + ReLU.
 * Replaces ImgPreprocessing.forward (lib/policy.py:39-45) and InverseActionNet._conv3d_forward
 * (lib/policy.py:394-403: Conv3d(3->Cout, kernel (5,1,1), padding (2,0,0)) over time, then ReLU).
 * img: uint8 [frames = B*T][H][W][3]; wfrag: bf16 [NT][4][64][8]; bias fp32 [NT*128];
 * y: blocked [frames][Cout/32][H][W][32]; stats_out (optional) receives the statistics of y. */
int vpt_conv3d_t5_forward(const uint8_t* img, const void* wfrag, const float* bias, void* y, double* stats_out,
                          int frames, int T, int H, int W, int Cout, void* stream);

/* Backward of vpt_conv3d_t5_forward w.r.t. its weight and bias (InverseActionNet._conv3d_forward, lib/policy.py:394-403; the input is the uint8
 * image, so there is no input gradient).  y is the forward's STORED output and supplies the ReLU gate, dy the gradient w.r.t. it (both blocked
 * [frames][Cout/32][H][W][32]); with g = dy * [y > 0]:
 *   dw[o][c][dt] += (1/255) sum_{f,p} g[f][p][o] * img[f + dt - 2][p][c]   (a tap outside frame f's own sequence of T frames reads zero),
 *   db[o]        += sum_{f,p} g[f][p][o]
 * dw fp32 [Cout][3][5] (the layout of conv3d_layer.layer.weight [Cout,3,5,1,1]), db fp32 [Cout]; both accumulated (caller zeroes).  The products are
 * exact in fp32; per-workgroup partial sums go to `partials` (VPT_WS_CONV3D_T5_BACKWARD (frames, H, W, -, Cout) bytes) and are added in a fixed
 * order: no atomics, the same inputs give the same bits.  H*W % 256 == 0, Cout % 32 == 0, Cout <= 128, frames % T == 0. */
int vpt_conv3d_t5_backward(const uint8_t* img, const void* y, const void* dy, float* dw, float* db, float* partials,
                           int frames, int T, int H, int W, int Cout, void* stream);

/* The same temporal conv with every output frame ("slot") addressed through an index: slot j is centred on img[src[j]], and tap
 * dt = 0..4 reads img[src[j] + dt - 2] iff lo[j] <= src[j] + dt - 2 < hi[j], zeros otherwise -- the zero padding of
 * InverseActionNet._conv3d_forward (lib/policy.py:394-403, padding (2,0,0)) at the edges of whichever window [lo, hi) of a longer
 * video the slot stands for, without copying that window's pixels (run_inverse_dynamics_model.py:146-163 and
 * inverse_dynamics_model.py:74-95 copy and run one window at a time).  One arithmetic with vpt_conv3d_t5_forward: a slot with
 * src = f, [lo, hi) = the sequence of frame f gets the bits that entry point gives frame f.
 * img: uint8 [img_frames][H][W][3]; src, lo, hi: int32 [slots] ([lo, hi) is clipped to [0, img_frames)); y: blocked
 * [slots][Cout/32][H][W][32]; stats_out (optional, [slots][2]) receives the statistics of y. */
int vpt_conv3d_t5_forward_indexed(const uint8_t* img, const int32_t* src, const int32_t* lo, const int32_t* hi, const void* wfrag, const float* bias,
                                  void* y, double* stats_out, int slots, int img_frames, int H, int W, int Cout, void* stream);

/* GroupNorm(1,Cin) -> Conv2d(3x3, pad 1, no bias) -> ReLU [-> + residual].
 * Replaces FanInInitReLULayer.forward (lib/util.py:75-82) for conv layers and the residual add of
 * CnnBasicBlock.forward (lib/impala_cnn.py:50-52).  x, res, y blocked bf16; wpk bf16 [NT][Cin/32][9][128][32];
 * edge_sa / edge_sg fp32 [9][NT*128]; stats_in = statistics of x; stats_out (optional) receives those of y. */
int vpt_conv3x3_forward(const void* x, const void* wpk, const float* edge_sa, const float* edge_sg,
                        const double* stats_in, const void* res, void* y, double* stats_out,
                        int frames, int H, int W, int Cin, int Cout, void* stream);
/* The same call with the workgroup tiling named by the caller: 1 = the throughput kernel (16x16 pixels x 128 output channels per
 * workgroup: batches of frames, what bench.py measures and what vpt_conv3x3_forward always runs), 2 = the latency kernel (x 32
 * output channels: 4x the workgroups, a quarter of the serial MFMA chain each -- the acting path of agent.py:190-206, where one
 * frame would otherwise occupy 2-32 of the 256 CUs), 3 = the throughput kernel on 32x16-pixel tiles with eight waves where H % 32 == 0
 * (one weight fetch per 512 pixels; bit-identical outputs, measured at parity with 1 -- kept for A/B measurements).  Any other value
 * is an error: the tiling is never derived from the grid size (a frame's result must not depend on how many frames share a launch).
 * Same layouts, same arithmetic, same K order. */
int vpt_conv3x3_forward_tiled(const void* x, const void* wpk, const float* edge_sa, const float* edge_sg,
                              const double* stats_in, const void* res, void* y, double* stats_out,
                              int frames, int H, int W, int Cin, int Cout, int tiling, void* stream);

/* The same layer FUSED with the max-pool that follows it in CnnDownStack.forward (lib/impala_cnn.py:114-117: x = firstconv(x);
 * x = F.max_pool2d(x, 3, 2, 1)) -- stacks 1.., inference: pooled [frames][Cout/32][H/2][W/2][32] and its frame statistics come out, the
 * pre-pool tensor never reaches HBM.  Two launches inside: the convolution pools every 16 x 16 output tile through LDS and writes the
 * tile's last row / column to seam_scratch (vpt_conv3x3_pool_seam_elems(frames, H, W, Cout) 16-bit elements, caller-owned); a small
 * second kernel completes the pooled pixels whose 3 x 3 window crosses a tile border.  Bit-identical to vpt_conv3x3_forward followed by
 * vpt_maxpool_forward (the statistics to the order of their fp32 / fp64 additions).  No residual, throughput tiling only.
 * phases: 3 = both launches (the normal call); 1 = the convolution only, 2 = the seam kernel only (a caller that times them apart).
 * out_gain, chs_out: as for vpt_conv_first_forward (the pooled tensor stored times GroupNorm `n`'s gain, statistics of the unscaled
 * values; per-channel sums of the stored tensor, accumulated by both launches). */
int64_t vpt_conv3x3_pool_seam_elems(int frames, int H, int W, int Cout);
int vpt_conv3x3_pool_forward(const void* x, const void* wpk, const float* edge_sa, const float* edge_sg, const double* stats_in,
                             void* pooled, void* seam_scratch, double* stats_out, const float* out_gain, double* chs_out, int frames, int H,
                             int W, int Cin, int Cout, int phases, void* stream);

/* Round 5, the TRAINING forward of a stack's firstconv -> max_pool2d (lib/impala_cnn.py:114-117 under behavioural_cloning.py:101): the same pass
 * that ALSO records, per pooled value, which positions of its 3 x 3 window hold the maximum -- pool_mask [F][Cout/32][H/2][W/2][32] uint16, bit
 * 8 - k set = scan position k = 3 (dy + 1) + (dx + 1) differs from the maximum or lies outside the image.  The backward
 * (vpt_conv_backward_prepare_pooled) routes the pooled gradient to the first zero bit -- torch's first-maximum rule -- so neither the
 * pre-pool tensor (2 MB per frame in stack 1) nor vpt_maxpool_forward's arg-max bytes exist in the BC step.  Pooled values and statistics
 * are those of vpt_conv3x3_pool_forward, bit for bit.  phases as there. */
int vpt_conv3x3_pool_argmax_forward(const void* x, const void* wpk, const float* edge_sa, const float* edge_sg, const double* stats_in,
                                    void* pooled, void* pool_mask, void* seam_scratch, double* stats_out, int frames, int H, int W, int Cin, int Cout, int phases, void* stream);

/* ---- GroupNorm `n` of a stack folded into its first residual block (CnnDownStack.forward, lib/impala_cnn.py:118-121: x = self.n(x);
 * for block in self.blocks: x = block(x)) -- inference.  The producer of the pooled tensor P stores Q = n.weight[c] * P (out_gain above);
 * x = n(P) = r_P Q + b[c] is never written:
 *   vpt_channel_stats: chs[f][c] = (sum_p Q, sum_p Q^2) over the HW pixels of a frame, fp64, ACCUMULATED (caller zeroes);
 *   vpt_nfold_coef:    from tot[f] = the frame statistics of P (the producer's stats_out), chs, n.weight / n.bias and four edge tables of
 *                      block 0's conv0 -- its own edge_sa / edge_sg plus tb / tg = the edge_sg sums with every input channel weighted by
 *                      n.bias / n.weight -- the per-frame epilogue table kk_frame [frames][9][ceil(Cout/128)*128], the accumulator scale
 *                      rs_frame [frames] (conv0) and res_scale [frames], res_bias [frames][C] (conv1's residual x = res_scale * Q + res_bias);
 *   vpt_conv3x3_forward_folded: vpt_conv3x3_forward with either of the two substitutions: (kk_frame, rs_frame) replace edge_sa and the
 *                      statistics of x (conv0 on Q; edge_sg must still point at a table of the right size, stats_in may be null);
 *                      (res_scale, res_bias) turn the residual into res_scale[f] * res + res_bias[f][c] (conv1, res = Q).
 * Saves the read and the write of every pooled tensor that vpt_frame_affine_forward costs. */
int vpt_channel_stats(const void* x, double* chs, int frames, int C, int HW, void* stream);
int vpt_nfold_coef(const double* tot, const double* chs, const float* gain, const float* bias, const float* sa, const float* sg,
                   const float* tb, const float* tg, float* kk_frame, float* rs_frame, float* res_scale, float* res_bias,
                   int frames, int C, int HW, int Cout, void* stream);
int vpt_conv3x3_forward_folded(const void* x, const void* wpk, const float* edge_sa, const float* edge_sg, const double* stats_in,
                               const float* kk_frame, const float* rs_frame, const void* res, const float* res_scale, const float* res_bias,
                               void* y, double* stats_out, int frames, int H, int W, int Cin, int Cout, void* stream);

/* F.max_pool2d(x, 3, 2, 1) on a post-ReLU blocked tensor (lib/impala_cnn.py:117, stacks 1..2).  argmax (optional, for
 * training): uint8, shaped like y, the window position kh*3+kw of the first maximum (15 when the window is all zero). */
int vpt_maxpool_forward(const void* x, void* y, double* stats_out, uint8_t* argmax, int frames, int C, int H, int W, void* stream);

/* y = (x - mean_f) * rstd_f * gain + bias with whole-frame statistics:
 * CnnDownStack.n (GroupNorm(1,C), lib/impala_cnn.py:99-100,118-119; per_element = 0, gain[C]) and the
 * LayerNorm of ImpalaCNN.dense over the flattened frame (lib/impala_cnn.py:177-184; per_element = 1,
 * gain[C*H*W] already permuted to the blocked order). */
int vpt_frame_affine_forward(const void* x, void* y, const float* gain, const float* bias,
                             const double* stats_in, double* stats_out,
                             int frames, int C, int HW, int per_element, void* stream);

/* C[M,N] = A[M,K] W[N,K]^T (+bias) (ReLU) (+res): every nn.Linear on the path (lib/util.py:58-82,
 * lib/xf.py:251-254, lib/action_head.py:164, lib/scaled_mse_head.py:35).  A bf16 [M][lda]; wpk bf16
 * [ceil(N/128)][K/32][128][32]; bias fp32[N] or NULL; res fp32 [M][ldr] or NULL; out_f32 [M][ldc] and/or
 * out_bf16 [M][ldcb].  splitk > 1 (no ReLU/res): out_f32 is a caller-zeroed [splitk][M][ldc] buffer, split s writes its
 * partial product to slice s and the caller sums the slices -- no atomics, so the result is bit-reproducible.  A bias is allowed with splitk > 1: it
 * is added in SLICE 0 only, by every kernel behind this entry point (MFMA vector and generic epilogues, weight-streaming kernel), so the sum of the
 * slices carries it exactly once.  A split whose K run is empty writes nothing: that slice keeps the caller's zeros.
 * mask (optional, bf16 [M][ldm]) zeroes outputs where mask <= 0 before the residual add: the ReLU backward of
 * the BC step's dgrad GEMMs.  The same entry point serves forward, dgrad (W^T packed) and wgrad (A = dY^T). */
int vpt_linear_forward(const void* A, const void* wpk, const float* bias, const float* res,
                       float* out_f32, void* out_bf16, int M, int N, int K,
                       int lda, int ldr, int ldc, int ldcb, int relu, int splitk, const void* mask, int ldm,
                       void* stream);
/* The same with the kernel named by the caller: 1 = the MFMA GEMM whatever M, 2 = the weight-streaming kernel of the acting step (M <= 8
 * rows), 0 = by M (what vpt_linear_forward does: <= 8 rows stream the weights).  The two kernels sum in different orders; a caller
 * whose rows must not depend on how many rows share the call (batches of sequences: chunking, sharding) passes 1.  4 = the MFMA GEMM on
 * 256 x 256 tiles with eight waves and LDS-DMA operands where that grid fills the chip (bit-identical to 1; measured neutral inside the
 * engine, kept for A/B measurements). */
int vpt_linear_forward_tiled(const void* A, const void* wpk, const float* bias, const float* res,
                             float* out_f32, void* out_bf16, int M, int N, int K,
                             int lda, int ldr, int ldc, int ldcb, int relu, int splitk, const void* mask, int ldm,
                             int tiling, void* stream);

/* Weight gradient of a linear layer without transposed copies: dw[n][k] (+)= sum_m dy[m][n] * x[m][k]; dy bf16 [M][ldy],
 * x bf16 [M][ldx] (both row-major over the M frames / tokens), dw fp32 [N][ldw]; N, K, ldy, ldx multiples of 8.
 * Replaces autograd's dW = dY^T X for every nn.Linear of the BC step (behavioural_cloning.py:117-119). */
int vpt_linear_wgrad(const void* dy, const void* x, float* dw, int M, int N, int K, int ldy, int ldx, int ldw, int accumulate, void* stream);

/* ImpalaCNN.dense with its LayerNorm folded into the GEMM (lib/impala_cnn.py:177-194; inference): run vpt_linear_forward with splitk > 1 on the RAW
 * block output x [M = frames][K = C*16*16] against weights packed from W * gain (per element), then this: out[f][n] = rstd_f * sum_s part[s][f][n]
 * - rstd_f * mean_f * sg[n] + sb[n], (mean_f, rstd_f) from stats [M][2] of x (count = K), sg[n] = sum_k op16(W gain)[n][k], sb[n] = sum_k W[n][k]
 * bias[k].  Replaces vpt_frame_affine_forward(per_element = 1) + the split-K sum. */
int vpt_dense_fold_epilogue(const float* part, int splitk, const double* stats, int count, const float* sg, const float* sb, float* out,
                            int M, int N, void* stream);

/* Second stage of a split-K linear: out = epilogue(sum_s part[s][M][N]) with the same epilogue options as
 * vpt_linear_forward (part = the [splitk][M][N] buffer a vpt_linear_forward call with splitk > 1 filled). */
int vpt_linear_splitk_epilogue(const float* part, int splitk, const float* bias, const float* res, float* out_f32, void* out_bf16,
                               int M, int N, int ldr, int ldc, int ldcb, int relu, const void* mask, int ldm, void* stream);

/* Merge of a low-rank adapter into an fp32 master weight: out[i][k] = W[i][k] + s * sum_j B[i][j] * A[j][k], W / out fp32 [n][K] (out may be W),
 * A fp32 [r][K], B fp32 [n][r], 1 <= r <= 64.  fp32 throughout, j ascending, every multiply and every add rounded on its own (no contraction):
 * acc = 0; acc = acc + B[i][j] * A[j][k]; out = W + s * acc -- a float32 restatement of these lines gives the same bits. */
int vpt_lowrank_merge(const float* W, const float* A, const float* B, float* out, int n, int K, int r, float s, void* stream);

/* Acting path (M = B*T <= 8 rows, K <= 3072; agent.py:190-206): nn.LayerNorm (optional ReLU on its input) FUSED into the linear
 * layer it feeds -- every LayerNorm of the policy does feed one (lib/xf.py:334-356 pre_r_ln -> q/k/v/r, ln -> mlp0; lib/util.py:58-82
 * FanInInitReLULayer(norm, linear); lib/policy.py:188,211-214 lastlayer, final_ln -> heads).  Same results, bit for bit, as
 * vpt_layernorm_forward followed by vpt_linear_forward; ln_out_f32 (optional, [M][K]) receives the normalised rows in fp32
 * (the residual branch / the latent).  Larger M or K: returns -1, call the two functions. */
int vpt_layernorm_linear_forward(const float* x, const float* ln_gain, const float* ln_bias, int relu_in, float* ln_out_f32,
                                 const void* wpk, const float* bias, const float* res, float* out_f32, void* out_bf16,
                                 int M, int N, int K, int ldr, int ldc, int ldcb, int relu, void* stream);

/* nn.LayerNorm over the last dim with optional ReLU on the input (lib/util.py:61-62,169; lib/policy.py:188,211-214). */
int vpt_layernorm_forward(const float* x, const float* gain, const float* bias, float* out_f32, void* out_bf16,
                          int M, int D, int relu_in, void* stream);

/* Attention of MaskedAttention.forward (lib/masked_attention.py:161-178) over attention() (lib/xf.py:18-71).
 * causal = 1 ("clipped_causal"): banded-causal with KV memory and relative-position bias; qkvr fp32 [B*t][ld] =
 * Q | K | V | R columns; kmem/vmem fp32 [B][maxlen][hid]; memvalid uint8 [B][maxlen] (= state_mask &
 * !first[:,0]); b_nd fp32 [10][maxlen].  causal = 0 (mask "none", the IDM): maxlen must be 0 (no memory; the
 * rel-pos bias is identically zero, lib/util.py:256-260), every query attends to all t <= 160 rows of its
 * chunk; kmem/vmem/memvalid/b_nd are ignored.  out bf16 [B*t][hid] (heads merged, lib/xf.py:125-131). */
int vpt_masked_attention_forward(const float* qkvr, const float* kmem, const float* vmem, const uint8_t* memvalid,
                                 const float* b_nd, void* out, int B, int t, int heads, int hid, int ld,
                                 int maxlen, int causal, void* stream);

/* vpt_masked_attention_forward (causal = 1) with episode starts honoured at EVERY frame of the chunk, not only at t = 0: what
 * MaskedAttention.forward (lib/masked_attention.py:161-178) computes when the same frames are stepped one at a time with one hidden state per
 * episode, as the BC loop does (behavioural_cloning.py:95-112).  qlo int32 [B*t] (vpt_episode_bounds): query i sees row j of [memory ; chunk]
 * iff it lies in the band, j >= qlo[i], and (j >= maxlen or memvalid[j]); memvalid is then the plain state_mask (qlo covers first[:,0]). */
int vpt_masked_attention_forward_episodes(const float* qkvr, const float* kmem, const float* vmem, const uint8_t* memvalid,
                                          const float* b_nd, void* out, const int32_t* qlo, int B, int t, int heads, int hid, int ld,
                                          int maxlen, void* stream);

/* Episode bounds of a chunk for the two *_episodes entry points (lib/masked_attention.py:161-178 applied per frame, behavioural_cloning.py:95-112):
 * first / state_mask: bool bytes [B][t] / [B][maxlen].  qlo int32 [B][t] = maxlen + (latest p <= i with first[b][p]), or 0 when there is none;
 * mask_out bool bytes [B][maxlen] = the next state mask: kept row j = t + r is valid iff j >= qlo[b][t-1] and (j >= maxlen or state_mask[b][j])
 * (the per-frame form of lib/masked_attention.py:86-92).  Either output may be NULL; mask_out must not alias state_mask.  t >= 1. */
int vpt_episode_bounds(const uint8_t* first, const uint8_t* state_mask, int32_t* qlo, uint8_t* mask_out, int B, int t, int maxlen, void* stream);

/* SelfAttentionLayer.update_state (lib/xf.py:366-391): kout/vout = last maxlen rows of [memory ; new]. */
int vpt_kv_memory_update(const float* qkvr, const float* kmem, const float* vmem, float* kout, float* vout,
                         int B, int t, int hid, int ld, int maxlen, void* stream);

/* Acting step (t = 1; agent.py:190-206): the whole recurrent-state step of one transformer block in ONE launch --
 * vpt_masked_attention_forward(causal = 1, t = 1), vpt_kv_memory_update and the mask bookkeeping of lib/xf.py:366-391
 * (memory visible where state_mask & ~first; next mask = cat(state_mask[1:] & ~first, [True])).  One query per (sequence, head)
 * against the newest maxlen - 1 memory rows and the token itself; the rows it reads are written one row up into kout / vout.
 * state_mask / mask_out: bool bytes [B][maxlen]; first: bool bytes [B].  kout / vout MAY alias kmem / vmem (in-place state, as
 * the captured acting graph uses it); mask_out must be a different buffer than state_mask.  maxlen <= 128.  Same formulas as the general kernel
 * (lib/xf.py:18-71, lib/masked_attention.py:161-178); sums in a different order: equal to fp32 rounding. */
int vpt_masked_attention_step(const float* qkvr, const float* kmem, const float* vmem, const uint8_t* state_mask, const uint8_t* first,
                              const float* b_nd, void* out, float* kout, float* vout, uint8_t* mask_out,
                              int B, int heads, int hid, int ld, int maxlen, void* stream);

/* The same step with EVERYTHING updated in place (what the captured acting graph uses: no copies of the recurrent state at all):
 * kmem / vmem / state_mask are read and overwritten.  The mask is safe to overwrite because the workgroup that arrives last at
 * done_counter ([B] ints, zero before the first launch; the kernel leaves them zero) writes it, after every other one has read it. */
int vpt_masked_attention_step_inplace(const float* qkvr, float* kmem, float* vmem, uint8_t* state_mask, const uint8_t* first,
                                      const float* b_nd, void* out, int* done_counter, int B, int heads, int hid, int ld, int maxlen, void* stream);

/* Tail of MinecraftAgentPolicy.act for the acting step (lib/policy.py:307-327) in one launch: log_prob = logp_buttons + logp_camera
 * (lib/action_head.py:227-237 sums the heads), value de-normalisation v * scale + shift (lib/normalize_ewma.py:27-31 with
 * scale = sqrt(var + eps), shift = mean), the NaN assertion of lib/policy.py:320-321 as a byte flag, and one packed record per
 * environment:  keep[b][4] (int64) = { buttons action, camera action, float bits of log_prob, float bits of the de-normalised value
 * (low half) | float bits of the raw value-head output (high half) }.  value_col: column of the value head in logits[B][ld].
 * rng_state (optional, device uint64 {seed, step}): step += 1 -- the stochastic heads of this acting step have drawn (vpt_action_head_forward). */
int vpt_act_epilogue(const int64_t* action_buttons, const int64_t* action_camera, const float* logp_buttons, const float* logp_camera,
                     const float* logits, int ld, int value_col, float scale, float shift, int64_t* keep, uint8_t* nan_flag, uint64_t* rng_state,
                     int B, void* stream);

/* CategoricalActionHead.forward tail (lib/action_head.py:170-174): out[M][n] = log_softmax(logits[:, col0:col0+n] / T). */
int vpt_log_softmax_forward(const float* logits, float* out, int M, int ld, int col0, int n, float temperature,
                            void* stream);

/* The whole CategoricalActionHead on one head's columns (lib/action_head.py:163-207): log-probs as above, with
 *   mask   [M][n] uint8, optional: 0 = unavailable action, its scaled logit becomes LOG0 = -100 before the softmax
 *          (shaped_out[~mask] = LOG0, lib/action_head.py:170-171; obs["mask"] of lib/policy.py:257-266);
 *   action [M] int64, optional: CategoricalActionHead.sample -- arg-max of the log-probs (deterministic), or of
 *          log-probs - log(-log u) with u = noise[M][n] uniform in [0,1] (Gumbel-max, u == 1 -> 0.999 as the reference);
 *          the FIRST maximum, as torch.argmax.  The random numbers are the caller's (noise; the reference draws them from torch's
 *          generator, lib/action_head.py:200) OR generated inside the kernel from rng_state = device uint64 {seed, step} and
 *          rng_stream (Philox4x32-10: key = seed, counter = (element / 4, row, step, stream << 24), u = (word >> 8) * 2^-24 --
 *          what a captured acting step needs: a fresh draw per replay with no host generator in the loop).  The kernel does not
 *          advance `step`: vpt_act_epilogue does, once per acting step (or the host between calls).  noise and rng_state are
 *          mutually exclusive; both null = deterministic.  The action is always in [0, n): a row on which no score compares greater
 *          than the start value -- every score NaN (one NaN logit makes the whole row's log-probs NaN) or every score -inf (a noise
 *          row of zeros) -- takes index 0, as torch.argmax does for an all-NaN and for an all--inf row; action_logp is then the
 *          log-prob of index 0, NaN on a NaN row, which vpt_act_epilogue's nan_flag reports;
 *   action_logp [M] fp32, optional: log-prob of that action (CategoricalActionHead.logprob, lib/action_head.py:176-184). */
int vpt_action_head_forward(const float* logits, const uint8_t* mask, const float* noise, const uint64_t* rng_state, uint32_t rng_stream,
                            float* out, int64_t* action, float* action_logp, int M, int ld, int col0, int n, float temperature, void* stream);
/* out[M][n] = exactly the uniforms vpt_action_head_forward generates for (rng_state, rng_stream) -- to inspect or replay a draw through
 * the `noise` argument (th.rand_like(logits), lib/action_head.py:200).  rng_state is not advanced. */
int vpt_uniform_noise(const uint64_t* rng_state, uint32_t rng_stream, float* out, int M, int n, void* stream);

/* Fused Adam update of one flat fp32 bucket: th.optim.Adam(lr, weight_decay).step() as configured by
 * behavioural_cloning.py:63-67,122 (L2 weight decay folded into the gradient, bias-corrected moments).
 * `step` counts from 1; grad_scale multiplies the gradient first (1/world_size of the data-parallel mean).
 * The hyper-parameters are taken as fp32 (0.999f, not 0.999: 1 - beta2 is then 0.000999987), and the bias corrections lr / (1 - beta1^step) and
 * 1 / sqrt(1 - beta2^step) are formed in double from those fp32 values and rounded to fp32 once; the same holds for every entry point below. */
int vpt_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint64_t n, int step,
                  float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream);

/* The same update for EVERY parameter tensor in one launch (th.optim.Adam(policy.parameters()).step(), behavioural_cloning.py:63-67,
 * 122).  `table` is a DEVICE array of `ntensors` descriptors { float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
 * uint64_t n; int64_t first_block; } (48 bytes each), sorted by first_block, where first_block counts 1024-element blocks:
 * first_block[0] = 0, first_block[i+1] = first_block[i] + ceil(n[i] / 1024); total_blocks = the sum.
 * skip_flag (device int32, optional): when non-zero the launch leaves every tensor untouched -- the found-inf result of
 * vpt_grads_nonfinite_multi for a loss-scaled step (fp16 operand format), consumed without a host round trip. */
int vpt_adam_step_multi(const void* table, int ntensors, int64_t total_blocks, int step, float lr, float beta1, float beta2,
                        float eps, float weight_decay, float grad_scale, const int32_t* skip_flag, void* stream);

/* Sets *flag = 1 (device int32, zeroed by the caller) if any gradient of the table (same layout as above; only `grad`, `n`,
 * `first_block` are read) is inf or nan.  The reference trains in fp32 and has no counterpart; this is what
 * torch.cuda.amp.GradScaler.unscale_ computes for an fp16 run of behavioural_cloning.py:117-122. */
int vpt_grads_nonfinite_multi(const void* table, int ntensors, int64_t total_blocks, int32_t* flag, void* stream);

/* Global-norm gradient clipping: th.nn.utils.clip_grad_norm_(params, MAX_GRAD_NORM) as behavioural_cloning.py:121 meant it (upstream
 * passes an exhausted generator, so the call does nothing there).  One read of the gradients over the SAME table as vpt_adam_step_multi
 * (only `grad`, `n`, `first_block` are read), fixed summation order, fp64 finish, no host round trip:
 *   norm_out[0] = || grad * grad_scale ||_2 over all tensors (fp32 squares, fp32 sum per 1024-element block, fp64 above that);
 *   norm_out[1] = min((1 / (norm + 1e-6)) * max_norm, 1) in fp32, torch's clip_coef_clamped; 1 when max_norm <= 0 (norm only);
 *                 0 when the squared sum is not finite;
 *   norm_out[2] = 1 if the squared sum is not finite, else 0;   norm_out[3] = 0.
 * per_tensor (optional, fp32 [ntensors]): each tensor's own norm.  flag (optional device int32, zeroed by the caller): set, never
 * cleared, when the sum is not finite or any raw gradient is inf / nan -- with it this call replaces vpt_grads_nonfinite_multi.
 * workspace: vpt_grad_norm_workspace_bytes(ntensors, total_blocks) bytes, 8-byte aligned, caller-owned.  (Today it is left holding
 * the intermediate sums -- [ntensors] fp64 per-tensor squared sums, then [total_blocks] fp32 block partials -- which the tests read;
 * that layout is NOT part of this interface and may change.) */
long vpt_grad_norm_workspace_bytes(int ntensors, int64_t total_blocks);
int vpt_grad_norm_multi(const void* table, int ntensors, int64_t total_blocks, float grad_scale, float max_norm, void* workspace,
                        float* norm_out, float* per_tensor, int32_t* flag, void* stream);

/* vpt_adam_step_multi with the gradient also multiplied by the DEVICE scalar *clip_coef (norm_out + 1 of vpt_grad_norm_multi):
 * g' = (g * grad_scale) * coef + wd * p.  clip_grad_norm_ + Adam.step() of behavioural_cloning.py:121-122 without the in-place
 * scaling pass.  A coefficient of exactly 1 gives vpt_adam_step_multi's result bit for bit. */
int vpt_adam_step_multi_clip(const void* table, int ntensors, int64_t total_blocks, int step, float lr, float beta1, float beta2,
                             float eps, float weight_decay, float grad_scale, const int32_t* skip_flag, const float* clip_coef,
                             void* stream);

/* Parameter groups (th.optim.Adam([dict(params=..., lr=..., weight_decay=...), ...]), the list form of the optimiser
 * behavioural_cloning.py:63-67 builds with one group) and decoupled decay, still ONE launch over the SAME table as vpt_adam_step_multi.
 * `groups` is a DEVICE array of `ntensors` records { float lr; float weight_decay; } (8 bytes each), record i belonging to table
 * entry i.  Coupled (decoupled == 0): per element the arithmetic of vpt_adam_step_multi[_clip] with the tensor's own lr and
 * weight_decay; the step size is (float)((double)lr / (1 - pow((double)beta1, step))), the same double expression on the float lr,
 * so a tensor whose record holds vpt_adam_step_multi's launch-wide values is updated bit for bit as by that entry point.
 * decoupled != 0 (th.optim.AdamW): param = param * (float)(1 - (double)lr * (double)weight_decay) first -- the factor formed in
 * double and rounded to float, one rounded multiply --, then the coupled update with weight_decay = 0.
 * skip_flag: as vpt_adam_step_multi.  clip_coef (optional device scalar): as vpt_adam_step_multi_clip; null = unclipped. */
int vpt_adam_step_groups(const void* table, const void* groups, int ntensors, int64_t total_blocks, int step, float beta1, float beta2,
                         float eps, float grad_scale, int decoupled, const int32_t* skip_flag, const float* clip_coef, void* stream);

/* Gradient accumulation over micro-batches: param[i] = param[i] + grad[i] (one fp32 add) for every tensor of the SAME table as
 * vpt_adam_step_multi, in one launch.  `param` names the fp32 accumulator (read and written), `grad` the addend (read only);
 * exp_avg and exp_avg_sq are ignored.  No reductions and no atomics -- the same inputs give the same bits -- and no byte outside
 * [param, param + n) is written.  inf / nan go through the sum: vpt_grads_nonfinite_multi / vpt_grad_norm_multi in front of the
 * Adam launch see them.  An accumulator must not overlap its addend.  (torch.autograd sums .grad in the same way when backward()
 * runs more than once before optimizer.step(); behavioural_cloning.py:117-122 takes one step per batch.) */
int vpt_grad_accumulate_multi(const void* table, int ntensors, int64_t total_blocks, void* stream);

/* ---- behavioural-cloning step: backward of the heads / trunk / transformer (the reference uses torch autograd,
 * behavioural_cloning.py:117-119).  Linear layers reuse vpt_linear_forward (dgrad: W^T packed; wgrad: A = dY^T). */

/* d loss / d logits for loss = -sum_rows[ log_softmax(z_b/T)[a_b] + log_softmax(z_c/T)[a_c] ] * (scale*T), written as
 * bf16 [M][ldz] (columns >= nb+nc zero): scale = 1 / (global frames * temperature).  lib/action_head.py:170-184. */
int vpt_bc_nll_backward(const float* lp_buttons, const float* lp_camera, const int64_t* act_buttons,
                        const int64_t* act_camera, void* dz, int M, int nb, int nc, int ldz, float scale, void* stream);

/* The BC loss with per-frame weights, its gradient and its metrics in one sweep over the log-probs:
 *   loss = sum_rows w (nll_b + nll_c) / sum_rows w   (behavioural_cloning.py:107 with w = 1; padding / left-out frames: w = 0),
 * plus what lib/action_head.py:176-193 offers per head -- logprob of the label, entropy -- and the arg-max hit.  Every output is optional (NULL):
 *   dz        16-bit [M][ldz], ldz >= nb + nc: (exp(lp) - onehot) * (scale * weight[row]), further columns zero -- vpt_bc_nll_backward's values at the
 *             row's own scale, bit for bit; the caller folds 1 / (sum w * temperature) (and the fp16 loss scale) into `scale`;
 *   frame_out fp32 [M][8]: nll_buttons, nll_camera, entropy_buttons, entropy_camera (-sum p lp, a term with p = 0 counts 0), hit_buttons, hit_camera
 *             (1 = the head's arg-max is the label; ties: lowest index), w, 0 -- the frame's own, unweighted values;
 *   totals    fp32 [8]: sum_rows w * frame_out[row][k] for k < 6, sum w, the number of rows with w > 0.  The rows' records are added in a fixed order
 *             through `workspace` (vpt_workspace_bytes(VPT_WS_BC_LOSS, M, ...) bytes, required with totals; M <= 65536): no atomics, the same inputs give the
 *             same bits.
 * weight fp32 [M] or NULL (all ones).  A row with weight 0 stores exact zeros in dz and adds exact zeros to totals whatever its log-probs hold (NaN
 * included); labels are only compared with column indices, so an out-of-range label (a padded frame's) reads nothing and matches nothing. */
int vpt_bc_loss(const float* lp_buttons, const float* lp_camera, const int64_t* act_buttons, const int64_t* act_camera,
                const float* weight, void* dz, float* frame_out, float* totals, float* workspace,
                int M, int nb, int nc, int ldz, float scale, void* stream);

/* The same boundary for an ARBITRARY incoming gradient -- what torch autograd hands to the outputs of
 * MinecraftAgentPolicy.forward / get_output_for_observation (lib/policy.py:252-305) when the caller writes its own loss, as
 * behavioural_cloning.py:101-119 does: g_buttons / g_camera = d loss / d log-prob ([M][nb] / [M][nc], either may be NULL),
 * g_value = d loss / d (raw value-head output) ([M], may be NULL).  dz = (g - exp(lp) * rowsum(g)) / temperature per head,
 * the value column passes through; 16-bit [M][ldz], ldz >= nb + nc + 1, padding zero.  grad_scale multiplies every written value
 * (the loss scale of the fp16 operand format, whose 16-bit gradient buffers would otherwise underflow; 1 for bf16).  mask_* (uint8 [M][n], optional): the
 * availability masks of the forward -- a masked logit was overwritten with the constant LOG0, so its dz is 0. */
int vpt_heads_logprob_backward(const float* lp_buttons, const float* lp_camera, const float* g_buttons, const float* g_camera,
                               const float* g_value, const uint8_t* mask_buttons, const uint8_t* mask_camera, void* dz,
                               int M, int nb, int nc, int ldz, float temperature, float grad_scale, void* stream);

/* nn.LayerNorm backward (optionally through a ReLU on the LayerNorm's input): dx = dx_add + dLN(x, dy);
 * dgain / dbias += the column sums (caller zeroes), reduced in a FIXED order through `partials` (fp32 workspace of
 * vpt_workspace_bytes(VPT_WS_LAYERNORM_BACKWARD, M, D, ...) bytes): the same inputs give the same bits, as torch autograd on one device does for
 * behavioural_cloning.py:117-119.  (ABI 5; ABI 4 accumulated with fp32 atomics in arrival order.) */
int vpt_layernorm_backward(const float* x, const float* gain, const float* dy, const float* dx_add, float* dx,
                           float* dgain, float* dbias, float* partials, int M, int D, int relu_in, void* stream);

/* out16[M][ldo] = (mask > 0 ? x : 0) with columns >= N zeroed: the ReLU backward gate (F.relu at lib/util.py:81,
 * lib/policy.py:211) fused with the cast / K-padding that turns an fp32 gradient into a GEMM A operand. */
int vpt_gate_cast(const float* x, const void* mask, void* out, int M, int N, int ldx, int ldm, int ldo, void* stream);

/* out[N] += column sums of a 16-bit [M][ld] matrix (bias gradients), in a fixed order through `partials` (VPT_WS_COLUMN_SUM (M, N) bytes; may be
 * NULL when that is 0). */
int vpt_column_sum(const void* x_bf16, float* out, float* partials, int M, int N, int ld, void* stream);

/* Backward of vpt_masked_attention_forward (causal = 1): dqkvr [B*t][ld] receives dQ, dK, dV and dR (every column written, nothing to zero);
 * db_nd [10][maxlen] accumulated (caller zeroes).  The KV memory is detached state (behavioural_cloning.py:111) and gets no gradient.
 * A key is reached by up to five 32-query tiles and b_nd by every workgroup: each contribution is written to its own slot of a workspace and the
 * slots are added in a fixed order (bit-reproducible).  dkv_slab: VPT_WS_ATTENTION_BACKWARD_DKV (B, t, hid) bytes, dbnd_slab:
 * VPT_WS_ATTENTION_BACKWARD_DBND (B, t, heads, maxlen) bytes.  ld must be a multiple of 4. */
int vpt_masked_attention_backward(const float* qkvr, const float* kmem, const float* vmem, const uint8_t* memvalid,
                                  const float* b_nd, const float* dout, float* dqkvr, float* db_nd, float* dkv_slab, float* dbnd_slab,
                                  int B, int t, int heads, int hid, int ld, int maxlen, void* stream);

/* Backward of vpt_masked_attention_forward_episodes: the same kernel with the forward's qlo (lib/masked_attention.py:161-178 per frame,
 * behavioural_cloning.py:95-112); keys outside a query's episode have P = 0 exactly and receive no gradient from it. */
int vpt_masked_attention_backward_episodes(const float* qkvr, const float* kmem, const float* vmem, const uint8_t* memvalid,
                                           const float* b_nd, const float* dout, float* dqkvr, float* db_nd, float* dkv_slab, float* dbnd_slab,
                                           const int32_t* qlo, int B, int t, int heads, int hid, int ld, int maxlen, void* stream);

/* ---- inverse-dynamics model training (everything behind the CNN; the reference has no IDM training script, the gradients are what torch
 * autograd gives for InverseActionNet.forward, lib/policy.py:374-392) ---- */

/* Backward of vpt_masked_attention_forward with causal = 0, maxlen = 0 -- mask "none" (lib/masked_attention.py:137-141: no band mask, an empty
 * memory) through lib/xf.py:18-63 (softmax(Q K^T / d_head) V per head, d_head = 128): every query sees all t <= 160 rows of its window.
 *   qkv fp32 [B*t][ld] (Q, K, V at columns 0, hid, 2 hid; ld >= 3 hid, ld % 4 == 0), dout fp32 [B*t][hid] -> dqkv fp32 [B*t][ld]: dQ, dK, dV, and
 *   zeros in the columns >= 3 hid (every element written, nothing to zero).
 * The probabilities are recomputed from qkv (the forward keeps nothing); all contractions run on the fp32 matrix cores.  Every 32-query tile writes
 * its piece of dK / dV to its own slot of dkv_slab (VPT_WS_FULL_ATTENTION_BACKWARD (B, t, hid) bytes) and the slots are added in slot order: no
 * atomics, the same inputs give the same bits, and a window's result does not depend on the other windows of the call. */
int vpt_full_attention_backward(const float* qkv, const float* dout, float* dqkv, float* dkv_slab,
                                int B, int t, int heads, int hid, int ld, void* stream);

/* The IDM's loss, its gradient and its metrics in one launch: gb independent nb-way button groups and gc nc-way camera groups per frame
 * (lib/action_head.py:136-160: a CategoricalActionHead of shape (20, 2) / (2, 11)),
 *   loss = sum_rows w (nll_b + nll_c) / sum_rows w,  nll_* = -sum over the head's groups of the label's log-prob (lib/action_head.py:176-184,252-253).
 * lp_buttons fp32 [M][gb][nb], lp_camera fp32 [M][gc][nc], act_buttons int64 [M][gb], act_camera int64 [M][gc], weight fp32 [M] or NULL.  Outputs as
 * vpt_bc_loss (each optional): dz 16-bit [M][ldz], ldz >= gb nb + gc nc, (exp(lp) - onehot) * (scale * weight[row]) in the column order of the two head
 * matrices concatenated, further columns zero; frame_out fp32 [M][8] = nll_b, nll_c, ent_b, ent_c (sums over the groups), hit_b, hit_c (fraction of
 * the head's groups whose arg-max, lowest index on ties, is the label), w, 0; totals fp32 [8] through `workspace` (VPT_WS_BC_LOSS (M) bytes,
 * M <= 65536) in a fixed order.  A row with weight 0 stores exact zeros in dz and adds exact zeros to totals; labels are only compared. */
int vpt_idm_loss(const float* lp_buttons, const float* lp_camera, const int64_t* act_buttons, const int64_t* act_camera,
                 const float* weight, void* dz, float* frame_out, float* totals, float* workspace,
                 int M, int gb, int nb, int gc, int nc, int ldz, float scale, void* stream);

/* Backward of the IDM's grouped log-softmax heads for an ARBITRARY incoming gradient -- what torch autograd hands to the outputs of
 * InverseActionPolicy.forward when the caller writes its own loss through pi_head.logprob / entropy / kl_divergence (lib/action_head.py:136-184: a
 * CategoricalActionHead of shape (groups, classes) is `groups` independent log-softmaxes of logits / temperature).  lp_buttons fp32 [M][gb][nb],
 * lp_camera fp32 [M][gc][nc] (the forward's log-probs); g_buttons / g_camera = d loss / d log-prob in the same shapes, either may be NULL (= zeros:
 * that head's block of dz is zero).  Per group, with log-probs l_j, incoming g_j and n classes, in fp32 without contraction:
 *   s = ((g_0 + g_1) + ...) + g_{n-1},  p_j = expf(l_j),  dz_j = ((g_j - p_j s) * (1 / temperature)) * grad_scale,  rounded once to the operand format.
 * mask_* (uint8, the log-probs' shapes, optional): the forward's availability masks -- a masked logit was overwritten with the constant LOG0, so its
 * dz is 0 (its g still counts in s).  dz: 16-bit [M][ldz], ldz >= gb nb + gc nc, in the column order of the two head matrices concatenated
 * ([group][class], buttons first), further columns zero; every element is written.  grad_scale: as vpt_heads_logprob_backward's.  No reduction
 * crosses a lane: the same inputs give the same bits.  Returns -1 for M <= 0, a non-positive temperature, a group or class count below 1 or a
 * short ldz. */
int vpt_grouped_logprob_backward(const float* lp_buttons, const float* lp_camera, const float* g_buttons, const float* g_camera,
                                 const uint8_t* mask_buttons, const uint8_t* mask_camera, void* dz,
                                 int M, int gb, int nb, int gc, int nc, int ldz, float temperature, float grad_scale, void* stream);

/* ---- reinforcement-learning fine-tuning of the cloned policy (the third stage of the method; the reference ships no RL training script, only the
 * pieces such a loss is made of: the heads' logprob / entropy / kl_divergence, lib/action_head.py:176-203,252-275, and the value head) ---- */

/* Clipped policy gradient + KL to a frozen prior + entropy bonus + value loss, their gradient w.r.t. the fused head logits and their metrics in one
 * launch.  With l, q the log-probs of the policy and of the prior, p = exp(l), per head K = sum p (l - q), H = -sum p l (a term with p = 0 counts 0):
 *   lp = l_b[a_b] + l_c[a_c]  (lib/action_head.py:252-253 sums the heads),  rho = expf(lp - old_log_prob),  t^ = (value_target - mean) / std,
 *   L_r = -min(rho A, clamp(rho, 1 - clip, 1 + clip) A) + kl_coef (K_b + K_c) - entropy_coef (H_b + H_c) + value_coef (v - t^)^2,
 *   loss = sum_rows w L / sum_rows w.
 * The KL is KL(pi || prior): the expectation runs over the CURRENT policy (lib/action_head.py:198-203, kl_divergence(pi, prior)).  The value term is
 * lib/scaled_mse_head.py:37-43: `value` is the raw head output (normalised space, element r at value[r * value_stride] -- the value column of the
 * fused head logits), value_target the denormalised return, vnorm a DEVICE pair (mean, std) of the normaliser (lib/normalize_ewma.py:27-31,55).
 * prior_buttons / prior_camera may both be NULL (no KL term, K = 0), value may be NULL (no value term; value_target and vnorm are then not read),
 * weight may be NULL (all ones).  A coefficient of 0 skips its term.  Every output is optional (NULL):
 *   dz        16-bit [M][ldz], ldz >= nb + nc + 1:  rs [ c (onehot - p) + kl_coef p ((l - q) - K) + entropy_coef p (l + H) ] / temperature per head with
 *             c = -A rho, or 0 where (A > 0 and rho > 1 + clip) or (A < 0 and rho < 1 - clip) (the gradient of torch.min / clamp), rs = scale weight[row];
 *             column nb + nc: rs 2 value_coef (v - t^); further columns zero.  The caller folds 1 / sum w (and the fp16 loss scale) into `scale`.
 *   frame_out fp32 [M][16]: the surrogate -min(.), K_b, K_c, H_b, H_c, (v - t^)^2, rho, clipped (1 where c was zeroed), lp, old_log_prob - lp, w,
 *             1 if w > 0, then four zeros -- the frame's own, unweighted values;
 *   totals    fp32 [16]: sum_rows w frame_out[row][k] for k < 10, sum w, the number of rows with w > 0, zeros; added in a fixed order through `workspace`
 *             (vpt_workspace_bytes(VPT_WS_RL_LOSS, M, ...) bytes, required with totals; M <= 65536): no atomics, the same inputs give the same bits.
 * A row with weight 0 stores exact zeros in dz and adds exact zeros to totals whatever its inputs hold (NaN included); actions are only compared with
 * column indices.  With kl_coef = entropy_coef = value_coef = 0, A = 1 and rho = 1 the policy columns of dz are vpt_bc_loss's at scale / temperature. */
int vpt_rl_loss(const float* lp_buttons, const float* lp_camera, const float* prior_buttons, const float* prior_camera,
                const int64_t* act_buttons, const int64_t* act_camera, const float* old_log_prob, const float* advantage,
                const float* value, int64_t value_stride, const float* value_target, const float* vnorm, const float* weight,
                void* dz, float* frame_out, float* totals, float* workspace, int M, int nb, int nc, int ldz,
                float clip, float kl_coef, float entropy_coef, float value_coef, float temperature, float scale, void* stream);

/* The auxiliary ("sleep") phase of phasic policy gradient for one network with one value head: a cloning term that holds the policy at a snapshot
 * pi_old + the value loss, their gradient w.r.t. the fused head logits and their metrics in ONE sweep over the log-probs.  With l, m the log-probs of
 * the policy and of the snapshot, p = expf(l), o = expf(m), per head
 *   D = sum o (m - l)  (a term with o = 0 counts 0),   S = sum o  (the teacher's mass, a diagnostic),   t^ = (value_target - mean) / std,
 *   L_r = clone_coef (D_b + D_c) + value_coef (v - t^)^2,   loss = sum_rows w L / sum_rows w.
 * The KL is KL(pi_old || pi): the expectation runs over the STORED TEACHER -- the opposite direction of vpt_rl_loss's KL(pi || prior), whose
 * expectation runs over the current policy.  It is the cross-entropy to a soft label minus the label's own entropy; with a one-hot teacher (m = 0 at
 * the label, -inf elsewhere) D is vpt_bc_loss's NLL and the policy columns of dz are that kernel's, bit for bit.
 * The gradient convention: dz holds p - o, the gradient of D for a teacher whose mass is EXACTLY 1.  The exact gradient is p S - o; frame_out carries
 * S_b and S_c so that a caller sees how far a teacher is from 1 (a snapshot stored in fp32: a few 1e-7 per class).
 * value, value_target, vnorm and weight are vpt_rl_loss's (value may be NULL: no value term, value_target and vnorm are then not read); old_buttons and
 * old_camera are both required.  A coefficient of 0 skips its term.  A class with o > 0 and l = -inf (live at the snapshot, masked now) gives
 * D = +inf with a finite dz: take the snapshot under the same logit masks.  Every output is optional (NULL):
 *   dz        16-bit [M][ldz], ldz >= nb + nc + 1:  (clone_coef (p - o)) rst per head, rst = (scale weight[row]) / temperature;
 *             column nb + nc: ((2 value_coef) (v - t^)) (scale weight[row]); further columns zero.  The caller folds 1 / sum w (and the fp16 loss scale)
 *             into `scale`.
 *   frame_out fp32 [M][8]: D_b, D_c, (v - t^)^2, S_b, S_c, w, 1 if w > 0, 0 -- the frame's own, unweighted values;
 *   totals    fp32 [8]: sum_rows w frame_out[row][k] for k < 5, sum w, the number of rows with w > 0, 0; added in a fixed order through `workspace`
 *             (vpt_workspace_bytes(VPT_WS_PPG_AUX_LOSS, M, ...) bytes, required with totals; M <= 65536, -2 above it): no atomics, the same inputs
 *             give the same bits.
 * A row with weight 0 stores exact zeros in dz and adds exact zeros to totals whatever its inputs hold (NaN included). */
int vpt_ppg_aux_loss(const float* lp_buttons, const float* lp_camera, const float* old_buttons, const float* old_camera,
                     const float* value, int64_t value_stride, const float* value_target, const float* vnorm, const float* weight,
                     void* dz, float* frame_out, float* totals, float* workspace, int M, int nb, int nc, int ldz,
                     float clone_coef, float value_coef, float temperature, float scale, void* stream);

/* Generalised advantage estimation over [B][T] rollouts (reward, value fp32; first uint8: frame t starts an episode; last_value [B] and next_first [B]
 * describe the frame after the rollout; `value` and `ret` are denormalised, lib/scaled_mse_head.py:45-47):
 *   nt = !first[t+1] (t = T-1: !next_first),  delta = r + (nt ? gamma V_{t+1} : 0) - V,  adv = delta + (nt ? (gamma lambda) adv_{t+1} : 0),  ret = adv + V,
 * one lane per sequence walking back over t, in this order of fp32 operations without contraction: a float32 host loop reproduces it bit for bit. */
int vpt_gae(const float* reward, const float* value, const uint8_t* first, const float* last_value, const uint8_t* next_first,
            float* adv, float* ret, int B, int T, float gamma, float lam, void* stream);

/* ---- rollout collection for RL fine-tuning (no reference counterpart: the reference ships no RL loop) ---- */

/* One acting step of B environments into column t of [B][T] rollout buffers, one launch: what MinecraftAgentPolicy.act (lib/policy.py:307-331) hands out
 * per step -- the frame, its `first` flag, the sampled action indices, their summed log-prob and the de-normalised value -- lands where the training step
 * reads it.  img uint8 [B][frame_bytes] -> img_buf [B][T][frame_bytes] with 16-byte vector loads and stores (frame_bytes % 16 == 0, both pointers 16-byte
 * aligned; a 128 x 128 x 3 frame is 3072 vectors); first uint8 [B] -> first_buf [B][T] (stored as 0 / 1).  The four scalar inputs are read through ELEMENT
 * strides (environment b's value is at [b * stride], stride >= 0), so the views of vpt_act_epilogue's packed record (stride 4 int64s / 8 floats) and
 * contiguous arrays (stride 1) both go in without a copy.  nan_flag uint8 [1] is STICKY: a NaN among the stored log-probs stores 1 (a plain byte store, no
 * atomic: every writer writes the same value); no launch clears it -- the caller zeroes it when a rollout begins and reads it once when it ends.
 * t outside [0, T) is rejected with -1; B <= 65535. */
int vpt_rollout_record(const uint8_t* img, const uint8_t* first, const int64_t* act_buttons, const int64_t* act_camera, const float* log_prob,
                       const float* vpred, int64_t stride_buttons, int64_t stride_camera, int64_t stride_log_prob, int64_t stride_vpred,
                       uint8_t* img_buf, uint8_t* first_buf, int64_t* act_buttons_buf, int64_t* act_camera_buf, float* old_log_prob_buf, float* vpred_buf,
                       uint8_t* nan_flag, int B, int T, int t, int64_t frame_bytes, void* stream);

/* The environment's answer to step t, one lane per environment: reward fp32 [B], done uint8 [B] (the NEXT frame starts an episode).
 *   reward_buf[b][t] = r;  R = ep_return[b] + r;  n = ep_length[b] + 1;
 *   done:      done_return[b][t] = R, done_length[b][t] = n, ep_return[b] = 0, ep_length[b] = 0;
 *   otherwise: done_return[b][t] = 0, done_length[b][t] = 0, ep_return[b] = R, ep_length[b] = n.
 * ep_return fp32 [B] / ep_length int32 [B] are the running totals of the episode in progress; the caller zeroes them once and keeps them across rollouts,
 * so an episode that spans two rollouts reports its whole return.  One fp32 add per lane per step, no contraction, no cross-lane reduction: a float32 host
 * loop reproduces every output bit for bit; totals over a rollout are the caller's sums over done_return / done_length. */
int vpt_rollout_reward(const float* reward, const uint8_t* done, float* reward_buf, float* done_return, int32_t* done_length, float* ep_return,
                       int32_t* ep_length, int B, int T, int t, void* stream);

/* ---- backward of the IMPALA CNN (behavioural_cloning.py:117-119 obtains these from torch autograd) ---- */

/* Per-element preparation of GN -> conv3x3 -> ReLU (+res) backward: dacc = rstd * dY * [v > 0] (blocked, Cout
 * channels); t12[f] = (T1, T2) = (sum dz (v - SA), sum dz SG) (optional output); coef[f] = (c0, c1) with
 * c1 = -rstd^2 T1 / n, c0 = -rstd T2 / n - c1 mu, the statistics terms vpt_conv3x3_dgrad adds as c0 + c1 x;
 * d_sa / d_sg [9][CoutPad] += sum dz / sum dz (-rstd mu) (accumulated: caller zeroes once per step).
 * stats_in are the statistics of the layer's INPUT (Cin*H*W elements).  With dy = NULL the layer is followed by the
 * max-pool and (dpooled, argmax) are given instead: the pool's backward is applied on the fly.  scratch: fp32 work buffer of
 * vpt_workspace_bytes(VPT_WS_CONV_BACKWARD_PREPARE, frames, 0, 0, 0, Cout) bytes (per-frame sums, then per-32-frame partial sums of d_sa / d_sg that
 * are added in a fixed order).  W in {8, 16, 32, 64} runs the tuned kernel; with dy given any other W >= 2 is served by a slower
 * pixel-per-thread kernel (the (dpooled, argmax) entry keeps the restriction). */
int vpt_conv_backward_prepare(const void* dy, const void* dpooled, const uint8_t* argmax, const void* y, const void* res,
                              const double* stats_in, const float* edge_sa, const float* edge_sg, void* dacc, double* t12,
                              float* coef, float* d_sa, float* d_sg, float* scratch, int frames, int H, int W, int Cin, int Cout, void* stream);

/* Input gradient of the layer: dx = conv^T(W', dacc) + skip + coef[f][0] + coef[f][1] * xin, i.e. the implicit-GEMM
 * kernel of vpt_conv3x3_forward on the transposed, spatially flipped weights (wpk_t: [ceil(Cin/128)][Cout/32][9][128][32])
 * with the GroupNorm-statistics terms c0_f + c1_f x added in its epilogue.  dacc has Cout channels, dx / xin / skip Cin.
 * xin and coef are required (rejected with -1 otherwise); skip may be NULL. */
int vpt_conv3x3_dgrad(const void* dacc, const void* wpk_t, const void* skip, const void* xin, const float* coef, void* dx,
                      int frames, int H, int W, int Cout, int Cin, void* stream);

/* Round 5: a block's conv1 -> conv0 backward without the per-element pass in between (lib/impala_cnn.py:50-52 under
 * behavioural_cloning.py:117-119).  vpt_conv3x3_dgrad_gated is vpt_conv3x3_dgrad (no skip) whose epilogue applies the NEXT layer-to-
 * differentiate's ReLU gate and statistic scale: xin is conv0's output y (conv1's input), conv0 has no residual, so
 *     dacc_out = rstd_g[f] * (conv^T(W', dacc) + c0 + c1 xin) * [xin > 0]
 * IS conv0's backward operand (what vpt_conv_backward_prepare(dy, y, res = NULL) would have written), rstd_g from gate_stats = the frame
 * statistics of conv0's INPUT over gate_cin * H * W elements; gate_u[f] += rstd_g * sum dy * xin (accumulated: caller zeroes).
 * vpt_conv_backward_reduce then produces what prepare produces besides dacc -- t12, coef, d_sa / d_sg -- from dacc_out and gate_u alone
 * (one read of one tensor instead of two reads and a write).  scratch as for vpt_conv_backward_prepare. */
int vpt_conv3x3_dgrad_gated(const void* dacc, const void* wpk_t, const void* xin, const float* coef, const double* gate_stats, int gate_cin,
                            void* dacc_out, double* gate_u, int frames, int H, int W, int Cout, int Cin, void* stream);
int vpt_conv_backward_reduce(const void* dacc, const double* gate_u, const double* stats_in, const float* edge_sa, const float* edge_sg,
                             double* t12, float* coef, float* d_sa, float* d_sg, float* scratch, int frames, int H, int W, int Cin, int Cout, void* stream);

/* vpt_conv_backward_prepare for the layer in front of the max-pool when its forward was vpt_conv3x3_pool_argmax_forward: (dpooled, pooled,
 * pool_mask) [F][Cout/32][H/2][W/2][32] in, dacc [F][Cout/32][H][W][32] and the same sums out.  The ReLU gate is [pooled > 0], the value at
 * the arg-max is the pooled value itself.  H, W: the PRE-pool size (W in {16, 32, 64, 128}; 128 -- stack 0 of the
 * inverse dynamics model -- runs one pooled row per pass).
 * n_gain != NULL: the stack's GroupNorm `n` (lib/impala_cnn.py:118-119) sits between the pool and the incoming gradient and its backward is applied
 * on the fly -- `dpooled` is then G = d loss / d n(pooled), pool_stats [F][2] the frame statistics of pooled and pool_ab [F][2] the sums of
 * vpt_frame_affine_backward's pass 1 (sum G gain, sum G gain xhat): d(pooled) = r (G gain - ab0 / n - xhat ab1 / n) is formed per element with the
 * separate pass's arithmetic and 16-bit rounding point, and vpt_frame_affine_backward's pass 2 is not run for this stack. */
int vpt_conv_backward_prepare_pooled(const void* dpooled, const void* pooled, const void* pool_mask, const double* stats_in, const float* edge_sa, const float* edge_sg,
                                     void* dacc, double* t12, float* coef, float* d_sa, float* d_sg, float* scratch,
                                     const float* n_gain, const double* pool_stats, const double* pool_ab, int frames, int H, int W, int Cin, int Cout, void* stream);

/* Backward of vpt_conv_first_forward w.r.t. its weight and bias (the input is the uint8 image): recomputes the pre-pool
 * tile, routes dpooled to the arg-max conv pixel of every pooling window and accumulates dw[Cout][27] (kh, kw, ch order)
 * and db[Cout] (caller zeroes) -- per-workgroup partial sums in `partials` (VPT_WS_CONV_FIRST_BACKWARD (frames, H, W, -, Cout) bytes), added in
 * a fixed order. */
int vpt_conv_first_backward(const uint8_t* img, const void* wfrag, const void* dpooled, float* dw, float* db, float* partials,
                            int frames, int H, int W, int Cout, void* stream);
/* ... with the stack's GroupNorm `n` backward (lib/impala_cnn.py:118-119) applied on the fly, as vpt_conv_backward_prepare_pooled does for stacks 1..:
 * `g` is d loss / d n(pooled), n_gain [Cout] the norm's gain, pool_stats [F][2] the frame statistics of the pooled tensor and pool_ab [F][2] the sums of
 * vpt_frame_affine_backward's pass 1.  d(pooled) = r (g gain - ab0 / n - xhat ab1 / n) is formed per element with the separate pass's arithmetic and 16-bit
 * rounding point; the pooled VALUE it needs is the window maximum the kernel's arg-max search finds anyway.  vpt_frame_affine_backward's pass 2 is not run
 * for stack 0. */
int vpt_conv_first_backward_nfold(const uint8_t* img, const void* wfrag, const void* g, const float* n_gain, const double* pool_stats, const double* pool_ab,
                                  float* dw, float* db, float* partials, int frames, int H, int W, int Cout, void* stream);

/* Weight gradient of the folded convolution: dw[o][tap][c] += sum_{f,p} dacc[f][o][p] * x[f][c][p + tap] (fp32; caller
 * zeroes or accumulates).  W in {16, 32, 64, 128} (128: one LDS buffer instead of two, not tuned).  scratch: fp32 work buffer of vpt_conv3x3_wgrad_scratch_floats() elements
 * (per-frame-group partial sums).  The host maps dw to dW, dgain, dbias (cnn_training.py). */
long vpt_conv3x3_wgrad_scratch_floats(int frames, int Cin, int Cout);
int vpt_conv3x3_wgrad(const void* dacc, const void* x, float* dw, float* scratch, int frames, int H, int W, int Cin, int Cout, void* stream);

/* F.max_pool2d(3, 2, 1) backward with torch's first-maximum tie rule. */
int vpt_maxpool_backward(const void* pre, const void* pooled, const void* dpooled, void* dpre,
                         int frames, int C, int H, int W, void* stream);

/* Backward of vpt_frame_affine_forward.  pass 1: ab[f] += (sum dy g, sum dy g xhat) and (per_element = 0) dgain/dbias;
 * pass 2: dx = rstd (dy g - ab0/n - xhat ab1/n) + dx_add; pass 3 (per_element = 1): dgain/dbias reduced over frames.
 * partials: fp32 workspace of VPT_WS_FRAME_AFFINE_BACKWARD (frames, HW, per_element, pass, C) bytes (0 for pass 2 and for pass 1 with
 * per_element = 1: may be NULL there): dgain / dbias are summed through it in a fixed order. */
int vpt_frame_affine_backward(const void* x, const void* dy, const void* dx_add, void* dx, const float* gain,
                              const double* stats_in, double* ab, float* dgain, float* dbias, float* partials,
                              int frames, int C, int HW, int per_element, int pass, void* stream);

/* ---- action codec on the device: int64 / fp64 arrays, one row per action ---- */

/* CameraQuantizer.discretize / undiscretize (lib/actions.py:88-108): n scalars (both camera axes flattened); mu_law = 1
 * selects the mu-law companding of agent.py:40-45 (maxval 10, binsize 2, mu 10), 0 the linear scheme.  fp64 arithmetic,
 * round-half-to-even like np.round. */
int vpt_camera_discretize(const double* xy, long* bins, long n, double maxval, double binsize, double mu, int mu_law, void* stream);
int vpt_camera_undiscretize(const long* bins, double* xy, long n, double maxval, double binsize, double mu, int mu_law, void* stream);

/* CameraHierarchicalMapping.from_factored / to_factored (lib/action_mapping.py:179-219): buttons int64 [n][20] in
 * Buttons.ALL order (lib/actions.py:21-33), camera int64 [n][2] bins <-> joint_buttons int64 [n] in 0..8640 and
 * joint_camera int64 [n] in 0..n_camera_bins^2-1.  Inputs are not validated (the reference raises KeyError on bins
 * outside the grid). */
int vpt_action_from_factored(const long* buttons, const long* camera, long* joint_buttons, long* joint_camera, long n, int n_camera_bins, void* stream);
int vpt_action_to_factored(const long* joint_buttons, const long* joint_camera, long* buttons, long* camera, long n, int n_camera_bins, void* stream);

/* ---- IDM video labelling on the device ---- */

/* y[i][:] = x[index[i]][:]: fp32 rows of D values, D % 4 == 0, x and y 16-byte aligned; x [rows_in][D], index int32 [n], y [n][D].
 * An index outside [0, rows_in) gives a row of zeros.  The windows of a video as lists of feature rows: replaces the host-side
 * windowing of the pixels in run_inverse_dynamics_model.py:146-163 (one agent.predict_actions(frames) per batch of frames). */
int vpt_gather_rows(const float* x, const int32_t* index, float* y, long rows_in, long n, int D, void* stream);

/* IDM log-probs -> labels, one launch over n frames.  Replaces InverseActionPolicy.predict's deterministic sample and log-prob
 * (lib/policy.py:448-464 over lib/action_head.py:176-207) and IDMAgent._agent_action_to_env (inverse_dynamics_model.py:61-72:
 * `.cpu().numpy()`, then the host's action mapping).  lp_buttons fp32 [n][20][2], lp_camera fp32 [n][2][n_camera_bins] ->
 *   buttons int64 [n][20], camera int64 [n][2]: arg-max per group, the lowest index on ties (torch.argmax);
 *   log_prob fp32 [n]: the 22 chosen log-probs added left to right in fp32, buttons first;
 *   joint_buttons, joint_camera int64 [n]: vpt_action_from_factored of (buttons, camera) (lib/action_mapping.py:179-207);
 *   camera_deg fp64 [n][2]: vpt_camera_undiscretize of camera (lib/actions.py:100-108) with (maxval, binsize, mu, mu_law);
 *   null_flag uint8 [n]: 1 iff no button is pressed and both camera bins are the centre bin n_camera_bins / 2 -- the frames the
 *   reference's loader drops (data_loader.py:48-128). */
int vpt_idm_decode(const float* lp_buttons, const float* lp_camera, int64_t* buttons, int64_t* camera, float* log_prob, int64_t* joint_buttons,
                   int64_t* joint_camera, double* camera_deg, uint8_t* null_flag, long n, int n_camera_bins, double maxval, double binsize, double mu,
                   int mu_law, void* stream);

/* ---- clip data path on the device ---- */

/* One launch turns `frames` decoded video frames (uint8 BGR [frames][height][width][3], as cv2.VideoCapture.read() returns
 * them) into the policy's input frames (uint8 RGB [frames][out_height][out_width][3]): the per-frame body of
 * data_loader.py:113-122 = composite_images_with_alpha (data_loader.py:34-46) where cursor_state[f] = (gui open, x, y) says a
 * GUI is open (x, y >= 0: the cursor's top-left corner, already scaled by height / 720), cv2.cvtColor(BGR2RGB) and
 * resize_image = cv2.resize(.., (out_width, out_height), INTER_LINEAR) (agent.py:100-103).  Bit-identical to that CPU path:
 * fp64 blend truncated like astype(uint8); OpenCV's 11-bit fixed-point bilinear (exact 2 x 2 decimation -> INTER_AREA).
 * cursor_state may be null (no compositing); cursor_bgr [cursor_h][cursor_w][3], cursor_alpha fp64 [cursor_h][cursor_w] in 0..1. */
int vpt_clip_frames(const uint8_t* src_bgr, int frames, int height, int width, const int32_t* cursor_state, const uint8_t* cursor_bgr,
                    const double* cursor_alpha, int cursor_h, int cursor_w, uint8_t* dst_rgb, int out_height, int out_width, void* stream);

/* ---- sequence-consistent frame augmentation (no reference counterpart: the reference trains on the loader's frames as they are) ---- */

/* out[frames][9] = the nine uniforms in [0, 1) of each frame, a pure function of (seed, epoch, keys[f]): Philox4x32-10 with key (seed lo, seed hi),
 * counter (draw >> 2, key lo, key hi, epoch), word draw & 3, u = (word >> 8) * 2^-24.  Draw order: hue, saturation, brightness, contrast, rotation,
 * scale, shear, tx, ty.  Frames with equal keys (a recording's id) get equal draws, in whichever launch they appear. */
int vpt_augment_uniforms(const int64_t* keys, float* out, long frames, uint64_t seed, uint32_t epoch, void* stream);
/* dst[f] = frame src[f] (uint8 [frames][H][W][3]) under tables[f] (fp32 [frames][16]: colour matrix C[3][3] row-major, mean gain k, inverse map G[2][3]
 * from an output pixel index (x, y) to a source pixel index):
 *   v_c = bilinear taps of channel c at ((G00 x + G01 y) + G02, (G10 x + G11 y) + G12), 0 outside the frame;
 *   out_c = (uint8) rint(min(max(((C[c][0] v_0 + C[c][1] v_1) + C[c][2] v_2) + k mu, 0), 255)),  mu = sum(77 R + 150 G + 29 B) / (256 H W) of the frame.
 * Fixed fp32 arithmetic without fused multiply-adds (csrc/vpt_augment_pixel.h); no table contents make it read outside a frame (non-finite coordinates
 * take the fill value).  H * W * 3 <= 65536 (the frame is staged in LDS), else -5.  dst may be src itself (in place); other overlaps are not supported. */
int vpt_augment_frames(const uint8_t* src, const float* tables, uint8_t* dst, long frames, int H, int W, void* stream);

/* ---- diagnostics ---- */

/* Fill the LDS of every compute unit with NaN bit patterns (0x7fc07fc0: a NaN as fp32 and as either 16-bit operand format), enqueued on
 * `stream`.  A kernel that reads LDS before writing it then produces NaN instead of whatever the previous workgroup on that CU left behind
 * (tools/diag_r06.py, VPT_POISON_LDS=1 in ops.py).  No reference counterpart; never on a product path. */
int vpt_debug_poison_lds(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPT_HIP_H */
