/* ia2p.h -- C ABI of libia2p_hip.so: the MI355X (gfx950) denoise hot path of InstructAny2Pix.
 *
 * The reference (pure Python, no FFI of its own) reaches this path through three seams; each entry point
 * below names the reference interface it stands in for (paths relative to the reference checkout):
 *
 *   UNet callable   unet(sample, t, encoder_hidden_states=, added_cond_kwargs={text_embeds,time_ids})[0]
 *                   instructany2pix/ddim/pnp_pipeline.py:253-260, instructany2pix/ddim/sdxl_pipeline.py:832-839
 *                   -> ia2p_unet_forward
 *   operator plugin attn.processor(attn, hidden_states, encoder_hidden_states)
 *                   instructany2pix/diffusion/ip_adapter/attention_processor.py:205-279 (AttnProcessor2_0),
 *                   :310-412 (IPAttnProcessor2_0); installed by ip_adapter.py:120-142, scale set by :211-214
 *                   -> ia2p_set_ip_adapter, ia2p_attention / ia2p_qproj_attention (+ ia2p_gemm for the projections);
 *                   with regional image prompts (diffusers' `ip_adapter_masks`, new here: one token group per subject, each under
 *                   its own mask) -> ia2p_attention_regions + ia2p_region_levels, and ia2p_unet_forward_r on the UNet callable
 *   sampler update  _backward_ddim pnp_pipeline.py:73-85; CFG combine sdxl_pipeline.py:842-844;
 *                   DDIMScheduler.step (diffusers 0.26.3) called at sdxl_pipeline.py:851
 *                   -> ia2p_ddim_step
 *
 * Conventions: plain pointers and sizes only (no torch types); every `const void*` / `void*` tensor argument
 * is a DEVICE pointer to fp16 data unless stated otherwise; kernels are enqueued on the caller's HIP stream
 * (`stream` is a hipStream_t passed as void*, NULL = default stream) with no hidden synchronisation;
 * functions return IA2P_OK or an error code and never abort; ia2p_last_error() gives the message.
 * A context is bound to the device that was current at ia2p_create and is not re-entrant.
 * Activations inside the library are channels-last ([B*H*W, C]); the latent boundary is NCHW like the reference.
 */
#ifndef IA2P_H
#define IA2P_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ia2p_ctx ia2p_ctx;

typedef enum {
  IA2P_OK = 0,
  IA2P_ERR_INVALID = 1,   /* bad argument (null pointer, negative size, unknown enum) */
  IA2P_ERR_SHAPE = 2,     /* shape / divisibility constraint violated */
  IA2P_ERR_KEY = 3,       /* unknown or duplicate parameter key, or parameters missing at finalize */
  IA2P_ERR_STATE = 4,     /* call order (weights not finalized, arena not bound, ...) */
  IA2P_ERR_NOMEM = 5,     /* arena / workspace too small */
  IA2P_ERR_HIP = 6,       /* HIP runtime error */
  IA2P_ERR_ARCH = 7       /* current device is not gfx950 */
} ia2p_status;

#define IA2P_MAX_BLOCKS 4

/* Mirrors the fields of diffusers' unet/config.json the reference reads (pnp_pipeline.py:44-47, ip_adapter.py:114,124-132). */
typedef struct {
  int in_channels, out_channels;
  int n_blocks;
  int block_out_channels[IA2P_MAX_BLOCKS];
  int transformer_layers_per_block[IA2P_MAX_BLOCKS];   /* 0 = no attention in that block */
  int num_heads[IA2P_MAX_BLOCKS];                      /* diffusers "attention_head_dim" (head counts for SDXL) */
  int layers_per_block;
  int cross_attention_dim;
  int norm_num_groups;
  float norm_eps;
  int addition_time_embed_dim;
  int projection_class_embeddings_input_dim;
  int time_embed_dim;
  int time_proj_dim;
  int mid_transformer_layers;   /* transformer layers of the mid block; < 0 = transformer_layers_per_block[n_blocks-1] (SDXL base). The
                                 * SDXL refiner (pipeline.py:128-131) ends in a plain DownBlock2D but has 4 layers in its mid block. */
  int num_time_ids;             /* micro-conditioning ids per sample: 6 (base: sizes + crop), 5 (refiner: + aesthetic score); <= 0 = 6 */
} ia2p_unet_config;

/* ---- lifetime ---------------------------------------------------------------------------------------------- */
ia2p_status ia2p_create(const ia2p_unet_config* cfg, ia2p_ctx** out);
void ia2p_destroy(ia2p_ctx* ctx);
const char* ia2p_last_error(ia2p_ctx* ctx);            /* ctx may be NULL: error of the failed ia2p_create */
int ia2p_device_is_gfx950(void);

/* ---- weights: one flat, position-deterministic arena (so ranks can RCCL-broadcast it as one buffer) ---------- */
size_t ia2p_arena_bytes(ia2p_ctx* ctx);
ia2p_status ia2p_bind_arena(ia2p_ctx* ctx, void* dev_arena, size_t bytes);   /* caller owns the memory */
/* Load one parameter by its diffusers state-dict key (e.g. "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight")
 * or IP-Adapter key ("ip_adapter.<idx>.to_k_ip.weight", idx = position in unet.attn_processors; ip_adapter.py:168-169).
 * `dev_src` is fp16 in the checkpoint's own layout; it is re-laid-out into the arena on `stream`. */
ia2p_status ia2p_load_tensor(ia2p_ctx* ctx, const char* key, const void* dev_src, const int64_t* shape, int ndim, void* stream);
/* The inverse of ia2p_load_tensor: the parameter `key` back in the checkpoint's own layout, fp16, into `dev_dst` on `stream` (the 3x3 convolutions from [Co][tap][Ci]
 * to [Co][Ci][3][3], the GEGLU pairing undone, conv_in without its padding: the re-layouts are permutations, so load then read returns the loaded bits). Same key,
 * shape and state checks as ia2p_load_tensor; a key that was never loaded (an IP-Adapter tensor of a UNet without one) is refused with IA2P_ERR_STATE. */
ia2p_status ia2p_read_tensor(ia2p_ctx* ctx, const char* key, void* dev_dst, const int64_t* shape, int ndim, void* stream);
ia2p_status ia2p_finalize_weights(ia2p_ctx* ctx);      /* verifies every UNet parameter was loaded; derives the LayerNorm-folded copies */
/* A tensor (re)loaded after finalize marks the derived data stale; the next forward re-derives it on its stream before running.
 * The arena is [head | tail]: head = the parameters as loaded (ia2p_arena_raw_bytes; what a data-parallel rank must RECEIVE), tail = data
 * derived from them at finalize (LayerNorm-folded weight copies, +43 %). ia2p_adopt_arena: the head was filled elsewhere (RCCL broadcast
 * from the rank that read the checkpoint) -- marks the UNet parameters (and, with_ip_adapter != 0, the IP-Adapter
 * tensors) present and derives the tail locally. */
size_t ia2p_arena_raw_bytes(ia2p_ctx* ctx);
ia2p_status ia2p_adopt_arena(ia2p_ctx* ctx, int with_ip_adapter);
/* the same with the fold kernels ordered on `stream` -- the stream the broadcast that filled the head was enqueued on -- and synchronised there */
ia2p_status ia2p_adopt_arena_on(ia2p_ctx* ctx, int with_ip_adapter, void* stream);
/* The weight distribution of the batch-data-parallel path as ONE call (BASELINE north_star: "RCCL broadcast of UNet weights over xGMI"; the reference itself is
 * single-GPU: pipeline.py:124,131 place one model on one device): ncclBroadcast of the arena head [0, ia2p_arena_raw_bytes) from rank `root` on the caller's
 * communicator and stream, in <= 1 GiB messages, then -- on every rank but `root` -- ia2p_adopt_arena_on (the LayerNorm-folded tail is derived per rank, 2.5 GB stay
 * off xGMI). `rccl_comm` is an ncclComm_t passed as void*, created by the host on the CURRENT device (one process per GPU); the rank is read from it. The stream is
 * synchronised before the call returns. RCCL is bound at run time from the instance already in the process (a PyTorch host: torch's bundled librccl.so.1), else
 * librccl.so.1 is loaded: the library has no link-time dependency on it (ia2p_rccl_available: 1 when the symbols resolved). Every rank of the communicator must call. */
ia2p_status ia2p_bcast_arena(ia2p_ctx* ctx, void* rccl_comm, int root, int with_ip_adapter, void* stream);
int ia2p_rccl_available(void);
/* GroupNorm + SiLU of the ResnetBlock2Ds (reference: diffusers ResnetBlock2D.norm1 / norm2 behind pnp_pipeline.py:253-260): 1 (default; IA2P_GN_FUSE) = applied inside the
 * halo-staged 3x3 convolution that consumes it, statistics from the producers' epilogues; 0 = GroupNorm launches of their own (round 4's path); 2 = the fused path's
 * unfused twin (the same statistics, ia2p_gn_apply_stats-style passes + plain convolutions: bit-identical to 1, for tests). Workspace sizes are valid for every mode. */
ia2p_status ia2p_set_gn_fuse(ia2p_ctx* ctx, int mode);
/* IP-Adapter plugin state: set_ip_adapter (ip_adapter.py:120-142) / set_scale (:211-214) / disable (:153-154). */
ia2p_status ia2p_set_ip_adapter(ia2p_ctx* ctx, int enabled, int num_tokens, float scale);

/* ---- the UNet callable -------------------------------------------------------------------------------------------
 * One evaluation is one record. Zero the record, set struct_size = sizeof(ia2p_unet_call), fill what the call uses. A size below the record as first published (it
 * ended with mid_residual) or above this library's own is IA2P_ERR_INVALID; fields a caller's older header did not have read as zero. Tensors are fp16 on the device:
 * sample, out [B, in/out_channels, h, w] NCHW; context [B, L, cross_attention_dim]; text_embeds [B, pooled]; time_ids [B, num_time_ids]. With the IP-Adapter enabled the
 * last num_tokens rows of each context are the image tokens.
 *
 *   field(s)                          may be set when                                                       otherwise
 *   context | kv                      exactly one: context, or its projections -- ia2p_project_context      IA2P_ERR_INVALID
 *   timestep                          timesteps == NULL: one timestep for the batch, by value               (ignored)
 *   timesteps   device float [B]      always; REQUIRED with ip_scales, regions or residuals                 IA2P_ERR_INVALID
 *   ip_scales   device float [B]      the IP-Adapter is enabled -- ia2p_set_ip_adapter                      IA2P_ERR_STATE
 *   region_masks, G                   together; 1 <= G <= 16 (IA2P_ERR_SHAPE); the adapter enabled with      IA2P_ERR_STATE
 *     fp16 [B, G, h, w]               num_tokens = 4 G; no residuals in the same call                       IA2P_ERR_INVALID
 *   down_residuals, n_down,           together; n_down == ia2p_unet_num_skips (IA2P_ERR_SHAPE); every        IA2P_ERR_INVALID
 *     mid_residual                    pointer non-NULL and 16-byte aligned; no regions in the same call     IA2P_ERR_INVALID
 *   the handle                        a UNet context (a ControlNet's: IA2P_ERR_STATE), weights finalized    IA2P_ERR_STATE
 *   B, h, w, L                        as ia2p_workspace_bytes accepts them                                  IA2P_ERR_SHAPE
 *
 * Every refusal comes before any launch. The workspace query reads B, h, w, L and G only (pointers may be NULL; residuals need no more than the plain pass; a regional
 * pass needs the plain pass's workspace plus the mask pyramid); 0 on a refusal. The argument-list forms below are thin callers of the record form. */
typedef struct ia2p_unet_call {
  uint32_t struct_size;
  int B, h, w, L;
  int G;                               /* token groups of region_masks; 0: no regions */
  int n_down;                          /* entries of down_residuals; 0: no residuals */
  float timestep;
  const void* sample;
  const void* context;
  const void* kv;
  const void* text_embeds;
  const void* time_ids;
  void* out;
  const float* timesteps;
  const float* ip_scales;
  const void* region_masks;
  const void* const* down_residuals;   /* residual k: channels-last [B * H_k * W_k, C_k], skip order */
  const void* mid_residual;
} ia2p_unet_call;
size_t ia2p_workspace_bytes_x(ia2p_ctx* ctx, const ia2p_unet_call* call);
ia2p_status ia2p_unet_forward_x(ia2p_ctx* ctx, void* stream, const ia2p_unet_call* call, void* workspace, size_t workspace_bytes);

size_t ia2p_workspace_bytes(ia2p_ctx* ctx, int B, int h, int w, int L);
/* sample, out: [B, in/out_channels, h, w] NCHW; context: [B, L, cross_attention_dim]; text_embeds: [B, pooled];
 * time_ids: [B, num_time_ids]. With the IP-Adapter enabled the last num_tokens rows of each context are the image tokens. */
ia2p_status ia2p_unet_forward(ia2p_ctx* ctx, void* stream, const void* sample, float timestep, const void* context, int L,
                              const void* text_embeds, const void* time_ids, void* out, int B, int h, int w,
                              void* workspace, size_t workspace_bytes);
/* Per-request knobs inside ONE evaluation (batched serving of independent edit requests). timesteps: device, float [B], one
 * timestep per batch element (diffusers' UNet2DConditionModel.forward accepts a [B] timestep tensor; the reference always passes a scalar,
 * pnp_pipeline.py:253-260 / sdxl_pipeline.py:832-839, because it serves one request at a time). ip_scales: device, float [B], or NULL --
 * the IP-Adapter scale of each batch element (reference: one `set_scale` value per call, ip_adapter.py:211-214; used at
 * attention_processor.py:397). Exactly one of context / kv (ia2p_project_context) is non-NULL. Batch element b gets the bits it gets in a
 * uniform batch of the same size evaluated at (timesteps[b], ip_scales[b]). */
ia2p_status ia2p_unet_forward_v(ia2p_ctx* ctx, void* stream, const void* sample, const float* timesteps, const float* ip_scales,
                                const void* context, const void* kv, int L, const void* text_embeds, const void* time_ids, void* out,
                                int B, int h, int w, void* workspace, size_t workspace_bytes);
/* ia2p_unet_forward_v with regional image prompts (what diffusers offers as cross_attention_kwargs={"ip_adapter_masks": ...}; the reference repaints one subject per
 * inpainting loop, gdino/lib.py:85-103). The adapter's image tokens are G groups of four (one group per subject; ia2p_set_ip_adapter(1, 4 G, scale) first, else
 * IA2P_ERR_STATE); group g acts on the queries of every cross-attention site under region_masks[b, g] -- fp16 [B, G, h, w] on the latent grid, device, any finite
 * values -- pooled to the site's resolution by the block mean (ia2p_region_levels: one launch per distinct attention resolution, once per forward, into the
 * workspace). Every cross-attention site runs its q GEMM and ia2p_attention_regions (the fused to_q launch has no regional form). Both routes to the context K/V
 * work: `context` (projected in the step, Li = 4 G image-token rows) or `kv` (ia2p_project_context under the same ia2p_set_ip_adapter state). The workspace is
 * sized by ia2p_workspace_bytes_r (the plain pass's plus the pyramid; 0 on a bad shape); ia2p_workspace_bytes is unchanged. No allocation, no synchronisation. */
size_t ia2p_workspace_bytes_r(ia2p_ctx* ctx, int B, int h, int w, int L, int G);
ia2p_status ia2p_unet_forward_r(ia2p_ctx* ctx, void* stream, const void* sample, const float* timesteps, const float* ip_scales,
                                const void* context, const void* kv, int L, const void* text_embeds, const void* time_ids, void* out,
                                int B, int h, int w, void* workspace, size_t workspace_bytes, const void* region_masks, int G);

/* ---- ControlNet: structure-guided sampling (diffusers 0.26.3 ControlNetModel + StableDiffusionXLControlNetPipeline) ---------------------------------------------------
 * New: the reference attaches no ControlNet (pipeline.py), it only prepares the attention seam -- IPAdapter.set_ip_adapter installs CNAttnProcessor on `pipe.controlnet`
 * when the pipe has one (diffusion/ip_adapter/ip_adapter.py:143-148), and CNAttnProcessor2_0 (attention_processor.py:481-568) cuts the image tokens off the context
 * (`encoder_hidden_states[:, :end_pos]`, :530-531). diffusers is not installed next to this library: parity with it is restated in tests/controlnet_ref.py, not pinned.
 *
 * A ControlNet is the UNet's conv_in, embeddings, down path and mid block under a second set of weights (same state-dict keys), plus
 *   controlnet_cond_embedding.{conv_in, blocks.0..5, conv_out}   eight 3x3 convolutions (pad 1, bias) over the condition image, RGB in [0, 1], [B, 3, 8 h, 8 w]:
 *       silu(conv_in 3 -> c0); for i < 3: silu(blocks[2 i]: c_i -> c_i, stride 1), silu(blocks[2 i + 1]: c_i -> c_(i+1), stride 2); conv_out c3 -> block_out_channels[0]
 *   controlnet_down_blocks.k, controlnet_mid_block               1x1 "zero" convolutions, one per skip of the down path (skip order) and one for the mid block's output
 * Forward: x = conv_in(sample) + cond_embedding; embeddings, down path and mid block exactly the UNet's, on the TEXT rows of the context only (L - num_tokens rows);
 *   residual_k = fp16(scale_b * fp16(zero_conv_k(skip_k))), the mid residual likewise. The UNet adds residual_k to skip_k after the whole down path has run (the hidden
 *   state flowing down is the unmodified one) and the mid residual to the mid block's output: skip' = fp16(skip + residual).
 * Handle lifecycle as every executor's: create -> arena_bytes -> bind_arena -> load_tensor per key -> finalize_weights (checks exactly the key set above) -> queries,
 * embed once per request, forward per step. The handle is an ia2p_ctx of its own kind: the UNet entry points refuse it and the other way round (IA2P_ERR_STATE). */
typedef struct {
  ia2p_unet_config unet;                          /* block_out_channels, layers_per_block, cross_attention_dim as the UNet it guides; transformer_layers_per_block may differ */
  int conditioning_channels;                      /* 3 */
  int conditioning_embedding_out_channels[4];     /* (16, 32, 96, 256): multiples of 16 in 16 .. 256 */
} ia2p_controlnet_config;
ia2p_status ia2p_controlnet_create(const ia2p_controlnet_config* cfg, ia2p_ctx** out);
void ia2p_controlnet_destroy(ia2p_ctx* ctx);
const char* ia2p_controlnet_last_error(ia2p_ctx* ctx);
size_t ia2p_controlnet_arena_bytes(ia2p_ctx* ctx);
ia2p_status ia2p_controlnet_bind_arena(ia2p_ctx* ctx, void* dev_arena, size_t bytes);
ia2p_status ia2p_controlnet_load_tensor(ia2p_ctx* ctx, const char* key, const void* dev_src, const int64_t* shape, int ndim, void* stream);
ia2p_status ia2p_controlnet_finalize_weights(ia2p_ctx* ctx);
/* the contexts handed to this ControlNet end in `num_tokens` image-token rows it must not see (0: none; CNAttnProcessor's rule) */
ia2p_status ia2p_controlnet_set_image_tokens(ia2p_ctx* ctx, int num_tokens);
/* IA2P_OK when the residuals of `ctx` fit the skips of `unet` (block_out_channels, layers_per_block, in_channels, cross_attention_dim), else IA2P_ERR_SHAPE */
ia2p_status ia2p_controlnet_check_unet(ia2p_ctx* ctx, ia2p_ctx* unet);
int ia2p_controlnet_num_residuals(ia2p_ctx* ctx);                   /* skips + 1 (the mid residual is the last) */
/* the residual buffer of a forward at (B, h, w): its bytes (0 on a bad shape); offsets (elements), channels and grid of residual k, arrays of num_residuals or NULL.
 * Residual k is channels-last [B * hs[k] * ws[k], channels[k]], dense, back to back. */
size_t ia2p_controlnet_residual_layout(ia2p_ctx* ctx, int B, int h, int w, int64_t* offsets, int* channels, int* hs, int* ws);
/* condition embedding: image fp16 NCHW [B, conditioning_channels, 8 h, 8 w] -> out [B * h * w, block_out_channels[0]] channels-last (ia2p_controlnet_embed_bytes).
 * Depends on the image and the weights only: once per request. Workspace: ia2p_controlnet_embed_workspace_bytes. */
size_t ia2p_controlnet_embed_bytes(ia2p_ctx* ctx, int B, int h, int w);
size_t ia2p_controlnet_embed_workspace_bytes(ia2p_ctx* ctx, int B, int h, int w);
ia2p_status ia2p_controlnet_embed(ia2p_ctx* ctx, void* stream, const void* image, int B, int h, int w, void* out, size_t out_bytes, void* workspace, size_t workspace_bytes);
size_t ia2p_controlnet_workspace_bytes(ia2p_ctx* ctx, int B, int h, int w, int L);
size_t ia2p_controlnet_context_kv_bytes(ia2p_ctx* ctx, int B, int L);
ia2p_status ia2p_controlnet_project_context(ia2p_ctx* ctx, void* stream, const void* context, int L, int B, void* kv, size_t kv_bytes, void* workspace, size_t workspace_bytes);
/* one evaluation: the arguments of ia2p_unet_forward_v (timesteps device float [B]; exactly one of context [B, L, cross_attention_dim] / kv), cond = the embedded
 * condition, scales = device float [B] (conditioning_scale of batch element b). Writes num_residuals tensors into `residuals` (ia2p_controlnet_residual_layout). */
ia2p_status ia2p_controlnet_forward(ia2p_ctx* ctx, void* stream, const void* sample, const float* timesteps, const void* context, const void* kv, int L,
                                    const void* text_embeds, const void* time_ids, const void* cond, const float* scales, void* residuals, size_t residual_bytes,
                                    int B, int h, int w, void* workspace, size_t workspace_bytes);
/* ia2p_unet_forward_v plus the residuals: down_residuals[k] (k < n_down = ia2p_unet_num_skips) is added to skip k where the up path pops it, mid_residual to the mid
 * block's output -- in place in the workspace, by ia2p_residual_add_gnstats, which also renews the GroupNorm column sums the tensor carries (every ia2p_set_gn_fuse
 * mode sees the injected tensors). Needs no more workspace than the plain pass (ia2p_workspace_bytes_c == ia2p_workspace_bytes; the plain query and the plain pass's
 * allocation order are untouched). Refusals, all before any launch: a null pointer or a residual off the 16-byte grid (IA2P_ERR_INVALID), n_down != the UNet's skips
 * (IA2P_ERR_SHAPE), region_masks != NULL or G != 0 (IA2P_ERR_INVALID: the regional pass is not combined with a ControlNet; pass NULL, 0). */
size_t ia2p_workspace_bytes_c(ia2p_ctx* ctx, int B, int h, int w, int L);
int ia2p_unet_num_skips(ia2p_ctx* ctx);
ia2p_status ia2p_unet_forward_c(ia2p_ctx* ctx, void* stream, const void* sample, const float* timesteps, const float* ip_scales, const void* context, const void* kv,
                                int L, const void* text_embeds, const void* time_ids, void* out, int B, int h, int w, void* workspace, size_t workspace_bytes,
                                const void* const* down_residuals, int n_down, const void* mid_residual, const void* region_masks, int G);
/* the operators of the path, one by one:
 *   conv_in_act        ia2p_conv_in with an optional SiLU: y = fp16(silu(fp16(conv + bias))) for silu = 1 (the embedding's 3 -> 16 convolution)
 *   conv3x3_narrow     3x3, pad 1, stride 1 | 2 over channels-last x [B, H, W, Cin], Cin % 16 == 0 in 16 .. 256 (the widths ia2p_conv3x3 and ia2p_conv_in do not take),
 *                      Co % 16 == 0; Wp [Co][3][3][Cin] (ia2p_pack_conv_out); y [B, (H - 1) / stride + 1, (W - 1) / stride + 1, Co]; the same two roundings
 *   gemm_rowscale      C[m, :] = fp16(scales[m / HW] * fp16(A . W^T + bias)), scales device float [M / HW]; K % 64 == 0, N % 4 == 0, no K split
 *   residual_add_gnstats   y = fp16(x + r) over [M, C] (y may alias x; C % 8 == 0, 16-byte aligned tensors); gn_out != NULL: the GroupNorm column sums of y,
 *                      [M / rows][C][2] fp64 with rows a multiple of 16 dividing M -- to the bit what ia2p_gn_colstats returns for y */
ia2p_status ia2p_conv_in_act(void* stream, const void* x_nchw, const void* w_oihw, const void* bias, void* y_nhwc, void* w_scratch, int B, int Cin, int H, int W, int Co, int silu);
ia2p_status ia2p_conv3x3_narrow(void* stream, const void* x, const void* Wp, const void* bias, void* y, int B, int H, int W, int Cin, int Co, int stride, int silu);
ia2p_status ia2p_gemm_rowscale(void* stream, const void* A, const void* W, const void* bias, const float* scales, void* C, int M, int N, int K, int HW);
ia2p_status ia2p_residual_add_gnstats(void* stream, const void* x, const void* r, void* y, int M, int C, int rows, double* gn_out);

/* ---- context K/V hoisted out of the step (optional) ------------------------------------------------------------------
 * The K/V projections of every cross-attention layer (reference attention_processor.py:358-359,379-380) depend only on the context and the
 * weights; over the 25-50 denoise steps of a request the context does not change. ia2p_project_context computes them once into a caller-owned
 * buffer (ia2p_context_kv_bytes), ia2p_unet_forward_kv is ia2p_unet_forward reading them from there: same kernels, same bits, one 420-GFLOP GEMM
 * and 1.36 GB of weight streaming less per step. Re-project after changing the context, the weights, or ia2p_set_ip_adapter(enabled, tokens). */
size_t ia2p_context_kv_bytes(ia2p_ctx* ctx, int B, int L);
ia2p_status ia2p_project_context(ia2p_ctx* ctx, void* stream, const void* context, int L, int B, void* kv, size_t kv_bytes,
                                 void* workspace, size_t workspace_bytes);
ia2p_status ia2p_unet_forward_kv(ia2p_ctx* ctx, void* stream, const void* sample, float timestep, const void* kv, int L,
                                 const void* text_embeds, const void* time_ids, void* out, int B, int h, int w,
                                 void* workspace, size_t workspace_bytes);

/* ---- measured kernel plans (optional) ---------------------------------------------------------------------------- */
/* Same arguments as ia2p_unet_forward, plus reps (timed launches per candidate, <1 = 5). Runs one forward in which every
 * GEMM / conv site of a shape without a measured plan times its candidate (tile, K-split) plans in place and records the
 * fastest in a process-wide table that all later launches of that shape use; *sites (optional) = shapes measured.
 * `out` is scratch. Tile choice never changes results; a K-split choice changes fp32 summation order (deterministic per
 * choice), so export the table from one rank and import it on the others to keep ranks bit-identical. Without this call
 * the library uses its built-in cost model. Call ia2p_workspace_bytes again afterwards. New: the reference has no
 * counterpart (cuDNN/cuBLAS pick their kernels internally). */
ia2p_status ia2p_autotune(ia2p_ctx* ctx, void* stream, const void* sample, float timestep, const void* context, int L,
                          const void* text_embeds, const void* time_ids, void* out, int B, int h, int w,
                          void* workspace, size_t workspace_bytes, int reps, int* sites);
size_t ia2p_plan_export(char* buf, size_t len);   /* "M,N,K,conv,geglu,variant,splitk;..." -> buf; returns the length needed */
int ia2p_plan_import(const char* text);           /* entries read, -1 if malformed */
void ia2p_plan_clear(void);
unsigned long long ia2p_plan_generation(void);   /* changes whenever the table does: re-query ia2p_workspace_bytes then */

/* ---- sampler update --------------------------------------------------------------------------------------------- */
/* out = c_x * x + c_e * (eps_u + g * (eps_c - eps_u)); eps_c may be NULL (no guidance); out2 may be NULL. */
ia2p_status ia2p_ddim_step(void* stream, const void* x, const void* eps_u, const void* eps_c, float g, float c_x, float c_e,
                           void* out, void* out2, int64_t n);
/* the same update with per-request coefficients: coef = device float [B][3] = {g, c_x, c_e} of batch element b (`per` elements each), so that
 * requests with their own guidance scale (reference pipeline.py:303 `cfg`) at their own step of their own schedule share one launch */
ia2p_status ia2p_ddim_step_v(void* stream, const void* x, const void* eps_u, const void* eps_c, const float* coef, void* out, void* out2,
                             int B, int64_t per);
/* out = (1 - m) * (c0 * init + c1 * noise) + m * x with m = mask[b, 0, :, :] ([B,1,h,w], shared by the C channels): the per-step
 * blend of the inpainting loop behind `pipe_inpainting` (reference pipeline.py:132-139, gdino/lib.py:89-102; diffusers
 * StableDiffusionXLInpaintPipeline, 4-channel UNet branch). c0 = sqrt(abar_next), c1 = sqrt(1 - abar_next) re-noise the known
 * region to the next timestep (DDIM add_noise); c0 = 1, c1 = 0 after the last step. out2 may be NULL. HW = h * w. */
ia2p_status ia2p_mask_blend(void* stream, const void* x, const void* init, const void* noise, const void* mask, float c0, float c1,
                            void* out, void* out2, int B, int C, int64_t HW);
/* the same blend with per-request coefficients: coef = device float [B][2] = {c0, c1} of batch element b, so that the inpaint passes of several requests
 * (reference gdino/lib.py:85-103, one pass per subject, called from pipeline.py:363-368 one request at a time), each at its own step of its own
 * strength-shortened schedule, share one launch. A request that is through carries {1, 0}: over a {0, 1} mask it gets x back where m = 1 and init where
 * m = 0, bit for bit. Null pointers (out2 excepted): IA2P_ERR_INVALID; B, C or HW < 1: IA2P_ERR_SHAPE; both before any launch. */
ia2p_status ia2p_mask_blend_v(void* stream, const void* x, const void* init, const void* noise, const void* mask, const float* coef,
                              void* out, void* out2, int B, int C, int64_t HW);

/* ---- edit mask: an edit that leaves the rest of the base image alone (mask-guided decoding, DiffEdit: Couairon et al. 2022) -------------------------------
 * New: the reference repaints the whole image (pipeline.py:303-386 has no mask). Outside the mask every sampling step is replaced by the DDIM-inverted latents
 * of the same noise level, so the last step lands on the base latents themselves; the decoded image is composited with the base image in 8 bits.
 *
 * known_blend_v: x, out, out2 fp16 [B, C, HW]; known fp16 [levels, B, C, HW] (the inversion trajectory, level 0 = the base latents); level device int32 [B];
 *   mask fp16 [B, 1, HW].   out[b, c, p] = mask[b, p] != 0 ? x[b, c, p] : known[level[b]][b, c, p]   (+0 and -0 are both "0")
 *   A selection, not arithmetic: the 16-bit patterns are copied. out2 may be NULL; out may alias x. A level outside [0, levels) is clamped into it on the
 *   device (the host checks its table before the upload). Null pointers (out2 excepted): IA2P_ERR_INVALID; B, C, HW or levels < 1: IA2P_ERR_SHAPE.
 * mask_to_latent: mask u8 [B, H, W] -> out fp16 [B, 1, H / f, W / f]: 1.0 where any pixel of the cell's f x f block is >= 128, else 0.0.
 *   f outside 1 .. 64: IA2P_ERR_INVALID; H % f or W % f non-zero: IA2P_ERR_SHAPE.
 * mask_feather_u8: mask, out u8 [B, H, W] (out may not alias mask); workspace: B * H * W 16-bit sums (2-byte aligned; 16-byte aligned for the vector path).
 *   bin = 255 where q >= 128 else 0;  S = sum of bin over the (2 r + 1)^2 window, coordinates clamped to the image (edge replicate), exact;
 *   a = (S + A / 2) / A in integers, A = (2 r + 1)^2;  out = min(bin, a).   The ramp falls inside the mask only: out = 0 wherever the mask is 0, an all-ones
 *   mask gives 255 everywhere, r = 0 gives bin. Two launches (rows, columns). r outside 0 .. 64: IA2P_ERR_INVALID.
 * image_composite_u8: edited, base, out u8 [B, H, W, C] (C = 1 or 3, else IA2P_ERR_SHAPE), alpha u8 [B, H, W].
 *   out = (a * e + (255 - a) * b + 127) / 255 in integers: a = 255 gives e and a = 0 gives b, exactly. out may alias edited.
 * All four: more than 2^31 - 1 elements in one image tensor is IA2P_ERR_SHAPE (known_blend_v counts in 64 bits); every refusal comes before any launch. */
ia2p_status ia2p_known_blend_v(void* stream, const void* x, const void* known, const int32_t* level, const void* mask, void* out, void* out2, int B, int C,
                               int64_t HW, int levels);
ia2p_status ia2p_mask_to_latent(void* stream, const void* mask_u8, void* out, int B, int H, int W, int f);
ia2p_status ia2p_mask_feather_u8(void* stream, const void* mask_u8, void* out, void* workspace, int B, int H, int W, int r);
ia2p_status ia2p_image_composite_u8(void* stream, const void* edited, const void* base, const void* alpha, void* out, int B, int H, int W, int C);

/* ---- Seeded noise: every normal draw of an edit request from the request's own stream ------------------------------------------------------------------
 * THE NOISE RULE. A request has a 64-bit `seed`; each of its normal draws has a 32-bit `draw` id (table below). Element e of a draw is the FLAT index inside
 * the request's own tensor (the batch is not counted), e < 2^34. Its value comes from block j = e >> 2:
 *   (w0, w1, w2, w3) = Philox4x32-10 at counter (j, draw, 0, 1) under key (low half of seed, high half of seed).
 *   The last counter word is a domain tag: the token sampler draws at counter (step, 0, 0, 0), so one seed serves both without ever sharing a block.
 *   For pair p = (e & 3) >> 1:   u1 = ((w[2p] >> 8) + 1) * 2^-24   in (0, 1], exact in fp32
 *                                u2 = (w[2p + 1] >> 8) * 2^-24     in [0, 1)
 *                                r  = sqrt(-2 ln u1)
 *                                z  = r * cospi(2 u2) for even e,  r * sinpi(2 u2) for odd e
 *   The argument 2 u2 is exact, and |z| <= sqrt(48 ln 2) < 5.77. logf, sqrtf and sincospif at full accuracy (no native approximation), one fp32 product.
 *   The value is fp32; an fp16 output is its round-to-nearest-even.
 * A value depends on (seed, draw, e) ONLY: not on the batch, the row's place in a launch, the output pointer's alignment, the grid or the sub-range asked for.
 * Draw ids of an edit request (instructany2pix_amd/noise.py): 0 base-image VAE posterior, 1 polar-mixing noise, 2 posterior of the refiner hand-off
 * re-encode, 3 refiner start noise, 4 + k inpaint noise of subject pass k (k < 65532: the ids stay below the next one), 65536 = 1 << 16 the n noises of an
 * automatic edit mask (below; element k * per + e is element e of noise k), 65537 = (1 << 16) + 1 the step noise of the consistency sampler (lcm_step_v below).
 * seeds, draws (and alphas below): HOST arrays [B]. They travel by value in the kernel arguments, 8 rows per launch; a larger B goes in chunks of 8 rows, one launch
 * each. No call copies anything to the device, allocates or waits. Every refusal is decided on the host before any launch: a null (or misaligned) pointer is
 * IA2P_ERR_INVALID; B < 1, per < 1, a `first` that is negative or no multiple of 4, first + per > 2^34 are IA2P_ERR_SHAPE.
 *
 * randn_seeded: row b of out ([B, per] dense, fp32, or fp16 with out_is_f16 = 1; element-size alignment is enough) receives elements first .. first + per - 1
 *   of stream (seeds[b], draws[b]). Ownership is by element index; 16-byte stores where a row starts on a 16-byte boundary, scalar stores elsewhere. */
ia2p_status ia2p_randn_seeded(void* stream, void* out, int out_is_f16, int B, int64_t per, int64_t first, const uint64_t* seeds, const uint32_t* draws);
/* the VAE posterior sample from a seeded draw (diffusers DiagonalGaussianDistribution.sample, then the scaling): moments fp16 [B, 2 C, HW] = means | log-variances
 * as the encoder leaves them, out fp16 [B, C, HW]. With z the fp32 normal of element e = c HW + p:
 *   x = fp16(fmaf(exp(0.5 * clamp(logvar, -30, 20)), z, mean));   out = fp16(x * scaling_factor)        (fp32 arithmetic, full-accuracy expf) */
ia2p_status ia2p_posterior_sample_seeded(void* stream, const void* moments, void* out, int B, int C, int64_t HW, float scaling_factor, const uint64_t* seeds,
                                         const uint32_t* draws);
/* the reference's `polar_intrtpolate` (pipeline.py:295-300) per request on the device: x, y, out fp16 [B, per]; per request, with a = alphas[b] and b1 = 1 - a,
 *   n0 = |x|, n1 = |y|, ll = a x + b1 y (kept in fp32), nl = |ll|, out = fp16(ll * ((a n0 + b1 n1) / nl)).
 * The three sums of squares have ONE fixed association that depends on `per` alone, so a row's bits do not depend on B or on its place in the batch.
 * nl = 0 gives the reference's non-finite result; it is not an error. The arithmetic is fp32: it is NOT the bit pattern of the reference's CPU fp16 tensor ops. */
ia2p_status ia2p_polar_mix_v(void* stream, const void* x, const void* y, const float* alphas, void* out, int B, int64_t per);

/* ---- Consistency sampler: the step of a latent consistency model (Luo et al. 2023; diffusers LCMScheduler.step), with its noise drawn in the kernel -------
 * The reference only points at it (pipeline.py:102, a commented-out `build_sdxl_ip(lcm_lora=True)`). One step of the sampler is, per element,
 *   x0 = c_skip x + c_out (x - sqrt(1 - abar_t) eps) / sqrt(abar_t),   x_next = sqrt(abar_next) x0 + sqrt(1 - abar_next) z,   z fresh, none after the last step,
 * which the host collapses to three numbers per request and step (instructany2pix_amd/scheduler.py `LCMScheduler.step_coeffs`).
 * lcm_step_v: x, eps_u, eps_c, out, out2 fp16 [B, per] dense; coef DEVICE float [B][4] = {g, c_x, c_e, c_n} of row b; noise DEVICE fp16 [B, per] or NULL;
 *   seeds, draws, firsts HOST arrays [B], all three or none. Per element i of row b, fp32 arithmetic in ONE order (fused multiply-adds as written, nothing
 *   contracted or reassociated), one rounding to fp16:
 *     e = eps_c ? fmaf(g, eps_c - eps_u, eps_u) : eps_u;    o = fmaf(c_e, e, c_x * x);    if (c_n != 0) o = fmaf(c_n, z, o);    out[i] = fp16(o)
 *   out2, when not NULL, receives the same 16 bits. eps_c NULL: no guidance (g is not read into the result).
 *   z: a row is SEEDED when the host arrays are given and firsts[b] >= 0; its z is element firsts[b] + i of stream (seeds[b], draws[b]) by THE NOISE RULE,
 *   rounded to fp16 before use -- so the launch equals, bit for bit, the same launch reading noise written by randn_seeded(out_is_f16 = 1, first = firsts[b]).
 *   Every other row reads noise[b, i]. A row with c_n == 0 forms no noise term: no Philox block is computed and `noise` is not read for it (it may hold
 *   anything). A held row {0, 1, 0, 0} returns x's bits when the eps values are finite (a -0 of x comes back as +0 where the zero product is +0).
 *   Draw id 65537 = (1 << 16) + 1 is the step noise of an edit request: the noise injected after step s of the request's own schedule is elements
 *   s P .. s P + per - 1 of that draw, P = per rounded up to a multiple of 4.
 *   Ownership is by element index, 8 elements (two Philox blocks) per thread; 16-byte accesses where a row pointer is 16-byte aligned and the group lies inside
 *   the row, guarded scalar accesses elsewhere. A row's bits depend on neither B, its place in the launch, pointer alignment nor the grid.
 *   seeds, draws and firsts travel by value, 8 rows per launch; a larger B goes in chunks of 8 rows. Nothing is copied to the device, allocated or waited for.
 *   Refusals, all on the host before any launch: a null x, eps_u, coef or out, a misaligned pointer (2 bytes for the tensors, 4 for coef), noise == NULL while
 *   some row is not seeded, only some of the three host arrays: IA2P_ERR_INVALID. B < 1, per < 1, a non-negative firsts[b] that is no multiple of 4 or with
 *   firsts[b] + per > 2^34: IA2P_ERR_SHAPE. */
ia2p_status ia2p_lcm_step_v(void* stream, const void* x, const void* eps_u, const void* eps_c, const float* coef, const void* noise, const uint64_t* seeds,
                            const uint32_t* draws, const int64_t* firsts, void* out, void* out2, int B, int64_t per);

/* ---- Automatic edit mask: where two noise predictions differ, the instruction wants a change (the DiffEdit construction, Couairon et al. 2022) ---------------
 * New: the reference has no mask at all. The result is a latent mask that goes into the edit-mask path above unchanged.
 * THE RULE, for one request with base latents x0 [1, C, h, w] (per = C h w, HW = h w), its own N-step DDIM schedule and the knobs (n, s, rho, d):
 *   1. t = timesteps[t_start], where strength s keeps the tail of the schedule that starts at index t_start = max(N - min(int(N s), N), 0); a strength that
 *      keeps no step is refused.
 *   2. n noises z_k [C, h, w]: supplied, else element k per + e of draw 65536 of the request's stream (Seeded noise), else n fp16 host normals.
 *   3. x_k = fp16(sqrt(abar_t) x0 + sqrt(1 - abar_t) z_k)                               (the sampler update launch)
 *   4. eps_src[k] = UNet of x_k at t as an inversion evaluation of the request runs it; eps_tgt[k] = UNet of x_k at t as the conditional half of one of its
 *      sampling evaluations runs it. No guidance combination.
 *   5. map[p] = (1 / (n C)) * sum_k sum_c |fp32(eps_tgt[k, c, p]) - fp32(eps_src[k, c, p])|    fp32; ONE order: k outer, c inner, sequential; then one product
 *      by fp32(1 / (n C)).
 *   6. mean = (sum_p map[p]) / fp32(HW), the sum in ONE association that depends on HW alone (the convention of polar_mix_v): with 1024 threads, thread t adds
 *      the groups of 4 at (j 1024 + t) 4, j = 0, 1, ..., in index order, 64 lanes fold by xor-butterfly, 16 wave totals are added in wave order.
 *      tau = fp32(0.5 rho) * mean, one fp32 product;   m[p] = map[p] > tau ? 1 : 0, strictly. Equal predictions give mean = 0 and an empty mask; nothing is
 *      non-finite unless an input is (a NaN map value compares false: 0).
 *   7. mask[y, x] = max of m over |dy|, |dx| <= d inside the grid (outside counts 0, no wrap at a row end); d = 0 is the identity.
 * eps_contrast_map: eps_tgt, eps_src fp16 [B, n, C, HW] -> map_out fp32 [B, HW]. 16-byte loads where HW % 8 == 0 and both bases are 16-byte aligned, scalar loads
 *   elsewhere; the same values either way. B <= 65535, n C <= 2^20, HW < 2^31.
 * contrast_mask: map fp32 [B, HW = h w]; ratio (rho) HOST float [B] and dilate (d) HOST int [B] travel by value, 8 requests per launch, one workgroup per request;
 *   mask_out fp16 [B, 1, h, w] in {0, 1}; stats_out fp32 [B, 2] = (mean, tau). No atomics, no workspace: the window reads the map. A request's mean, tau and
 *   mask depend on its own map, ratio and dilate only: not on B, its place in the call or any pointer's alignment.
 * Refusals, all on the host before any launch: a null or misaligned pointer (2 bytes for fp16, 4 for fp32) is IA2P_ERR_INVALID; B, n, C, HW, h or w < 1, a ratio
 *   that is not finite and positive, a dilate outside 0 .. 16 are IA2P_ERR_SHAPE. */
ia2p_status ia2p_eps_contrast_map(void* stream, const void* eps_tgt, const void* eps_src, float* map_out, int B, int n, int C, int64_t HW);
ia2p_status ia2p_contrast_mask(void* stream, const float* map, const float* ratio, const int* dilate, void* mask_out, float* stats_out, int B, int h, int w);

/* ---- per-operator entry points (unit tests, and hosts that keep their own module tree) ----------------------------- */
/* Operand size: the linear-layer tiles (buffer-load staging), the halo-staged 3x3 convolution and the fused attention tiles address an operand (activations,
 * weights) with a 31-bit byte offset and REFUSE a matrix of 2 GiB or more with IA2P_ERR_HIP / invalid value; the gathered 3x3 convolution kernels use 64-bit
 * pointers and carry no such limit (a halo-ineligible site runs there). The largest operand of the reference's path, the stacked context K/V weights, is 0.68 GB. */
ia2p_status ia2p_groupnorm_silu(void* stream, const void* x, void* y, const void* gamma, const void* beta, int B, int HW, int C,
                                int groups, float eps, int silu, float* partial_ws /* >= B*64*groups*2 floats */);
ia2p_status ia2p_layernorm(void* stream, const void* x, void* y, const void* gamma, const void* beta, int M, int C, float eps);
/* C[M,N] = A[M,K] . W[N,K]^T + bias + residual ; geglu: W/bias packed by ia2p_pack_geglu, C is [M, N/2] */
ia2p_status ia2p_gemm(void* stream, const void* A, const void* W, const void* bias, const void* residual, void* C,
                      int M, int N, int K, int geglu);
/* LayerNorm folded into the contraction that consumes it (what the executor does for norm1/2/3 of every BasicTransformerBlock;
 * reference call sites: diffusers BasicTransformerBlock `attn1(norm1(x))`, `attn2(norm2(x), ctx)`, `ff(norm3(x))` behind
 * pnp_pipeline.py:253-260). Two pieces:
 *   ia2p_fold_layernorm: W [N,K], gamma/beta [K], bias [N] or NULL  ->  Wf = fp16(W * gamma), colsum[n] = sum_k Wf[n][k], fbias = bias + W . beta
 *   ia2p_gemm_ex:        C = epilogue(A . W^T) like ia2p_gemm, plus
 *       ln != NULL   : A holds the UN-normalised rows, W = Wf; out = rstd_m * (acc - mean_m * colsum[n]) + fbias[n] (then GEGLU if geglu);
 *                      mean/rstd from ln->stats = {sum, sum of squares} partials per row, `slots` of them ([slot][M] float2), eps = ln->eps
 *       stats_out    : this launch also writes the {sum, sum^2} partials of ITS fp16 output rows (for the next folded LayerNorm);
 *                      *stats_slots = number of slots written; stats_out must hold (N/64 + 1) * M float2
 *       splitk > 1   : K split as in ia2p_gemm_splitk (partial: splitk*M*N floats); 0/1 = the library's unsplit choice */
typedef struct { const float* stats; int slots; const float* colsum; const float* fbias; float eps; } ia2p_ln_fold;
/* GEGLU feed-forward of a BasicTransformerBlock (diffusers FeedForward: ff.net.0 GEGLU + ff.net.2): H = geglu(X W1p^T + b1p) [M, 4C]
 * (W1p / b1p packed by ia2p_pack_geglu), out = H W2^T + b2 + R, as two launches under the library's plans. splitk > 1: K split of the second GEMM
 * (partial: splitk*M*C floats). */
ia2p_status ia2p_ffn(void* stream, const void* X, const void* W1p, const void* b1p, const void* W2, const void* b2, const void* R, void* H, void* out,
                     int M, int C, int splitk, float* partial);
ia2p_status ia2p_fold_layernorm(void* stream, const void* W, const void* gamma, const void* beta, const void* bias, void* Wf,
                                float* colsum, float* fbias, int N, int K);
ia2p_status ia2p_gemm_ex(void* stream, const void* A, const void* W, const void* bias, const void* residual, void* C, int M, int N, int K,
                         int geglu, const ia2p_ln_fold* ln, float* stats_out, int* stats_slots, int splitk, float* partial);
/* same with K split over `splitk` workgroups per tile (1 .. min(K / 64, 255): the split rides in 8 bits of a preloaded kernel argument); partial holds splitk*M*N floats
 * (deterministic slab reduce) */
ia2p_status ia2p_gemm_splitk(void* stream, const void* A, const void* W, const void* bias, const void* residual, void* C,
                             int M, int N, int K, int splitk, float* partial);
/* 3x3 conv, pad 1, over channels-last x[B,Hs,Ws,Cin] with W packed by ia2p_pack_conv3x3 ([Co][3][3][Cin]);
 * stride 1|2; up=1 convolves the nearest-x2 upsampled x; rowvec [B,Co] (time embedding) and residual optional. */
ia2p_status ia2p_conv3x3(void* stream, const void* x, const void* Wp, const void* bias, const void* rowvec, const void* residual,
                         void* y, int B, int Hs, int Ws, int Cin, int Co, int stride, int up);
/* The GEMM and the 3x3 convolution with every option an executor sets on its own launch descriptor, as records (zero a record, fill what the launch uses):
 *   C[m, n] = fp16(fp16(act(acc_scale * sum_k A[row(m), k] W[n, k] + bias_scale * bias[n])) + bias_scale * rowvec[m / rows_per_batch, n] + residual[m, n])
 * with the fp16 rounding in the middle only where a row vector or a residual follows, and with ln != NULL the folded LayerNorm of ia2p_gemm_ex in place of the scales
 * and the bias. row(m) = m, or with rpb > 0 (m / rpb) * bstride + m % rpb + roff: rows [roff, roff + rpb) of every block of bstride rows (the text rows or the
 * image-token rows of a [B, L, K] context). lda / ldw >= K and ldc / ldr >= N are row strides in elements: an operand may be a column block of a wider tensor, C a
 * column block of a wider output (pass C + col0). act: 0 none, 1 GELU (erf), 2 quick-GELU x sigmoid(1.702 x), 3 GELU (tanh, GPT-2's). acc_scale / bias_scale: 0 = 1.
 * stats_out / stats_slots, splitk / partial: as ia2p_gemm_ex. The library's plan picks the tile (ia2p_debug_set_gemm_tile forces one).
 * Refusals, all on the host before any launch: a NULL record, A, W or C, an incomplete ln, act outside 0 .. 3, a scale that is not finite, A or W not 16-byte aligned
 *   or lda / ldw no multiple of 8, C / bias / residual / rowvec not 8-byte aligned or ldc / ldr / rowvec_ld no multiple of 4, ln->colsum / ln->fbias / partial not
 *   16-byte or ln->stats / stats_out not 8-byte aligned are IA2P_ERR_INVALID; M < 1, N % 4, K % 64, a stride below its width, splitk outside 0 .. min(K / 64, 255),
 *   rpb or roff outside 0 .. 65535 (they travel in 16 bits each), bstride < 0, a stride or offset without rpb, an operand of 2 GiB or more are IA2P_ERR_SHAPE.
 * ia2p_conv3x3_form: ia2p_conv3x3 plus pad_lo (zero rows / columns in front of the image: 1, or 0 -- the VAE encoder's stride-2 downsample pads only behind it; one row
 *   and column behind the image in every mode: Ho = ((Hs << up) + pad_lo - 2) / stride + 1), the two scales and the K split (partial: splitk * B Ho Wo * Co floats).
 *   Refused on the host like ia2p_gemm_form's: NULL x, Wp or y, scales that are not finite, x / Wp / partial not 16-byte or y / bias / rowvec / residual not 8-byte
 *   aligned IA2P_ERR_INVALID; Cin % 64, Co % 4, stride, up or pad_lo outside their two values, an image without an output pixel, splitk outside
 *   0 .. min(9 Cin / 64, 255), an operand of 2 GiB or more (whichever tile the plan picks) IA2P_ERR_SHAPE. */
struct ia2p_gemm_form {
  const void* A; int lda; const void* W; int ldw; const void* bias; const void* residual; int ldr; void* C; int ldc; int M, N, K;
  int rpb, bstride, roff;
  int act; float acc_scale, bias_scale;
  const void* rowvec; int rowvec_ld, rows_per_batch;
  const ia2p_ln_fold* ln; float* stats_out; int* stats_slots;
  int splitk; float* partial;
};      /* (a struct tag: the entry point carries the same name) */
ia2p_status ia2p_gemm_form(void* stream, const struct ia2p_gemm_form* d);
typedef struct {
  const void* x; const void* Wp; const void* bias; const void* rowvec; const void* residual; void* y;
  int B, Hs, Ws, Cin, Co, stride, up, pad_lo;
  float acc_scale, bias_scale;
  int splitk; float* partial;
} ia2p_conv_form;
ia2p_status ia2p_conv3x3_form(void* stream, const ia2p_conv_form* d);
/* ---- GroupNorm + SiLU fused into the 3x3 convolution that consumes it (round 5). Reference: diffusers ResnetBlock2D `conv1(nonlinearity(norm1(x)))` /
 * `conv2(dropout(nonlinearity(norm2(h))))` behind instructany2pix/ddim/pnp_pipeline.py:253-260 (in-tree twin: llm/model/vae/modules/blocks.py:122-142).
 * The norm's statistics come from the PRODUCER of its input: per slot of `rows` consecutive rows (one M-tile; HW / rows slots per image) and per channel, fp64
 * {sum, sum of squares}. A producer launch leaves them for its own output (ia2p_conv3x3_gn's gn_out, ia2p_gemm_gnstats); ia2p_gn_colstats computes the same numbers
 * for any tensor. The consumer folds them per image (slot order, then channel order, fp64) and applies y = fp16(silu(fma(x, rstd*gamma, beta - mean*rstd*gamma))):
 * inside the convolution's LDS images (ia2p_conv3x3_gn) or as a pass of its own (ia2p_gn_apply_stats) -- the two agree to the bit. */
ia2p_status ia2p_gn_colstats(void* stream, const void* x, int M, int C, int rows, double* out /* [M / rows][C][2] */);
ia2p_status ia2p_gn_apply_stats(void* stream, const void* x0, int C0, const double* st0, int rows0, const void* x1 /* or NULL */, int C1, const double* st1, int rows1,
                                const void* gamma, const void* beta, void* y /* [B*HW, C0 + C1] */, int B, int HW, int groups, float eps, int silu);
typedef struct {
  const void* x0; int C0; const double* st0; int rows0;     /* operand [B*H*W, C0] and its producer's column sums; st0 == NULL: plain convolution of x0 (no norm) */
  const void* x1; int C1; const double* st1; int rows1;     /* optional second source, channels [C0, C0 + C1): the up path's [hidden | skip] pair, never concatenated */
  const void* gamma; const void* beta; int groups; float eps;   /* the GroupNorm's affine parameters over the C0 + C1 channels */
  const void* Wp; const void* bias; const void* rowvec; const void* residual; void* y;   /* as ia2p_conv3x3 (Wp: ia2p_pack_conv3x3 over C0 + C1 [+ appended Ca columns]) */
  int B, H, W, Co;
  const void* xa; int Ca;                                   /* appended 1x1 block (conv2 + conv_shortcut as one implicit GEMM) or NULL / 0 */
  int splitk; float* partial;                               /* K split (<= 1: none); partial: splitk * B*H*W * Co floats */
  double* gn_out;                                           /* or NULL: column sums of y, [B*H*W / rows][Co][2] with rows = *gn_out_rows */
} ia2p_conv_gn;
ia2p_status ia2p_conv3x3_gn(void* stream, const ia2p_conv_gn* d, int* gn_out_rows);
ia2p_status ia2p_gemm_gnstats(void* stream, const void* A, const void* W, const void* bias, const void* residual, void* C, int M, int N, int K, int splitk, float* partial,
                              int HW, double* gn_out, int* rows);
/* stride 1, no upsampling, with K split over `splitk` workgroups per tile (what the executor launches on the 16 x 16 feature maps); partial holds
 * splitk * B*Hs*Ws * Co floats. Same reference call sites as ia2p_conv3x3 (diffusers ResnetBlock2D conv1 / conv2 behind pnp_pipeline.py:253-260). */
ia2p_status ia2p_conv3x3_splitk(void* stream, const void* x, const void* Wp, const void* bias, const void* rowvec, const void* residual,
                                void* y, int B, int Hs, int Ws, int Cin, int Co, int splitk, float* partial);
/* The tail of a ResnetBlock2D with a channel change as ONE implicit GEMM (what the executor does; diffusers ResnetBlock2D `conv2(h) + conv_shortcut(x)`
 * behind pnp_pipeline.py:253-260):  y = conv3x3(x, W2) + conv1x1(x2, Wsc) + bias, K = 9 Cin + Cin2, stride 1. Wcat [Co][9 Cin + Cin2] holds, per output
 * channel, the ia2p_pack_conv3x3 row of W2 followed by the row of Wsc; bias = b2 + bsc; x [B,Hs,Ws,Cin], x2 [B,Hs,Ws,Cin2] channels-last. */
ia2p_status ia2p_conv3x3_cat(void* stream, const void* x, const void* x2, const void* Wcat, const void* bias, void* y,
                             int B, int Hs, int Ws, int Cin, int Cin2, int Co);
ia2p_status ia2p_pack_conv3x3(void* stream, const void* w_oihw, void* w_packed, int Co, int Cin);   /* [Co][Cin][3][3] -> the implicit-GEMM K order ia2p_conv3x3 / _cat walk ([Co][3][3][Cin] in the shipped library); Cin % 64 == 0. Opaque to callers: pack with this, pass to those */
ia2p_status ia2p_pack_conv_out(void* stream, const void* w_oihw, void* w_packed, int Co, int C);       /* [Co][C][3][3] -> [Co][3][3][C]: the layout ia2p_conv_out reads (any C % 32 == 0) */
ia2p_status ia2p_pack_geglu(void* stream, const void* src, void* dst, int rows, int rowlen);
/* The UNet's latent-boundary 3x3 convolutions (diffusers UNet2DConditionModel.conv_in / .conv_out behind pnp_pipeline.py:253-260; the VAE's too), pad 1:
 *   ia2p_conv_in : x NCHW [B,Cin,H,W] (Cin*9 <= 64), w OIHW [Co,Cin,3,3] (Co % 8 == 0), bias [Co] -> y channels-last [B*H*W, Co];
 *                  w_scratch: Co*64 fp16 elements for the zero-padded [Co][64] weight image the kernel reads (the executors keep it in their arena)
 *   ia2p_conv_out: x channels-last [B*H*W, C] (C % 32 == 0), w packed [Co][3][3][C] (ia2p_pack_conv_out), Co <= 8, bias [Co] -> y NCHW [B,Co,H,W] */
ia2p_status ia2p_conv_in(void* stream, const void* x_nchw, const void* w_oihw, const void* bias, void* y_nhwc, void* w_scratch,
                         int B, int Cin, int H, int W, int Co);
ia2p_status ia2p_conv_out(void* stream, const void* x_nhwc, const void* w_packed, const void* bias, void* y_nchw, int B, int C, int H, int W, int Co);
/* O[b,q,h*64:] = sum_s weight_s * softmax(Q K_s^T / 8) V_s over nseg <= 2 key segments (head_dim 64).
 * Q rows have stride ldq, K_s/V_s rows stride ld_s; segment s has nkeys_s keys per batch. Strides are multiples of 8 elements, O is 16-byte aligned
 * (a query's 64 channels of one head leave as one 128-byte line). */
ia2p_status ia2p_attention(void* stream, const void* Q, int ldq, void* O, int ldo, int B, int heads, int Nq, int nseg,
                           const void* K0, const void* V0, int ld0, int nkeys0, float w0,
                           const void* K1, const void* V1, int ld1, int nkeys1, float w1);
/* Regional image prompts -- what diffusers offers as cross_attention_kwargs={"ip_adapter_masks": ...}: every subject's four image tokens ride in ONE context, each
 * token group has a softmax of its own and acts only where its own spatial mask says so, so S subjects cost one denoising loop instead of S:
 *   O[b,q,h*64:] = w0 softmax_j(q . k_text_j / 8) v_text_j + sum_{g < G} s[b] m[b,g,q] softmax_{j in group g}(q . k_ip_j / 8) v_ip_j
 * The arguments of ia2p_attention (nseg must be 2), plus: region_w = m, fp16 [B, G, Nq], device memory, any finite values (usually [0, 1]; a per-group scale is folded
 * into it by the host); G token groups, group g = rows 4 g .. 4 g + 3 of segment 1, 1 <= G <= 16 and nkeys1 == 4 G; s[b] = w1_b[b] (device, float [B]) or, w1_b NULL,
 * w1. m == 0 puts a probability of exactly +0 into the P.V product: a group's keys and values cannot move a bit of the output at queries its mask leaves out, and
 * all-zero groups appended to a call (padding a batch to its largest G) leave every bit as it was. The text softmax never sees an image-token key, a group's softmax
 * never another group's keys. Refusals, all before any launch: a NULL pointer (w1_b may be NULL), nseg != 2 or w0 == 0 (the merged accumulator divides by it)
 * IA2P_ERR_INVALID; G outside 1 .. 16, nkeys1 != 4 G or a stride that is no multiple of 8 elements IA2P_ERR_SHAPE. */
ia2p_status ia2p_attention_regions(void* stream, const void* Q, int ldq, void* O, int ldo, int B, int heads, int Nq, int nseg,
                                   const void* K0, const void* V0, int ld0, int nkeys0, float w0,
                                   const void* K1, const void* V1, int ld1, int nkeys1, float w1,
                                   const void* region_w, int G, const float* w1_b);
/* The mask pyramid of the launch above: masks fp16 [B, G, h, w] on the latent grid -> out fp16 [B, G, (h / f) * (w / f)], the mean of each f x f block -- summed in
 * fp32 in row-major order (one fixed order, no atomics), scaled by the exact 1 / f^2 and rounded once. {0, 1} masks come out exact. f is 1, 2, 4 or 8 (anything
 * else IA2P_ERR_INVALID); h % f or w % f non-zero is IA2P_ERR_SHAPE. */
ia2p_status ia2p_region_levels(void* stream, const void* masks, void* out, int B, int G, int h, int w, int f);
/* `to_q` fused with the cross-attention that consumes it (reference attention_processor.py:344 + :371 / :387 / :397; AttnProcessor2_0 :239 + :259):
 *   O = ia2p_attention(Q = epilogue(X . Wq^T), ...)  in ONE launch, Q never written -- bit-identical to ia2p_gemm_ex on a 128 x 64 tile followed
 *   by ia2p_attention. X [B*Nq, K], Wq [heads*64, K] (gamma-folded when ln != NULL, as ia2p_gemm_ex), bias [heads*64] or NULL (ignored with ln).
 *   Nq must be a multiple of 128 (one tile = 128 queries of one batch element x one head), K of 64. */
ia2p_status ia2p_qproj_attention(void* stream, const void* X, const void* Wq, const void* bias, const ia2p_ln_fold* ln, void* O, int ldo,
                                 int B, int heads, int Nq, int K, int nseg,
                                 const void* K0, const void* V0, int ld0, int nkeys0, float w0,
                                 const void* K1, const void* V1, int ld1, int nkeys1, float w1);
/* Self-attention of AttnProcessor2_0 at 256 tokens per image (the 16 x 16 level) with its three projections, ONE launch (reference attention_processor.py:239 to_q,
 * :246-247 to_k / to_v, :259 scaled_dot_product_attention): O[b, q, h*64:] = softmax(Q K^T / 8) V with [Q | K | V] = epilogue(X . Wqkv^T), the projected
 * tensors never written -- bit-identical to ia2p_gemm_ex (N = 3 * heads * 64) followed by ia2p_attention. X [B*256, K]; Wqkv the stacked [3*heads*64, K]
 * weight (rows: all of to_q, then to_k, then to_v; gamma-folded when ln != NULL, as ia2p_gemm_ex); bias [3*heads*64] or NULL (ignored with ln). */
ia2p_status ia2p_qkv_self_attention(void* stream, const void* X, const void* Wqkv, const void* bias, const ia2p_ln_fold* ln, void* O, int ldo,
                                    int B, int heads, int K);
/* The same launch carrying the layer's slice of the context K/V projection (reference attention_processor.py:358-359 `attn.to_k` / `attn.to_v` of the text rows,
 * :379-380 `to_k_ip` / `to_v_ip` of the image-token rows of IPAttnProcessor2_0) on the compute units its (image, head) tiles leave empty -- what ia2p_unet_forward does
 * in every step for each block that takes the fused launch. context [B, L, ctx_dim]: rows [0, L - Li) of every context are text, the last Li the image tokens (Li = 0:
 * text only, Wkv_ip / kv_ip NULL). Wkv_text / Wkv_ip [N, ctx_dim] (K rows then V rows, N = 2 * heads * 64 in the UNet); kv_text [B * (L - Li), ldkv], kv_ip [B * Li, ldkv].
 * O and the K/V written have the bits of ia2p_qkv_self_attention and of ia2p_project_context's columns of the layer. When B * heads tiles + the slice's 128 x 160 tiles
 * exceed the device's compute units the projections run as launches of their own in front; *in_launch (optional) says which way it went. */
ia2p_status ia2p_qkv_self_attention_ctx(void* stream, const void* X, const void* Wqkv, const void* bias, const ia2p_ln_fold* ln, void* O, int ldo,
                                        int B, int heads, int K, const void* context, int L, int Li, int ctx_dim, const void* Wkv_text, const void* Wkv_ip,
                                        void* kv_text, void* kv_ip, int ldkv, int N, int* in_launch);
/* The `attn_map` side effect of IPAttnProcessor2_0 (reference attention_processor.py:390-391; stored on the processor, read only by the
 * attention-map hooks of diffusion/ip_adapter/utils.py:15-20):  out[b,h,q,t] = sum_d Q[b,q,h*64+d] * softmax_t(Kip[b,t,h*64+d]) -- the
 * softmax binds to ip_key^T, i.e. runs over the TOKEN axis, unscaled, before the matmul. Q rows stride ldq, Kip [B*ntok, ldk], out fp16
 * [B, heads, Nq, ntok], ntok <= 16. */
ia2p_status ia2p_ip_attn_map(void* stream, const void* Q, int ldq, const void* Kip, int ldk, void* out, int B, int heads, int Nq, int ntok);
ia2p_status ia2p_linear_small(void* stream, const void* X, const void* W, const void* bias, void* out, int M, int N, int K,
                              int silu_in, int silu_out);

/* Test / tuning hooks (ia2p_debug_*) and the per-kernel timing interface of bench.py's roofline leg (ia2p_profile_*) are declared in ia2p_debug.h: they are
 * exported by the same library but are not part of the product boundary. */

/* ---- VAE (diffusers AutoencoderKL): pipe.vae.encode / pipe.vae.decode ----------------------------
 * reference call sites: ddim/pnp_pipeline.py:190-204 (prepare_latents of the img2img base class), ddim/sdxl_pipeline.py:859-871.
 * NCHW fp16 at both ends; h, w are LATENT sizes in both directions (image side = latent side * 2^(n_blocks-1)).
 * encode returns the posterior moments [B, 2*latent_channels, h, w] (mean | logvar); sampling and the 0.13025 scaling
 * stay on the host. The reference upcasts this model to fp32 (its activations overflow fp16); this build keeps fp16 storage with fp32
 * accumulation and extends the range of the residual stream by a power-of-two storage scale (ia2p_vae_config.stream_scale). */
typedef struct ia2p_vae ia2p_vae;
typedef struct {
  int in_channels, out_channels, latent_channels;
  int n_blocks;
  int block_out_channels[IA2P_MAX_BLOCKS];
  int layers_per_block;
  int norm_num_groups;
  float norm_eps;
  float stream_scale;   /* range extension in place of the reference's fp32 upcast (sdxl_pipeline.py:860-865): the residual stream is stored
                         * multiplied by this power of two in [2^-16, 1] (<= 0 means 1 = plain fp16 storage); 2^-7 covers +-8.4e6 */
} ia2p_vae_config;
ia2p_status ia2p_vae_create(const ia2p_vae_config* cfg, ia2p_vae** out);
void ia2p_vae_destroy(ia2p_vae* vae);
const char* ia2p_vae_last_error(ia2p_vae* vae);
size_t ia2p_vae_arena_bytes(ia2p_vae* vae);
ia2p_status ia2p_vae_bind_arena(ia2p_vae* vae, void* dev_arena, size_t bytes);
ia2p_status ia2p_vae_load_tensor(ia2p_vae* vae, const char* key, const void* dev_src, const int64_t* shape, int ndim, void* stream);
ia2p_status ia2p_vae_finalize_weights(ia2p_vae* vae);
size_t ia2p_vae_workspace_bytes(ia2p_vae* vae, int B, int h, int w, int decode);
ia2p_status ia2p_vae_decode(ia2p_vae* vae, void* stream, const void* latents, void* image, int B, int h, int w, void* workspace, size_t workspace_bytes);
ia2p_status ia2p_vae_encode(ia2p_vae* vae, void* stream, const void* image, void* moments, int B, int h, int w, void* workspace, size_t workspace_bytes);

/* ---- image codec: 8-bit images <-> the VAE's fp16 tensors ---------------------------------------------------------------------------------
 * The reference takes a base image FILE (pipeline.py:289-293 `loas_base_img`: open, `resize_and_crop`, resize to 1024^2; :328), runs it through
 * `image_processor.preprocess` before the VAE encode (ddim/pnp_pipeline.py:190-204) and returns PIL images (pipeline.py:356-386, after
 * `image_processor.postprocess` in ddim/sdxl_pipeline.py:859-880). Resizing stays on the host (PIL); these kernels do the per-pixel work, bit for
 * bit with diffusers 0.26.3 VaeImageProcessor: src / dst are device pointers; u8 images are [B,H,W,C] (HWC, as PIL / numpy hold them); fp16
 * tensors are NCHW; C is 1 or 3; B*H*W*C < 2^31. Arguments are checked before any HIP call (IA2P_ERR_INVALID / IA2P_ERR_SHAPE). */
/* u8 -> fp16 [B,C,H,W]: normalize = 1: 2 (q / 255) - 1 (pil_to_numpy -> numpy_to_pt -> normalize -> .to(float16): fp32 math, one rounding to fp16);
 * normalize = 0: q / 255 (masks) */
ia2p_status ia2p_image_from_u8(void* stream, const void* src, void* dst, int B, int H, int W, int C, int normalize);
/* fp16 [B,C,H,W] in [-1, 1] -> u8 [B,H,W,C]: rint_half_even(clamp(x / 2 + 0.5, 0, 1) * 255) in fp32 (postprocess + numpy_to_pil); NaN -> 0 */
ia2p_status ia2p_image_to_u8(void* stream, const void* src, void* dst, int B, int H, int W, int C);
/* fp16 [B,C,H,W] -> fp32 clamp(x / 2 + 0.5, 0, 1) (denormalize) as [B,H,W,C] (nhwc = 1: output_type "np") or [B,C,H,W] (nhwc = 0: "pt") */
ia2p_status ia2p_image_to_f32(void* stream, const void* src, float* dst, int B, int H, int W, int C, int nhwc);
/* fp16 [n] -> fp16 [n]: the 8-bit round trip of the refiner hand-over (pipeline.py:358-361: postprocess to PIL, then preprocess) in one launch,
 * = ia2p_image_from_u8(ia2p_image_to_u8(x), normalize = 1) element-wise. dst may equal src. */
ia2p_status ia2p_image_requantize(void* stream, const void* src, void* dst, int64_t n);

/* ---- condition maps: what a ControlNet is guided by, made from the base image on the device ---------------------------------------------------
 * New: the reference attaches no ControlNet and makes no condition map. The Canny detector restates OpenCV's cv::Canny (8-bit input, aperture 3) and its 8-bit
 * RGB2GRAY rule; OpenCV is not installed next to this library: parity with it is restated in tests/canny_ref.py, not pinned.
 * All images are device pointers, u8, [B, H, W] or [B, H, W, C] (HWC, as the image codec above); 1 <= H, W and B*H*W*3 < 2^31. Integer arithmetic only: every
 * result is exact, independent of summation order and of scheduling. Arguments are checked before any HIP call: null pointers, aliasing, misalignment, bad knobs
 * are IA2P_ERR_INVALID, bad sizes IA2P_ERR_SHAPE, a workspace that is too small IA2P_ERR_NOMEM.
 *
 * image_grey_u8: rgb [B, H, W, 3] -> grey [B, H, W]:  Y = (4899 R + 9617 G + 1868 B + 8192) >> 14.
 * image_gauss_u8: src, dst [B, H, W, C], C = 1 or 3; separable blur with a replicated border. taps: a HOST array of r + 1 integers q_0 .. q_r (centre first, the
 *   kernel is symmetric), 0 <= r <= 32, q_0 + 2 sum_{i >= 1} q_i == 4096 (checked). rows: row = sum_i q_|i| src[x + i] (32-bit, to the workspace); columns:
 *   dst = (sum_j q_|j| row[y + j] + 2^23) >> 24. r = 0 copies. dst may equal src. workspace: ia2p_image_gauss_workspace_bytes, 4-byte aligned.
 * canny_u8: grey [B, H, W] -> edges [B, H, W] in {0, 255}.
 *   gradients  dx, dy: the 3x3 Sobel responses ([-1 0 1; -2 0 2; -1 0 1] and its transpose) of the grey image with a REPLICATED border.
 *   magnitude  m = |dx| + |dy|, lo = floor(low), hi = floor(high); with l2_gradient: m = dx^2 + dy^2, lo = floor(low)^2, hi = floor(high)^2. m is 0 outside the image.
 *   non-maximum suppression, only where m > lo; with x = |dx|, y = |dy| << 15, t22 = x * 13573, t67 = t22 + (x << 16):
 *     y < t22:   keep iff m > m[y, x-1] and m >= m[y, x+1]
 *     y > t67:   keep iff m > m[y-1, x] and m >= m[y+1, x]
 *     otherwise, s = -1 if (dx ^ dy) < 0 else 1:  keep iff m > m[y-1, x-s] and m > m[y+1, x+s]
 *     a kept pixel is STRONG if m > hi, else WEAK; every other pixel is OFF.
 *   hysteresis a weak pixel is an edge iff it is 8-connected, through weak or strong pixels, to a strong one. 255 on edges, 0 elsewhere.
 *   low > high swaps the two; negative or non-finite thresholds are IA2P_ERR_INVALID. edges may not alias grey.
 *   The hysteresis runs in rounds over 64 x 64 tiles of a state map (0 off, 1 weak, 2 edge) until a round promotes nothing; the host reads a 16-byte flag block per
 *   group of four rounds, so the call SYNCHRONISES the stream and cannot be captured into a graph. *rounds_out (may be NULL): the first round that promoted nothing.
 *   The loop is bounded by ia2p_canny_max_rounds = 2 B ring(H, W) + 2, ring = the pixels on the outermost ring of their tile (condition maps); on
 *   reaching the bound the call returns IA2P_ERR_STATE and no map. workspace: ia2p_canny_workspace_bytes (the state map, then the flags), 4-byte aligned.
 * canny_hysteresis_u8: the second half of canny_u8 on a state map [B, H, W] the caller brings (values other than 1 and 2 count as off); the map is not changed.
 * condition_from_u8: map [B, H, W, C_in], C_in = 1 or 3 -> fp16 [B, 3, H, W], q / 255 with one rounding: bit for bit what ia2p_image_from_u8 with normalize = 0 gives
 *   for the same byte; a one-channel map is replicated to three. */
ia2p_status ia2p_image_grey_u8(void* stream, const void* rgb, void* grey, int B, int H, int W);
size_t ia2p_image_gauss_workspace_bytes(int B, int H, int W, int C);
ia2p_status ia2p_image_gauss_u8(void* stream, const void* src, void* dst, void* workspace, int B, int H, int W, int C, const uint16_t* taps, int r);
size_t ia2p_canny_workspace_bytes(int B, int H, int W);
int64_t ia2p_canny_max_rounds(int B, int H, int W);
ia2p_status ia2p_canny_u8(void* stream, const void* grey, void* edges, void* workspace, size_t workspace_bytes, int B, int H, int W, float low, float high,
                          int l2_gradient, int* rounds_out);
ia2p_status ia2p_canny_hysteresis_u8(void* stream, const void* state, void* edges, void* workspace, size_t workspace_bytes, int B, int H, int W, int* rounds_out);
ia2p_status ia2p_condition_from_u8(void* stream, const void* map_u8, void* dst_f16, int B, int H, int W, int C_in);

/* ---- CLIP text encoders (conditioning side): the two encoders behind `encode_prompt` ------------------
 * (reference ddim/sdxl_pipeline.py:202-395: `text_encoder(ids, output_hidden_states=True)`, `.hidden_states[-2]` of both encoders
 * concatenated, pooled `[0]` of the second). transformers `CLIPTextModel` / `CLIPTextModelWithProjection` semantics: token + position
 * embeddings, pre-LayerNorm blocks with causal self-attention (head_dim 64) and a GELU / quick-GELU MLP, final LayerNorm, pooled row
 * = final-normed hidden state at the EOS position (eos_token_id 2: position of the largest id), optional bias-free projection.
 * Parameter keys are the transformers state-dict keys ("text_model.encoder.layers.0.self_attn.q_proj.weight", ...). */
typedef struct ia2p_clip ia2p_clip;
typedef struct {
  int vocab_size, hidden_size, num_layers, num_heads, intermediate_size, max_positions;
  int projection_dim;     /* 0: no text_projection (CLIPTextModel) */
  int hidden_act;         /* 1 = gelu, 2 = quick_gelu, 3 = gelu_new (tanh form; GPT-2) */
  int eos_token_id;
  float layer_norm_eps;
} ia2p_clip_config;
ia2p_status ia2p_clip_create(const ia2p_clip_config* cfg, ia2p_clip** out);
void ia2p_clip_destroy(ia2p_clip* clip);
const char* ia2p_clip_last_error(ia2p_clip* clip);
size_t ia2p_clip_arena_bytes(ia2p_clip* clip);
ia2p_status ia2p_clip_bind_arena(ia2p_clip* clip, void* dev_arena, size_t bytes);
ia2p_status ia2p_clip_load_tensor(ia2p_clip* clip, const char* key, const void* dev_src, const int64_t* shape, int ndim, void* stream);
ia2p_status ia2p_clip_finalize_weights(ia2p_clip* clip);
size_t ia2p_clip_workspace_bytes(ia2p_clip* clip, int B, int T);
/* input_ids: int32 [B, T] on the device (T <= max_positions, <= 128). Outputs (each may be NULL): hidden_penultimate [B, T, hidden]
 * (= hidden_states[-2], the input of the last layer), last_hidden [B, T, hidden] (= last_hidden_state: final LayerNorm of the last
 * layer's output), pooled [B, projection_dim or hidden] (text_embeds / pooler_output). The last layer is skipped when only
 * hidden_penultimate is requested. */
ia2p_status ia2p_clip_encode(ia2p_clip* clip, void* stream, const int32_t* input_ids, int B, int T, void* hidden_penultimate,
                             void* last_hidden, void* pooled, void* workspace, size_t workspace_bytes);
/* The same pre-LayerNorm causal transformer driven with `inputs_embeds` [B, T, hidden] fp16 instead of token ids (position embeddings
 * are added inside): how the reference runs the GPT-2 sequence model of its embedding prior, `self.model(inputs_embeds=...,
 * attention_mask=ones)["last_hidden_state"]` (instructany2pix/prior/model.py:493-495, :611-613; transformers GPT2Model with
 * hidden_act 3, created with vocab_size 0 since the token table is never read). All-ones attention mask only. */
ia2p_status ia2p_clip_encode_embeds(ia2p_clip* clip, void* stream, const void* inputs_embeds, int B, int T, void* hidden_penultimate,
                                    void* last_hidden, void* workspace, size_t workspace_bytes);
/* Sampler update of the embedding prior in fp32 (prior/model.py:208-240 `get_eps`, :627-637 guidance + diffusers DDPMScheduler.step):
 *   eps_i = (sample - sqrt_a * o_i) / sqrt_b;  eps = eps_u + g * (eps_c - eps_u);  x0 = (sample - sqrt_b * eps) / sqrt_a;
 *   out = k0 * x0 + k1 * sample + sigma * noise
 * sample / noise / out: fp32 [n] device; out_cond / out_uncond: fp16 [n] outputs of the sequence model (out_cond NULL = no guidance;
 * noise NULL = none). sqrt_a = sqrt(abar_t), sqrt_b = sqrt(1 - abar_t); k0, k1, sigma from the DDPM posterior (host: scheduler.py). */
ia2p_status ia2p_prior_step(void* stream, const float* sample, const void* out_cond, const void* out_uncond, const float* noise, float g,
                            float sqrt_a, float sqrt_b, float k0, float k1, float sigma, float* out, int64_t n);

/* ---- ViT towers: ImageBind's vision and audio encoders (reference pipeline.py:118-121 `imagebind_huge`, :155-168: every mm_data entry becomes a
 * 1024-d vector) ------------------------------------------------------------------------------------------------------------------------
 * One tower: a bias-free patch convolution (patch x patch, stride patch_stride; the grid is floor((size - patch) / stride) + 1 per axis), optional
 * LayerNorm of the patch rows (stem_ln), class token in front, learned position embeddings, optional pre-transformer LayerNorm (pre_ln), pre-LayerNorm
 * blocks with non-causal self-attention at head dim 64 or 80 and an exact-GELU MLP, LayerNorm of the class row, bias-free projection to out_dim.
 * bias_kv: every attention sees one more key / value row, `attn.bias_k` / `attn.bias_v` (torch nn.MultiheadAttention(add_bias_kv=True)).
 * Parameter keys: "stem.weight" [hidden, C, patch, patch], "stem.norm.{weight,bias}", "cls_token", "pos_embed" [tokens, hidden],
 * "pre_ln.{weight,bias}", "blocks.<i>.norm_1|norm_2.{weight,bias}", "blocks.<i>.attn.in_proj_weight|in_proj_bias|out_proj.weight|out_proj.bias|bias_k|bias_v",
 * "blocks.<i>.mlp.fc1|fc2.{weight,bias}", "head.norm.{weight,bias}", "head.proj.weight" [out_dim, hidden]; all fp16.
 * IA2P_ERR_SHAPE at create: hidden not a multiple of 64, a head dim other than 64 / 80, a patch larger than the input, more than 272 keys per image. */
typedef struct ia2p_vit ia2p_vit;
typedef struct {
  int hidden_size, num_layers, num_heads, intermediate_size;
  int in_channels, image_h, image_w;
  int patch_size, patch_stride;
  int pre_ln, stem_ln, bias_kv;     /* 0 / 1 each */
  int out_dim;
  float layer_norm_eps;             /* <= 0: 1e-6 */
} ia2p_vit_config;
ia2p_status ia2p_vit_create(const ia2p_vit_config* cfg, ia2p_vit** out);
void ia2p_vit_destroy(ia2p_vit* vit);
const char* ia2p_vit_last_error(ia2p_vit* vit);
size_t ia2p_vit_arena_bytes(ia2p_vit* vit);
int ia2p_vit_tokens(ia2p_vit* vit);                /* class token + patches */
ia2p_status ia2p_vit_bind_arena(ia2p_vit* vit, void* dev_arena, size_t bytes);
ia2p_status ia2p_vit_load_tensor(ia2p_vit* vit, const char* key, const void* dev_src, const int64_t* shape, int ndim, void* stream);
ia2p_status ia2p_vit_finalize_weights(ia2p_vit* vit);
size_t ia2p_vit_workspace_bytes(ia2p_vit* vit, int B);
/* pixels: fp16 [B, C, H, W] on the device. out: fp32 [B, out_dim], the head's output (no normalisation). last_hidden (optional): fp16 [B, tokens, hidden],
 * the last block's output before the head's LayerNorm. */
ia2p_status ia2p_vit_encode(ia2p_vit* vit, void* stream, const void* pixels, int B, float* out, void* last_hidden, void* workspace, size_t workspace_bytes);
/* The towers' attention launch alone: O = softmax(Q K^T / sqrt(D)) V over all T keys of an image, no mask. qkv: fp16 [B*T, 3*heads*D] rows = [q | k | v];
 * out: fp16 [B*T, heads*D]; D = 64 or 80. bias_k / bias_v (both or neither): fp16 [heads*D], one more key / value row after the T token rows.
 * At most 272 keys (IA2P_ERR_SHAPE). Scores and softmax in fp32, fixed reduction order. */
ia2p_status ia2p_attention_full(void* stream, const void* qkv, void* out, const void* bias_k, const void* bias_v, int B, int T, int heads, int D);

/* ---- Segment Anything: the subject segmenter of the subject-consistency pass (reference gdino/lib.py:21-51 `get_mask`: `SamPredictor.set_image`, then
 * `predict(box=...)` per subject; pipeline.py:363-368). transformers `SamModel` semantics: a ViT image encoder whose blocks attend inside
 * window x window tiles of the token grid or, at global_attn_indexes, over the whole grid, both with the decomposed relative-position bias; a neck to
 * output_channels; a prompt encoder for ONE box per mask (evaluated on the host in fp32); the two-way mask decoder (dec_layers blocks, dec_heads heads,
 * attention inner width dec_hidden / dec_downsample_rate) with the single-mask output (mask token 0, `multimask_output=False`). Head dim 64 or 80 in the
 * encoder, 16 or 32 in the decoder; window <= 16; image_size a multiple of patch_size; dec_hidden == output_channels (IA2P_ERR_SHAPE otherwise, also for a
 * grid whose bias rows do not fit the attention launch's LDS). Parameter keys: see instructany2pix_amd/sam.py (`internal_state_dict`), fp16. */
#define IA2P_SAM_MAX_GLOBAL 8
typedef struct ia2p_sam ia2p_sam;
typedef struct {
  int hidden_size, num_layers, num_heads, mlp_dim, image_size, patch_size, window_size;
  int num_global, global_attn_indexes[IA2P_SAM_MAX_GLOBAL];
  int output_channels;
  int dec_hidden, dec_layers, dec_heads, dec_mlp_dim, dec_downsample_rate;
  float layer_norm_eps;   /* <= 0: 1e-6 */
} ia2p_sam_config;
ia2p_status ia2p_sam_create(const ia2p_sam_config* cfg, ia2p_sam** out);
void ia2p_sam_destroy(ia2p_sam* sam);
const char* ia2p_sam_last_error(ia2p_sam* sam);
size_t ia2p_sam_arena_bytes(ia2p_sam* sam);
ia2p_status ia2p_sam_bind_arena(ia2p_sam* sam, void* dev_arena, size_t bytes);
ia2p_status ia2p_sam_load_tensor(ia2p_sam* sam, const char* key, const void* dev_src, const int64_t* shape, int ndim, void* stream);
/* also reads the small prompt tensors back to the host and uploads the dense positional encoding of the token grid (synchronises the device) */
ia2p_status ia2p_sam_finalize_weights(ia2p_sam* sam);
/* workspace that serves ia2p_sam_encode_image of B images and ia2p_sam_predict_boxes of up to n_boxes boxes (1..64 each; 0 otherwise) */
size_t ia2p_sam_workspace_bytes(ia2p_sam* sam, int B, int n_boxes);
/* pixels: fp16 [B, 3, S, S] on the device (normalised, zero-padded to the square). embeddings: fp16 [B, gh * gw, output_channels], channels-last rows. */
ia2p_status ia2p_sam_encode_image(ia2p_sam* sam, void* stream, const void* pixels, int B, void* embeddings, void* workspace, size_t workspace_bytes);
/* embeddings: ONE image's rows. boxes: HOST fp32 [n, 4], x0 y0 x1 y1 in pixels of the S x S input; a box that is not inside the input is IA2P_ERR_SHAPE.
 * low_res_logits: fp32 [n, 4 gh, 4 gw], iou: fp32 [n], both on the device. Waits for the stream's earlier work before it reuses its host staging buffer. */
ia2p_status ia2p_sam_predict_boxes(ia2p_sam* sam, void* stream, const void* embeddings, const float* boxes, int n, float* low_res_logits, float* iou,
                                   void* workspace, size_t workspace_bytes);
/* The executor's own launches one by one (unit tests, tools/sam_bench.py). Scores and softmax in fp32, fixed reduction order, no atomics.
 * Attention with SAM's decomposed relative-position bias over the [gh, gw] token grid of each image, from the fused QKV buffer: qkv fp16 [B * gh * gw, 3 heads D]
 * rows = [q | k | v] in grid order, out fp16 [B * gh * gw, heads D], D = 64 or 80;
 *   score[q][k] = (q . k) / sqrt(D) + q . rel_h[qh - kh + S - 1] + q . rel_w[qw - kw + S - 1]        (the bias terms on the unscaled q)
 * window: S = window <= 16, rel_h / rel_w fp16 [2 S - 1, D]; the grid is cut into S x S tiles from the top-left corner, a tile's positions past the grid's edge
 * are keys whose k / v are rows [H, 2H) / [2H, 3H) of qkv_bias (fp16 [3 heads D]: SAM pads after norm1) and are no queries.
 * global: one tile, the whole grid; rel_h fp16 [2 gh - 1, D], rel_w fp16 [2 gw - 1, D]; IA2P_ERR_SHAPE when gh + gw bias rows of 64 queries do not fit in LDS. */
ia2p_status ia2p_attention_window_relpos(void* stream, const void* qkv, void* out, const void* qkv_bias, const void* rel_h, const void* rel_w, int B, int gh, int gw,
                                         int heads, int D, int window);
ia2p_status ia2p_attention_global_relpos(void* stream, const void* qkv, void* out, const void* rel_h, const void* rel_w, int B, int gh, int gw, int heads, int D);
/* the mask decoder's attention: q fp16 [B, Tq, heads D], k / v fp16 [B, Tk, heads D], out as q; D = 16 or 32, any Tq / Tk; scale 1 / sqrt(D) */
ia2p_status ia2p_attention_small_head(void* stream, const void* q, const void* k, const void* v, void* out, int B, int Tq, int Tk, int heads, int D);
/* bilinear resize (torch `F.interpolate(mode="bilinear", align_corners=False)`) of n fp32 images, src_h x src_w pixels at row stride src_ld and image stride
 * src_image_stride (a crop is a smaller src_h / src_w over the same strides), to H x W: out_logits fp32 [n, H, W] and / or out_mask uint8 [n, H, W] =
 * (value > threshold ? 255 : 0); either may be NULL. */
ia2p_status ia2p_mask_upsample_threshold(void* stream, const float* logits, int n, int src_h, int src_w, int src_ld, int64_t src_image_stride, int H, int W,
                                         float threshold, float* out_logits, void* out_mask);
/* erode (is_dilate = 0: minimum) or dilate (maximum) a uint8 [H, W] image with a k x k window of offsets -(k / 2) .. k - k / 2 - 1 on both axes; pixels outside
 * the image are ignored. tmp: uint8 [H, W] scratch (the row pass); dst may be src. */
ia2p_status ia2p_mask_morph(void* stream, const void* src, void* dst, void* tmp, int H, int W, int k, int is_dilate);

/* ---- the instruction LLM: LLaMA decoder with a KV cache (reference pipeline.py:151-279 `forward_llm`; the model is a Vicuna-7B shaped
 * `LlamaForCausalLM`, llm/model/language_model/any2pix_llama.py, driven by `any2pix_lm.generate(...)` at pipeline.py:201-211 with use_cache=False:
 * one full forward per new token there, one cached row here). transformers `LlamaModel` + `lm_head` semantics: pre-RMSNorm blocks, rotary
 * embeddings (rotate_half convention, rope_theta), multi-head attention at head dim 128 (num_kv_heads must equal num_heads), bias-free
 * projections, SwiGLU MLP, final `model.norm`, untied `lm_head`. Batch 1 (the reference asserts it, llm/mm_utils.py:93). Parameter keys are
 * the `LlamaForCausalLM` state-dict names ("model.layers.0.self_attn.q_proj.weight", ...), fp16. The reference's live call loads the checkpoint with
 * `load_in_4bit=True, bnb_4bit_compute_dtype=torch.float32` and names no quant type (pipeline.py:28-31); the default of the transformers version it pins
 * is believed to be "fp4" without double quantisation, which could not be verified where this was written (neither that version nor bitsandbytes was at
 * hand). Its unused llm/model/builder.py:31-37 asks for NF4 with double quantisation. This engine computes from the fp16 weights by default and from
 * 4-bit codes of either codebook after ia2p_llm_set_weight_format. */
typedef struct ia2p_llm ia2p_llm;
typedef struct {
  int vocab_size, hidden_size, num_layers, num_heads, num_kv_heads, intermediate_size;
  float rms_norm_eps;     /* <= 0: 1e-5 */
  float rope_theta;       /* <= 0: 10000 */
} ia2p_llm_config;
ia2p_status ia2p_llm_create(const ia2p_llm_config* cfg, ia2p_llm** out);
void ia2p_llm_destroy(ia2p_llm* llm);
const char* ia2p_llm_last_error(ia2p_llm* llm);
size_t ia2p_llm_arena_bytes(ia2p_llm* llm);
ia2p_status ia2p_llm_bind_arena(ia2p_llm* llm, void* dev_arena, size_t bytes);
ia2p_status ia2p_llm_load_tensor(ia2p_llm* llm, const char* key, const void* dev_src, const int64_t* shape, int ndim, void* stream);
ia2p_status ia2p_llm_finalize_weights(ia2p_llm* llm);
/* After ia2p_llm_create, before ia2p_llm_bind_arena: bits = 4 holds the seven projections of every decoder layer as 4-bit codes of `codebook` (16 values,
 * index = code), quantised block-wise at load as bitsandbytes does: blocks of 64 along the flattened tensor, absmax = max |w| as fp32, code = the entry
 * nearest to w / absmax (thresholds: the fp32 midpoints of the sorted codebook; a value on a threshold takes the lower entry; an all-zero block stores
 * absmax 0). Embeddings, norms and lm_head stay fp16. ia2p_llm_load_tensor still takes the fp16 tensor of a projection and quantises it into the arena;
 * ia2p_llm_arena_bytes and ia2p_llm_workspace_bytes (a prefill dequantises one projection at a time into the workspace) follow the format. Decode reads
 * the codes directly; rows of up to 14336 weights. bits = 16 restores the default. IA2P_ERR_INVALID for other bit counts or a null codebook,
 * IA2P_ERR_STATE once an arena is bound. */
ia2p_status ia2p_llm_set_weight_format(ia2p_llm* llm, int bits, const float* codebook);
int ia2p_llm_weight_bits(ia2p_llm* llm);
/* KV cache: fp16 [layer][k | v][max_positions][hidden], caller-owned device memory (16-byte aligned), max_positions <= 8192 (0 bytes otherwise).
 * Binding a cache sets the position to 0. */
size_t ia2p_llm_kv_bytes(ia2p_llm* llm, int max_positions);
ia2p_status ia2p_llm_bind_kv(ia2p_llm* llm, void* dev_cache, size_t bytes, int max_positions);
/* workspace that serves a prefill of up to max_T rows and any decode step */
size_t ia2p_llm_workspace_bytes(ia2p_llm* llm, int max_T);
/* a new request: position 0 (the cache's contents past the position are never read) */
ia2p_status ia2p_llm_reset(ia2p_llm* llm);
int ia2p_llm_position(ia2p_llm* llm);
/* rows of `model.embed_tokens` for int32 device ids [T] -> fp16 [T, hidden] (`embed_tokens(input_ids)`, any2pix_llama.py:277; ids are clamped to the table) */
ia2p_status ia2p_llm_embed(ia2p_llm* llm, void* stream, const int32_t* input_ids, int T, void* out);
/* T rows of `inputs_embeds` (fp16 [T, hidden], device) at positions position .. position + T - 1: fills the cache and returns, for the LAST row,
 * the final-normed hidden state (fp32 [hidden]: `hidden_states[-1][:, -1:]`, what pipeline.py:236,242,257 read) and the logits (fp32 [vocab_size]).
 * IA2P_ERR_SHAPE when the rows do not fit the cache, IA2P_ERR_NOMEM when they do not fit the workspace. */
ia2p_status ia2p_llm_prefill(ia2p_llm* llm, void* stream, const void* inputs_embeds, int T, float* hidden_out, float* logits_out, void* workspace,
                             size_t workspace_bytes);
/* one row at the current position: the table embedding of token_id (generated tokens are always embedded from the table, `<video>` included:
 * any2pix_llama.py:286-287 touches the first n `<video>` positions only). Same outputs.
 * IA2P_ERR_STATE before a prefill (position 0), IA2P_ERR_SHAPE when the position is past the cache or the token outside the vocabulary. */
ia2p_status ia2p_llm_decode(ia2p_llm* llm, void* stream, int token_id, float* hidden_out, float* logits_out, void* workspace, size_t workspace_bytes);
/* the weight-streaming GEMV of the decode path on its own (tools/llm_decode_bench.py measures it against ia2p_linear_small):
 * out[N] fp32 = W[N, K] fp16 . x[K] fp32, K a multiple of 8 */
ia2p_status ia2p_llm_gemv(void* stream, const void* W, const float* x, float* out, int N, int K);
/* The 4-bit format per operation (unit tests, tools/llm_decode_bench.py). W: fp16 [N, K] on the device, K a multiple of 64; `packed`:
 * ia2p_llm_q4_packed_bytes(N, K) bytes (0 for a K that cannot be packed; the layout inside is the engine's own); absmax: fp32 [N * K / 64]; codebook: 16
 * host floats. Dequantising gives fp16(codebook[code] * absmax). The GEMV is the decode path's: out[N] fp32 = dequantised W . x[K] fp32, K <= 14336. */
size_t ia2p_llm_q4_packed_bytes(int64_t N, int64_t K);
ia2p_status ia2p_llm_quantize_q4(void* stream, const void* W, int64_t N, int64_t K, const float* codebook, void* packed, float* absmax);
ia2p_status ia2p_llm_dequantize_q4(void* stream, const void* packed, const float* absmax, int64_t N, int64_t K, const float* codebook, void* W);
ia2p_status ia2p_llm_gemv_q4(void* stream, const void* packed, const float* absmax, const float* codebook, const float* x, float* out, int N, int K);
/* ---- Several sequences per weight pass ----------------------------------------------------------------------------------------------------------
 * The cache as n_slots independent sequences, fp16 [slot][layer][k | v][max_positions][hidden] (one slot: the layout above), each slot with its own
 * position. ia2p_llm_bind_kv is the one-slot form; ia2p_llm_prefill / _decode / _reset / _position act on slot 0 and run the single-sequence kernels.
 * ia2p_llm_kv_slots_bytes: 0 for n_slots < 1 or max_positions outside 1..8192. Binding sets every position to 0. */
#define IA2P_LLM_MAX_ROWS 8
size_t ia2p_llm_kv_slots_bytes(ia2p_llm* llm, int max_positions, int n_slots);
ia2p_status ia2p_llm_bind_kv_slots(ia2p_llm* llm, void* dev_cache, size_t bytes, int max_positions, int n_slots);
int ia2p_llm_slots(ia2p_llm* llm);
ia2p_status ia2p_llm_reset_slot(ia2p_llm* llm, int slot);            /* IA2P_ERR_INVALID for a slot outside the cache */
int ia2p_llm_slot_position(ia2p_llm* llm, int slot);                 /* -1 for a slot outside the cache */
/* ia2p_llm_prefill on the cache and position of `slot` (prompts differ in length: they are prefilled one at a time); other slots are not touched.
 * IA2P_ERR_INVALID for a slot outside the cache. */
ia2p_status ia2p_llm_prefill_slot(ia2p_llm* llm, void* stream, int slot, const void* inputs_embeds, int T, float* hidden_out, float* logits_out,
                                  void* workspace, size_t workspace_bytes);
/* One decode step for n = 1..IA2P_LLM_MAX_ROWS sequences. `slots` and `token_ids` are HOST arrays [n]: row r embeds token_ids[r] from the table and runs at
 * the position of slot slots[r], which then advances by one. Per layer five weight launches and one attention launch serve all rows, then one launch for
 * the final norm and lm_head: every weight is read (4 bits: decoded) once per step. hidden_out: fp32 [n, hidden], logits_out: fp32 [n, vocab_size]
 * (device). Row r equals, bit for bit, what ia2p_llm_decode returns for that sequence alone.
 * IA2P_ERR_INVALID: n outside 1..8, a slot outside the cache, a slot named twice. IA2P_ERR_STATE: a slot at position 0, weights or cache not bound.
 * IA2P_ERR_SHAPE: a slot whose position is past the cache, a token outside the vocabulary. IA2P_ERR_NOMEM: the (256-byte aligned) workspace is smaller
 * than ia2p_llm_batch_workspace_bytes(llm, 0, n). A refused call changes no position. */
ia2p_status ia2p_llm_decode_batch(ia2p_llm* llm, void* stream, const int32_t* slots, const int32_t* token_ids, int n, float* hidden_out, float* logits_out,
                                  void* workspace, size_t workspace_bytes);
/* ia2p_llm_decode_batch with the ids in DEVICE memory: row r embeds dev_tokens[token_index[r]] (dev_tokens: int32, device, e.g. what ia2p_sample_tokens wrote on
 * the same stream; token_index: HOST array [n] of non-negative indices into it, or NULL for 0..n-1 -- the caller answers for the buffer holding them). The host
 * never reads the ids: the embedding kernel does, and clamps an id outside [0, vocab_size) into the table (a sampler's -1 embeds row 0; the caller finds the -1
 * when it reads the token and discards the step). Everything else -- checks, statuses, launches, bits of a row given its id -- is ia2p_llm_decode_batch's; the
 * vocabulary check of the ids is the one check that cannot be made on the host. */
ia2p_status ia2p_llm_decode_batch_dev(ia2p_llm* llm, void* stream, const int32_t* slots, const int32_t* dev_tokens, const int32_t* token_index, int n,
                                      float* hidden_out, float* logits_out, void* workspace, size_t workspace_bytes);
/* ---- Sampling on the device -------------------------------------------------------------------------------------------------------------------------
 * One token per logits row, by the step transformers' sampling loop applies (TemperatureLogitsWarper -> TopKLogitsWarper -> softmax -> one draw):
 * logits fp32, row r at logits + r * ld (device; ld = 0 draws M times from one row, otherwise ld >= V), M = 1..4096 rows, V = 1..2^20, any alignment of a row.
 *   do_sample = 0   tokens_out[r] = the lowest index among the row's maxima; nothing else is written, seeds / steps may be NULL
 *   do_sample = 1   score = logit / temperature (fp32, temperature > 0). 0 < top_k < V keeps every index whose score is >= the k-th largest score of the row
 *                   (ties at that value are all kept, as `scores < kth` removes nothing equal); any other top_k keeps everything. p = exp(score - max) / sum over
 *                   the kept set, fp32. tokens_out[r] = the first kept index, in ascending order, whose inclusive cumulative sum exceeds u * sum; if rounding
 *                   leaves none, the last index with a positive term. An index whose term is 0 (a -inf entry, an underflow) is never drawn.
 *   u               = (word 0 of Philox4x32-10 at counter (steps[r], 0, 0, 0) under key (low, high half of seeds[r])) >> 8, times 2^-24: in [0, 1). The draw of
 *                   a row depends on its logits, its seed and its step only -- not on M, the row's place or alignment, or the other rows.
 * A row holding NaN or +inf (also: a score that overflows), or whose maximum is -inf, gets token -1 and no probs_out row.
 * seeds, steps: HOST arrays [M]. For M <= 8 they travel by value in the kernel arguments and nothing is copied to the device. For M > 8 the call allocates a
 * device staging block, copies both arrays into it on `stream`, and waits for the stream before it frees the block and returns (a path for tests and tools;
 * a decode step never has more than IA2P_LLM_MAX_ROWS rows).
 * tokens_out: int32 [M], device. probs_out: fp32 [M, V] dense, device, or NULL: the whole row, exactly 0.0f outside the kept set. u_out: fp32 [M], device,
 * or NULL. Every sum has one fixed association: two launches give the same tokens and the same probs_out bits.
 * IA2P_ERR_INVALID: a null or misaligned pointer, do_sample outside {0, 1}, a temperature that is not positive and finite. IA2P_ERR_SHAPE: M, V or ld. */
ia2p_status ia2p_sample_tokens(void* stream, const float* logits, int64_t ld, int M, int V, float temperature, int top_k, int do_sample, const uint64_t* seeds,
                               const uint32_t* steps, int32_t* tokens_out, float* probs_out, float* u_out);
/* ia2p_sample_tokens with a nucleus (TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> softmax -> one draw). Limits on M, V, ld and alignment,
 * do_sample = 0 (which ignores top_p), u, the -1 of a row that cannot be sampled, the by-value path for M <= 8 and the statuses are ia2p_sample_tokens's;
 * top_p = 1 IS ia2p_sample_tokens, bit for bit (that call forwards here). A top_p that is NaN, <= 0 or > 1 is refused with IA2P_ERR_INVALID before any HIP call,
 * whatever do_sample says.
 * The rule for top_p < 1. Let K be the set top-k keeps (ties included, as above), e_i = exp(score_i - max) for i in K and Z their sum; for a score value v let
 * T(v) be the sum of e_i over the i in K with score_i <= v. Index i is in the nucleus iff e_i > 0 and T(score_i) > (1 - top_p) * Z. For distinct scores this is
 * transformers' rule (sort ascending, remove while the cumulative probability is <= 1 - top_p, always keep the last). Equal scores are kept or dropped
 * TOGETHER: transformers splits a tied group by its position in the sort, which is unspecified; here a group that reaches into the nucleus is kept whole, as the
 * top-k step keeps the ties at the k-th value. The maximum (with its ties) is always in the nucleus.
 * Then p = e / Z' over the nucleus (Z' its fp32 sum), the cumulative sum in index order against u * Z', and probs_out exactly 0 outside the nucleus, all as above.
 * T and Z are integer sums of trunc(e_i * 2^43) (1 - top_p taken in double from the fp32 top_p; the comparison is made on integers, with the threshold capped at
 * Z - 1), so they have no summation order: the nucleus of a row does not depend on the launch, M, the row's place or its alignment. A term below 2^-43 of the
 * largest counts as 0 there. */
ia2p_status ia2p_sample_tokens_p(void* stream, const float* logits, int64_t ld, int M, int V, float temperature, int top_k, float top_p, int do_sample,
                                 const uint64_t* seeds, const uint32_t* steps, int32_t* tokens_out, float* probs_out, float* u_out);
/* workspace that serves a prefill of any row count up to max_T (0: none; the largest need over 1..max_T, which is not monotone in T) and decode steps of up to
 * max_rows rows; 0 for max_T < 0 or max_rows outside 1..8 */
size_t ia2p_llm_batch_workspace_bytes(ia2p_llm* llm, int max_T, int max_rows);
/* the multi-row GEMVs of ia2p_llm_decode_batch on their own: x fp32 [M, K], out fp32 [M, N], M = 1..8 (IA2P_ERR_SHAPE otherwise); K as for the
 * single-row calls. out[m] equals the single-row call on x[m] bit for bit. */
ia2p_status ia2p_llm_gemv_rows(void* stream, const void* W, const float* x, float* out, int N, int K, int M);
ia2p_status ia2p_llm_gemv_q4_rows(void* stream, const void* packed, const float* absmax, const float* codebook, const float* x, float* out, int N, int K,
                                  int M);
/* ---- The other launches of the decode and prefill paths on their own (unit tests, tools) ---------------------------------------------------------------
 * Each runs the launcher or kernel the drivers run, with the arithmetic and the fixed summation order it has inside a model; tests/llm_ops_ref.py holds an fp64
 * reference and an error bound per operation. Every refusal is decided on the host before any launch, and a refused call writes nothing.
 * Weights: W is fp16 [N, K] (absmax and codebook NULL, K a multiple of 8) or the packed codes of ia2p_llm_quantize_q4 with their absmax and codebook (K a multiple
 * of 64, at most 14336). x: fp32 [M, K], M = 1..8 rows; one row runs the single-row kernels, and row m of a launch equals the single-row launch on that row bit
 * for bit. gamma (optional, fp16 [K]) with eps folds RMSNorm(x) * gamma into the product: out = rstd * (W . (x gamma)), rstd = 1 / sqrt(mean(x^2) + eps).
 * IA2P_ERR_INVALID: a null pointer, absmax without codebook or the reverse, an epilogue outside 0..2, hid without the plain epilogue and a gamma, a negative eps,
 * a cache that is not 16-byte aligned (attention). IA2P_ERR_SHAPE: N, K, M as for ia2p_llm_gemv_rows / ia2p_llm_gemv_q4_rows, an odd N with SwiGLU, H not
 * heads * 128, a position outside 0..8191 or rows that run past it. */
#define IA2P_LLM_EPI_PLAIN 0  /* out[m][n] = r[n]: fp32 [M, N] */
#define IA2P_LLM_EPI_RESID 1  /* out[m][n] += r[n]: fp32 [M, N], read and written */
#define IA2P_LLM_EPI_SWIGLU 2 /* out[m][i] = silu(r[i]) * r[N / 2 + i]: fp32 [M, N / 2]; rows 0 .. N / 2 - 1 of W are the gate, the rest the up projection */
/* the GEMV with an epilogue (o_proj, gate / up, down_proj, lm_head). hid (optional; plain epilogue with gamma): fp32 [M, K], the normed input rows x rstd gamma */
ia2p_status ia2p_llm_gemv_epi(void* stream, const void* W, const float* absmax, const float* codebook, const float* x, const void* gamma, float eps, int epi,
                              float* out, float* hid, int N, int K, int M);
/* the QKV GEMV, W [3 H, K] = q | k | v rows: rotary embedding of q and k at the row's position (angle = fp32 product of the position and inv_freq[i], i the
 * index of the pair (c, c + 64) inside its head; rotate_half convention) and the cache write. pos, k_cache, v_cache: HOST arrays [M] -- row m writes row pos[m]
 * of its own caches (device, fp16 [positions, H]; k rotated, v as computed) and nothing else of them. q: fp32 [M, H], rotated. inv_freq: fp32 [64], device. */
ia2p_status ia2p_llm_gemv_qkv(void* stream, const void* W, const float* absmax, const float* codebook, const float* x, const void* gamma, float eps,
                              const float* inv_freq, const int32_t* pos, float* q, void* const* k_cache, void* const* v_cache, int H, int K, int M);
/* attention of decoded rows: row m = softmax(q[m] . K^T / sqrt(128)) V per head over rows 0 .. pos[m] of its own caches; rows past pos[m] are never read.
 * q, out: fp32 [M, H]; pos, k_cache, v_cache: HOST arrays [M]. */
ia2p_status ia2p_llm_attention_rows(void* stream, const float* q, const void* const* k_cache, const void* const* v_cache, const int32_t* pos, float* out, int heads,
                                    int H, int M);
/* causal attention of prefill rows: row t of q (fp32 [T, H]) is at position p0 + t of one cache and sees its rows 0 .. p0 + t. out: fp16 [T, H]. */
ia2p_status ia2p_llm_attention_prefill(void* stream, const float* q, const void* k_cache, const void* v_cache, void* out, int heads, int H, int p0, int T);
/* the row kernels of the prefill path, fp16 in and out:
 *   rmsnorm_rows     y [T, H] = x rstd gamma, the product rounded once
 *   rope_cache_rows  qkv [T, 3 H] (q | k | v) -> q fp32 [T, H] rotated, rows p0 .. p0 + T - 1 of k_cache (rotated) and v_cache (copied)
 *   silu_mul_rows    gate_up [T, 2 I] (gate | up) -> act [T, I] = silu(gate) * up */
ia2p_status ia2p_llm_rmsnorm_rows(void* stream, const void* x, const void* gamma, float eps, void* y, int T, int H);
ia2p_status ia2p_llm_rope_cache_rows(void* stream, const void* qkv, const float* inv_freq, float* q, void* k_cache, void* v_cache, int H, int p0, int T);
ia2p_status ia2p_llm_silu_mul_rows(void* stream, const void* gate_up, void* act, int T, int I);
/* the 64 rotary frequencies ia2p_llm_finalize_weights derives for a rope_theta (a host function; inv_freq: HOST fp32 [64]): 1 / theta^(2 i / 128).
 * IA2P_ERR_INVALID for a theta that is not positive and finite. */
ia2p_status ia2p_llm_rope_inv_freq(float rope_theta, float* inv_freq);
/* exact (erf) GELU in place on fp16 [n]: the activation of an `mlpNx_gelu` projector head between two ia2p_linear_small calls
 * (llm/model/multimodal_projector/builder.py:33-74 `nn.GELU()`) */
ia2p_status ia2p_gelu(void* stream, void* x, int64_t n);

/* ---- the small launches around the UNet, one by one (every refusal is decided on the host, before a launch; device pointers, fp16 unless said otherwise) ----
 * clip_embed             x [rows, H] = tok[clamp(ids[row], 0, vocab - 1)] + pos[row % T] (embeds != NULL: embeds[row] instead of the table row; ids and tok may be
 *                        NULL then); stats: fp32 [rows, 2] = {sum, sum of squares} of the fp16 row of x. H % 8 == 0.
 * causal_attention_small qkv [B T, 3 heads D] = q | k | v -> out [B T, heads D], softmax(q . k / 8) over keys 0 .. q. D == 64, T <= 128.
 * clip_pool              out [B, H] = LayerNorm(x[b, p_b]), p_b the first position of the largest id (eos_id == 2), else the first position of eos_id (0 when absent).
 *                        ids: int32 [B, T], not negative.
 * softmax_rows           in place, x[r, :n] = softmax(scale x[r, :n]) for rows of stride ld >= n; n % 8 == 0, n <= 16384, ld % 8 == 0.
 * conv1x1_nchw           y [B, Co, HW] = w [Co, Ci] x [B, Ci, HW] + bias, Ci and Co <= 8.
 * patch_gather           px [B, C, Hi, Wi] -> cols [B gh gw, Kpad]: column (c, ky, kx) of the patch at (py stride, px stride), zero for columns >= C ps ps.
 * vit_embed              x [B, T, H]: row 0 = cls + pos[0], row 1 + p = LN_stem?(patches[b, p]) + pos[1 + p], then LN_pre?; stats as clip_embed. A gamma and its
 *                        beta are both given or both NULL. H % 64 == 0, H <= 2048, T >= 2.
 * vit_project            out fp32 [B, N] = X [B, K] . W [N, K]^T, K % 8 == 0.
 * embed                  tsin [B, Tp] = [cos(t f_i) | sin(t f_i)], f_i = exp(-ln(10000) i / (Tp / 2)); addin [B, P + nids Ad] = [text_embeds[b] | the same sinusoid
 *                        of width Ad of each of time_ids [B, nids]]. ts (optional, device fp32 [B]): one t per batch element. Tp and Ad even.
 * concat                 y [M, Ca + Cb] = [a[m, :Ca] | b[m, :Cb]], rows of stride lda / ldb; multiples of 8.
 * cat_rows               dst [rows, Ka + Kb] = [a[r] | b[r]], bias_dst = bias_a + bias_b (one rounding); multiples of 8. */
ia2p_status ia2p_clip_embed(void* stream, const int32_t* ids, const void* tok, const void* embeds, const void* pos, void* x, float* stats, int rows, int T, int H, int vocab);
ia2p_status ia2p_causal_attention_small(void* stream, const void* qkv, void* out, int B, int T, int heads, int D);
ia2p_status ia2p_clip_pool(void* stream, const int32_t* ids, const void* x, const void* gamma, const void* beta, void* out, int B, int T, int H, int eos_id, float eps);
ia2p_status ia2p_softmax_rows(void* stream, void* x, int64_t ld, int rows, int n, float scale);
ia2p_status ia2p_conv1x1_nchw(void* stream, const void* x, const void* w, const void* bias, void* y, int B, int Ci, int Co, int64_t HW);
ia2p_status ia2p_patch_gather(void* stream, const void* px, void* cols, int B, int C, int Hi, int Wi, int ps, int stride, int gh, int gw, int Kpad);
ia2p_status ia2p_vit_embed(void* stream, const void* patches, const void* cls, const void* pos, const void* stem_g, const void* stem_b, const void* pre_g, const void* pre_b,
                           void* x, float* stats, int B, int T, int H, float eps);
ia2p_status ia2p_vit_project(void* stream, const void* X, const void* W, float* out, int B, int N, int K);
ia2p_status ia2p_embed(void* stream, float t, const float* ts, const void* text_embeds, const void* time_ids, void* tsin, void* addin, int B, int Tp, int P, int Ad, int nids);
ia2p_status ia2p_concat(void* stream, const void* a, int lda, int Ca, const void* b, int ldb, int Cb, void* y, int64_t M);
ia2p_status ia2p_cat_rows(void* stream, const void* a, int Ka, const void* b, int Kb, const void* bias_a, const void* bias_b, void* dst, void* bias_dst, int rows);
/* the small launches of the SAM mask decoder:
 *   pixel_shuffle2  g [B, Hs, Ws, (ky, kx, co)] -> y [B, 2 Hs, 2 Ws, Co] (the GEMM form of a ConvTranspose2d(k = 2, s = 2)); Co % 8 == 0
 *   hyper_dot       mask fp32 [n, P] = sum_c hyper[n, c] up[n, p, c], rows of hyper at stride hyper_stride >= C; C % 8 == 0, no upper limit on C
 *   sam_act         in place on fp16 [n]: kind 0 ReLU, 1 exact (erf) GELU
 *   sam_add_rows    out[i] = a[i] + b[i % period] (out may alias a); n, period multiples of 8, period dividing n
 *   sam_take_col    dst fp32 [n] = src[i ld] */
ia2p_status ia2p_pixel_shuffle2(void* stream, const void* g, void* y, int B, int Hs, int Ws, int Co);
ia2p_status ia2p_hyper_dot(void* stream, const void* hyper, int64_t hyper_stride, const void* up, float* mask, int n, int P, int C);
ia2p_status ia2p_sam_act(void* stream, void* x, int64_t n, int kind);
ia2p_status ia2p_sam_add_rows(void* stream, const void* a, const void* b, void* out, int64_t n, int64_t period);
ia2p_status ia2p_sam_take_col(void* stream, const void* src, int64_t ld, float* dst, int n);

/* ---- LoRA adapters: a weight with its low-rank updates merged in, one launch per weight ------------------------------------------------------------------------
 * base, out: fp16 [N][K] row-major in the checkpoint's layout (a [Co][Ci][kh][kw] convolution weight is K = Ci kh kw); out == base (in place) is allowed, any other
 * overlap of out with base, up or down is refused. up[a]: fp16 [N][rank[a]], down[a]: fp16 [rank[a]][K], device memory; up, down, rank and coef are HOST arrays of
 * n entries, 1 <= n <= IA2P_LORA_MAX_ADAPTERS, 1 <= rank[a] <= IA2P_LORA_MAX_RANK. No divisibility rule on N, K or the ranks (guarded edges); rows move in 16-byte
 * accesses where K % 8 == 0 (rank[a] % 8 == 0 for up) and the pointer is 16-byte aligned.
 *   out[i][k] = fp16_rn( s_n ),  s_0 = float(base[i][k]),  s_{a+1} = fma(coef[a], acc_a[i][k], s_a)   (fp32, adapters in list order, one rounding each)
 *   acc_a[i][k] = the fp32 accumulation of the products up_a[i][j] down_a[j][k] (each exact in fp32) on v_mfma_f32_16x16x32_f16, the rank zero-padded to a multiple of
 *   32, 32-rank steps in ascending order into one accumulator; the order inside a step is the instruction's.
 * ONE rounding to fp16, at the store. coef[a] = weight_a alpha_a / rank_a is the caller's, computed in fp32. An element's bits depend on its row of up, its column
 * of down, its base value and coef alone -- not on N, K, the tile it falls in or the launch; no atomics. Refusals (null pointer, n or a rank out of range, a
 * non-finite coefficient, N or K not positive, an overlap) are made on the host before anything is launched: IA2P_ERR_INVALID / IA2P_ERR_SHAPE, text through
 * ia2p_last_error(NULL). */
#define IA2P_LORA_MAX_ADAPTERS 8
#define IA2P_LORA_MAX_RANK 256
ia2p_status ia2p_lora_merge(void* stream, const void* base, void* out, int N, int64_t K, int n, const void* const* up, const void* const* down, const int* rank, const float* coef);

#ifdef __cplusplus
}
#endif
#endif /* IA2P_H */
