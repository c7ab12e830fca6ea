// The context-less C ABI (include/ia2p.h, ia2p_debug.h): the sampler updates and one entry point per operator -- argument checks, a launch descriptor from launch_args.h,
// the launcher. The surface the per-operator GPU tests go through; needs engine_rt.hip (error state, zero page, plan helpers), nothing of any executor.
#include "engine_rt.h"
#include "gemm_tile.h"      // ia2p_pack_rowmap: ia2p_gemm_form refuses a row map by the launcher's own rule

extern "C" {

int ia2p_device_is_gfx950(void) {
  int dev = 0;
  hipDeviceProp_t p;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return 0;
  return strncmp(p.gcnArchName, "gfx950", 6) == 0;
}

ia2p_status ia2p_ddim_step(void* stream, const void* x, const void* eu, const void* ec, float g, float c_x, float c_e, void* out, void* out2, int64_t n) {
  if (!x || !eu || !out || n < 0) return fail(nullptr, IA2P_ERR_INVALID, "ddim_step: null argument");
  hipError_t e = ia2p_launch_ddim_step((const half_t*)x, (const half_t*)eu, (const half_t*)ec, g, c_x, c_e, (half_t*)out, (half_t*)out2, (long)n, (hipStream_t)stream);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "ddim_step");
}

// The same update with per-request coefficients: coef (device, float [B][3]) = {guidance g, c_x, c_e} of batch element b, `per` elements each --
// requests with their own guidance scale (reference pipeline.py:303 `cfg`) at their own step of their own schedule share one launch.
ia2p_status ia2p_ddim_step_v(void* stream, const void* x, const void* eu, const void* ec, const float* coef, void* out, void* out2, int B, int64_t per) {
  if (!x || !eu || !out || !coef || B < 0 || per < 1) return fail(nullptr, IA2P_ERR_INVALID, "ddim_step_v: bad argument");
  hipError_t e = ia2p_launch_ddim_step((const half_t*)x, (const half_t*)eu, (const half_t*)ec, 0.f, 0.f, 0.f, (half_t*)out, (half_t*)out2, (long)B * per, (hipStream_t)stream, coef, (long)per);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "ddim_step_v");
}

ia2p_status ia2p_mask_blend(void* stream, const void* x, const void* init, const void* noise, const void* mask, float c0, float c1,
                            void* out, void* out2, int B, int C, int64_t HW) {
  if (!x || !init || !noise || !mask || !out || B < 0 || C < 1 || HW < 1) return fail(nullptr, IA2P_ERR_INVALID, "mask_blend: bad argument");
  hipError_t e = ia2p_launch_mask_blend((const half_t*)x, (const half_t*)init, (const half_t*)noise, (const half_t*)mask, c0, c1, (half_t*)out, (half_t*)out2,
                                        B, C, (long)HW, (hipStream_t)stream);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "mask_blend");
}

// The same blend with per-request coefficients: coef (device, float [B][2]) = {c0, c1} of batch element b -- requests at their own step of their own
// inpainting schedule share one launch; a request that is through carries {1, 0}.
ia2p_status ia2p_mask_blend_v(void* stream, const void* x, const void* init, const void* noise, const void* mask, const float* coef,
                              void* out, void* out2, int B, int C, int64_t HW) {
  if (!x || !init || !noise || !mask || !coef || !out) return fail(nullptr, IA2P_ERR_INVALID, "mask_blend_v: null argument");
  if (B < 1 || C < 1 || HW < 1) return fail(nullptr, IA2P_ERR_SHAPE, "mask_blend_v: B=%d C=%d HW=%lld must all be >= 1", B, C, (long long)HW);
  hipError_t e = ia2p_launch_mask_blend((const half_t*)x, (const half_t*)init, (const half_t*)noise, (const half_t*)mask, 0.f, 0.f, (half_t*)out, (half_t*)out2,
                                        B, C, (long)HW, (hipStream_t)stream, coef);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "mask_blend_v");
}

// ---- editing inside a mask: the selection of the sampling loops and the three image kernels. Every refusal comes before any HIP call. ----------------------
ia2p_status ia2p_known_blend_v(void* stream, const void* x, const void* known, const int32_t* level, const void* mask, void* out, void* out2, int B, int C,
                               int64_t HW, int levels) {
  if (!x || !known || !level || !mask || !out) return fail(nullptr, IA2P_ERR_INVALID, "known_blend_v: null argument");
  if (B < 1 || C < 1 || HW < 1 || levels < 1) return fail(nullptr, IA2P_ERR_SHAPE, "known_blend_v: B=%d C=%d HW=%lld levels=%d must all be >= 1", B, C, (long long)HW, levels);
  if ((double)B * C * (double)HW * levels > 4.0e18) return fail(nullptr, IA2P_ERR_SHAPE, "known_blend_v: the trajectory store exceeds a 64-bit element count");
  hipError_t e = ia2p_launch_known_blend((const half_t*)x, (const half_t*)known, (const int*)level, (const half_t*)mask, (half_t*)out, (half_t*)out2, B, C, (long)HW,
                                         levels, (hipStream_t)stream);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "known_blend_v");
}

static ia2p_status check_mask_image(const char* what, int B, int H, int W, int C) {
  if (B < 0 || H < 0 || W < 0) return fail(nullptr, IA2P_ERR_INVALID, "%s: negative size B=%d H=%d W=%d", what, B, H, W);
  if (B < 1 || H < 1 || W < 1) return fail(nullptr, IA2P_ERR_SHAPE, "%s: empty image B=%d H=%d W=%d", what, B, H, W);
  if ((int64_t)B * H * W * C > INT32_MAX) return fail(nullptr, IA2P_ERR_SHAPE, "%s: %lld elements exceed the 32-bit count of one launch", what, (long long)B * H * W * C);
  return IA2P_OK;
}

ia2p_status ia2p_mask_to_latent(void* stream, const void* mask_u8, void* out, int B, int H, int W, int f) {
  if (!mask_u8 || !out) return fail(nullptr, IA2P_ERR_INVALID, "mask_to_latent: null pointer");
  ia2p_status st = check_mask_image("mask_to_latent", B, H, W, 1);
  if (st != IA2P_OK) return st;
  if (f < 1 || f > 64) return fail(nullptr, IA2P_ERR_INVALID, "mask_to_latent: f=%d (1 .. 64)", f);
  if (H % f || W % f) return fail(nullptr, IA2P_ERR_SHAPE, "mask_to_latent: H=%d W=%d are not multiples of f=%d", H, W, f);
  hipError_t e = ia2p_launch_mask_to_latent((const uint8_t*)mask_u8, (half_t*)out, B, H, W, f, (hipStream_t)stream);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "mask_to_latent");
}

ia2p_status ia2p_mask_feather_u8(void* stream, const void* mask_u8, void* out, void* workspace, int B, int H, int W, int r) {
  if (!mask_u8 || !out || !workspace) return fail(nullptr, IA2P_ERR_INVALID, "mask_feather_u8: null pointer");
  if (((uintptr_t)workspace & 1) != 0) return fail(nullptr, IA2P_ERR_INVALID, "mask_feather_u8: the workspace holds 16-bit sums and must be 2-byte aligned");
  if (out == mask_u8) return fail(nullptr, IA2P_ERR_INVALID, "mask_feather_u8: out may not alias the mask (the column pass reads it)");
  ia2p_status st = check_mask_image("mask_feather_u8", B, H, W, 2);
  if (st != IA2P_OK) return st;
  if (r < 0 || r > 64) return fail(nullptr, IA2P_ERR_INVALID, "mask_feather_u8: r=%d (0 .. 64)", r);
  hipError_t e = ia2p_launch_mask_feather_u8((const uint8_t*)mask_u8, (uint8_t*)out, (uint16_t*)workspace, B, H, W, r, (hipStream_t)stream);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "mask_feather_u8");
}

ia2p_status ia2p_image_composite_u8(void* stream, const void* edited, const void* base, const void* alpha, void* out, int B, int H, int W, int C) {
  if (!edited || !base || !alpha || !out) return fail(nullptr, IA2P_ERR_INVALID, "image_composite_u8: null pointer");
  if (C != 1 && C != 3) return fail(nullptr, IA2P_ERR_SHAPE, "image_composite_u8: C=%d (1 or 3 channels)", C);
  ia2p_status st = check_mask_image("image_composite_u8", B, H, W, C);
  if (st != IA2P_OK) return st;
  hipError_t e = ia2p_launch_image_composite_u8((const uint8_t*)edited, (const uint8_t*)base, (const uint8_t*)alpha, (uint8_t*)out, B, H, W, C, (hipStream_t)stream);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "image_composite_u8");
}

// ---- condition maps from the base image (condition.hip): grey, Gaussian blur, Canny, and the conversion a ControlNet takes. Every refusal comes before any HIP call. ----
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}
static size_t canny_state_bytes(int B, int H, int W) { return (((size_t)B * H * W) + 15) & ~(size_t)15; }

ia2p_status ia2p_image_grey_u8(void* stream, const void* rgb, void* grey, int B, int H, int W) {
  if (!rgb || !grey) return fail(nullptr, IA2P_ERR_INVALID, "image_grey_u8: null pointer");
  ia2p_status st = check_mask_image("image_grey_u8", B, H, W, 3);
  if (st != IA2P_OK) return st;
  if (ranges_overlap(rgb, (size_t)B * H * W * 3, grey, (size_t)B * H * W)) return fail(nullptr, IA2P_ERR_INVALID, "image_grey_u8: grey may not overlap rgb");
  hipError_t e = ia2p_launch_grey_u8((const uint8_t*)rgb, (uint8_t*)grey, B * H * W, (hipStream_t)stream);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "image_grey_u8");
}

size_t ia2p_image_gauss_workspace_bytes(int B, int H, int W, int C) {
  if (B < 1 || H < 1 || W < 1 || C < 1) return 0;
  return (size_t)B * H * W * C * sizeof(uint32_t);
}

ia2p_status ia2p_image_gauss_u8(void* stream, const void* src, void* dst, void* workspace, int B, int H, int W, int C, const uint16_t* taps, int r) {
  if (!src || !dst || !workspace || !taps) return fail(nullptr, IA2P_ERR_INVALID, "image_gauss_u8: null pointer");
  if (((uintptr_t)workspace & 3) != 0) return fail(nullptr, IA2P_ERR_INVALID, "image_gauss_u8: the workspace holds 32-bit sums and must be 4-byte aligned");
  if (C != 1 && C != 3) return fail(nullptr, IA2P_ERR_SHAPE, "image_gauss_u8: C=%d (1 or 3 channels)", C);
  ia2p_status st = check_mask_image("image_gauss_u8", B, H, W, 3);
  if (st != IA2P_OK) return st;
  if (r < 0 || r > 32) return fail(nullptr, IA2P_ERR_INVALID, "image_gauss_u8: r=%d (0 .. 32)", r);
  const size_t n = (size_t)B * H * W * C;
  if (ranges_overlap(workspace, n * 4, src, n) || ranges_overlap(workspace, n * 4, dst, n)) return fail(nullptr, IA2P_ERR_INVALID, "image_gauss_u8: the workspace overlaps an image");
  if (dst != src && ranges_overlap(src, n, dst, n)) return fail(nullptr, IA2P_ERR_INVALID, "image_gauss_u8: dst overlaps src (dst == src, in place, is allowed)");
  GaussTaps t;
  memset(&t, 0, sizeof t);
  uint32_t sum = taps[0];
  t.q[0] = taps[0];
  for (int i = 1; i <= r; ++i) { t.q[i] = taps[i]; sum += 2u * taps[i]; }
  if (sum != 4096u) return fail(nullptr, IA2P_ERR_INVALID, "image_gauss_u8: q_0 + 2 sum q_i = %u, must be 4096", sum);
  hipError_t e = ia2p_launch_gauss_u8((const uint8_t*)src, (uint8_t*)dst, (uint32_t*)workspace, B, H, W, C, t, r, (hipStream_t)stream);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "image_gauss_u8");
}

size_t ia2p_canny_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return canny_state_bytes(B, H, W) + 16;      // the state map, then the round flags
}

int64_t ia2p_canny_max_rounds(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return ia2p_canny_round_bound(B, H, W);
}

static ia2p_status check_canny(const char* what, const void* in, const void* edges, const void* workspace, size_t workspace_bytes, int B, int H, int W) {
  if (!in || !edges || !workspace) return fail(nullptr, IA2P_ERR_INVALID, "%s: null pointer", what);
  if (((uintptr_t)workspace & 3) != 0) return fail(nullptr, IA2P_ERR_INVALID, "%s: the workspace must be 4-byte aligned", what);
  ia2p_status st = check_mask_image(what, B, H, W, 3);
  if (st != IA2P_OK) return st;
  const size_t n = (size_t)B * H * W;
  if (ranges_overlap(in, n, edges, n)) return fail(nullptr, IA2P_ERR_INVALID, "%s: edges may not alias the input", what);
  if (workspace_bytes < ia2p_canny_workspace_bytes(B, H, W)) return fail(nullptr, IA2P_ERR_NOMEM, "%s: workspace too small (%zu bytes, %zu needed)", what, workspace_bytes, ia2p_canny_workspace_bytes(B, H, W));
  if (ranges_overlap(workspace, workspace_bytes, in, n) || ranges_overlap(workspace, workspace_bytes, edges, n)) return fail(nullptr, IA2P_ERR_INVALID, "%s: the workspace overlaps an image", what);
  return IA2P_OK;
}

// the rounds of the hysteresis over the state map at the head of the workspace, then the 0 / 255 output
static ia2p_status canny_finish_from_state(const char* what, void* stream, void* edges, void* workspace, int B, int H, int W, int* rounds_out) {
  uint8_t* state = (uint8_t*)workspace;
  uint32_t* flags = (uint32_t*)(state + canny_state_bytes(B, H, W));
  const int64_t bound = ia2p_canny_round_bound(B, H, W);
  int64_t rounds = 0;
  bool converged = false;
  hipError_t e = ia2p_run_canny_hysteresis(state, flags, B, H, W, bound, &rounds, &converged, (hipStream_t)stream);
  if (rounds_out) *rounds_out = (int)std::min<int64_t>(rounds, INT32_MAX);
  if (e != hipSuccess) return fail_hip(nullptr, e, what);
  if (!converged) return fail(nullptr, IA2P_ERR_STATE, "%s: the hysteresis still promoted pixels in round %lld, its bound for B=%d H=%d W=%d: no map is returned", what, (long long)bound, B, H, W);
  e = ia2p_launch_canny_finish(state, (uint8_t*)edges, B * H * W, (hipStream_t)stream);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, what);
}

ia2p_status ia2p_canny_u8(void* stream, const void* grey, void* edges, void* workspace, size_t workspace_bytes, int B, int H, int W, float low, float high,
                          int l2_gradient, int* rounds_out) {
  if (rounds_out) *rounds_out = 0;
  ia2p_status st = check_canny("canny_u8", grey, edges, workspace, workspace_bytes, B, H, W);
  if (st != IA2P_OK) return st;
  if (!(low >= 0.f) || !(high >= 0.f) || std::isinf(low) || std::isinf(high)) return fail(nullptr, IA2P_ERR_INVALID, "canny_u8: thresholds low=%g high=%g must be finite and >= 0", (double)low, (double)high);
  if (l2_gradient != 0 && l2_gradient != 1) return fail(nullptr, IA2P_ERR_INVALID, "canny_u8: l2_gradient=%d (0 or 1)", l2_gradient);
  if (low > high) std::swap(low, high);
  // no magnitude exceeds 2040 (|dx| + |dy|) or 2 * 1020^2: thresholds are clamped to 4096 before the square, which keeps every comparison as it was
  int lo = (int)std::floor(std::min(low, 4096.f)), hi = (int)std::floor(std::min(high, 4096.f));
  if (l2_gradient) { lo *= lo; hi *= hi; }
  hipError_t e = ia2p_launch_canny_classify((const uint8_t*)grey, (uint8_t*)workspace, B, H, W, lo, hi, l2_gradient, (hipStream_t)stream);
  if (e != hipSuccess) return fail_hip(nullptr, e, "canny_u8");
  return canny_finish_from_state("canny_u8", stream, edges, workspace, B, H, W, rounds_out);
}

// the second half of ia2p_canny_u8 on a state map the caller brings (0 off, 1 weak, 2 strong; any other value counts as off)
ia2p_status ia2p_canny_hysteresis_u8(void* stream, const void* state, void* edges, void* workspace, size_t workspace_bytes, int B, int H, int W, int* rounds_out) {
  if (rounds_out) *rounds_out = 0;
  ia2p_status st = check_canny("canny_hysteresis_u8", state, edges, workspace, workspace_bytes, B, H, W);
  if (st != IA2P_OK) return st;
  hipError_t e = hipMemcpyAsync(workspace, state, (size_t)B * H * W, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e != hipSuccess) return fail_hip(nullptr, e, "canny_hysteresis_u8");
  return canny_finish_from_state("canny_hysteresis_u8", stream, edges, workspace, B, H, W, rounds_out);
}

ia2p_status ia2p_condition_from_u8(void* stream, const void* map_u8, void* dst_f16, int B, int H, int W, int C_in) {
  if (!map_u8 || !dst_f16) return fail(nullptr, IA2P_ERR_INVALID, "condition_from_u8: null pointer");
  if (((uintptr_t)dst_f16 & 1) != 0) return fail(nullptr, IA2P_ERR_INVALID, "condition_from_u8: dst holds 16-bit values and must be 2-byte aligned");
  if (C_in != 1 && C_in != 3) return fail(nullptr, IA2P_ERR_SHAPE, "condition_from_u8: C_in=%d (1 or 3 channels)", C_in);
  ia2p_status st = check_mask_image("condition_from_u8", B, H, W, 3);
  if (st != IA2P_OK) return st;
  if (ranges_overlap(map_u8, (size_t)B * H * W * C_in, dst_f16, (size_t)B * H * W * 6)) return fail(nullptr, IA2P_ERR_INVALID, "condition_from_u8: dst overlaps the map");
  if (C_in == 3) return ia2p_image_from_u8(stream, map_u8, dst_f16, B, H, W, 3, 0);
  hipError_t e = ia2p_launch_condition_from_u8_c1((const uint8_t*)map_u8, (half_t*)dst_f16, B, H * W, (hipStream_t)stream);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "condition_from_u8");
}

ia2p_status ia2p_prior_step(void* stream, const float* sample, const void* out_cond, const void* out_uncond, const float* noise, float g, float sqrt_a,
                            float sqrt_b, float k0, float k1, float sigma, float* out, int64_t n) {
  if (!sample || !out_uncond || !out || n < 0 || !(sqrt_a > 0.f) || !(sqrt_b > 0.f)) return fail(nullptr, IA2P_ERR_INVALID, "prior_step: bad argument");
  hipError_t e = ia2p_launch_prior_step(sample, (const half_t*)out_cond, (const half_t*)out_uncond, noise, g, sqrt_a, sqrt_b, k0, k1, sigma, out, (long)n, (hipStream_t)stream);
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "prior_step");
}

// ---- per-operator entry points ---------------------------------------------------------------------------------------

ia2p_status ia2p_groupnorm_silu(void* stream, const void* x, void* y, const void* gamma, const void* beta, int B, int HW, int C, int groups, float eps, int silu, float* partial) {
  if (!x || !y || !gamma || !beta || !partial) return fail(nullptr, IA2P_ERR_INVALID, "groupnorm: null argument");
  if (C % 8 || C % groups || groups > 256) return fail(nullptr, IA2P_ERR_SHAPE, "groupnorm: C=%d groups=%d", C, groups);
  hipError_t e = ia2p_launch_groupnorm((const half_t*)x, C, (half_t*)y, C, (const half_t*)gamma, (const half_t*)beta, partial, B, HW, C, groups, eps, silu, (hipStream_t)stream);
  RET_HIP(e, "groupnorm");
}
ia2p_status ia2p_layernorm(void* stream, const void* x, void* y, const void* gamma, const void* beta, int M, int C, float eps) {
  if (!x || !y || !gamma || !beta) return fail(nullptr, IA2P_ERR_INVALID, "layernorm: null argument");
  if (C % 8 || C > 2048) return fail(nullptr, IA2P_ERR_SHAPE, "layernorm: C=%d must be a multiple of 8 and <= 2048", C);
  hipError_t e = ia2p_launch_layernorm((const half_t*)x, C, (half_t*)y, C, (const half_t*)gamma, (const half_t*)beta, M, C, eps, (hipStream_t)stream);
  RET_HIP(e, "layernorm");
}
ia2p_status ia2p_gemm(void* stream, const void* A, const void* W, const void* bias, const void* residual, void* C, int M, int N, int K, int geglu) {
  if (!A || !W || !C) return fail(nullptr, IA2P_ERR_INVALID, "gemm: null argument");
  if (K % 64 || N % 4 || (geglu && (N % 32 || !bias))) return fail(nullptr, IA2P_ERR_SHAPE, "gemm: K=%d must be a multiple of 64, N=%d of 4 (GEGLU: 32, with bias)", K, N);
  const int No = geglu ? N / 2 : N;
  const GemmArgs a = gemm_desc(zero_page(), (const half_t*)A, K, (const half_t*)W, K, (const half_t*)bias, (const half_t*)residual, No, (half_t*)C, No, M, N, K, geglu);
  hipError_t e = ia2p_launch_gemm(a, false, (hipStream_t)stream, nullptr);
  RET_HIP(e, "gemm");
}
// GEGLU feed-forward of a BasicTransformerBlock as an operator: H = geglu(X . W1p^T + b1p) [M, 4 C] (packed weights: ia2p_pack_geglu), out = H . W2^T + b2 + R,
// as the executor runs it (two launches, the library's plans). splitk / partial: K split of the second GEMM (partial: splitk * M * C floats) or 0.
ia2p_status ia2p_ffn(void* stream, const void* X, const void* W1p, const void* b1p, const void* W2, const void* b2, const void* R, void* H, void* out,
                     int M, int C, int splitk, float* partial) {
  if (!X || !W1p || !b1p || !W2 || !H || !out) return fail(nullptr, IA2P_ERR_INVALID, "ffn: null argument");
  if (C % 64 || (splitk > 1 && (!partial || splitk > 4 * C / 64 || splitk > 255))) return fail(nullptr, IA2P_ERR_SHAPE, "ffn: C=%d must be a multiple of 64, splitk=%d needs slabs", C, splitk);
  const GemmArgs a = gemm_desc(zero_page(), (const half_t*)X, C, (const half_t*)W1p, C, (const half_t*)b1p, nullptr, 0, (half_t*)H, 4 * C, M, 8 * C, C, 1);
  GemmArgs b = gemm_desc(zero_page(), (const half_t*)H, 4 * C, (const half_t*)W2, 4 * C, (const half_t*)b2, (const half_t*)R, C, (half_t*)out, C, M, C, 4 * C);
  if (splitk > 1) { b.splitk = splitk; b.partial = partial; }
  const GemmPlan pa = ia2p_gemm_plan(a.M, a.N, a.K, false, true), pb = ia2p_gemm_plan(b.M, b.N, b.K, false, false);
  hipError_t e = ia2p_launch_gemm_variant(a, false, pa.variant, (hipStream_t)stream);
  if (e == hipSuccess) e = ia2p_launch_gemm_variant(b, false, pb.variant, (hipStream_t)stream);
  RET_HIP(e, "ffn");
}
ia2p_status ia2p_fold_layernorm(void* stream, const void* W, const void* gamma, const void* beta, const void* bias, void* Wf, float* colsum,
                                float* fbias, int N, int K) {
  if (!W || !gamma || !beta || !Wf || !colsum || !fbias || N < 1 || K < 1) return fail(nullptr, IA2P_ERR_INVALID, "fold_layernorm: bad argument");
  hipError_t e = ia2p_launch_fold_ln((const half_t*)W, (const half_t*)gamma, (const half_t*)beta, (const half_t*)bias, (half_t*)Wf, colsum, fbias, N, K, (hipStream_t)stream);
  RET_HIP(e, "fold_layernorm");
}
ia2p_status ia2p_gemm_ex(void* stream, const void* A, const void* W, const void* bias, const void* residual, void* C, int M, int N, int K, int geglu,
                         const ia2p_ln_fold* ln, float* stats_out, int* stats_slots, int splitk, float* partial) {
  if (!A || !W || !C) return fail(nullptr, IA2P_ERR_INVALID, "gemm_ex: null argument");
  if (K % 64 || N % 4 || (geglu && (N % 32 || (!bias && !ln)))) return fail(nullptr, IA2P_ERR_SHAPE, "gemm_ex: K=%d must be a multiple of 64, N=%d of 4 (GEGLU: 32, with bias)", K, N);
  if (splitk > 1 && (!partial || geglu || splitk > K / 64 || splitk > 255)) return fail(nullptr, IA2P_ERR_SHAPE, "gemm_ex: splitk=%d needs a slab, no GEGLU, and <= min(K/64, 255)", splitk);
  if (!ln_fold_ok(ln)) return fail(nullptr, IA2P_ERR_INVALID, "gemm_ex: incomplete ia2p_ln_fold");
  if (stats_out && geglu) return fail(nullptr, IA2P_ERR_INVALID, "gemm_ex: row statistics of a GEGLU output are not provided");
  const int No = geglu ? N / 2 : N;
  GemmArgs a = gemm_desc(zero_page(), (const half_t*)A, K, (const half_t*)W, K, (const half_t*)bias, (const half_t*)residual, No, (half_t*)C, No, M, N, K, geglu);
  ln_attach(a, ln);
  a.stats_out = stats_out;
  if (splitk > 1) { a.splitk = splitk; a.partial = partial; }
#ifdef IA2P_CLOCK_STAMP
  else if (partial) a.partial = partial;      // (diagnostic builds: the in-kernel stamps of an unsplit launch go to the caller's buffer, tools/insitu_stamps.py)
#endif
  int pick = 0, combined = 0;
  hipError_t e = ia2p_launch_gemm(a, false, (hipStream_t)stream, &pick, &combined);
  if (stats_slots && pick >= 0 && pick < IA2P_GEMM_NVARIANT) *stats_slots = (splitk > 1 && !combined) ? 1 : (N + IA2P_GEMM_TILES[pick].bn - 1) / IA2P_GEMM_TILES[pick].bn;
  RET_HIP(e, "gemm_ex");
}
ia2p_status ia2p_gemm_splitk(void* stream, const void* A, const void* W, const void* bias, const void* residual, void* C, int M, int N, int K,
                             int splitk, float* partial) {
  if (!A || !W || !C || !partial) return fail(nullptr, IA2P_ERR_INVALID, "gemm_splitk: null argument");
  if (K % 64 || N % 4 || splitk < 1 || splitk > K / 64 || splitk > 255) return fail(nullptr, IA2P_ERR_SHAPE, "gemm_splitk: K=%d N=%d splitk=%d (1 .. min(K / 64, 255))", K, N, splitk);
  GemmArgs a = gemm_desc(zero_page(), (const half_t*)A, K, (const half_t*)W, K, (const half_t*)bias, (const half_t*)residual, N, (half_t*)C, N, M, N, K);
  a.splitk = splitk; a.partial = partial;
  hipError_t e = ia2p_launch_gemm(a, false, (hipStream_t)stream, nullptr);
  RET_HIP(e, "gemm_splitk");
}
ia2p_status ia2p_conv3x3(void* stream, const void* x, const void* Wp, const void* bias, const void* rowvec, const void* residual, void* y,
                         int B, int Hs, int Ws, int Cin, int Co, int stride, int up) {
  if (!x || !Wp || !y) return fail(nullptr, IA2P_ERR_INVALID, "conv3x3: null argument");
  if (Cin % 64 || Co % 4 || (stride != 1 && stride != 2) || (up != 0 && up != 1)) return fail(nullptr, IA2P_ERR_SHAPE, "conv3x3: Cin=%d (mult of 64) Co=%d (mult of 4) stride=%d up=%d", Cin, Co, stride, up);
  const GemmArgs a = conv3_desc(zero_page(), (const half_t*)x, B, Hs, Ws, Cin, (const half_t*)Wp, (const half_t*)bias, Co, stride, up, 1, (const half_t*)rowvec, Co, (const half_t*)residual, (half_t*)y);
  hipError_t e = ia2p_launch_gemm(a, true, (hipStream_t)stream, nullptr);
  RET_HIP(e, "conv3x3");
}
// the stride-1 form with K split over `splitk` workgroups per tile (what the executor launches for the 16 x 16 feature maps); partial: splitk * B*Hs*Ws * Co floats
ia2p_status ia2p_conv3x3_splitk(void* stream, const void* x, const void* Wp, const void* bias, const void* rowvec, const void* residual, void* y,
                                int B, int Hs, int Ws, int Cin, int Co, int splitk, float* partial) {
  if (!x || !Wp || !y || (splitk > 1 && !partial)) return fail(nullptr, IA2P_ERR_INVALID, "conv3x3_splitk: null argument (partial is needed for splitk > 1 only)");
  if (Cin % 64 || Co % 4 || splitk < 1 || splitk > 9 * Cin / 64 || splitk > 255) return fail(nullptr, IA2P_ERR_SHAPE, "conv3x3_splitk: Cin=%d (mult of 64) Co=%d (mult of 4) splitk=%d (1 .. 9 Cin / 64)", Cin, Co, splitk);
  GemmArgs a = conv3_desc(zero_page(), (const half_t*)x, B, Hs, Ws, Cin, (const half_t*)Wp, (const half_t*)bias, Co, 1, 0, 1, (const half_t*)rowvec, Co, (const half_t*)residual, (half_t*)y);
  if (splitk > 1) { a.splitk = splitk; a.partial = partial; }
  hipError_t e = ia2p_launch_gemm(a, true, (hipStream_t)stream, nullptr);
  RET_HIP(e, "conv3x3_splitk");
}
// ---- the GEMM and the 3x3 convolution with every option an executor sets on its own descriptor (CLIP / ViT / SAM / prior: activation on a folded LayerNorm; VAE: epilogue
//      scales, operand strides, pad_lo = 0; context K/V projection: row map, column offset): gemm_desc / conv3_desc plus the fields a site writes itself, then the
//      launcher. Every refusal comes before any launch: what the kernels assume (16-byte operand rows, 8-byte epilogue pieces) the launcher does not all check.
static bool al_(const void* q, uintptr_t a) { return (((uintptr_t)q) & (a - 1)) == 0; }
ia2p_status ia2p_gemm_form(void* stream, const struct ia2p_gemm_form* d) {
  if (d && d->stats_slots) *d->stats_slots = 0;
  if (!d || !d->A || !d->W || !d->C || (d->splitk > 1 && !d->partial)) return fail(nullptr, IA2P_ERR_INVALID, "gemm_form: null argument (partial is needed for splitk > 1)");
  if (d->M < 1 || d->N < 4 || d->N % 4 || d->K < 64 || d->K % 64) return fail(nullptr, IA2P_ERR_SHAPE, "gemm_form: M=%d (>= 1) N=%d (multiple of 4) K=%d (multiple of 64)", d->M, d->N, d->K);
  if (d->lda < d->K || d->ldw < d->K || d->ldc < d->N || (d->residual && d->ldr < d->N) || (d->rowvec && (d->rowvec_ld < d->N || d->rows_per_batch < 1)))
    return fail(nullptr, IA2P_ERR_SHAPE, "gemm_form: lda=%d ldw=%d (>= K=%d) ldc=%d ldr=%d rowvec_ld=%d (>= N=%d) rows_per_batch=%d (>= 1)", d->lda, d->ldw, d->K, d->ldc, d->ldr, d->rowvec_ld, d->N, d->rows_per_batch);
  if (d->act < 0 || d->act > 3) return fail(nullptr, IA2P_ERR_INVALID, "gemm_form: act=%d (0 none, 1 GELU erf, 2 quick-GELU, 3 GELU tanh; the per-image scale is ia2p_gemm_rowscale)", d->act);
  if (!std::isfinite(d->acc_scale) || !std::isfinite(d->bias_scale)) return fail(nullptr, IA2P_ERR_INVALID, "gemm_form: acc_scale / bias_scale must be finite (0: 1)");
  // operand rows are staged in 16-byte pieces; the epilogue's narrowest accesses are 8 bytes (4 columns), the folded-LayerNorm constants and the slabs 16
  if (d->lda % 8 || d->ldw % 8 || !al_(d->A, 16) || !al_(d->W, 16)) return fail(nullptr, IA2P_ERR_INVALID, "gemm_form: A and W must be 16-byte aligned with lda=%d ldw=%d multiples of 8", d->lda, d->ldw);
  if (d->ldc % 4 || !al_(d->C, 8) || (d->bias && !al_(d->bias, 8)) || (d->residual && (d->ldr % 4 || !al_(d->residual, 8))) || (d->rowvec && (d->rowvec_ld % 4 || !al_(d->rowvec, 8))))
    return fail(nullptr, IA2P_ERR_INVALID, "gemm_form: C, bias, residual and rowvec must be 8-byte aligned with ldc=%d ldr=%d rowvec_ld=%d multiples of 4", d->ldc, d->ldr, d->rowvec_ld);
  if (!ln_fold_ok(d->ln)) return fail(nullptr, IA2P_ERR_INVALID, "gemm_form: incomplete ia2p_ln_fold");
  if (d->ln && (!al_(d->ln->stats, 8) || !al_(d->ln->colsum, 16) || !al_(d->ln->fbias, 16))) return fail(nullptr, IA2P_ERR_INVALID, "gemm_form: ln->stats must be 8-byte, ln->colsum and ln->fbias 16-byte aligned");
  if ((d->stats_out && !al_(d->stats_out, 8)) || (d->splitk > 1 && !al_(d->partial, 16))) return fail(nullptr, IA2P_ERR_INVALID, "gemm_form: stats_out must be 8-byte, partial 16-byte aligned");
  if (d->splitk < 0 || d->splitk > d->K / 64 || d->splitk > 255) return fail(nullptr, IA2P_ERR_SHAPE, "gemm_form: splitk=%d (0 .. min(K / 64, 255))", d->splitk);
  int rowmap = 0;
  if (d->bstride < 0 || !ia2p_pack_rowmap(d->rpb, d->roff, &rowmap) || (!d->rpb && (d->bstride || d->roff)))
    return fail(nullptr, IA2P_ERR_SHAPE, "gemm_form: row map rpb=%d bstride=%d roff=%d (rpb and roff in 0 .. 65535, bstride >= 0; rpb == 0 is the identity and takes neither)", d->rpb, d->bstride, d->roff);
  const size_t a_rows = d->rpb ? ((size_t)d->M / d->rpb + 1) * (size_t)d->bstride + d->roff + d->rpb : (size_t)d->M;
  if (!ia2p_fits_buffer(a_rows, d->lda) || !ia2p_fits_buffer(d->N, d->ldw)) return fail(nullptr, IA2P_ERR_SHAPE, "gemm_form: an operand of 2 GiB or more (%zu rows of lda=%d, N=%d rows of ldw=%d)", a_rows, d->lda, d->N, d->ldw);
  GemmArgs a = gemm_desc(zero_page(), (const half_t*)d->A, d->lda, (const half_t*)d->W, d->ldw, (const half_t*)d->bias, (const half_t*)d->residual, d->residual ? d->ldr : 0, (half_t*)d->C, d->ldc,
                         d->M, d->N, d->K, 0, d->rpb, d->bstride, d->roff, d->act);
  a.acc_scale = d->acc_scale == 0.f ? 1.f : d->acc_scale; a.bias_scale = d->bias_scale == 0.f ? 1.f : d->bias_scale;
  if (d->rowvec) { a.rowvec = (const half_t*)d->rowvec; a.rowvec_ld = d->rowvec_ld; a.rows_per_batch = d->rows_per_batch; }
  ln_attach(a, d->ln);
  a.stats_out = d->stats_out;
  if (d->splitk > 1) { a.splitk = d->splitk; a.partial = d->partial; }
  int pick = 0, combined = 0;
  hipError_t e = ia2p_launch_gemm(a, false, (hipStream_t)stream, &pick, &combined);
  if (e == hipSuccess && d->stats_slots && d->stats_out && pick >= 0 && pick < IA2P_GEMM_NVARIANT) *d->stats_slots = (d->splitk > 1 && !combined) ? 1 : (d->N + IA2P_GEMM_TILES[pick].bn - 1) / IA2P_GEMM_TILES[pick].bn;
  RET_HIP(e, "gemm_form");
}
ia2p_status ia2p_conv3x3_form(void* stream, const ia2p_conv_form* d) {
  if (!d || !d->x || !d->Wp || !d->y || (d->splitk > 1 && !d->partial)) return fail(nullptr, IA2P_ERR_INVALID, "conv3x3_form: null argument (partial is needed for splitk > 1)");
  if (d->B < 1 || d->Hs < 1 || d->Ws < 1 || d->Cin < 64 || d->Cin % 64 || d->Co < 4 || d->Co % 4 || (d->stride != 1 && d->stride != 2) || (d->up != 0 && d->up != 1) || (d->pad_lo != 0 && d->pad_lo != 1))
    return fail(nullptr, IA2P_ERR_SHAPE, "conv3x3_form: B=%d Hs=%d Ws=%d Cin=%d (mult of 64) Co=%d (mult of 4) stride=%d (1 | 2) up=%d pad_lo=%d (0 | 1)", d->B, d->Hs, d->Ws, d->Cin, d->Co, d->stride, d->up, d->pad_lo);
  if (((d->Hs << d->up) + d->pad_lo + 1 < 3) || ((d->Ws << d->up) + d->pad_lo + 1 < 3)) return fail(nullptr, IA2P_ERR_SHAPE, "conv3x3_form: a %d x %d image with pad_lo=%d has no output pixel", d->Hs, d->Ws, d->pad_lo);
  if (d->splitk < 0 || d->splitk > 9 * d->Cin / 64 || d->splitk > 255) return fail(nullptr, IA2P_ERR_SHAPE, "conv3x3_form: splitk=%d (0 .. min(9 Cin / 64, 255))", d->splitk);
  if (!std::isfinite(d->acc_scale) || !std::isfinite(d->bias_scale)) return fail(nullptr, IA2P_ERR_INVALID, "conv3x3_form: acc_scale / bias_scale must be finite (0: 1)");
  if (!al_(d->x, 16) || !al_(d->Wp, 16) || !al_(d->y, 8) || (d->bias && !al_(d->bias, 8)) || (d->rowvec && !al_(d->rowvec, 8)) || (d->residual && !al_(d->residual, 8)) || (d->splitk > 1 && !al_(d->partial, 16)))
    return fail(nullptr, IA2P_ERR_INVALID, "conv3x3_form: x, Wp and partial must be 16-byte, y, bias, rowvec and residual 8-byte aligned");
  GemmArgs a = conv3_desc(zero_page(), (const half_t*)d->x, d->B, d->Hs, d->Ws, d->Cin, (const half_t*)d->Wp, (const half_t*)d->bias, d->Co, d->stride, d->up, d->pad_lo, (const half_t*)d->rowvec, d->Co,
                          (const half_t*)d->residual, (half_t*)d->y);
  if ((int64_t)d->B * a.Ho * a.Wo > INT32_MAX || !ia2p_fits_buffer((size_t)d->B * d->Hs * d->Ws, d->Cin) || !ia2p_fits_buffer(d->Co, a.K) || !ia2p_fits_buffer((size_t)d->B * a.Ho * a.Wo, d->Co))
    return fail(nullptr, IA2P_ERR_SHAPE, "conv3x3_form: an operand of 2 GiB or more");
  a.acc_scale = d->acc_scale == 0.f ? 1.f : d->acc_scale; a.bias_scale = d->bias_scale == 0.f ? 1.f : d->bias_scale;
  if (d->splitk > 1) { a.splitk = d->splitk; a.partial = d->partial; }
  hipError_t e = ia2p_launch_gemm(a, true, (hipStream_t)stream, nullptr);
  RET_HIP(e, "conv3x3_form");
}
// ---- GroupNorm from producer-side column sums (round 5; csrc/gn_fold.h): the operators of the fused path, one by one -----------------------------------------------
// canonical statistics of a tensor x [M, C]: out[(slot * C + c) * 2 + {0, 1}] = {sum, sum of squares} (fp64) over the `rows` rows of slot `slot` (what a GEMM / conv epilogue
// leaves for its own output when asked: ia2p_gemm_gnstats, ia2p_conv3x3_gn)
ia2p_status ia2p_gn_colstats(void* stream, const void* x, int M, int C, int rows, double* out) {
  if (!x || !out) return fail(nullptr, IA2P_ERR_INVALID, "gn_colstats: null argument");
  if (C < 8 || C % 8 || rows < 16 || rows % 16 || M < 1 || M % rows) return fail(nullptr, IA2P_ERR_SHAPE, "gn_colstats: C=%d (multiple of 8), rows=%d (multiple of 16 dividing M=%d)", C, rows, M);
  hipError_t e = ia2p_launch_gn_colstats((const half_t*)x, C, M, C, rows, out, (hipStream_t)stream);
  RET_HIP(e, "gn_colstats");
}
static ia2p_status gn_in_from_abi(const char* what, GemmArgs::GnIn* g, int C0, const double* st0, int rows0, int C1, const double* st1, int rows1, const void* gamma, const void* beta, int groups, float eps, int silu, int HW) {
  const int C = C0 + C1;
  if (!st0 || !gamma || !beta || (C1 > 0 && !st1)) return fail(nullptr, IA2P_ERR_INVALID, "%s: null argument", what);
  if (groups < 1 || groups > 64 || C % groups || C0 < 8 || C0 % 8 || C1 < 0 || C1 % 8 || rows0 < 1 || HW % rows0 || (C1 > 0 && (rows1 < 1 || HW % rows1)))
    return fail(nullptr, IA2P_ERR_SHAPE, "%s: C0=%d C1=%d groups=%d rows0=%d rows1=%d HW=%d", what, C0, C1, groups, rows0, rows1, HW);
  *g = gn_in_desc(st0, rows0, C1 > 0 ? st1 : nullptr, rows1, C0, C, (const half_t*)gamma, (const half_t*)beta, groups, eps, silu);
  return IA2P_OK;
}
// y = [silu](GroupNorm(groups)([x0 | x1])) with the statistics folded from the column sums of the sources' producers: the stand-alone twin of what ia2p_conv3x3_gn
// does to its operand inside the convolution (same fold, same scale / shift, same element formula: the two agree to the bit)
ia2p_status ia2p_gn_apply_stats(void* stream, const void* x0, int C0, const double* st0, int rows0, const void* x1, int C1, const double* st1, int rows1,
                                const void* gamma, const void* beta, void* y, int B, int HW, int groups, float eps, int silu) {
  if (!x0 || !y || (C1 > 0 && !x1)) return fail(nullptr, IA2P_ERR_INVALID, "gn_apply_stats: null argument");
  GemmArgs::GnIn g;
  const ia2p_status st = gn_in_from_abi("gn_apply_stats", &g, C0, st0, rows0, C1, st1, rows1, gamma, beta, groups, eps, silu, HW);
  if (st != IA2P_OK) return st;
  hipError_t e = ia2p_launch_gn_apply_stats((const half_t*)x0, C0, C1 > 0 ? (const half_t*)x1 : nullptr, C1, (half_t*)y, C0 + C1, B, HW, C0 + C1, g, (hipStream_t)stream);
  RET_HIP(e, "gn_apply_stats");
}
// 3x3 convolution (stride 1) of silu(GroupNorm([x0 | x1])) with the norm applied INSIDE the convolution (d->st0 != NULL; conv_halo_kernel.h GN = 1), or of x0 itself
// (d->st0 == NULL), + optional appended 1x1 block, time-embedding row, residual, K split; d->gn_out != NULL: also the column sums of y (*gn_out_rows: rows per slot,
// 0 when this launch could not take them). Fused form: the site must have a halo-staged plan (IA2P_ERR_SHAPE otherwise; tests force one with ia2p_debug_set_gemm_tile).
ia2p_status ia2p_conv3x3_gn(void* stream, const ia2p_conv_gn* d, int* gn_out_rows) {
  if (gn_out_rows) *gn_out_rows = 0;
  if (!d || !d->x0 || !d->Wp || !d->y || (d->splitk > 1 && !d->partial) || (d->Ca > 0 && !d->xa)) return fail(nullptr, IA2P_ERR_INVALID, "conv3x3_gn: null argument");
  const int Cin = d->C0 + (d->st0 ? d->C1 : 0), HW = d->H * d->W;
  if (Cin % 64 || d->C0 % 64 || d->Co % 8 || d->Ca % 64 || d->B < 1 || HW < 1 || d->splitk < 0 || d->splitk > (9 * Cin + d->Ca) / 64 || d->splitk > 255) return fail(nullptr, IA2P_ERR_SHAPE, "conv3x3_gn: C0=%d C1=%d Co=%d Ca=%d splitk=%d", d->C0, d->C1, d->Co, d->Ca, d->splitk);
  GemmArgs a = conv3_desc(zero_page(), (const half_t*)d->x0, d->B, d->H, d->W, Cin, (const half_t*)d->Wp, (const half_t*)d->bias, d->Co, 1, 0, 1, (const half_t*)d->rowvec, d->Co, (const half_t*)d->residual, (half_t*)d->y,
                          d->Ca > 0 ? (const half_t*)d->xa : nullptr, d->Ca > 0 ? d->Ca : 0);
  a.lda = d->C0;
  if (d->splitk > 1) { a.splitk = d->splitk; a.partial = d->partial; }
  const GemmPlan pl = ia2p_gemm_plan(a.M, a.N, a.K, true, false);
  if (d->st0) {
    const ia2p_status st = gn_in_from_abi("conv3x3_gn", &a.gn, d->C0, d->st0, d->rows0, d->C1, d->st1, d->rows1, d->gamma, d->beta, d->groups, d->eps, 1, HW);
    if (st != IA2P_OK) return st;
    a.A1b = d->C1 > 0 ? (const half_t*)d->x1 : nullptr; a.lda1b = d->C1;
    if (d->C1 > 0 && !d->x1) return fail(nullptr, IA2P_ERR_INVALID, "conv3x3_gn: null second source");
    if (!ia2p_conv_gn_fusable(a, pl.variant, a.splitk) || !ia2p_conv_gn_ok(a)) return fail(nullptr, IA2P_ERR_SHAPE, "conv3x3_gn: this site has no halo-staged plan (variant %d) or its statistics do not fit the fused kernel", pl.variant);
  }
  const bool combined = a.splitk > 1 && ia2p_splitk_inkernel(a.M, a.N, a.splitk);
  int rows = 0;
  if (d->gn_out) { rows = gn_epilogue_rows(a, true, pl.variant, a.splitk, combined, HW); if (rows) a.gn_out = d->gn_out; }
  int comb = 0;
  hipError_t e = ia2p_launch_gemm_variant(a, true, pl.variant, (hipStream_t)stream, true, &comb);
  if (e == hipSuccess && gn_out_rows) *gn_out_rows = (rows && (a.splitk <= 1 || comb)) ? rows : 0;
  RET_HIP(e, "conv3x3_gn");
}
// C = A . W^T + bias + residual as ia2p_gemm_splitk (splitk <= 1: no split), also leaving the GroupNorm column sums of C for images of HW rows (a Transformer2DModel's
// proj_out in front of the next ResnetBlock2D); *rows: rows per slot, 0 when the tile the plan picked cannot take them (the caller runs ia2p_gn_colstats)
ia2p_status ia2p_gemm_gnstats(void* stream, const void* A, const void* W, const void* bias, const void* residual, void* C, int M, int N, int K, int splitk, float* partial,
                              int HW, double* gn_out, int* rows) {
  if (rows) *rows = 0;
  if (!A || !W || !C || !gn_out || !rows || (splitk > 1 && !partial)) return fail(nullptr, IA2P_ERR_INVALID, "gemm_gnstats: null argument");
  if (K % 64 || N % 8 || HW < 16 || M % HW || splitk < 0 || splitk > K / 64 || splitk > 255) return fail(nullptr, IA2P_ERR_SHAPE, "gemm_gnstats: K=%d N=%d HW=%d splitk=%d", K, N, HW, splitk);
  GemmArgs a = gemm_desc(zero_page(), (const half_t*)A, K, (const half_t*)W, K, (const half_t*)bias, (const half_t*)residual, N, (half_t*)C, N, M, N, K);
  if (splitk > 1) { a.splitk = splitk; a.partial = partial; }
  const GemmPlan pl = ia2p_gemm_plan(M, N, K, false, false);
  const bool combined = splitk > 1 && ia2p_splitk_inkernel(M, N, splitk);
  const int r = gn_epilogue_rows(a, false, pl.variant, a.splitk, combined, HW);
  if (r) a.gn_out = gn_out;
  int comb = 0;
  hipError_t e = ia2p_launch_gemm_variant(a, false, pl.variant, (hipStream_t)stream, true, &comb);
  if (e == hipSuccess) *rows = (r && (a.splitk <= 1 || comb)) ? r : 0;
  RET_HIP(e, "gemm_gnstats");
}
// ResnetBlock2D tail as one implicit GEMM: y = conv3x3(x, W2) + conv1x1(x2, Wsc) + bias (+ rowvec), K = 9 Cin + Cin2; Wcat rows = [packed W2 row | Wsc row]
ia2p_status ia2p_conv3x3_cat(void* stream, const void* x, const void* x2, const void* Wcat, const void* bias, void* y, int B, int Hs, int Ws, int Cin, int Cin2, int Co) {
  if (!x || !x2 || !Wcat || !y) return fail(nullptr, IA2P_ERR_INVALID, "conv3x3_cat: null argument");
  if (Cin % 64 || Cin2 % 64 || Cin2 < 64 || Co % 4) return fail(nullptr, IA2P_ERR_SHAPE, "conv3x3_cat: Cin=%d, Cin2=%d (multiples of 64) Co=%d (mult of 4)", Cin, Cin2, Co);
  const GemmArgs a = conv3_desc(zero_page(), (const half_t*)x, B, Hs, Ws, Cin, (const half_t*)Wcat, (const half_t*)bias, Co, 1, 0, 1, nullptr, 0, nullptr, (half_t*)y, (const half_t*)x2, Cin2);
  hipError_t e = ia2p_launch_gemm(a, true, (hipStream_t)stream, nullptr);
  RET_HIP(e, "conv3x3_cat");
}
ia2p_status ia2p_pack_conv3x3(void* stream, const void* src, void* dst, int Co, int Cin) {
  if (!src || !dst) return fail(nullptr, IA2P_ERR_INVALID, "pack_conv3x3: null argument");
  if (Cin % 64) return fail(nullptr, IA2P_ERR_SHAPE, "pack_conv3x3: Cin=%d must be a multiple of 64 (the layout of ia2p_conv3x3; ia2p_pack_conv_out packs for ia2p_conv_out)", Cin);
  hipError_t e = ia2p_launch_pack_conv((const half_t*)src, (half_t*)dst, Co, Cin, (hipStream_t)stream);
  RET_HIP(e, "pack_conv3x3");
}
ia2p_status ia2p_pack_conv_out(void* stream, const void* src, void* dst, int Co, int C) {
  if (!src || !dst) return fail(nullptr, IA2P_ERR_INVALID, "pack_conv_out: null argument");
  hipError_t e = ia2p_launch_pack_conv((const half_t*)src, (half_t*)dst, Co, C, (hipStream_t)stream);
  RET_HIP(e, "pack_conv_out");
}
// latent-boundary convolutions as operators (the executors call the launchers directly): conv_in reads NCHW and writes channels-last,
// conv_out reads channels-last and writes NCHW; reference call sites: the diffusers UNet's conv_in / conv_out behind pnp_pipeline.py:253-260
ia2p_status ia2p_conv_in(void* stream, const void* x_nchw, const void* w_oihw, const void* bias, void* y_nhwc, void* w_scratch, int B, int Cin, int H, int W, int Co) {
  if (!x_nchw || !w_oihw || !bias || !y_nhwc || !w_scratch) return fail(nullptr, IA2P_ERR_INVALID, "conv_in: null argument");
  if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cin * 9 > 64 || Co < 8 || Co % 8) return fail(nullptr, IA2P_ERR_SHAPE, "conv_in: Cin*9=%d must be <= 64, Co=%d a multiple of 8", Cin * 9, Co);
  hipError_t e = ia2p_launch_pack_conv_in((const half_t*)w_oihw, (half_t*)w_scratch, Co, Cin * 9, (hipStream_t)stream);
  if (e == hipSuccess) e = ia2p_launch_conv_in((const half_t*)x_nchw, (const half_t*)w_scratch, (const half_t*)bias, (half_t*)y_nhwc, B, Cin, H, W, Co, (hipStream_t)stream);
  RET_HIP(e, "conv_in");
}
// ---- the ControlNet path's operators (controlnet.hip; diffusers ControlNetModel: ControlNetConditioningEmbedding, controlnet_down_blocks / controlnet_mid_block, and the
//      `sample + residual` of UNet2DConditionModel.forward). Every refusal comes before any launch.
ia2p_status ia2p_conv_in_act(void* stream, const void* x_nchw, const void* w_oihw, const void* bias, void* y_nhwc, void* w_scratch, int B, int Cin, int H, int W, int Co, int silu) {
  if (!x_nchw || !w_oihw || !bias || !y_nhwc || !w_scratch) return fail(nullptr, IA2P_ERR_INVALID, "conv_in_act: null argument");
  if (silu != 0 && silu != 1) return fail(nullptr, IA2P_ERR_INVALID, "conv_in_act: silu=%d (0 or 1)", silu);
  if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cin * 9 > 64 || Co < 8 || Co % 8) return fail(nullptr, IA2P_ERR_SHAPE, "conv_in_act: Cin*9=%d must be <= 64, Co=%d a multiple of 8", Cin * 9, Co);
  hipError_t e = ia2p_launch_pack_conv_in((const half_t*)w_oihw, (half_t*)w_scratch, Co, Cin * 9, (hipStream_t)stream);
  if (e == hipSuccess) e = ia2p_launch_conv_in((const half_t*)x_nchw, (const half_t*)w_scratch, (const half_t*)bias, (half_t*)y_nhwc, B, Cin, H, W, Co, (hipStream_t)stream, 1.0f, silu);
  RET_HIP(e, "conv_in_act");
}
ia2p_status ia2p_conv3x3_narrow(void* stream, const void* x, const void* Wp, const void* bias, void* y, int B, int H, int W, int Cin, int Co, int stride, int silu) {
  if (!x || !Wp || !bias || !y) return fail(nullptr, IA2P_ERR_INVALID, "conv3x3_narrow: null argument");
  if (silu != 0 && silu != 1) return fail(nullptr, IA2P_ERR_INVALID, "conv3x3_narrow: silu=%d (0 or 1)", silu);
  if (B < 1 || H < 1 || W < 1 || Cin < 16 || Cin > 256 || Cin % 16 || Co < 16 || Co % 16 || (stride != 1 && stride != 2))
    return fail(nullptr, IA2P_ERR_SHAPE, "conv3x3_narrow: Cin=%d (multiple of 16, 16 .. 256) Co=%d (multiple of 16) stride=%d (1 or 2)", Cin, Co, stride);
  if ((int64_t)B * H * W > INT32_MAX - 64) return fail(nullptr, IA2P_ERR_SHAPE, "conv3x3_narrow: %lld pixels exceed the 32-bit count of one launch", (long long)B * H * W);
  hipError_t e = ia2p_launch_conv3x3_narrow((const half_t*)x, (const half_t*)Wp, (const half_t*)bias, (half_t*)y, B, H, W, Cin, Co, stride, silu, (hipStream_t)stream);
  RET_HIP(e, "conv3x3_narrow");
}
// C[m, :] = fp16(scales[m / HW] * fp16(A . W^T + bias)): a zero convolution (1x1) with its image's conditioning scale in the epilogue; no K split
ia2p_status ia2p_gemm_rowscale(void* stream, const void* A, const void* W, const void* bias, const float* scales, void* C, int M, int N, int K, int HW) {
  if (!A || !W || !C || !scales) return fail(nullptr, IA2P_ERR_INVALID, "gemm_rowscale: null argument");
  if (((uintptr_t)scales) & 3) return fail(nullptr, IA2P_ERR_INVALID, "gemm_rowscale: scales must be 4-byte aligned");
  if (M < 1 || K < 64 || K % 64 || N < 4 || N % 4 || HW < 1 || M % HW) return fail(nullptr, IA2P_ERR_SHAPE, "gemm_rowscale: K=%d must be a multiple of 64, N=%d of 4, HW=%d must divide M=%d", K, N, HW, M);
  GemmArgs a = gemm_desc(zero_page(), (const half_t*)A, K, (const half_t*)W, K, (const half_t*)bias, nullptr, 0, (half_t*)C, N, M, N, K);
  a.act = 4; a.rscale = scales; a.rows_per_batch = HW;
  hipError_t e = ia2p_launch_gemm_variant(a, false, ia2p_gemm_plan(M, N, K, false, false).variant, (hipStream_t)stream);
  RET_HIP(e, "gemm_rowscale");
}
// y = fp16(x + r) over [M, C] (y may alias x); gn_out != NULL: also the GroupNorm column sums of y, [M / rows][C][2] fp64, to the bit what ia2p_gn_colstats(y) returns
ia2p_status ia2p_residual_add_gnstats(void* stream, const void* x, const void* r, void* y, int M, int C, int rows, double* gn_out) {
  if (!x || !r || !y) return fail(nullptr, IA2P_ERR_INVALID, "residual_add_gnstats: null argument");
  if ((((uintptr_t)x) | ((uintptr_t)r) | ((uintptr_t)y)) & 15) return fail(nullptr, IA2P_ERR_INVALID, "residual_add_gnstats: tensors must be 16-byte aligned");
  if (M < 1 || C < 8 || C % 8 || (int64_t)M * C > INT32_MAX) return fail(nullptr, IA2P_ERR_SHAPE, "residual_add_gnstats: M=%d C=%d (C a multiple of 8, M C below 2^31)", M, C);
  if (gn_out && (rows < 16 || rows % 16 || M % rows)) return fail(nullptr, IA2P_ERR_SHAPE, "residual_add_gnstats: rows=%d (multiple of 16 dividing M=%d)", rows, M);
  hipError_t e = ia2p_launch_residual_add_gnstats((const half_t*)x, (const half_t*)r, (half_t*)y, M, C, rows, gn_out, (hipStream_t)stream);
  RET_HIP(e, "residual_add_gnstats");
}
ia2p_status ia2p_conv_out(void* stream, const void* x_nhwc, const void* w_packed, const void* bias, void* y_nchw, int B, int C, int H, int W, int Co) {
  if (!x_nhwc || !w_packed || !bias || !y_nchw) return fail(nullptr, IA2P_ERR_INVALID, "conv_out: null argument");
  if (B < 1 || H < 1 || W < 1 || C < 32 || C % 32 || Co < 1 || Co > 8) return fail(nullptr, IA2P_ERR_SHAPE, "conv_out: C=%d must be a multiple of 32, Co=%d <= 8", C, Co);
  hipError_t e = ia2p_launch_conv_out((const half_t*)x_nhwc, C, (const half_t*)w_packed, (const half_t*)bias, (half_t*)y_nchw, B, C, H, W, Co, (hipStream_t)stream);
  RET_HIP(e, "conv_out");
}
ia2p_status ia2p_pack_geglu(void* stream, const void* src, void* dst, int rows, int rowlen) {
  if (!src || !dst || rows % 32) return fail(nullptr, IA2P_ERR_SHAPE, "pack_geglu: rows must be a multiple of 32");
  hipError_t e = ia2p_launch_pack_geglu((const half_t*)src, (half_t*)dst, rows, rowlen, (hipStream_t)stream);
  RET_HIP(e, "pack_geglu");
}
ia2p_status ia2p_attention(void* stream, const void* Q, int ldq, void* O, int ldo, int B, int heads, int Nq, int nseg,
                           const void* K0, const void* V0, int ld0, int nkeys0, float w0, const void* K1, const void* V1, int ld1, int nkeys1, float w1) {
  if (!Q || !O || !K0 || !V0 || nseg < 1 || nseg > 2 || (nseg == 2 && (!K1 || !V1))) return fail(nullptr, IA2P_ERR_INVALID, "attention: bad argument");
  if (nkeys0 < 1 || (nseg == 2 && nkeys1 < 1) || ldq % 8 || ldo % 8 || (((uintptr_t)O) & 15) || ld0 % 8 || (nseg == 2 && ld1 % 8)) return fail(nullptr, IA2P_ERR_SHAPE, "attention: key counts must be >= 1, strides multiples of 8, O 16-byte aligned");
  const AttnArgs a = attn_desc((const half_t*)Q, ldq, (half_t*)O, ldo, B, heads, Nq, nseg, AttnSeg{(const half_t*)K0, (const half_t*)V0, nkeys0, ld0, nkeys0, w0},
                               AttnSeg{(const half_t*)K1, (const half_t*)V1, nkeys1, ld1, nkeys1, w1});
  hipError_t e = ia2p_launch_attention(a, (hipStream_t)stream);
  RET_HIP(e, "attention");
}
// Regional image prompts (diffusers' `ip_adapter_masks`): segment 1 is G groups of four image-token keys, each with its own softmax and its own per-query weight.
// Every refusal comes before any HIP call.
ia2p_status ia2p_attention_regions(void* stream, const void* Q, int ldq, void* O, int ldo, int B, int heads, int Nq, int nseg,
                                   const void* K0, const void* V0, int ld0, int nkeys0, float w0, const void* K1, const void* V1, int ld1, int nkeys1, float w1,
                                   const void* region_w, int G, const float* w1_b) {
  if (!Q || !O || !K0 || !V0 || !K1 || !V1 || !region_w) return fail(nullptr, IA2P_ERR_INVALID, "attention_regions: null pointer");
  if (nseg != 2) return fail(nullptr, IA2P_ERR_INVALID, "attention_regions: nseg=%d (text keys and image-token keys: 2)", nseg);
  if (w0 == 0.f) return fail(nullptr, IA2P_ERR_INVALID, "attention_regions: w0 == 0 (the merged accumulator divides by it)");
  if (G < 1 || G > 16 || nkeys1 != 4 * G) return fail(nullptr, IA2P_ERR_SHAPE, "attention_regions: G=%d (1 .. 16), nkeys1=%d must be 4 G", G, nkeys1);
  if (ldq % 8 || ldo % 8 || ld0 % 8 || ld1 % 8) return fail(nullptr, IA2P_ERR_SHAPE, "attention_regions: strides ldq=%d ldo=%d ld0=%d ld1=%d must be multiples of 8", ldq, ldo, ld0, ld1);
  if (B < 1 || heads < 1 || Nq < 1 || nkeys0 < 1 || (((uintptr_t)O) & 15) || (((uintptr_t)region_w) & 1))
    return fail(nullptr, IA2P_ERR_SHAPE, "attention_regions: B=%d heads=%d Nq=%d nkeys0=%d must be >= 1, O 16-byte aligned", B, heads, Nq, nkeys0);
  if ((int64_t)((Nq + 127) / 128) * heads * B > INT32_MAX) return fail(nullptr, IA2P_ERR_SHAPE, "attention_regions: too many workgroups for one launch");
  AttnArgs a = attn_desc((const half_t*)Q, ldq, (half_t*)O, ldo, B, heads, Nq, 2, AttnSeg{(const half_t*)K0, (const half_t*)V0, nkeys0, ld0, nkeys0, w0},
                         AttnSeg{(const half_t*)K1, (const half_t*)V1, nkeys1, ld1, nkeys1, w1});
  a.w1_b = w1_b;
  hipError_t e = ia2p_launch_attention_regions(a, (const half_t*)region_w, G, (hipStream_t)stream);
  RET_HIP(e, "attention_regions");
}
// masks [B, G, h, w] on the latent grid -> [B, G, (h / f) (w / f)]: the mean of each f x f block (fp32 sum in row-major order, rounded once)
ia2p_status ia2p_region_levels(void* stream, const void* masks, void* out, int B, int G, int h, int w, int f) {
  if (!masks || !out) return fail(nullptr, IA2P_ERR_INVALID, "region_levels: null pointer");
  if (f != 1 && f != 2 && f != 4 && f != 8) return fail(nullptr, IA2P_ERR_INVALID, "region_levels: f=%d (1, 2, 4 or 8)", f);
  if (B < 1 || G < 1 || h < 1 || w < 1 || h % f || w % f) return fail(nullptr, IA2P_ERR_SHAPE, "region_levels: B=%d G=%d h=%d w=%d must be >= 1, h and w multiples of f=%d", B, G, h, w, f);
  if ((int64_t)B * G * h * w > INT32_MAX) return fail(nullptr, IA2P_ERR_SHAPE, "region_levels: %lld elements exceed the 32-bit count of one launch", (long long)B * G * h * w);
  hipError_t e = ia2p_launch_region_levels((const half_t*)masks, (half_t*)out, B, G, h, w, f, (hipStream_t)stream);
  RET_HIP(e, "region_levels");
}
ia2p_status ia2p_qproj_attention(void* stream, const void* X, const void* Wq, const void* bias, const ia2p_ln_fold* ln, void* O, int ldo, int B, int heads,
                                 int Nq, int K, int nseg, const void* K0, const void* V0, int ld0, int nkeys0, float w0,
                                 const void* K1, const void* V1, int ld1, int nkeys1, float w1) {
  if (!X || !Wq || !O || !K0 || !V0 || nseg < 1 || nseg > 2 || (nseg == 2 && (!K1 || !V1))) return fail(nullptr, IA2P_ERR_INVALID, "qproj_attention: bad argument");
  if (!ln_fold_ok(ln)) return fail(nullptr, IA2P_ERR_INVALID, "qproj_attention: incomplete ia2p_ln_fold");
  if (B < 1 || heads < 1 || Nq < 128 || Nq % 128 || K < 64 || K % 64 || nkeys0 < 1 || (nseg == 2 && nkeys1 < 1) || ldo % 8 || (((uintptr_t)O) & 15) || ld0 % 8 || (nseg == 2 && ld1 % 8))
    return fail(nullptr, IA2P_ERR_SHAPE, "qproj_attention: Nq=%d must be a multiple of 128, K=%d of 64, key counts >= 1, strides multiples of 8, O 16-byte aligned", Nq, K);
  GemmArgs a = gemm_desc(zero_page(), (const half_t*)X, K, (const half_t*)Wq, K, (const half_t*)bias, nullptr, 0, nullptr, heads * 64, B * Nq, heads * 64, K);
  ln_attach(a, ln);
  const AttnArgs x = attn_desc(nullptr, 0, (half_t*)O, ldo, B, heads, Nq, nseg, AttnSeg{(const half_t*)K0, (const half_t*)V0, nkeys0, ld0, nkeys0, w0},
                               AttnSeg{(const half_t*)K1, (const half_t*)V1, nkeys1, ld1, nkeys1, w1});
  if (!ia2p_qproj_xattn_ok(a, x)) return fail(nullptr, IA2P_ERR_SHAPE, "qproj_attention: shape not supported by the fused tile (bias must be 16-byte aligned)");
  hipError_t e = ia2p_launch_qproj_xattn(a, x, (hipStream_t)stream);
  RET_HIP(e, "qproj_attention");
}
ia2p_status ia2p_qkv_self_attention(void* stream, const void* X, const void* Wqkv, const void* bias, const ia2p_ln_fold* ln, void* O, int ldo, int B, int heads, int K) {
  if (!X || !Wqkv || !O) return fail(nullptr, IA2P_ERR_INVALID, "qkv_self_attention: null argument");
  if (!ln_fold_ok(ln)) return fail(nullptr, IA2P_ERR_INVALID, "qkv_self_attention: incomplete ia2p_ln_fold");
  if (B < 1 || heads < 1 || K < 64 || K % 64 || ldo % 8 || (((uintptr_t)O) & 15)) return fail(nullptr, IA2P_ERR_SHAPE, "qkv_self_attention: K=%d (multiple of 64), ldo=%d (multiple of 8), O 16-byte aligned", K, ldo);
  GemmArgs a = qkv_desc(zero_page(), (const half_t*)X, K, (const half_t*)Wqkv, (const half_t*)bias, B * 256, 3 * heads * 64, K);
  ln_attach(a, ln);
  const AttnArgs x = sattn_desc((half_t*)O, ldo, B, heads, 256);
  if (!ia2p_qkv_sattn_ok(a, x)) return fail(nullptr, IA2P_ERR_SHAPE, "qkv_self_attention: shape / alignment not supported by the fused tile");
  hipError_t e = ia2p_launch_qkv_sattn(a, x, (hipStream_t)stream);
  RET_HIP(e, "qkv_self_attention");
}
// The same launch with the layer's slice of the context K/V projection riding on the CUs the (image, head) tiles leave empty (what the executor does per step for every
// block that takes the fused launch; reference attention_processor.py:358-359 to_k / to_v on the text rows, :379-380 to_k_ip / to_v_ip on the image-token rows).
// *in_launch (optional) = 1 when the slice ran inside the launch, 0 when fused tiles + context tiles exceed the device's compute units and the two projections ran as
// launches of their own in front of it (the executor's route for such a block). Same bits either way.
ia2p_status ia2p_qkv_self_attention_ctx(void* stream, const void* X, const void* Wqkv, const void* bias, const ia2p_ln_fold* ln, void* O, int ldo, int B, int heads, int K,
                                        const void* context, int L, int Li, int ctx_dim, const void* Wkv_text, const void* Wkv_ip, void* kv_text, void* kv_ip, int ldkv, int N,
                                        int* in_launch) {
  if (!X || !Wqkv || !O || !context || !Wkv_text || !kv_text || (Li > 0 && (!Wkv_ip || !kv_ip))) return fail(nullptr, IA2P_ERR_INVALID, "qkv_self_attention_ctx: null argument");
  if (!ln_fold_ok(ln)) return fail(nullptr, IA2P_ERR_INVALID, "qkv_self_attention_ctx: incomplete ia2p_ln_fold");
  if (B < 1 || heads < 1 || K < 64 || K % 64 || ldo % 8 || (((uintptr_t)O) & 15)) return fail(nullptr, IA2P_ERR_SHAPE, "qkv_self_attention_ctx: K=%d (multiple of 64), ldo=%d (multiple of 8), O 16-byte aligned", K, ldo);
  if (Li < 0 || L <= Li || L > 0xffff || ctx_dim < 64 || ctx_dim % 64 || N < 8 || N % 8 || ldkv < N || ldkv % 8 || (((uintptr_t)kv_text) & 15) || (Li > 0 && (((uintptr_t)kv_ip) & 15)))
    return fail(nullptr, IA2P_ERR_SHAPE, "qkv_self_attention_ctx: L=%d > Li=%d >= 0, ctx_dim=%d (multiple of 64), N=%d and ldkv=%d (multiples of 8, ldkv >= N), outputs 16-byte aligned", L, Li, ctx_dim, N, ldkv);
  if (!zero_page()) return fail(nullptr, IA2P_ERR_HIP, "cannot allocate zero page");
  GemmArgs a = qkv_desc(zero_page(), (const half_t*)X, K, (const half_t*)Wqkv, (const half_t*)bias, B * 256, 3 * heads * 64, K);
  ln_attach(a, ln);
  const AttnArgs x = sattn_desc((half_t*)O, ldo, B, heads, 256);
  if (!ia2p_qkv_sattn_ok(a, x)) return fail(nullptr, IA2P_ERR_SHAPE, "qkv_self_attention_ctx: shape / alignment not supported by the fused tile");
  const int Lt = L - Li;
  CtxKvSlice k;
  memset(&k, 0, sizeof k);
  k.ctx = (const half_t*)context; k.lda = ctx_dim; k.L = L; k.Lt = Lt; k.Li = Li; k.B = B; k.Wt = (const half_t*)Wkv_text; k.Wi = (const half_t*)Wkv_ip;
  k.Ct = (half_t*)kv_text; k.Ci = (half_t*)kv_ip; k.ldc = ldkv; k.N = N; k.K = ctx_dim;
  const bool inl = ia2p_qkv_sattn_ctx_ok(x, k);
  if (in_launch) *in_launch = inl ? 1 : 0;
  hipError_t e = hipSuccess;
  if (!inl) {      // the two projections as launches of their own (project_context's, for this slice)
    for (int seg = 0; seg < (Li > 0 ? 2 : 1) && e == hipSuccess; ++seg) {
      const GemmArgs g = gemm_desc(zero_page(), k.ctx, ctx_dim, seg ? k.Wi : k.Wt, ctx_dim, nullptr, nullptr, 0, seg ? k.Ci : k.Ct, ldkv, B * (seg ? Li : Lt), N, ctx_dim, 0, seg ? Li : Lt, L, seg ? Lt : 0);
      e = ia2p_launch_gemm_variant(g, false, ia2p_gemm_plan(g.M, g.N, g.K, false, false).variant, (hipStream_t)stream);
    }
  }
  if (e == hipSuccess) e = ia2p_launch_qkv_sattn(a, x, (hipStream_t)stream, inl ? &k : nullptr);
  RET_HIP(e, "qkv_self_attention_ctx");
}
ia2p_status ia2p_ip_attn_map(void* stream, const void* Q, int ldq, const void* Kip, int ldk, void* out, int B, int heads, int Nq, int ntok) {
  if (!Q || !Kip || !out || B < 1 || heads < 1 || Nq < 1) return fail(nullptr, IA2P_ERR_INVALID, "ip_attn_map: bad argument");
  if (ntok < 1 || ntok > 16 || ldq % 8 || ldq < heads * 64 || ldk < heads * 64) return fail(nullptr, IA2P_ERR_SHAPE, "ip_attn_map: ntok=%d (1..16), ldq=%d (mult of 8), ldk=%d", ntok, ldq, ldk);
  hipError_t e = ia2p_launch_ip_attn_map((const half_t*)Q, ldq, (const half_t*)Kip, ldk, (half_t*)out, B, heads, Nq, ntok, (hipStream_t)stream);
  RET_HIP(e, "ip_attn_map");
}
ia2p_status ia2p_linear_small(void* stream, const void* X, const void* W, const void* bias, void* out, int M, int N, int K, int silu_in, int silu_out) {
  if (!X || !W || !out) return fail(nullptr, IA2P_ERR_INVALID, "linear_small: null argument");
  if (M > 16 || K % 8) return fail(nullptr, IA2P_ERR_SHAPE, "linear_small: M=%d (<=16) K=%d (mult of 8)", M, K);
  hipError_t e = ia2p_launch_linear_small((const half_t*)X, K, (const half_t*)W, (const half_t*)bias, nullptr, 0, (half_t*)out, N, M, N, K, silu_in, silu_out, (hipStream_t)stream);
  RET_HIP(e, "linear_small");
}
ia2p_status ia2p_attention_full(void* stream, const void* qkv, void* out, const void* bias_k, const void* bias_v, int B, int T, int heads, int D) {
  if (!qkv || !out || B < 1 || T < 1 || heads < 1 || (!bias_k) != (!bias_v)) return fail(nullptr, IA2P_ERR_INVALID, "attention_full: bad argument");
  if ((D != 64 && D != 80) || T + (bias_k ? 1 : 0) > ia2p_full_attention_max_keys() || (size_t)B * heads > 65535)
    return fail(nullptr, IA2P_ERR_SHAPE, "attention_full: D=%d (64 or 80), %d keys (<= %d)", D, T + (bias_k ? 1 : 0), ia2p_full_attention_max_keys());
  hipError_t e = ia2p_launch_full_attention((const half_t*)qkv, (half_t*)out, (const half_t*)bias_k, (const half_t*)bias_v, B, T, heads, D, (hipStream_t)stream);
  RET_HIP(e, "attention_full");
}

// ---- the small launches around the UNet, one by one (tests/test_encoder_ops_gpu.py): CLIP text / prior stem and pooling, VAE softmax and 1x1 convolution, ViT stem and
//      head projection, the UNet's embeddings, channel concat and weight-row concat. Every refusal is decided here, before a launch: what the kernels assume
//      (head dim 64, even sinusoid widths, 16-byte rows, a gamma with its beta) the launchers do not all check.
ia2p_status ia2p_clip_embed(void* stream, const int32_t* ids, const void* tok, const void* embeds, const void* pos, void* x, float* stats, int rows, int T, int H, int vocab) {
  if (!pos || !x || !stats || (!embeds && (!ids || !tok))) return fail(nullptr, IA2P_ERR_INVALID, "clip_embed: null argument (embeds, or ids with the token table)");
  if (rows < 1 || T < 1 || H < 8 || H % 8 || (!embeds && vocab < 1)) return fail(nullptr, IA2P_ERR_SHAPE, "clip_embed: rows=%d T=%d H=%d (multiple of 8) vocab=%d", rows, T, H, vocab);
  hipError_t e = ia2p_launch_clip_embed((const int*)ids, (const half_t*)tok, (const half_t*)embeds, (const half_t*)pos, (half_t*)x, stats, rows, T, H, vocab, (hipStream_t)stream);
  RET_HIP(e, "clip_embed");
}
ia2p_status ia2p_causal_attention_small(void* stream, const void* qkv, void* out, int B, int T, int heads, int D) {
  if (!qkv || !out) return fail(nullptr, IA2P_ERR_INVALID, "causal_attention_small: null argument");
  if (B < 1 || heads < 1 || T < 1 || T > 128 || D != 64 || (size_t)B * heads > 0x7fffffff) return fail(nullptr, IA2P_ERR_SHAPE, "causal_attention_small: B=%d heads=%d T=%d (1..128) D=%d (64)", B, heads, T, D);
  hipError_t e = ia2p_launch_causal_attention_small((const half_t*)qkv, (half_t*)out, B, T, heads, (hipStream_t)stream);
  RET_HIP(e, "causal_attention_small");
}
ia2p_status ia2p_clip_pool(void* stream, const int32_t* ids, const void* x, const void* gamma, const void* beta, void* out, int B, int T, int H, int eos_id, float eps) {
  if (!ids || !x || !gamma || !beta || !out || !(eps >= 0.f)) return fail(nullptr, IA2P_ERR_INVALID, "clip_pool: null argument or negative eps");
  if (B < 1 || T < 1 || H < 1) return fail(nullptr, IA2P_ERR_SHAPE, "clip_pool: B=%d T=%d H=%d", B, T, H);
  hipError_t e = ia2p_launch_clip_pool((const int*)ids, (const half_t*)x, (const half_t*)gamma, (const half_t*)beta, (half_t*)out, B, T, H, eos_id, eps, (hipStream_t)stream);
  RET_HIP(e, "clip_pool");
}
ia2p_status ia2p_softmax_rows(void* stream, void* x, int64_t ld, int rows, int n, float scale) {
  if (!x) return fail(nullptr, IA2P_ERR_INVALID, "softmax_rows: null argument");
  if (rows < 1 || n < 8 || n % 8 || n > 8 * 256 * 8 || ld < n || ld % 8) return fail(nullptr, IA2P_ERR_SHAPE, "softmax_rows: rows=%d n=%d (multiple of 8, <= 16384) ld=%lld (multiple of 8, >= n)", rows, n, (long long)ld);
  hipError_t e = ia2p_launch_softmax_rows((half_t*)x, (long)ld, rows, n, scale, (hipStream_t)stream);
  RET_HIP(e, "softmax_rows");
}
ia2p_status ia2p_conv1x1_nchw(void* stream, const void* x, const void* w, const void* bias, void* y, int B, int Ci, int Co, int64_t HW) {
  if (!x || !w || !bias || !y) return fail(nullptr, IA2P_ERR_INVALID, "conv1x1_nchw: null argument");
  if (B < 1 || Ci < 1 || Ci > 8 || Co < 1 || Co > 8 || HW < 1) return fail(nullptr, IA2P_ERR_SHAPE, "conv1x1_nchw: B=%d Ci=%d Co=%d (1..8) HW=%lld", B, Ci, Co, (long long)HW);
  hipError_t e = ia2p_launch_conv1x1_nchw((const half_t*)x, (const half_t*)w, (const half_t*)bias, (half_t*)y, B, Ci, Co, (long)HW, (hipStream_t)stream);
  RET_HIP(e, "conv1x1_nchw");
}
ia2p_status ia2p_patch_gather(void* stream, const void* px, void* cols, int B, int C, int Hi, int Wi, int ps, int stride, int gh, int gw, int Kpad) {
  if (!px || !cols) return fail(nullptr, IA2P_ERR_INVALID, "patch_gather: null argument");
  if (B < 1 || C < 1 || ps < 1 || stride < 1 || gh < 1 || gw < 1 || (long)(gh - 1) * stride + ps > Hi || (long)(gw - 1) * stride + ps > Wi || (long)Kpad < (long)C * ps * ps || (long)B * gh * gw > 0x7fffffffL)
    return fail(nullptr, IA2P_ERR_SHAPE, "patch_gather: a %d x %d grid of %d-pixel patches at stride %d does not fit %d x %d, or Kpad=%d < C ps ps", gh, gw, ps, stride, Hi, Wi, Kpad);
  hipError_t e = ia2p_launch_patch_gather((const half_t*)px, (half_t*)cols, B, C, Hi, Wi, ps, stride, gh, gw, Kpad, (hipStream_t)stream);
  RET_HIP(e, "patch_gather");
}
ia2p_status ia2p_vit_embed(void* stream, const void* patches, const void* cls, const void* pos, const void* stem_g, const void* stem_b, const void* pre_g, const void* pre_b,
                           void* x, float* stats, int B, int T, int H, float eps) {
  if (!patches || !cls || !pos || !x || !stats || (!stem_g) != (!stem_b) || (!pre_g) != (!pre_b) || !(eps >= 0.f)) return fail(nullptr, IA2P_ERR_INVALID, "vit_embed: null argument, a gamma without its beta, or negative eps");
  if (B < 1 || T < 2 || H < 64 || H % 64 || H > 2048 || (long)B * T > 0x7fffffffL) return fail(nullptr, IA2P_ERR_SHAPE, "vit_embed: B=%d T=%d (>= 2) H=%d (multiple of 64, <= 2048)", B, T, H);
  hipError_t e = ia2p_launch_vit_embed((const half_t*)patches, (const half_t*)cls, (const half_t*)pos, (const half_t*)stem_g, (const half_t*)stem_b, (const half_t*)pre_g, (const half_t*)pre_b,
                                       (half_t*)x, stats, B, T, H, eps, (hipStream_t)stream);
  RET_HIP(e, "vit_embed");
}
ia2p_status ia2p_vit_project(void* stream, const void* X, const void* W, float* out, int B, int N, int K) {
  if (!X || !W || !out) return fail(nullptr, IA2P_ERR_INVALID, "vit_project: null argument");
  if (B < 1 || B > 65535 || N < 1 || K < 8 || K % 8) return fail(nullptr, IA2P_ERR_SHAPE, "vit_project: B=%d (1..65535) N=%d K=%d (multiple of 8)", B, N, K);
  hipError_t e = ia2p_launch_vit_project((const half_t*)X, (const half_t*)W, out, B, N, K, (hipStream_t)stream);
  RET_HIP(e, "vit_project");
}
// ts != NULL: one timestep per batch element (device, fp32 [B]) instead of the scalar t
ia2p_status ia2p_embed(void* stream, float t, const float* ts, const void* text_embeds, const void* time_ids, void* tsin, void* addin, int B, int Tp, int P, int Ad, int nids) {
  if (!tsin || !addin || (P > 0 && !text_embeds) || (nids > 0 && !time_ids)) return fail(nullptr, IA2P_ERR_INVALID, "embed: null argument");
  if (B < 1 || Tp < 2 || Tp % 2 || P < 0 || nids < 0 || (nids > 0 && (Ad < 2 || Ad % 2)) || (long)P + (long)nids * Ad > 0x7fffffffL)
    return fail(nullptr, IA2P_ERR_SHAPE, "embed: B=%d Tp=%d Ad=%d (even, >= 2) P=%d nids=%d", B, Tp, Ad, P, nids);
  hipError_t e = ia2p_launch_embed(t, ts, (const half_t*)text_embeds, (const half_t*)time_ids, (half_t*)tsin, (half_t*)addin, B, Tp, P, nids > 0 ? Ad : 0, nids, (hipStream_t)stream);
  RET_HIP(e, "embed");
}
ia2p_status ia2p_concat(void* stream, const void* a, int lda, int Ca, const void* b, int ldb, int Cb, void* y, int64_t M) {
  if (!a || !b || !y) return fail(nullptr, IA2P_ERR_INVALID, "concat: null argument");
  if (M < 1 || Ca < 8 || Ca % 8 || Cb < 8 || Cb % 8 || lda < Ca || lda % 8 || ldb < Cb || ldb % 8) return fail(nullptr, IA2P_ERR_SHAPE, "concat: Ca=%d Cb=%d lda=%d ldb=%d (multiples of 8, ld >= C) M=%lld", Ca, Cb, lda, ldb, (long long)M);
  hipError_t e = ia2p_launch_concat((const half_t*)a, lda, Ca, (const half_t*)b, ldb, Cb, (half_t*)y, (long)M, (hipStream_t)stream);
  RET_HIP(e, "concat");
}
ia2p_status ia2p_cat_rows(void* stream, const void* a, int Ka, const void* b, int Kb, const void* bias_a, const void* bias_b, void* dst, void* bias_dst, int rows) {
  if (!a || !b || !bias_a || !bias_b || !dst || !bias_dst) return fail(nullptr, IA2P_ERR_INVALID, "cat_rows: null argument");
  if (rows < 1 || Ka < 8 || Ka % 8 || Kb < 8 || Kb % 8) return fail(nullptr, IA2P_ERR_SHAPE, "cat_rows: Ka=%d Kb=%d (multiples of 8) rows=%d", Ka, Kb, rows);
  hipError_t e = ia2p_launch_cat_rows((const half_t*)a, Ka, (const half_t*)b, Kb, (const half_t*)bias_a, (const half_t*)bias_b, (half_t*)dst, (half_t*)bias_dst, rows, (hipStream_t)stream);
  RET_HIP(e, "cat_rows");
}

}  // extern "C"
