// ViT executor and its C ABI (ia2p_vit_*): see include/ia2p.h and DESIGN.md §11. Runtime and operator wrappers: engine_rt.h / engine_rt.hip; the block: xf_layer.h.
#include "xf_layer.h"

// =====================================================================================================================
// ImageBind's vision and audio towers (reference pipeline.py:118-121, :155-168 `imagebind_huge`): a patch stem (im2col gather + op_gemm), class token +
// position embeddings (+ the stem / pre-transformer LayerNorms) in one row pass, the pre-LayerNorm blocks of xf_layer.h with non-causal attention at
// head dim 64 / 80 (optionally one learned key / value row appended: add_bias_kv), LayerNorm of the class row and a bias-free projection in fp32.
// =====================================================================================================================
struct ia2p_vit : RunCtx {
  ia2p_vit_config cfg;
  int gh, gw, P, T, D, Kraw, Kpad;
  size_t stem, sng, snb, cls, pos, plg, plb, hng, hnb, wproj;
  std::vector<CLayer> layers;
  std::vector<size_t> bk, bv;
};

static ia2p_status vit_plan(ia2p_vit* c) {
  const ia2p_vit_config& g = c->cfg;
  const int H = g.hidden_size, I = g.intermediate_size;
  if (g.num_layers < 1 || g.num_heads < 1 || H < 64 || H % 64 || H > 2048 || I < 64 || I % 64 || g.out_dim < 1)
    return fail(c, IA2P_ERR_SHAPE, "vit: hidden %d must be a multiple of 64 (<= 2048), intermediate %d a multiple of 64", H, I);
  if (H % g.num_heads || (H / g.num_heads != 64 && H / g.num_heads != 80)) return fail(c, IA2P_ERR_SHAPE, "vit: head dim must be 64 or 80 (hidden %d, %d heads)", H, g.num_heads);
  if (g.in_channels < 1 || g.patch_size < 1 || g.patch_stride < 1 || g.patch_size > g.image_h || g.patch_size > g.image_w)
    return fail(c, IA2P_ERR_SHAPE, "vit: a %d x %d patch does not fit a %d x %d input", g.patch_size, g.patch_size, g.image_h, g.image_w);
  c->D = H / g.num_heads;
  c->gh = (g.image_h - g.patch_size) / g.patch_stride + 1; c->gw = (g.image_w - g.patch_size) / g.patch_stride + 1;
  c->P = c->gh * c->gw; c->T = c->P + 1;
  if (c->T + (g.bias_kv ? 1 : 0) > ia2p_full_attention_max_keys())
    return fail(c, IA2P_ERR_SHAPE, "vit: %d x %d patches + class token%s exceed the %d keys the attention launch holds", c->gh, c->gw, g.bias_kv ? " + bias row" : "", ia2p_full_attention_max_keys());
  c->Kraw = g.in_channels * g.patch_size * g.patch_size; c->Kpad = (c->Kraw + 63) & ~63;
  ArenaPlan A{c};
  c->stem = A.take((size_t)H * c->Kpad); A.reg("stem.weight", c->stem, (size_t)H * c->Kraw);      // arena rows padded to Kpad with zeros (ia2p_vit_load_tensor)
  c->sng = c->snb = c->plg = c->plb = 0;
  if (g.stem_ln) { c->sng = A.par("stem.norm.weight", H); c->snb = A.par("stem.norm.bias", H); }
  c->cls = A.par("cls_token", H);
  c->pos = A.par("pos_embed", (size_t)c->T * H);
  if (g.pre_ln) { c->plg = A.par("pre_ln.weight", H); c->plb = A.par("pre_ln.bias", H); }
  for (int i = 0; i < g.num_layers; ++i) {
    const std::string p = "blocks." + std::to_string(i) + ".";
    CLayer l;
    l.ln1g = A.par(p + "norm_1.weight", H); l.ln1b = A.par(p + "norm_1.bias", H);
    l.wqkv = A.par(p + "attn.in_proj_weight", (size_t)3 * H * H); l.bqkv = A.par(p + "attn.in_proj_bias", (size_t)3 * H);
    l.wo = A.par(p + "attn.out_proj.weight", (size_t)H * H); l.bo = A.par(p + "attn.out_proj.bias", H);
    if (g.bias_kv) { c->bk.push_back(A.par(p + "attn.bias_k", H)); c->bv.push_back(A.par(p + "attn.bias_v", H)); }
    l.ln2g = A.par(p + "norm_2.weight", H); l.ln2b = A.par(p + "norm_2.bias", H);
    l.w1 = A.par(p + "mlp.fc1.weight", (size_t)I * H); l.b1 = A.par(p + "mlp.fc1.bias", I);
    l.w2 = A.par(p + "mlp.fc2.weight", (size_t)H * I); l.b2 = A.par(p + "mlp.fc2.bias", H);
    xf_take_folds(A, l, H, I);
    c->layers.push_back(l);
  }
  c->hng = A.par("head.norm.weight", H); c->hnb = A.par("head.norm.bias", H);
  c->wproj = A.par("head.proj.weight", (size_t)g.out_dim * H);
  c->arena_elems = A.cur;
  return IA2P_OK;
}

static ia2p_status vit_fold(ia2p_vit* c, hipStream_t stream = nullptr, bool sync = true) {
  return xf_refold(c, c->layers, c->cfg.hidden_size, c->cfg.intermediate_size, stream, sync, "vit");
}

static ia2p_status vit_run(ia2p_vit* c, const half_t* pixels, int B, float* out, half_t* last) {
  const ia2p_vit_config& g = c->cfg;
  const int H = g.hidden_size, I = g.intermediate_size, T = c->T, M = B * T, MP = B * c->P;
  T2 x = wsalloc(c, (size_t)M * H), qkv = wsalloc(c, (size_t)M * 3 * H), att = wsalloc(c, (size_t)M * H), ff = wsalloc(c, (size_t)M * I);
  T2 stt = wsalloc(c, (size_t)M * ((H + 63) / 64) * 2 * 2);
  float* st = (float*)stt.p;
  int slots = 1;
  {      // stem: patch rows through the GEMM, then class token / positions / LayerNorms and the first block's row statistics in one pass
    T2 cols = wsalloc(c, (size_t)MP * c->Kpad), pat = wsalloc(c, (size_t)MP * H);
    CHECK_LAUNCH(c, ia2p_launch_patch_gather(pixels, cols.p, B, g.in_channels, g.image_h, g.image_w, g.patch_size, g.patch_stride, c->gh, c->gw, c->Kpad, c->stream), "vit patch gather");
    op_gemm(c, cols.p, c->Kpad, W_(c, c->stem), nullptr, nullptr, 0, pat.p, H, MP, H, c->Kpad);
    CHECK_LAUNCH(c, ia2p_launch_vit_embed(pat.p, W_(c, c->cls), W_(c, c->pos), g.stem_ln ? W_(c, c->sng) : nullptr, g.stem_ln ? W_(c, c->snb) : nullptr,
                                          g.pre_ln ? W_(c, c->plg) : nullptr, g.pre_ln ? W_(c, c->plb) : nullptr, x.p, st, B, T, H, g.layer_norm_eps, c->stream), "vit embeddings");
    wsfree(c, pat); wsfree(c, cols);
  }
  for (int i = 0; i < g.num_layers; ++i)
    xf_layer(c, c->layers[i], x.p, qkv.p, att.p, ff.p, st, slots, M, H, I, g.layer_norm_eps, 1, [&] {
      CHECK_LAUNCH(c, ia2p_launch_full_attention(qkv.p, att.p, g.bias_kv ? W_(c, c->bk[i]) : nullptr, g.bias_kv ? W_(c, c->bv[i]) : nullptr, B, T, g.num_heads, c->D, c->stream), "vit attention");
    });
  if (last && !c->dry && !c->failed) {
    hipError_t e = hipMemcpyAsync(last, x.p, (size_t)M * H * sizeof(half_t), hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) fail_hip(c, e, "vit");
  }
  {      // head: LayerNorm of the class rows (row b * T of x), bias-free projection in fp32
    T2 pr = wsalloc(c, (size_t)B * H);
    CHECK_LAUNCH(c, ia2p_launch_layernorm(x.p, T * H, pr.p, H, W_(c, c->hng), W_(c, c->hnb), B, H, g.layer_norm_eps, c->stream), "vit head LayerNorm");
    CHECK_LAUNCH(c, ia2p_launch_vit_project(pr.p, W_(c, c->wproj), out, B, g.out_dim, H, c->stream), "vit head projection");
    wsfree(c, pr);
  }
  wsfree(c, stt); wsfree(c, ff); wsfree(c, att); wsfree(c, qkv); wsfree(c, x);
  return c->failed ? IA2P_ERR_HIP : IA2P_OK;
}

ia2p_status ia2p_vit_create(const ia2p_vit_config* cfg, ia2p_vit** out) {
  return rc_create(cfg, out, "ia2p_vit_create", [](ia2p_vit* c) {
    if (c->cfg.layer_norm_eps <= 0.f) c->cfg.layer_norm_eps = 1e-6f;
    return vit_plan(c);
  });
}
void ia2p_vit_destroy(ia2p_vit* c) { delete c; }
const char* ia2p_vit_last_error(ia2p_vit* c) { return rc_last_error(c); }
size_t ia2p_vit_arena_bytes(ia2p_vit* c) { return rc_arena_bytes(c); }
int ia2p_vit_tokens(ia2p_vit* c) { return c ? c->T : 0; }
ia2p_status ia2p_vit_bind_arena(ia2p_vit* c, void* dev, size_t bytes) { return rc_bind_arena(c, dev, bytes); }
ia2p_status ia2p_vit_load_tensor(ia2p_vit* c, const char* key, const void* src, const int64_t* shape, int ndim, void* stream) {
  if (c && key && src && shape && c->arena && c->Kpad != c->Kraw && !strcmp(key, "stem.weight"))      // [hidden, C * p * p] rows into rows of Kpad, the rest zero
    return rc_load_padded_rows(c, key, c->stem, c->cfg.hidden_size, c->Kraw, c->Kpad, src, shape, ndim, stream);
  return rc_load_tensor(c, key, src, shape, ndim, stream);
}
ia2p_status ia2p_vit_finalize_weights(ia2p_vit* c) {
  const ia2p_status st = rc_finalize(c, "ViT");
  return st == IA2P_OK ? vit_fold(c) : st;
}
static ia2p_status vit_check(ia2p_vit* c, int B) {
  if (B < 1 || (size_t)B * c->cfg.num_heads > 65535) return fail(c, IA2P_ERR_SHAPE, "vit: B=%d", B);
  return IA2P_OK;
}
size_t ia2p_vit_workspace_bytes(ia2p_vit* c, int B) {
  if (!c || vit_check(c, B) != IA2P_OK) return 0;
  return pass_dry(c, [&] { return vit_run(c, nullptr, B, nullptr, (half_t*)1); });
}
ia2p_status ia2p_vit_encode(ia2p_vit* c, void* stream, const void* pixels, int B, float* out, void* last_hidden, void* ws, size_t ws_bytes) {
  if (!c || !pixels || !out || !ws) return fail(c, IA2P_ERR_INVALID, "vit_encode: null argument");
  if (!c->finalized) return fail(c, IA2P_ERR_STATE, "vit_encode before weights were finalized");
  ia2p_status st = vit_check(c, B);
  if (st != IA2P_OK) return st;
  st = pass_ready(c, [&] { return vit_fold(c, (hipStream_t)stream, false); });
  if (st == IA2P_OK) st = pass_enter(c, stream, ws, ws_bytes);
  if (st != IA2P_OK) return st;
  pass_record(c, 1, [&] { return vit_run(c, nullptr, B, nullptr, nullptr); });      // weight-prefetch plan: the contractions of a pass in launch order (the same for every B)
  return pass_leave(c, vit_run(c, (const half_t*)pixels, B, out, (half_t*)last_hidden));
}
