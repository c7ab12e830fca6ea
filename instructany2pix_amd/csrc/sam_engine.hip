// SAM executor and its C ABI (ia2p_sam_*): see include/ia2p.h and DESIGN.md §12. Runtime and operator wrappers: engine_rt.h / engine_rt.hip; the encoder block: xf_layer.h;
// the kernels that are SAM's own: sam.hip.
#include "xf_layer.h"

// sam.hip
size_t ia2p_relpos_attention_lds(int D, int Sh, int Sw);
hipError_t ia2p_launch_relpos_attention(const half_t* qkv, half_t* out, const half_t* bqkv, const half_t* Rh, const half_t* Rw, int B, int gh, int gw, int Sh, int Sw, int heads, int D,
                                        hipStream_t s);
hipError_t ia2p_launch_small_head_attention(const half_t* q, const half_t* k, const half_t* v, half_t* out, int B, int Tq, int Tk, int heads, int D, hipStream_t s);
hipError_t ia2p_launch_mask_upsample(const float* src, float* dstf, unsigned char* dstu, int n, int sh, int sw, int lds, long img_stride, int H, int W, float thr, hipStream_t s);
hipError_t ia2p_launch_mask_morph(const unsigned char* src, unsigned char* dst, unsigned char* tmp, int H, int W, int k, int dilate, hipStream_t s);
hipError_t ia2p_launch_pixel_shuffle2(const half_t* g, half_t* y, int B, int Hs, int Ws, int Co, hipStream_t s);
hipError_t ia2p_launch_hyper_dot(const half_t* hyper, long hyper_stride, const half_t* up, float* mask, int n, int P, int C, hipStream_t s);
hipError_t ia2p_launch_sam_act(half_t* x, long n, int kind, hipStream_t s);
hipError_t ia2p_launch_sam_add_rows(const half_t* a, const half_t* b, half_t* out, long n, long period, hipStream_t s);
hipError_t ia2p_launch_sam_take_col(const half_t* src, long ld, float* dst, int n, hipStream_t s);

// =====================================================================================================================
// Segment Anything (reference gdino/lib.py:21-51 `get_mask`: `SamPredictor.set_image` + `predict(box=...)`): the ViT image encoder -- patch stem, absolute positions,
// pre-LayerNorm blocks of xf_layer.h whose attention runs over 14 x 14 windows or, in the global blocks, the whole grid, both with the decomposed relative-position
// bias; the neck (1x1 conv, LayerNorm2d, 3x3 conv, LayerNorm2d) -- and, per box, the prompt encoder (on the host, fp32) and the two-way mask decoder.
// =====================================================================================================================
constexpr int SAM_TOK = 7, SAM_MASK_TOKENS = 4;      // iou token + 4 mask tokens + the box's two corners
struct SamAttn { size_t wq, bq, wk, bk, wv, bv, wo, bo; int Ci; };
struct SamDecLayer { SamAttn self, t2i, i2t; size_t n1g, n1b, n2g, n2b, n3g, n3b, n4g, n4b, w1, b1, w2, b2; };
struct ia2p_sam : RunCtx {
  ia2p_sam_config cfg;
  int g, P, D, Kraw, Kpad, C;
  size_t stem, stemb, pos, nc1, n1g, n1b, nc2, n2g, n2b;
  std::vector<CLayer> layers;
  std::vector<size_t> rph, rpw;
  std::vector<char> is_global;
  size_t gauss, pe2, pe3, nomask, ioutok, masktok, densepe;
  std::vector<SamDecLayer> dec;
  SamAttn fin;
  size_t nfg, nfb, up1w, up1b, upng, upnb, up2w, up2b, hy[3][2], io[3][2];
  // host copies (finalize): the random-Fourier matrix [2][C / 2], point embeddings 2 / 3, the output tokens [5][C]
  std::vector<float> h_gauss, h_pe2, h_pe3, h_tok;
  std::vector<half_t> h_stage;
};

static ia2p_status sam_plan(ia2p_sam* c) {
  const ia2p_sam_config& g = c->cfg;
  const int H = g.hidden_size, I = g.mlp_dim, C = g.output_channels;
  if (g.num_layers < 1 || g.num_heads < 1 || H < 64 || H % 64 || H > 2048 || I < 64 || I % 64)
    return fail(c, IA2P_ERR_SHAPE, "sam: hidden %d must be a multiple of 64 (<= 2048), mlp dim %d a multiple of 64", H, I);
  if (H % g.num_heads || (H / g.num_heads != 64 && H / g.num_heads != 80)) return fail(c, IA2P_ERR_SHAPE, "sam: head dim must be 64 or 80 (hidden %d, %d heads)", H, g.num_heads);
  if (g.patch_size < 1 || g.image_size < g.patch_size || g.image_size % g.patch_size) return fail(c, IA2P_ERR_SHAPE, "sam: image size %d is no multiple of the patch size %d", g.image_size, g.patch_size);
  if (g.window_size < 1 || g.window_size > 16) return fail(c, IA2P_ERR_SHAPE, "sam: window size %d (1..16)", g.window_size);
  if (g.num_global < 0 || g.num_global > IA2P_SAM_MAX_GLOBAL) return fail(c, IA2P_ERR_SHAPE, "sam: %d global-attention blocks (<= %d)", g.num_global, IA2P_SAM_MAX_GLOBAL);
  c->D = H / g.num_heads; c->g = g.image_size / g.patch_size; c->P = c->g * c->g; c->C = C;
  if (ia2p_relpos_attention_lds(c->D, c->g, c->g) > (size_t)64 * 1024) return fail(c, IA2P_ERR_SHAPE, "sam: a %d x %d grid is too large for the bias rows of a query tile in LDS", c->g, c->g);
  if (C < 64 || C % 64 || C != g.dec_hidden || g.dec_layers < 1 || g.dec_heads < 1 || g.dec_downsample_rate < 1 || g.dec_mlp_dim < 64 || g.dec_mlp_dim % 64)
    return fail(c, IA2P_ERR_SHAPE, "sam: output channels %d must equal the decoder's hidden size %d (a multiple of 64), decoder mlp dim %d a multiple of 64", C, g.dec_hidden, g.dec_mlp_dim);
  for (int ds : {1, g.dec_downsample_rate}) {
    const int Ci = C / ds;
    if (C % ds || Ci % 64 || Ci % g.dec_heads || (Ci / g.dec_heads != 16 && Ci / g.dec_heads != 32))
      return fail(c, IA2P_ERR_SHAPE, "sam: the decoder's attention needs head dim 16 or 32 (hidden %d / %d over %d heads)", C, ds, g.dec_heads);
  }
  c->Kraw = 3 * g.patch_size * g.patch_size; c->Kpad = (c->Kraw + 63) & ~63;
  ArenaPlan A{c};
  c->stem = A.take((size_t)H * c->Kpad); A.reg("patch_embed.weight", c->stem, (size_t)H * c->Kraw);
  c->stemb = A.par("patch_embed.bias", H);
  c->pos = A.par("pos_embed", (size_t)c->P * H);
  c->is_global.assign(g.num_layers, 0);
  for (int i = 0; i < g.num_global; ++i) {
    if (g.global_attn_indexes[i] < 0 || g.global_attn_indexes[i] >= g.num_layers) return fail(c, IA2P_ERR_SHAPE, "sam: global-attention block index %d outside 0..%d", g.global_attn_indexes[i], g.num_layers - 1);
    c->is_global[g.global_attn_indexes[i]] = 1;
  }
  for (int i = 0; i < g.num_layers; ++i) {
    const std::string p = "blocks." + std::to_string(i) + ".";
    const int S = c->is_global[i] ? c->g : g.window_size;
    CLayer l;
    l.ln1g = A.par(p + "norm1.weight", H); l.ln1b = A.par(p + "norm1.bias", H);
    l.wqkv = A.par(p + "attn.qkv.weight", (size_t)3 * H * H); l.bqkv = A.par(p + "attn.qkv.bias", (size_t)3 * H);
    l.wo = A.par(p + "attn.proj.weight", (size_t)H * H); l.bo = A.par(p + "attn.proj.bias", H);
    c->rph.push_back(A.par(p + "attn.rel_pos_h", (size_t)(2 * S - 1) * c->D)); c->rpw.push_back(A.par(p + "attn.rel_pos_w", (size_t)(2 * S - 1) * c->D));
    l.ln2g = A.par(p + "norm2.weight", H); l.ln2b = A.par(p + "norm2.bias", H);
    l.w1 = A.par(p + "mlp.lin1.weight", (size_t)I * H); l.b1 = A.par(p + "mlp.lin1.bias", I);
    l.w2 = A.par(p + "mlp.lin2.weight", (size_t)H * I); l.b2 = A.par(p + "mlp.lin2.bias", H);
    xf_take_folds(A, l, H, I);
    c->layers.push_back(l);
  }
  c->nc1 = A.par("neck.conv1.weight", (size_t)C * H);
  c->n1g = A.par("neck.norm1.weight", C); c->n1b = A.par("neck.norm1.bias", C);
  c->nc2 = A.take((size_t)C * 9 * C); c->params["neck.conv2.weight"] = Param{c->nc2, (size_t)C * 9 * C, PK_CONV, C, C, false, false};
  c->n2g = A.par("neck.norm2.weight", C); c->n2b = A.par("neck.norm2.bias", C);
  // prompt encoder
  c->gauss = A.par("prompt.pe_gaussian", (size_t)2 * (C / 2));
  c->pe2 = A.par("prompt.point_embed.2", C); c->pe3 = A.par("prompt.point_embed.3", C);
  c->nomask = A.par("prompt.no_mask_embed", C);
  c->densepe = A.take((size_t)c->P * C);
  // mask decoder
  c->ioutok = A.par("decoder.iou_token", C); c->masktok = A.par("decoder.mask_tokens", (size_t)SAM_MASK_TOKENS * C);
  auto attn = [&](const std::string& p, int ds) {
    SamAttn a; a.Ci = C / ds;
    a.wq = A.par(p + "q.weight", (size_t)a.Ci * C); a.bq = A.par(p + "q.bias", a.Ci);
    a.wk = A.par(p + "k.weight", (size_t)a.Ci * C); a.bk = A.par(p + "k.bias", a.Ci);
    a.wv = A.par(p + "v.weight", (size_t)a.Ci * C); a.bv = A.par(p + "v.bias", a.Ci);
    a.wo = A.par(p + "out.weight", (size_t)C * a.Ci); a.bo = A.par(p + "out.bias", C);
    return a;
  };
  for (int i = 0; i < g.dec_layers; ++i) {
    const std::string p = "decoder.layers." + std::to_string(i) + ".";
    SamDecLayer l;
    l.self = attn(p + "self_attn.", 1); l.t2i = attn(p + "t2i.", g.dec_downsample_rate); l.i2t = attn(p + "i2t.", g.dec_downsample_rate);
    l.n1g = A.par(p + "norm1.weight", C); l.n1b = A.par(p + "norm1.bias", C); l.n2g = A.par(p + "norm2.weight", C); l.n2b = A.par(p + "norm2.bias", C);
    l.n3g = A.par(p + "norm3.weight", C); l.n3b = A.par(p + "norm3.bias", C); l.n4g = A.par(p + "norm4.weight", C); l.n4b = A.par(p + "norm4.bias", C);
    l.w1 = A.par(p + "mlp.lin1.weight", (size_t)g.dec_mlp_dim * C); l.b1 = A.par(p + "mlp.lin1.bias", g.dec_mlp_dim);
    l.w2 = A.par(p + "mlp.lin2.weight", (size_t)C * g.dec_mlp_dim); l.b2 = A.par(p + "mlp.lin2.bias", C);
    c->dec.push_back(l);
  }
  c->fin = attn("decoder.final_attn.", g.dec_downsample_rate);
  c->nfg = A.par("decoder.norm_final.weight", C); c->nfb = A.par("decoder.norm_final.bias", C);
  // the two ConvTranspose2d(k = 2, s = 2) as GEMMs: rows (ky, kx, co) of [4 Co, Ci], the bias four times (the Python loader permutes the checkpoint's [Ci, Co, 2, 2])
  c->up1w = A.par("decoder.upscale1.weight", (size_t)C * C); c->up1b = A.par("decoder.upscale1.bias", C);
  c->upng = A.par("decoder.upscale_norm.weight", C / 4); c->upnb = A.par("decoder.upscale_norm.bias", C / 4);
  c->up2w = A.par("decoder.upscale2.weight", (size_t)(C / 2) * (C / 4)); c->up2b = A.par("decoder.upscale2.bias", C / 2);
  for (int k = 0; k < 3; ++k) {
    const int no = k == 2 ? C / 8 : C;
    c->hy[k][0] = A.par("decoder.hyper0." + std::to_string(k) + ".weight", (size_t)no * C); c->hy[k][1] = A.par("decoder.hyper0." + std::to_string(k) + ".bias", no);
    const int ni = k == 2 ? SAM_MASK_TOKENS : C;
    c->io[k][0] = A.par("decoder.iou_head." + std::to_string(k) + ".weight", (size_t)ni * C); c->io[k][1] = A.par("decoder.iou_head." + std::to_string(k) + ".bias", ni);
  }
  c->arena_elems = A.cur;
  return IA2P_OK;
}

static ia2p_status sam_fold(ia2p_sam* c, hipStream_t stream = nullptr, bool sync = true) {
  return xf_refold(c, c->layers, c->cfg.hidden_size, c->cfg.mlp_dim, stream, sync, "sam");
}

// sin / cos random-Fourier features of a point in [0, 1]^2 (SamPositionalEmbedding): [sin(2 pi (2 p - 1) G) | cos(...)], fp32
static void sam_pe(const ia2p_sam* c, float x, float y, float* out) {
  const int F = c->C / 2;
  const float cx = 2.f * x - 1.f, cy = 2.f * y - 1.f;
  for (int j = 0; j < F; ++j) {
    const float v = 6.283185307179586f * (cx * c->h_gauss[j] + cy * c->h_gauss[F + j]);
    out[j] = sinf(v); out[F + j] = cosf(v);
  }
}

// host side of finalize: copies of the small prompt tensors, and the dense positional encoding of the token grid uploaded next to the weights
static ia2p_status sam_host_tables(ia2p_sam* c) {
  const int C = c->C;
  auto fetch = [&](size_t off, size_t n, std::vector<float>& dst) {
    std::vector<half_t> t(n);
    if (hipMemcpy(t.data(), c->arena + off, n * sizeof(half_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
    dst.resize(n);
    for (size_t i = 0; i < n; ++i) dst[i] = (float)t[i];
    return true;
  };
  std::vector<float> iou, mt;
  if (!fetch(c->gauss, (size_t)C, c->h_gauss) || !fetch(c->pe2, C, c->h_pe2) || !fetch(c->pe3, C, c->h_pe3) || !fetch(c->ioutok, C, iou) || !fetch(c->masktok, (size_t)SAM_MASK_TOKENS * C, mt))
    return fail(c, IA2P_ERR_HIP, "sam: cannot read the prompt tensors back");
  c->h_tok = iou; c->h_tok.insert(c->h_tok.end(), mt.begin(), mt.end());
  std::vector<half_t> pe((size_t)c->P * C);
  std::vector<float> row(C);
  for (int y = 0; y < c->g; ++y)
    for (int x = 0; x < c->g; ++x) {
      sam_pe(c, ((float)x + 0.5f) / (float)c->g, ((float)y + 0.5f) / (float)c->g, row.data());
      for (int j = 0; j < C; ++j) pe[((size_t)y * c->g + x) * C + j] = (half_t)row[j];
    }
  if (hipMemcpy(c->arena + c->densepe, pe.data(), pe.size() * sizeof(half_t), hipMemcpyHostToDevice) != hipSuccess) return fail(c, IA2P_ERR_HIP, "sam: cannot upload the dense positional encoding");
  return IA2P_OK;
}

static ia2p_status sam_encode_run(ia2p_sam* c, const half_t* pixels, int B, half_t* emb) {
  const ia2p_sam_config& g = c->cfg;
  const int H = g.hidden_size, I = g.mlp_dim, P = c->P, C = c->C, S = g.image_size;
  T2 x = wsalloc(c, (size_t)P * H), qkv = wsalloc(c, (size_t)P * 3 * H), att = wsalloc(c, (size_t)P * H), ff = wsalloc(c, (size_t)P * I);
  T2 stt = wsalloc(c, (size_t)P * ((H + 63) / 64) * 2 * 2);
  T2 n1 = wsalloc(c, (size_t)P * C), n2 = wsalloc(c, (size_t)P * C);
  float* st = (float*)stt.p;
  for (int b = 0; b < B; ++b) {      // one image at a time: the global blocks already fill the chip
    int slots = 1;
    {      // stem: patch rows through the GEMM (+ bias + absolute positions), the first block's row statistics from its epilogue
      T2 cols = wsalloc(c, (size_t)P * c->Kpad);
      CHECK_LAUNCH(c, ia2p_launch_patch_gather(pixels + (size_t)b * 3 * S * S, cols.p, 1, 3, S, S, g.patch_size, g.patch_size, c->g, c->g, c->Kpad, c->stream), "sam patch gather");
      GemmOpt o; o.stats = st; o.stat_slots = &slots;
      op_gemm(c, cols.p, c->Kpad, W_(c, c->stem), W_(c, c->stemb), W_(c, c->pos), H, x.p, H, P, H, c->Kpad, o);
      wsfree(c, cols);
    }
    for (int i = 0; i < g.num_layers; ++i)
      xf_layer(c, c->layers[i], x.p, qkv.p, att.p, ff.p, st, slots, P, H, I, g.layer_norm_eps, 1, [&] {
        const int Sw = c->is_global[i] ? c->g : g.window_size;
        CHECK_LAUNCH(c, ia2p_launch_relpos_attention(qkv.p, att.p, W_(c, c->layers[i].bqkv), W_(c, c->rph[i]), W_(c, c->rpw[i]), 1, c->g, c->g, Sw, Sw, g.num_heads, c->D, c->stream),
                     c->is_global[i] ? "sam global attention" : "sam window attention");
      });
    // neck: 1x1 conv (no bias), LayerNorm2d, 3x3 conv (no bias), LayerNorm2d -- channels-last rows throughout
    op_gemm(c, x.p, H, W_(c, c->nc1), nullptr, nullptr, 0, n1.p, C, P, C, H);
    CHECK_LAUNCH(c, ia2p_launch_layernorm(n1.p, C, n1.p, C, W_(c, c->n1g), W_(c, c->n1b), P, C, 1e-6f, c->stream), "sam neck LayerNorm");
    op_conv3(c, n1.p, 1, c->g, c->g, C, W_(c, c->nc2), nullptr, C, n2.p);
    CHECK_LAUNCH(c, ia2p_launch_layernorm(n2.p, C, emb ? emb + (size_t)b * P * C : nullptr, C, W_(c, c->n2g), W_(c, c->n2b), P, C, 1e-6f, c->stream), "sam neck LayerNorm");
  }
  wsfree(c, n2); wsfree(c, n1); wsfree(c, stt); wsfree(c, ff); wsfree(c, att); wsfree(c, qkv); wsfree(c, x);
  return c->failed ? IA2P_ERR_HIP : IA2P_OK;
}

// tok: fp16 [n, 7, C] point embeddings (output tokens + the box's corner embeddings), already on the device
static ia2p_status sam_decode_run(ia2p_sam* c, const half_t* emb, const half_t* tok, int n, float* low_res, float* iou) {
  const ia2p_sam_config& g = c->cfg;
  const int C = c->C, P = c->P, T = SAM_TOK, MT = n * T, MP = n * P, heads = g.dec_heads;
  const size_t big = (size_t)MP * C;
  T2 q = wsalloc(c, (size_t)MT * C), qq = wsalloc(c, (size_t)MT * C), keys = wsalloc(c, big), kk = wsalloc(c, big);
  T2 pq = wsalloc(c, big), pk = wsalloc(c, big), pv = wsalloc(c, big), at = wsalloc(c, big), mlp = wsalloc(c, (size_t)MT * g.dec_mlp_dim);
  auto ln = [&](half_t* x, size_t gm, size_t bt, int M, int Cn, float eps, const char* what) { CHECK_LAUNCH(c, ia2p_launch_layernorm(x, Cn, x, Cn, W_(c, gm), W_(c, bt), M, Cn, eps, c->stream), what); };
  auto add = [&](const half_t* a, const half_t* b, half_t* o, size_t nel, size_t period) { CHECK_LAUNCH(c, ia2p_launch_sam_add_rows(a, b, o, (long)nel, (long)period, c->stream), "sam add"); };
  // out = residual + out_proj(softmax(q_proj(Aq) k_proj(Ak)^T / sqrt(d)) v_proj(Av))
  auto attention = [&](const SamAttn& a, const half_t* Aq, int Tq, const half_t* Ak, const half_t* Av, int Tk, const half_t* residual, half_t* out) {
    op_gemm(c, Aq, C, W_(c, a.wq), W_(c, a.bq), nullptr, 0, pq.p, a.Ci, n * Tq, a.Ci, C);
    op_gemm(c, Ak, C, W_(c, a.wk), W_(c, a.bk), nullptr, 0, pk.p, a.Ci, n * Tk, a.Ci, C);
    op_gemm(c, Av, C, W_(c, a.wv), W_(c, a.bv), nullptr, 0, pv.p, a.Ci, n * Tk, a.Ci, C);
    CHECK_LAUNCH(c, ia2p_launch_small_head_attention(pq.p, pk.p, pv.p, at.p, n, Tq, Tk, heads, a.Ci / heads, c->stream), "sam decoder attention");
    op_gemm(c, at.p, a.Ci, W_(c, a.wo), W_(c, a.bo), residual, C, out, C, n * Tq, C, a.Ci);
  };
  if (!c->dry && !c->failed) {
    hipError_t e = hipMemcpyAsync(q.p, tok, (size_t)MT * C * sizeof(half_t), hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) fail_hip(c, e, "sam decoder tokens");
  }
  for (int j = 0; j < n; ++j) add(emb, W_(c, c->nomask), keys.p + (size_t)j * P * C, (size_t)P * C, C);      // image embedding + the "no mask" dense prompt, once per box
  for (int i = 0; i < g.dec_layers; ++i) {
    const SamDecLayer& l = c->dec[i];
    if (i == 0) attention(l.self, q.p, T, q.p, q.p, T, nullptr, qq.p);      // the first block's self-attention REPLACES the tokens (no positional term, no residual)
    else { add(q.p, tok, qq.p, (size_t)MT * C, (size_t)MT * C); attention(l.self, qq.p, T, qq.p, q.p, T, q.p, qq.p); }
    std::swap(q, qq);
    ln(q.p, l.n1g, l.n1b, MT, C, g.layer_norm_eps, "sam decoder norm1");
    add(q.p, tok, qq.p, (size_t)MT * C, (size_t)MT * C);
    add(keys.p, W_(c, c->densepe), kk.p, big, (size_t)P * C);
    attention(l.t2i, qq.p, T, kk.p, keys.p, P, q.p, q.p);
    ln(q.p, l.n2g, l.n2b, MT, C, g.layer_norm_eps, "sam decoder norm2");
    op_gemm(c, q.p, C, W_(c, l.w1), W_(c, l.b1), nullptr, 0, mlp.p, g.dec_mlp_dim, MT, g.dec_mlp_dim, C);
    CHECK_LAUNCH(c, ia2p_launch_sam_act(mlp.p, (long)MT * g.dec_mlp_dim, 0, c->stream), "sam decoder ReLU");
    op_gemm(c, mlp.p, g.dec_mlp_dim, W_(c, l.w2), W_(c, l.b2), q.p, C, q.p, C, MT, C, g.dec_mlp_dim);
    ln(q.p, l.n3g, l.n3b, MT, C, g.layer_norm_eps, "sam decoder norm3");
    add(q.p, tok, qq.p, (size_t)MT * C, (size_t)MT * C);
    attention(l.i2t, kk.p, P, qq.p, q.p, T, keys.p, keys.p);
    ln(keys.p, l.n4g, l.n4b, MP, C, g.layer_norm_eps, "sam decoder norm4");
  }
  add(q.p, tok, qq.p, (size_t)MT * C, (size_t)MT * C);
  add(keys.p, W_(c, c->densepe), kk.p, big, (size_t)P * C);
  attention(c->fin, qq.p, T, kk.p, keys.p, P, q.p, q.p);
  ln(q.p, c->nfg, c->nfb, MT, C, 1e-5f, "sam decoder final norm");
  {      // upscaling: ConvTranspose2d = GEMM to (ky, kx, co) columns + pixel shuffle; LayerNorm2d + GELU between, GELU after (in the second GEMM's epilogue: it commutes with the shuffle)
    const int C4 = C / 4, C8 = C / 8, gs = c->g;
    T2 u1 = wsalloc(c, (size_t)MP * 4 * C4), u2 = wsalloc(c, (size_t)MP * 16 * C8);
    op_gemm(c, keys.p, C, W_(c, c->up1w), W_(c, c->up1b), nullptr, 0, kk.p, C, MP, C, C);
    CHECK_LAUNCH(c, ia2p_launch_pixel_shuffle2(kk.p, u1.p, n, gs, gs, C4, c->stream), "sam pixel shuffle");
    ln(u1.p, c->upng, c->upnb, MP * 4, C4, 1e-6f, "sam upscale LayerNorm");
    CHECK_LAUNCH(c, ia2p_launch_sam_act(u1.p, (long)MP * 4 * C4, 1, c->stream), "sam upscale GELU");
    T2 g2 = wsalloc(c, (size_t)MP * 4 * 4 * C8);
    GemmOpt o; o.act = 1;
    op_gemm(c, u1.p, C4, W_(c, c->up2w), W_(c, c->up2b), nullptr, 0, g2.p, 4 * C8, MP * 4, 4 * C8, C4, o);
    CHECK_LAUNCH(c, ia2p_launch_pixel_shuffle2(g2.p, u2.p, n, 2 * gs, 2 * gs, C8, c->stream), "sam pixel shuffle");
    wsfree(c, g2);
    // hypernetwork of mask token 0 (token row 1) and the IoU head (token row 0): three linears with ReLU between
    T2 h0 = wsalloc(c, (size_t)n * C), h1 = wsalloc(c, (size_t)n * C);
    auto head = [&](const size_t (*w)[2], int row, int nout, half_t* out) {
      op_gemm(c, q.p + (size_t)row * C, T * C, W_(c, w[0][0]), W_(c, w[0][1]), nullptr, 0, h0.p, C, n, C, C);
      CHECK_LAUNCH(c, ia2p_launch_sam_act(h0.p, (long)n * C, 0, c->stream), "sam head ReLU");
      op_gemm(c, h0.p, C, W_(c, w[1][0]), W_(c, w[1][1]), nullptr, 0, h1.p, C, n, C, C);
      CHECK_LAUNCH(c, ia2p_launch_sam_act(h1.p, (long)n * C, 0, c->stream), "sam head ReLU");
      op_gemm(c, h1.p, C, W_(c, w[2][0]), W_(c, w[2][1]), nullptr, 0, out, nout, n, nout, C);
    };
    head(c->hy, 1, C8, h0.p);      // (h0 is free again once the second linear has read it: the launches are stream-ordered)
    CHECK_LAUNCH(c, ia2p_launch_hyper_dot(h0.p, C8, u2.p, low_res, n, 16 * P, C8, c->stream), "sam hypernetwork product");
    head(c->io, 0, SAM_MASK_TOKENS, h0.p);
    CHECK_LAUNCH(c, ia2p_launch_sam_take_col(h0.p, SAM_MASK_TOKENS, iou, n, c->stream), "sam IoU");
    wsfree(c, h1); wsfree(c, h0); wsfree(c, u2); wsfree(c, u1);
  }
  wsfree(c, mlp); wsfree(c, at); wsfree(c, pv); wsfree(c, pk); wsfree(c, pq); wsfree(c, kk); wsfree(c, keys); wsfree(c, qq); wsfree(c, q);
  return c->failed ? IA2P_ERR_HIP : IA2P_OK;
}

extern "C" {

ia2p_status ia2p_sam_create(const ia2p_sam_config* cfg, ia2p_sam** out) {
  return rc_create(cfg, out, "ia2p_sam_create", [](ia2p_sam* c) {
    if (c->cfg.layer_norm_eps <= 0.f) c->cfg.layer_norm_eps = 1e-6f;
    return sam_plan(c);
  });
}
void ia2p_sam_destroy(ia2p_sam* c) { delete c; }
const char* ia2p_sam_last_error(ia2p_sam* c) { return rc_last_error(c); }
size_t ia2p_sam_arena_bytes(ia2p_sam* c) { return rc_arena_bytes(c); }
ia2p_status ia2p_sam_bind_arena(ia2p_sam* c, void* dev, size_t bytes) { return rc_bind_arena(c, dev, bytes); }
ia2p_status ia2p_sam_load_tensor(ia2p_sam* c, const char* key, const void* src, const int64_t* shape, int ndim, void* stream) {
  if (c && key && src && shape && c->arena && c->Kpad != c->Kraw && !strcmp(key, "patch_embed.weight"))      // [hidden, 3 * p * p] rows into rows of Kpad, the rest zero
    return rc_load_padded_rows(c, key, c->stem, c->cfg.hidden_size, c->Kraw, c->Kpad, src, shape, ndim, stream);
  return rc_load_tensor(c, key, src, shape, ndim, stream);
}
ia2p_status ia2p_sam_finalize_weights(ia2p_sam* c) {
  ia2p_status st = rc_finalize(c, "SAM");
  if (st != IA2P_OK) return st;
  if (hipDeviceSynchronize() != hipSuccess) return fail(c, IA2P_ERR_HIP, "sam: the weight copies failed");
  st = sam_host_tables(c);
  if (st != IA2P_OK) { c->finalized = false; return st; }
  return sam_fold(c);
}
static ia2p_status sam_check(ia2p_sam* c, int B, int n) {
  if (B < 1 || B > 64 || n < 1 || n > 64) return fail(c, IA2P_ERR_SHAPE, "sam: %d images, %d boxes (1..64 each)", B, n);
  return IA2P_OK;
}
size_t ia2p_sam_workspace_bytes(ia2p_sam* c, int B, int n_boxes) {
  if (!c || sam_check(c, B, n_boxes) != IA2P_OK) return 0;
  const size_t a = pass_dry(c, [&] { return sam_encode_run(c, nullptr, B, nullptr); });
  const size_t b = pass_dry(c, [&] { return sam_decode_run(c, nullptr, nullptr, n_boxes, nullptr, nullptr); });
  return a && b ? std::max(a, b + (((size_t)n_boxes * SAM_TOK * c->C * sizeof(half_t) + 255) & ~(size_t)255)) : 0;
}
static ia2p_status sam_ready(ia2p_sam* c, void* stream, const char* what) {
  if (!c->finalized) return fail(c, IA2P_ERR_STATE, "%s before weights were finalized", what);
  return pass_ready(c, [&] {      // a tensor was reloaded after finalize: the host tables again too (they read the arena: the reload's copies must have landed)
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail(c, IA2P_ERR_HIP, "%s: stream", what);
    const ia2p_status st = sam_host_tables(c);
    return st == IA2P_OK ? sam_fold(c, (hipStream_t)stream, false) : st;
  });
}
ia2p_status ia2p_sam_encode_image(ia2p_sam* c, void* stream, const void* pixels, int B, void* embeddings, void* ws, size_t ws_bytes) {
  if (!c || !pixels || !embeddings || !ws) return fail(c, IA2P_ERR_INVALID, "sam_encode_image: null argument");
  ia2p_status st = sam_check(c, B, 1);
  if (st == IA2P_OK) st = sam_ready(c, stream, "sam_encode_image");
  if (st != IA2P_OK) return st;
  st = pass_enter(c, stream, ws, ws_bytes);
  if (st != IA2P_OK) return st;
  pass_record(c, 1, [&] { return sam_encode_run(c, nullptr, 1, nullptr); });
  return pass_leave(c, sam_encode_run(c, (const half_t*)pixels, B, (half_t*)embeddings));
}
ia2p_status ia2p_sam_predict_boxes(ia2p_sam* c, void* stream, const void* embeddings, const float* boxes, int n, float* low_res_logits, float* iou, void* ws, size_t ws_bytes) {
  if (!c || !embeddings || !boxes || !low_res_logits || !iou || !ws) return fail(c, IA2P_ERR_INVALID, "sam_predict_boxes: null argument");
  ia2p_status st = sam_check(c, 1, n);
  if (st != IA2P_OK) return st;
  const float S = (float)c->cfg.image_size;
  for (int i = 0; i < n; ++i) {
    const float* b = boxes + 4 * i;
    if (!(b[0] >= 0.f && b[1] >= 0.f && b[2] <= S && b[3] <= S && b[0] <= b[2] && b[1] <= b[3]))
      return fail(c, IA2P_ERR_SHAPE, "sam: box %d (%g, %g, %g, %g) is not inside the %d x %d input", i, b[0], b[1], b[2], b[3], c->cfg.image_size, c->cfg.image_size);
  }
  st = sam_ready(c, stream, "sam_predict_boxes");
  if (st != IA2P_OK) return st;
  // prompt encoder on the host (fp32): tokens [n][iou, mask 0..3, corner 0 + point_embed[2], corner 1 + point_embed[3]]
  const int C = c->C;
  const size_t tok_elems = (size_t)n * SAM_TOK * C, tok_bytes = (tok_elems * sizeof(half_t) + 255) & ~(size_t)255;
  if (ws_bytes < tok_bytes + 512) return fail(c, IA2P_ERR_NOMEM, "sam_predict_boxes: workspace too small");
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail(c, IA2P_ERR_HIP, "sam_predict_boxes: stream");      // (the staging buffer of an earlier call is free)
  c->h_stage.resize(tok_elems);
  std::vector<float> row(C);
  for (int i = 0; i < n; ++i) {
    half_t* t = c->h_stage.data() + (size_t)i * SAM_TOK * C;
    for (size_t j = 0; j < (size_t)(1 + SAM_MASK_TOKENS) * C; ++j) t[j] = (half_t)c->h_tok[j];
    for (int k = 0; k < 2; ++k) {
      sam_pe(c, (boxes[4 * i + 2 * k] + 0.5f) / S, (boxes[4 * i + 2 * k + 1] + 0.5f) / S, row.data());
      const std::vector<float>& pe = k ? c->h_pe3 : c->h_pe2;
      for (int j = 0; j < C; ++j) t[(size_t)(1 + SAM_MASK_TOKENS + k) * C + j] = (half_t)(row[j] + pe[j]);
    }
  }
  char* wsb = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  const size_t lost = (size_t)(wsb - (char*)ws);
  half_t* tok = (half_t*)wsb;
  if (hipMemcpyAsync(tok, c->h_stage.data(), tok_elems * sizeof(half_t), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) return fail(c, IA2P_ERR_HIP, "sam_predict_boxes: token upload");
  st = pass_enter(c, stream, wsb + tok_bytes, ws_bytes - lost - tok_bytes);
  if (st != IA2P_OK) return st;
  pass_record(c, 100 + n, [&] { return sam_decode_run(c, nullptr, nullptr, n, nullptr, nullptr); });
  return pass_leave(c, sam_decode_run(c, (const half_t*)embeddings, tok, n, low_res_logits, iou));
}

// ---- the launches of sam.hip on their own (unit tests, tools/sam_bench.py) -----------------------------------------------------------------------------------
ia2p_status ia2p_attention_window_relpos(void* stream, const void* qkv, void* out, const void* qkv_bias, const void* rel_h, const void* rel_w, int B, int gh, int gw, int heads, int D,
                                         int window) {
  if (!qkv || !out || !qkv_bias || !rel_h || !rel_w || B < 1 || gh < 1 || gw < 1 || heads < 1) return fail(nullptr, IA2P_ERR_INVALID, "attention_window_relpos: bad argument");
  if ((D != 64 && D != 80) || window < 1 || window > 16) return fail(nullptr, IA2P_ERR_SHAPE, "attention_window_relpos: D=%d (64 or 80), window %d (1..16)", D, window);
  const size_t wg = (size_t)B * ((gh + window - 1) / window) * ((gw + window - 1) / window) * heads;
  if (wg > 65535) return fail(nullptr, IA2P_ERR_SHAPE, "attention_window_relpos: %zu (image, window, head) triples (<= 65535)", wg);
  hipError_t e = ia2p_launch_relpos_attention((const half_t*)qkv, (half_t*)out, (const half_t*)qkv_bias, (const half_t*)rel_h, (const half_t*)rel_w, B, gh, gw, window, window, heads, D, (hipStream_t)stream);
  RET_HIP(e, "attention_window_relpos");
}
ia2p_status ia2p_attention_global_relpos(void* stream, const void* qkv, void* out, const void* rel_h, const void* rel_w, int B, int gh, int gw, int heads, int D) {
  if (!qkv || !out || !rel_h || !rel_w || B < 1 || gh < 1 || gw < 1 || heads < 1) return fail(nullptr, IA2P_ERR_INVALID, "attention_global_relpos: bad argument");
  if (D != 64 && D != 80) return fail(nullptr, IA2P_ERR_SHAPE, "attention_global_relpos: D=%d (64 or 80)", D);
  if (gh > 32767 || gw > 32767 || ia2p_relpos_attention_lds(D, gh, gw) > (size_t)64 * 1024 || (size_t)B * heads > 65535)
    return fail(nullptr, IA2P_ERR_SHAPE, "attention_global_relpos: a %d x %d grid is too large for the bias rows of a query tile in LDS (or B * heads > 65535)", gh, gw);
  hipError_t e = ia2p_launch_relpos_attention((const half_t*)qkv, (half_t*)out, nullptr, (const half_t*)rel_h, (const half_t*)rel_w, B, gh, gw, gh, gw, heads, D, (hipStream_t)stream);
  RET_HIP(e, "attention_global_relpos");
}
ia2p_status ia2p_attention_small_head(void* stream, const void* q, const void* k, const void* v, void* out, int B, int Tq, int Tk, int heads, int D) {
  if (!q || !k || !v || !out || B < 1 || Tq < 1 || Tk < 1 || heads < 1) return fail(nullptr, IA2P_ERR_INVALID, "attention_small_head: bad argument");
  if (D != 16 && D != 32) return fail(nullptr, IA2P_ERR_SHAPE, "attention_small_head: D=%d (16 or 32)", D);
  hipError_t e = ia2p_launch_small_head_attention((const half_t*)q, (const half_t*)k, (const half_t*)v, (half_t*)out, B, Tq, Tk, heads, D, (hipStream_t)stream);
  RET_HIP(e, "attention_small_head");
}
ia2p_status ia2p_mask_upsample_threshold(void* stream, const float* logits, int n, int src_h, int src_w, int src_ld, int64_t src_image_stride, int H, int W, float threshold,
                                         float* out_logits, void* out_mask) {
  if (!logits || (!out_logits && !out_mask)) return fail(nullptr, IA2P_ERR_INVALID, "mask_upsample_threshold: null argument");
  if (n < 1 || n > 65535 || src_h < 1 || src_w < 1 || src_ld < src_w || src_image_stride < (int64_t)(src_h - 1) * src_ld + src_w || H < 1 || H > 65535 || W < 1)
    return fail(nullptr, IA2P_ERR_SHAPE, "mask_upsample_threshold: n=%d src %d x %d (ld %d) -> %d x %d", n, src_h, src_w, src_ld, H, W);
  hipError_t e = ia2p_launch_mask_upsample(logits, out_logits, (unsigned char*)out_mask, n, src_h, src_w, src_ld, (long)src_image_stride, H, W, threshold, (hipStream_t)stream);
  RET_HIP(e, "mask_upsample_threshold");
}
ia2p_status ia2p_mask_morph(void* stream, const void* src, void* dst, void* tmp, int H, int W, int k, int is_dilate) {
  if (!src || !dst || !tmp || src == tmp || dst == tmp) return fail(nullptr, IA2P_ERR_INVALID, "mask_morph: null or aliased argument");
  if (H < 1 || H > 65535 || W < 1 || k < 1) return fail(nullptr, IA2P_ERR_SHAPE, "mask_morph: %d x %d, k=%d", H, W, k);
  hipError_t e = ia2p_launch_mask_morph((const unsigned char*)src, (unsigned char*)dst, (unsigned char*)tmp, H, W, k, is_dilate != 0, (hipStream_t)stream);
  RET_HIP(e, "mask_morph");
}
// the small launches of the mask decoder, one by one (tests/test_encoder_ops_gpu.py)
ia2p_status ia2p_pixel_shuffle2(void* stream, const void* g, void* y, int B, int Hs, int Ws, int Co) {
  if (!g || !y) return fail(nullptr, IA2P_ERR_INVALID, "pixel_shuffle2: null argument");
  if (B < 1 || Hs < 1 || Ws < 1 || Co < 8 || Co % 8 || ((long)B * Hs * Ws * 4 * (Co / 8) + 255) / 256 > 0x7fffffffL) return fail(nullptr, IA2P_ERR_SHAPE, "pixel_shuffle2: B=%d %d x %d Co=%d (multiple of 8)", B, Hs, Ws, Co);
  hipError_t e = ia2p_launch_pixel_shuffle2((const half_t*)g, (half_t*)y, B, Hs, Ws, Co, (hipStream_t)stream);
  RET_HIP(e, "pixel_shuffle2");
}
ia2p_status ia2p_hyper_dot(void* stream, const void* hyper, int64_t hyper_stride, const void* up, float* mask, int n, int P, int C) {
  if (!hyper || !up || !mask) return fail(nullptr, IA2P_ERR_INVALID, "hyper_dot: null argument");
  if (n < 1 || n > 65535 || P < 1 || C < 8 || C % 8 || hyper_stride < C || hyper_stride % 8) return fail(nullptr, IA2P_ERR_SHAPE, "hyper_dot: n=%d (1..65535) P=%d C=%d stride=%lld (multiples of 8, stride >= C)", n, P, C, (long long)hyper_stride);
  hipError_t e = ia2p_launch_hyper_dot((const half_t*)hyper, (long)hyper_stride, (const half_t*)up, mask, n, P, C, (hipStream_t)stream);
  RET_HIP(e, "hyper_dot");
}
ia2p_status ia2p_sam_act(void* stream, void* x, int64_t n, int kind) {
  if (!x) return fail(nullptr, IA2P_ERR_INVALID, "sam_act: null argument");
  if (n < 1 || (n + 255) / 256 > 0x7fffffffL || (kind != 0 && kind != 1)) return fail(nullptr, IA2P_ERR_SHAPE, "sam_act: n=%lld kind=%d (0 ReLU, 1 GELU)", (long long)n, kind);
  hipError_t e = ia2p_launch_sam_act((half_t*)x, (long)n, kind, (hipStream_t)stream);
  RET_HIP(e, "sam_act");
}
ia2p_status ia2p_sam_add_rows(void* stream, const void* a, const void* b, void* out, int64_t n, int64_t period) {
  if (!a || !b || !out) return fail(nullptr, IA2P_ERR_INVALID, "sam_add_rows: null argument");
  if (n < 8 || n % 8 || period < 8 || period % 8 || n % period || (n / 8 + 255) / 256 > 0x7fffffffL) return fail(nullptr, IA2P_ERR_SHAPE, "sam_add_rows: n=%lld period=%lld (multiples of 8, period dividing n)", (long long)n, (long long)period);
  hipError_t e = ia2p_launch_sam_add_rows((const half_t*)a, (const half_t*)b, (half_t*)out, (long)n, (long)period, (hipStream_t)stream);
  RET_HIP(e, "sam_add_rows");
}
ia2p_status ia2p_sam_take_col(void* stream, const void* src, int64_t ld, float* dst, int n) {
  if (!src || !dst) return fail(nullptr, IA2P_ERR_INVALID, "sam_take_col: null argument");
  if (n < 1 || ld < 1) return fail(nullptr, IA2P_ERR_SHAPE, "sam_take_col: n=%d ld=%lld", n, (long long)ld);
  hipError_t e = ia2p_launch_sam_take_col((const half_t*)src, (long)ld, dst, n, (hipStream_t)stream);
  RET_HIP(e, "sam_take_col");
}

}  // extern "C"
