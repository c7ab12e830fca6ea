// Host-side executor of one conditional-UNet evaluation + the ia2p_ctx C ABI (include/ia2p.h). The runtime it runs on is engine_rt.hip (shared with the other
// executors), the context-less per-operator entry points are ops_abi.hip: nothing outside this file needs anything defined in it.
//
// The module wiring follows diffusers' UNet2DConditionModel with the SDXL-base config, i.e. the object the
// reference calls at instructany2pix/ddim/pnp_pipeline.py:253-260 and ddim/sdxl_pipeline.py:832-839
// (SURVEY.md §3.4, Appendix A). All launches of a forward are issued from here on the caller's stream: ~1.2k
// launches per evaluation would be host-bound if driven op-by-op from Python.
//
// Memory: weights live in ONE flat fp16 arena whose layout depends only on the config (so data-parallel ranks
// can receive it with a single RCCL broadcast); activations come from a caller-provided workspace managed by a
// deterministic first-fit allocator (sized by a dry run of the same code path).
#include "engine_rt.h"

#include <dlfcn.h>
#include <rccl/rccl.h>      // types and prototypes only: the symbols are bound at run time (ia2p_bcast_arena), the library is not linked

struct Resnet {
  int cin, cout, temb_off;
  bool shortcut;
  size_t n1g, n1b, w1, b1, n2g, n2b, w2, b2, wsc, bsc;
  size_t wcat, bcat;      // derived at finalize when the block has a shortcut: [cout][9 cout + cin] = conv2 rows with the shortcut rows appended; b2 + bsc
};
struct TBlock {
  size_t ln1g, ln1b, wqkv, wo1, bo1, ln2g, ln2b, wq2, wkv2, wkvip, wo2, bo2, ln3g, ln3b, wff1, bff1, wff2, bff2;
  // LayerNorms folded into their consumers at finalize (fold_all): gamma-scaled weight copies + fp32 column sums / biases.
  // The raw tensors above stay as loaded, so finalize can be repeated and single tensors reloaded.
  size_t fqkv, fq2, fff1, cs1, lb1, cs2, lb2, cs3, lb3;
  int kv_col;   // column of this layer's [K | V] block in the batched context projection
};
struct Transformer {
  int c, heads;
  size_t ng, nb, win, bin, wout, bout;
  std::vector<TBlock> blocks;
};
struct Stage {            // one down/up block
  std::vector<Resnet> res;
  std::vector<Transformer> att;   // empty or same length as res
  bool resample;
  size_t rw, rb;
  int rc;
};

struct ia2p_ctx : RunCtx {
  ia2p_unet_config cfg;
  int ip_enabled = 0, ip_tokens = 4;
  float ip_scale = 1.0f;
  // plan
  size_t conv_in_w, conv_in_b, te1w, te1b, te2w, te2b, ae1w, ae1b, ae2w, ae2b, tw_all, tb_all, ngo, nbo, conv_out_w, conv_out_b;
  int temb_total = 0;
  size_t embed_lo = 0, embed_hi = 0;
  // context K/V projection weights of ALL cross-attention layers, stacked [kv_rows, ctx] (text) / (image tokens):
  // the context is the same for every layer, so one GEMM per step projects it for all of them
  size_t kv_text_base = 0, kv_ip_base = 0;
  int kv_rows = 0;
  std::vector<Stage> down, up;
  Resnet mid_r0, mid_r1;
  Transformer mid_t;
  int n_attn2 = 0;
  size_t arena_raw_elems = 0;   // head of the arena: everything a checkpoint provides; [arena_raw_elems, arena_elems) is derived at finalize
  int n_skips = 0;              // tensors the down path leaves for the up path: conv_in's output, every block's, every downsampler's
  // ---- ControlNet (ia2p_controlnet_*; diffusers 0.26.3 ControlNetModel): this context is the UNet's conv_in, embeddings, down path and mid block under a second set of
  //      weights -- no up path, no conv_norm_out / conv_out -- plus the condition embedding (eight 3x3 convolutions over the condition image) and one 1x1 "zero"
  //      convolution per skip and for the mid block's output
  bool cn = false;
  int ctx_drop = 0;             // trailing rows of every context that are not text: a ControlNet under an IP-Adapter pipe sees the text rows only (reference CNAttnProcessor2_0, attention_processor.py:530-531)
  int ce_in_ch = 3, ce_ch[4] = {16, 32, 96, 256};
  size_t ce_in_w = 0, ce_in_b = 0, ce_w[6] = {0}, ce_b[6] = {0}, ce_out_w = 0, ce_out_b = 0, zm_w = 0, zm_b = 0;
  std::vector<size_t> zc_w, zc_b;
};
// the context rows a cross-attention layer sees as text / as image tokens
static inline int ctx_li(const ia2p_ctx* c) { return c->ip_enabled ? c->ip_tokens : 0; }
static inline int ctx_lt(const ia2p_ctx* c, int L) { return L - ctx_li(c) - c->ctx_drop; }

// ---------------------------------------------------------------------------------------------------------------------
// plan: enumerate parameters in the diffusers key layout (same walk as instructany2pix_amd/weights.py)
// ---------------------------------------------------------------------------------------------------------------------
struct Planner {
  ia2p_ctx* c;
  size_t cur = 0;
  int kv_cursor = 0;
  // derived data (LayerNorm-folded weight copies, fp32 column sums / biases) goes to a TAIL region [fold_base, fold_base + fold_cur): the
  // head [0, fold_base) then holds exactly what a checkpoint provides, and a rank that receives only the head re-derives the tail itself
  size_t fold_base = 0, fold_cur = 0;
  size_t take(size_t elems) { size_t o = cur; cur += (elems + 127) & ~(size_t)127; return o; }
  size_t take_fold(size_t elems) { size_t o = fold_base + fold_cur; fold_cur += (elems + 127) & ~(size_t)127; return o; }
  void reg(const std::string& key, size_t off, size_t elems, int kind = PK_COPY, int d0 = 0, int d1 = 0, bool optional = false) {
    c->params[key] = Param{off, elems, kind, d0, d1, false, optional};
  }
  size_t vec(const std::string& key, int n) { size_t o = take(n); reg(key, o, n); return o; }
  size_t mat(const std::string& key, int rows, int cols) { size_t o = take((size_t)rows * cols); reg(key, o, (size_t)rows * cols); return o; }
  size_t conv3(const std::string& key, int co, int ci, PKind kind = PK_CONV) { size_t o = take((size_t)co * ci * 9); reg(key, o, (size_t)co * ci * 9, kind, co, ci); return o; }

  Resnet resnet(const std::string& p, int cin, int cout, int temb, size_t tw_all, size_t tb_all) {
    Resnet r;
    r.cin = cin; r.cout = cout; r.shortcut = cin != cout;
    r.n1g = vec(p + ".norm1.weight", cin); r.n1b = vec(p + ".norm1.bias", cin);
    r.w1 = conv3(p + ".conv1.weight", cout, cin); r.b1 = vec(p + ".conv1.bias", cout);
    r.temb_off = c->temb_total;
    reg(p + ".time_emb_proj.weight", tw_all + (size_t)r.temb_off * temb, (size_t)cout * temb);
    reg(p + ".time_emb_proj.bias", tb_all + r.temb_off, cout);
    c->temb_total += cout;
    r.n2g = vec(p + ".norm2.weight", cout); r.n2b = vec(p + ".norm2.bias", cout);
    r.w2 = conv3(p + ".conv2.weight", cout, cout); r.b2 = vec(p + ".conv2.bias", cout);
    r.wsc = r.bsc = 0;
    r.wcat = r.bcat = 0;
    if (r.shortcut) {
      r.wsc = mat(p + ".conv_shortcut.weight", cout, cin); r.bsc = vec(p + ".conv_shortcut.bias", cout);
      r.wcat = take_fold((size_t)cout * (9 * cout + cin)); r.bcat = take_fold(cout);
    }
    return r;
  }
  Transformer transformer(const std::string& p, int ch, int heads, int depth, int ctx, std::vector<std::pair<std::string, size_t>>& ipslots) {
    Transformer t;
    t.c = ch; t.heads = heads;
    t.ng = vec(p + ".norm.weight", ch); t.nb = vec(p + ".norm.bias", ch);
    t.win = mat(p + ".proj_in.weight", ch, ch); t.bin = vec(p + ".proj_in.bias", ch);
    for (int k = 0; k < depth; ++k) {
      const std::string q = p + ".transformer_blocks." + std::to_string(k);
      TBlock b;
      b.ln1g = vec(q + ".norm1.weight", ch); b.ln1b = vec(q + ".norm1.bias", ch);
      b.wqkv = take((size_t)3 * ch * ch);
      reg(q + ".attn1.to_q.weight", b.wqkv, (size_t)ch * ch);
      reg(q + ".attn1.to_k.weight", b.wqkv + (size_t)ch * ch, (size_t)ch * ch);
      reg(q + ".attn1.to_v.weight", b.wqkv + (size_t)2 * ch * ch, (size_t)ch * ch);
      b.wo1 = mat(q + ".attn1.to_out.0.weight", ch, ch); b.bo1 = vec(q + ".attn1.to_out.0.bias", ch);
      b.ln2g = vec(q + ".norm2.weight", ch); b.ln2b = vec(q + ".norm2.bias", ch);
      b.wq2 = mat(q + ".attn2.to_q.weight", ch, ch);
      b.kv_col = kv_cursor;
      b.wkv2 = c->kv_text_base + (size_t)kv_cursor * ctx;
      reg(q + ".attn2.to_k.weight", b.wkv2, (size_t)ch * ctx);
      reg(q + ".attn2.to_v.weight", b.wkv2 + (size_t)ch * ctx, (size_t)ch * ctx);
      b.wkvip = c->kv_ip_base + (size_t)kv_cursor * ctx;
      ipslots.push_back({q, b.wkvip});
      kv_cursor += 2 * ch;
      b.wo2 = mat(q + ".attn2.to_out.0.weight", ch, ch); b.bo2 = vec(q + ".attn2.to_out.0.bias", ch);
      b.ln3g = vec(q + ".norm3.weight", ch); b.ln3b = vec(q + ".norm3.bias", ch);
      b.wff1 = take((size_t)8 * ch * ch); reg(q + ".ff.net.0.proj.weight", b.wff1, (size_t)8 * ch * ch, PK_GEGLU_W, 8 * ch, ch);
      b.bff1 = take((size_t)8 * ch); reg(q + ".ff.net.0.proj.bias", b.bff1, (size_t)8 * ch, PK_GEGLU_B, 8 * ch, 1);
      b.wff2 = mat(q + ".ff.net.2.weight", ch, 4 * ch); b.bff2 = vec(q + ".ff.net.2.bias", ch);
      b.fqkv = take_fold((size_t)3 * ch * ch); b.fq2 = take_fold((size_t)ch * ch); b.fff1 = take_fold((size_t)8 * ch * ch);
      b.cs1 = take_fold((size_t)2 * 3 * ch); b.lb1 = take_fold((size_t)2 * 3 * ch);         // fp32 arrays: 2 half-slots per value
      b.cs2 = take_fold((size_t)2 * ch); b.lb2 = take_fold((size_t)2 * ch);
      b.cs3 = take_fold((size_t)2 * 8 * ch); b.lb3 = take_fold((size_t)2 * 8 * ch);
      t.blocks.push_back(b);
    }
    t.wout = mat(p + ".proj_out.weight", ch, ch); t.bout = vec(p + ".proj_out.bias", ch);
    return t;
  }
};

static ia2p_status plan_pass(ia2p_ctx* c, size_t fold_base, size_t* raw_elems, size_t* fold_elems) {
  c->params.clear(); c->down.clear(); c->up.clear();
  const ia2p_unet_config& g = c->cfg;
  const int n = g.n_blocks;
  if (n < 1 || n > IA2P_MAX_BLOCKS) return fail(c, IA2P_ERR_INVALID, "n_blocks %d out of range", n);
  for (int i = 0; i < n; ++i) {
    const int ch = g.block_out_channels[i];
    if (ch % 64 || ch % g.norm_num_groups) return fail(c, IA2P_ERR_SHAPE, "block_out_channels[%d]=%d must be a multiple of 64 and of norm_num_groups", i, ch);
    if (g.transformer_layers_per_block[i] > 0 && g.num_heads[i] * 64 != ch)
      return fail(c, IA2P_ERR_SHAPE, "block %d: heads*64 must equal channels (head_dim is fixed to 64)", i);
  }
  if (g.cross_attention_dim % 64 || g.time_embed_dim % 8 || g.projection_class_embeddings_input_dim % 8 || g.time_proj_dim % 8 || g.time_proj_dim % 2 || g.addition_time_embed_dim % 2)
    return fail(c, IA2P_ERR_SHAPE, "embedding / context dims violate the 8/64 divisibility rules");
  if (g.in_channels * 9 > 64 || g.out_channels > 8) return fail(c, IA2P_ERR_SHAPE, "latent channels too large for the boundary convolutions");
  if (c->cfg.num_time_ids <= 0) c->cfg.num_time_ids = 6;
  if (c->cfg.mid_transformer_layers < 0) c->cfg.mid_transformer_layers = g.transformer_layers_per_block[n - 1];
  if (g.num_time_ids > 8) return fail(c, IA2P_ERR_SHAPE, "num_time_ids %d out of range", g.num_time_ids);
  if (g.mid_transformer_layers < 1 || g.num_heads[n - 1] * 64 != g.block_out_channels[n - 1])
    return fail(c, IA2P_ERR_SHAPE, "mid block: needs >= 1 transformer layer and heads*64 == channels");
  const int pooled = g.projection_class_embeddings_input_dim - g.num_time_ids * g.addition_time_embed_dim;
  if (pooled <= 0) return fail(c, IA2P_ERR_SHAPE, "projection_class_embeddings_input_dim smaller than the time ids");

  Planner P{c};
  P.fold_base = fold_base;
  const int T = g.time_embed_dim, ctx = g.cross_attention_dim;
  const int* ch = g.block_out_channels;
  c->conv_in_w = P.take((size_t)ch[0] * 64); P.reg("conv_in.weight", c->conv_in_w, (size_t)ch[0] * g.in_channels * 9, PK_PAD_CONV_IN, ch[0], g.in_channels * 9);
  c->conv_in_b = P.vec("conv_in.bias", ch[0]);
  c->te1w = P.mat("time_embedding.linear_1.weight", T, g.time_proj_dim); c->te1b = P.vec("time_embedding.linear_1.bias", T);
  c->te2w = P.mat("time_embedding.linear_2.weight", T, T); c->te2b = P.vec("time_embedding.linear_2.bias", T);
  c->ae1w = P.mat("add_embedding.linear_1.weight", T, g.projection_class_embeddings_input_dim); c->ae1b = P.vec("add_embedding.linear_1.bias", T);
  c->ae2w = P.mat("add_embedding.linear_2.weight", T, T); c->ae2b = P.vec("add_embedding.linear_2.bias", T);
  // all time_emb_proj matrices stacked into one [sum Cout, T] projection
  int tot = 2 * ch[n - 1];
  for (int i = 0; i < n; ++i) tot += g.layers_per_block * ch[i] + (c->cn ? 0 : (g.layers_per_block + 1) * ch[n - 1 - i]);
  c->tw_all = P.take((size_t)tot * T);
  c->tb_all = P.take(tot);
  c->embed_lo = c->te1w; c->embed_hi = P.cur;      // [time/add embedding MLPs | stacked time_emb_proj]: the first weights a pass reads
  c->temb_total = 0;
  {
    int rows = 0;
    for (int i = 0; i < n; ++i) rows += g.layers_per_block * g.transformer_layers_per_block[i] * 2 * ch[i];          // down
    rows += g.mid_transformer_layers * 2 * ch[n - 1];                                                               // mid
    for (int i = 0; i < n && !c->cn; ++i) rows += (g.layers_per_block + 1) * g.transformer_layers_per_block[n - 1 - i] * 2 * ch[n - 1 - i];   // up
    c->kv_rows = rows;
    c->kv_text_base = P.take((size_t)rows * ctx);
    c->kv_ip_base = c->cn ? c->kv_text_base : P.take((size_t)rows * ctx);      // (a ControlNet carries no IP-Adapter: its image-token slots are never registered nor read)
  }

  std::vector<std::pair<std::string, size_t>> ipslots_down, ipslots_up, ipslots_mid;
  std::vector<int> skip_ch;
  skip_ch.push_back(ch[0]);
  int cprev = ch[0];
  for (int i = 0; i < n; ++i) {
    Stage st;
    const std::string bp = "down_blocks." + std::to_string(i);
    for (int j = 0; j < g.layers_per_block; ++j) {
      st.res.push_back(P.resnet(bp + ".resnets." + std::to_string(j), j == 0 ? cprev : ch[i], ch[i], T, c->tw_all, c->tb_all));
      if (g.transformer_layers_per_block[i] > 0)
        st.att.push_back(P.transformer(bp + ".attentions." + std::to_string(j), ch[i], g.num_heads[i], g.transformer_layers_per_block[i], ctx, ipslots_down));
      skip_ch.push_back(ch[i]);
    }
    cprev = ch[i];
    st.resample = i != n - 1;
    st.rc = ch[i];
    if (st.resample) {
      st.rw = P.conv3(bp + ".downsamplers.0.conv.weight", ch[i], ch[i]); st.rb = P.vec(bp + ".downsamplers.0.conv.bias", ch[i]);
      skip_ch.push_back(ch[i]);
    }
    c->down.push_back(st);
  }
  const int cm = ch[n - 1];
  c->mid_r0 = P.resnet("mid_block.resnets.0", cm, cm, T, c->tw_all, c->tb_all);
  c->mid_t = P.transformer("mid_block.attentions.0", cm, g.num_heads[n - 1], g.mid_transformer_layers, ctx, ipslots_mid);
  c->mid_r1 = P.resnet("mid_block.resnets.1", cm, cm, T, c->tw_all, c->tb_all);
  cprev = cm;
  c->n_skips = (int)skip_ch.size();
  for (int i = 0; i < n && !c->cn; ++i) {
    Stage st;
    const int co = ch[n - 1 - i];
    const std::string bp = "up_blocks." + std::to_string(i);
    for (int j = 0; j < g.layers_per_block + 1; ++j) {
      const int cs = skip_ch.back(); skip_ch.pop_back();
      st.res.push_back(P.resnet(bp + ".resnets." + std::to_string(j), (j == 0 ? cprev : co) + cs, co, T, c->tw_all, c->tb_all));
      if (g.transformer_layers_per_block[n - 1 - i] > 0)
        st.att.push_back(P.transformer(bp + ".attentions." + std::to_string(j), co, g.num_heads[n - 1 - i], g.transformer_layers_per_block[n - 1 - i], ctx, ipslots_up));
    }
    cprev = co;
    st.resample = i != n - 1;
    st.rc = co;
    if (st.resample) { st.rw = P.conv3(bp + ".upsamplers.0.conv.weight", co, co); st.rb = P.vec(bp + ".upsamplers.0.conv.bias", co); }
    c->up.push_back(st);
  }
  if (c->temb_total != tot) return fail(c, IA2P_ERR_STATE, "internal: time_emb_proj stacking mismatch %d != %d", c->temb_total, tot);
  if (P.kv_cursor != c->kv_rows) return fail(c, IA2P_ERR_STATE, "internal: context K/V stacking mismatch %d != %d", P.kv_cursor, c->kv_rows);
  if (c->cn) {
    // condition embedding (ControlNetConditioningEmbedding): conv_in, blocks.{0..5} (pairs: same width stride 1, next width stride 2), conv_out -- all 3x3, pad 1
    const std::string ep = "controlnet_cond_embedding.";
    c->ce_in_w = P.take((size_t)c->ce_ch[0] * 64); P.reg(ep + "conv_in.weight", c->ce_in_w, (size_t)c->ce_ch[0] * c->ce_in_ch * 9, PK_PAD_CONV_IN, c->ce_ch[0], c->ce_in_ch * 9);
    c->ce_in_b = P.vec(ep + "conv_in.bias", c->ce_ch[0]);
    for (int i = 0; i < 3; ++i) {
      c->ce_w[2 * i] = P.conv3(ep + "blocks." + std::to_string(2 * i) + ".weight", c->ce_ch[i], c->ce_ch[i], PK_CONV_TAP); c->ce_b[2 * i] = P.vec(ep + "blocks." + std::to_string(2 * i) + ".bias", c->ce_ch[i]);
      c->ce_w[2 * i + 1] = P.conv3(ep + "blocks." + std::to_string(2 * i + 1) + ".weight", c->ce_ch[i + 1], c->ce_ch[i], PK_CONV_TAP); c->ce_b[2 * i + 1] = P.vec(ep + "blocks." + std::to_string(2 * i + 1) + ".bias", c->ce_ch[i + 1]);
    }
    c->ce_out_w = P.conv3(ep + "conv_out.weight", ch[0], c->ce_ch[3], PK_CONV_TAP); c->ce_out_b = P.vec(ep + "conv_out.bias", ch[0]);
    // zero convolutions: 1x1, one per skip in skip order, one for the mid block's output ([C, C, 1, 1] in the checkpoint = the GEMM's [N, K])
    c->zc_w.clear(); c->zc_b.clear();
    for (size_t k = 0; k < skip_ch.size(); ++k) {
      const std::string zp = "controlnet_down_blocks." + std::to_string(k);
      c->zc_w.push_back(P.mat(zp + ".weight", skip_ch[k], skip_ch[k])); c->zc_b.push_back(P.vec(zp + ".bias", skip_ch[k]));
    }
    c->zm_w = P.mat("controlnet_mid_block.weight", cm, cm); c->zm_b = P.vec("controlnet_mid_block.bias", cm);
    *raw_elems = P.cur; *fold_elems = P.fold_cur;
    return IA2P_OK;
  }
  c->ngo = P.vec("conv_norm_out.weight", ch[0]); c->nbo = P.vec("conv_norm_out.bias", ch[0]);
  c->conv_out_w = P.conv3("conv_out.weight", g.out_channels, ch[0], PK_CONV_TAP); c->conv_out_b = P.vec("conv_out.bias", g.out_channels);

  // IP-Adapter keys: index = position in unet.attn_processors = down, up, mid (attn1 even, attn2 odd)
  int idx = 0;
  auto add_ip = [&](std::vector<std::pair<std::string, size_t>>& v) {
    for (auto& s : v) {
      const std::string& q = s.first;
      // channel count from the attn2.to_q registration
      const size_t cc = (size_t)std::llround(std::sqrt((double)c->params[q + ".attn2.to_q.weight"].elems));
      const std::string k = "ip_adapter." + std::to_string(2 * idx + 1);
      P.reg(k + ".to_k_ip.weight", s.second, cc * ctx, PK_COPY, 0, 0, true);
      P.reg(k + ".to_v_ip.weight", s.second + cc * ctx, cc * ctx, PK_COPY, 0, 0, true);
      ++idx;
    }
  };
  add_ip(ipslots_down); add_ip(ipslots_up); add_ip(ipslots_mid);
  c->n_attn2 = idx;
  *raw_elems = P.cur; *fold_elems = P.fold_cur;
  return IA2P_OK;
}
// two passes of the same deterministic walk: the first measures the head (checkpoint data), the second places the derived tail behind it
static ia2p_status build_plan(ia2p_ctx* c) {
  size_t raw = 0, fold = 0;
  ia2p_status st = plan_pass(c, 0, &raw, &fold);
  if (st != IA2P_OK) return st;
  st = plan_pass(c, raw, &raw, &fold);
  if (st != IA2P_OK) return st;
  c->arena_raw_elems = raw;
  c->arena_elems = raw + fold;
  return IA2P_OK;
}

// GEGLU feed-forward: ff.net.0 (a: K = C, N = 8 C packed, GEGLU epilogue -> H [M, 4 C]) then ff.net.2 (b: reads H, + bias + residual): two launches.
// (One launch with a per-row-panel hand-off between the two was built and measured in round 3: +0.45 ... +0.8 ms per step, docs/LOG.md; removed in round 4.)
static void run_ffn(RunCtx* c, GemmArgs& a, GemmArgs& b, int* stat_slots_b) {
  set_prefetch(c, a, a.W, (size_t)a.N * a.K * sizeof(half_t));
  set_prefetch(c, b, b.W, (size_t)b.N * b.K * sizeof(half_t));
  { RoleScope role(c, ROLE_FF_IN); run_gemm(c, a, false, "ff.net.0", 2.0 * a.M * (double)a.N * a.K, gemm_bytes(a.M, a.N, a.K, 1, false)); }
  RoleScope role(c, ROLE_FF_OUT);
  RunOpt r; r.stat_slots = stat_slots_b;
  run_gemm(c, b, false, "ff.net.2", 2.0 * b.M * (double)b.N * b.K, gemm_bytes(b.M, b.N, b.K, 0, true), r);
}

struct Fwd {
  ia2p_ctx* c;
  int B, h, w, L;
  const half_t* ctxp;
  T2 temb_all;
  float* gn_partial;
  T2 kv_text, kv_ip;   // [B*Lt, kv_rows], [B*Li, kv_rows]
  const float* ip_scales = nullptr;   // device [B] or null: per-request IP-Adapter scale (else the context's one value)
  // GroupNorm statistics of live activation tensors (keyed by workspace offset): left by the producer's epilogue, read by the GroupNorm-fused convolution that consumes
  // the tensor -- possibly much later (the skips of the down path) --, released with the tensor
  std::unordered_map<size_t, GnStats> gst;
  int gn_mode = 0;             // GroupNorm mode of this pass (run_forward): 0 launches, 1 fused into the convolutions, 2 the fused path's unfused twin, 3 the autotune pass's sizing
  bool gn_on = false;
  std::unordered_map<int, int> kv_inlaunch;      // context K/V column (TBlock::kv_col) -> 1: left for the block's fused QKV + self-attention launch to project (plan_context_kv); 2: done
  bool tune_like = false;      // the autotune pass (or the dry pass that sizes the workspace for it): GroupNorm launches, plus what tune_site needs to time the fused forms beside them
  // regional image prompts (ia2p_unet_forward_r): G token groups and the per-query weights [B, G, HW] of every distinct attention resolution (region_levels),
  // built once per forward at the front of the workspace
  int G = 0, n_rlev = 0;
  struct { int HW; T2 w; } rlev[IA2P_MAX_BLOCKS + 1];
};
static void gst_put(Fwd& f, T2 t, const GnStats& s) { if (s.ok() && t.off != (size_t)-1) f.gst[t.off] = s; else if (s.buf.off != (size_t)-1) wsfree(f.c, s.buf); }
static GnStats gst_get(Fwd& f, T2 t) { auto it = f.gst.find(t.off); return it == f.gst.end() ? GnStats{} : it->second; }
static void act_free(Fwd& f, T2 t) {      // release an activation tensor and its statistics
  auto it = f.gst.find(t.off);
  if (it != f.gst.end()) { wsfree(f.c, it->second.buf); f.gst.erase(it); }
  wsfree(f.c, t);
}

// autotune pass: times a GroupNorm launch in place, for the tune_site call of the convolution behind it (ConvGn::gn_ms)
struct TuneGnTimer {
  RunCtx* c; hipEvent_t e0{}, e1{}; bool on;
  explicit TuneGnTimer(RunCtx* c_) : c(c_), on(c_->tuning && !c_->dry && !c_->failed && c_->gn_fuse != 0) {
    if (on) { e0 = get_event(c); e1 = get_event(c); (void)hipEventRecord(e0, c->stream); }
  }
  float stop() {      // ms; 0: not timed
    if (!on) return 0.f;
    float ms = 0.f;
    if (!(hipEventRecord(e1, c->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess)) ms = 0.f;
    c->evpool.push_back(e0); c->evpool.push_back(e1);
    on = false;
    return ms;
  }
};
struct RegionScope { RunCtx* c; int prev; RegionScope(RunCtx* c_, int r) : c(c_), prev(c_->region) { c->region = r; } ~RegionScope() { c->region = prev; } };

// x2 != null: the block input is [x (cx channels) | x2 (cin - cx channels)], never concatenated (up path: hidden state | skip) -- GroupNorm reads the two
// tensors, and the shortcut rides in conv2 as two appended K-blocks. Only with the fused shortcut (c->sc_fuse); the caller concatenates otherwise.
// may the GroupNorm in front of a stride-1 3x3 convolution of `cin` -> `cout` channels (+ cin2 + cin3 appended 1x1 channels) run inside that convolution? The shape part:
// the plan table gives the site a halo-staged tile; the statistics part: every source has its producer's column sums, at most IA2P_GN_MAX_SLOTS slots per image
static bool gn_conv_fusable(Fwd& f, int H, int Wd, int cin, int cout, int cin2, int cin3, const GnStats& s0, const GnStats* s1, int c0) {
  if (!f.gn_on || !s0.ok() || (s1 && !s1->ok())) return false;
  const half_t* const any = (const half_t*)16;      // (shape query: any non-null pointer for the appended blocks)
  GemmArgs a = conv3_desc(nullptr, nullptr, f.B, H, Wd, cin, nullptr, nullptr, cout, 1, 0, 1, nullptr, 0, nullptr, nullptr, cin2 ? any : nullptr, cin2, cin3 ? any : nullptr, cin3);
  a.lda = c0;
  const GemmPlan pl = ia2p_gemm_plan(a.M, a.N, a.K, true, false);
  if (!pl.gn || !ia2p_conv_gn_fusable(a, pl.variant, pl.splitk)) return false;      // (the measured plan of the site says whether fusing pays there: tune_site)
  const int HW = H * Wd, groups = f.c->groups;
  if (cin % groups || cin / groups > 96 || c0 % 64 || (cin - c0) % 64 || cin > 3072) return false;
  return HW % s0.rows == 0 && HW / s0.rows <= IA2P_GN_MAX_SLOTS && (!s1 || (HW % s1->rows == 0 && HW / s1->rows <= IA2P_GN_MAX_SLOTS));
}

// statistics of tensor t ([B*HW, C]) for a consumer that is going to fuse: what its producer's epilogue left, or -- when the producer's tile could not (or left more than
// IA2P_GN_MAX_SLOTS slots per image) -- the canonical pass over the tensor, run once and kept with it (conv_in's output feeds two such consumers)
static GnStats gn_ensure_stats(Fwd& f, T2 t, int C, int HW) {
  GnStats s = gst_get(f, t);
  if (s.ok() && HW % s.rows == 0 && HW / s.rows <= IA2P_GN_MAX_SLOTS) return s;
  RunCtx* c = f.c;
  const int rows = gn_fallback_rows(HW);
  if (!rows || C % 8) return GnStats{};
  auto it = f.gst.find(t.off);
  if (it != f.gst.end()) { wsfree(c, it->second.buf); f.gst.erase(it); }
  s = GnStats{};
  s.buf = wsalloc(c, (size_t)(f.B * HW / rows) * C * 8);
  s.rows = rows;
  {
    RoleScope role(c, ROLE_GROUPNORM);
    ProfScope ps(c, PK_GN, 4.0 * f.B * HW * C, 2.0 * f.B * HW * C);
    CHECK_LAUNCH(c, ia2p_launch_gn_colstats(t.p, C, f.B * HW, C, rows, (double*)s.buf.p, c->stream), "groupnorm statistics");
  }
  f.gst[t.off] = s;
  return s;
}

// GroupNorm + SiLU over [x (c0 channels) | x2 (C - c0)] in front of a 3x3 convolution of a ResnetBlock2D, one of three ways: inside the convolution (`fusable`: the site is a
// halo-staged one and g.s0 / g.s1 hold the producers' statistics); as the fused path's unfused twin (gn_mode 2: the SAME statistics, normalised by a pass of its own, then the
// plain convolution); or as a GroupNorm launch. The autotune pass (`tune`; tune_like implies !gn_on, so only ever beside a GroupNorm launch) measures the site both ways: the
// launch is timed, and g describes the fused form -- raw tensor(s) with their statistics -- for tune_site. Fills g for op_conv3 and returns the normalised tensor the
// convolution reads (none when fused: it reads x). stats_first: whether the autotune pass's statistics are allocated before the normalised tensor or behind it -- the
// workspace is first-fit, the order of allocations decides ia2p_workspace_bytes, and the two convolutions of a block have always differed in it.
static T2 gn_before_conv(Fwd& f, T2 x, const T2* x2t, int c0, int C, size_t gam, size_t bet, int HW, bool fusable, bool tune, bool stats_first, ConvGn& g) {
  ia2p_ctx* c = f.c;
  const int M = f.B * HW;
  const half_t* x2 = x2t ? x2t->p : nullptr;
  g.X1b = x2; g.C0 = c0; g.gamma = W_(c, gam); g.beta = W_(c, bet); g.eps = c->cfg.norm_eps; g.groups = c->groups;
  g.fused = fusable && f.gn_mode != 2;
  if (g.fused) return T2{(size_t)-1, nullptr};
  tune = tune && !fusable;
  auto tune_stats = [&] { g.tune = true; g.Xraw = x.p; g.s0 = gn_ensure_stats(f, x, c0, HW); if (x2t) g.s1 = gn_ensure_stats(f, *x2t, C - c0, HW); };
  if (tune && stats_first) tune_stats();
  T2 n = wsalloc(c, (size_t)M * C);
  if (tune && !stats_first) tune_stats();
  if (fusable) {
    const GemmArgs::GnIn gi = gn_in_desc((const double*)g.s0.buf.p, g.s0.rows, x2 ? (const double*)g.s1.buf.p : nullptr, g.s1.rows, c0, C, g.gamma, g.beta, g.groups, g.eps, 1);
    RoleScope role(c, ROLE_GROUPNORM);
    ProfScope ps(c, PK_GN, 8.0 * M * C, 4.0 * M * C);
    CHECK_LAUNCH(c, ia2p_launch_gn_apply_stats(x.p, c0, x2, C - c0, n.p, C, f.B, HW, C, gi, c->stream), "groupnorm (apply from producer statistics)");
  } else {
    TuneGnTimer tg(c);
    op_gn(c, x.p, n.p, gam, bet, f.B, HW, C, g.eps, 1, f.gn_partial, x2, c0);
    g.gn_ms = tg.stop();
  }
  return n;
}

// out_stats: the block's output feeds another GroupNorm-fusable convolution (the next ResnetBlock2D, or -- as a skip -- one of the up path): its statistics are taken
static T2 run_resnet(Fwd& f, const Resnet& r, T2 x, int H, int Wd, const T2* x2t = nullptr, int cx = 0, bool out_stats = false) {
  const half_t* x2 = x2t ? x2t->p : nullptr;
  const bool two = x2t != nullptr;
  ia2p_ctx* c = f.c;
  RegionScope rs(c, PR_CONV_BLOCK);
  const int HW = H * Wd, M = f.B * HW, c0 = two ? cx : r.cin;
  // norm1 + SiLU + conv1: inside the convolution when the site is a halo-staged one and the producers left their statistics (conv_halo_kernel.h, GN = 1)
  // (first by shape alone -- does the plan give conv1 a halo-staged tile? -- then with the statistics, fetched or computed only when the site can use them)
  GnStats probe; probe.rows = gn_fallback_rows(HW);
  ConvGn g1, g2;
  bool fuse1 = probe.ok() && gn_conv_fusable(f, H, Wd, r.cin, r.cout, 0, 0, probe, two ? &probe : nullptr, c0);
  if (fuse1) {
    g1.s0 = gn_ensure_stats(f, x, c0, HW);
    if (two) g1.s1 = gn_ensure_stats(f, *x2t, r.cin - cx, HW);
    fuse1 = gn_conv_fusable(f, H, Wd, r.cin, r.cout, 0, 0, g1.s0, two ? &g1.s1 : nullptr, c0);
  }
  GnWant w1{HW};
  const bool cat = r.shortcut && c->sc_fuse;      // conv2(h) + conv_shortcut(x) as ONE implicit GEMM (K = 9 cout + cin): no shortcut launch, no xs round trip
  const int cat2 = cat ? c0 : 0, cat3 = cat && two ? r.cin - cx : 0;      // ... its appended 1x1 blocks: x [| x2]
  // (conv1's statistics are wanted when conv2 can take them: its plan is a halo-staged one)
  const bool want1 = f.gn_on && probe.ok() && gn_conv_fusable(f, H, Wd, r.cout, r.cout, cat2, cat3, probe, nullptr, r.cout);
  // autotune pass: both convolutions are measured both ways -- GroupNorm launch + the best plain plan against the fused launch on the raw tensor(s) with their statistics
  const bool tune = f.tune_like && probe.ok() && H % 16 == 0 && Wd % 16 == 0;
  T2 hh = wsalloc(c, (size_t)M * r.cout);
  T2 n1 = gn_before_conv(f, x, x2t, c0, r.cin, r.n1g, r.n1b, HW, fuse1, tune, false, g1);
  ConvOpt o1;
  o1.rowvec = c->dry ? nullptr : f.temb_all.p + r.temb_off; o1.rowvec_ld = c->temb_total;
  o1.gn = &g1; o1.gw = want1 ? &w1 : nullptr;
  op_conv3(c, g1.fused ? x.p : n1.p, f.B, H, Wd, r.cin, W_(c, r.w1), W_(c, r.b1), r.cout, hh.p, o1);
  wsfree(c, n1);
  // norm2 + SiLU + conv2, the same three ways, on the statistics conv1's epilogue left
  g2.s0 = w1.out;
  const bool fuse2 = want1 && gn_conv_fusable(f, H, Wd, r.cout, r.cout, cat2, cat3, g2.s0, nullptr, r.cout);
  T2 n2 = gn_before_conv(f, hh, nullptr, r.cout, r.cout, r.n2g, r.n2b, HW, fuse2, tune, true, g2);
  if (!g2.fused && !tune) wsfree(c, hh);      // (autotune pass: hh stays alive, the fused candidates read it)
  GnWant w2{HW};
  ConvOpt o2;
  o2.gn = &g2;
  o2.gw = f.gn_on && out_stats && ia2p_plan_any_gn(M) ? &w2 : nullptr;      // (only when some 3x3 site of this resolution level fuses its GroupNorm under the measured plans)
  T2 xs{(size_t)-1, nullptr};
  const half_t* resid = x.p;
  if (r.shortcut && !cat) {
    xs = wsalloc(c, (size_t)M * r.cout);
    { RoleScope role(c, ROLE_CONV3X3); op_gemm(c, x.p, r.cin, W_(c, r.wsc), W_(c, r.bsc), nullptr, 0, xs.p, r.cout, M, r.cout, r.cin); }
    resid = xs.p;
  }
  T2 out = wsalloc(c, (size_t)M * r.cout);
  if (cat) { o2.X2 = x.p; o2.Cin2 = cat2; o2.X3 = x2; o2.Cin3 = cat3; }
  else o2.residual = c->dry ? nullptr : resid;
  op_conv3(c, g2.fused ? hh.p : n2.p, f.B, H, Wd, r.cout, W_(c, cat ? r.wcat : r.w2), W_(c, cat ? r.bcat : r.b2), r.cout, out.p, o2);
  if (g2.fused) wsfree(c, hh); else { wsfree(c, n2); if (tune) act_free(f, hh); }
  if (w1.out.buf.off != (size_t)-1) wsfree(c, w1.out.buf);
  if (r.shortcut && !cat) wsfree(c, xs);
  if (o2.gw) gst_put(f, out, w2.out);
  return out;
}

// QKV projection (LayerNorm folded) + the self-attention that consumes it in ONE launch (qxattn.hip): Q, K, V never leave the CU. x: O / ldo / B / heads / Nq = 256
// ck != nullptr: the launch also projects the layer's context K / V on the CUs its (image, head) tiles leave empty (CtxKvSlice; the caller asked ia2p_qkv_sattn_ctx_ok)
static void op_qkv_sattn(RunCtx* c, const half_t* A, int lda, const half_t* W, const LnIn* ln, int M, int C, const AttnArgs& x, const CtxKvSlice* ck = nullptr) {
  GemmArgs a = qkv_desc(zero_page(), A, lda, W, nullptr, M, 3 * C, C);
  ln_attach(a, ln);
  set_prefetch(c, a, W, (size_t)3 * C * C * sizeof(half_t));
  RoleScope role(c, ROLE_QKV_SATTN);
#ifdef IA2P_CLOCK_STAMP
  if (c->stamp_buf && c->role == c->stamp_role && !c->dry && !c->tuning && c->stamp_n < c->stamp_cap && x.B * x.heads <= RunCtx::STAMP_WG) {
    a.partial = (float*)(c->stamp_buf + (size_t)c->stamp_n * RunCtx::STAMP_WG * 8);
    c->stamp_meta.push_back({a.M, a.N, a.K, -4, x.B * x.heads});      // (variant -4: the fused QKV + self-attention tile)
    ++c->stamp_n;
  }
#endif
  const double ck_rows = ck ? (double)ck->B * ck->L : 0.0;      // (the slices' work is booked with the launch that carries it: the role's TFLOP/s stays what the launch did)
  ProfScope ps(c, PK_QKVATTN, 2.0 * M * 3.0 * C * C + 4.0 * x.B * x.heads * (double)x.Nq * x.Nq * 64 + (ck ? 2.0 * ck_rows * ck->N * ck->K : 0.0),
               2.0 * ((double)M * C + 3.0 * C * C + (double)M * C) + (ck ? 2.0 * (ck_rows * ck->K + (ck->Li > 0 ? 2.0 : 1.0) * ck->N * ck->K + ck_rows * ck->N) : 0.0));
  ps.pf = a.pf ? (double)a.pf_bytes : 0.0;
  CHECK_LAUNCH(c, ia2p_launch_qkv_sattn(a, x, c->stream, ck), "qkv projection + self-attention");
}

// cross-attention with G image-token groups, each under its own per-query weight (attention_regions.hip)
static void op_attn_regions(RunCtx* c, const AttnArgs& a, const half_t* region_w, int G) {
  const double keys = a.seg[0].nkeys + a.seg[1].nkeys;
  ProfScope ps(c, PK_ATTN, 4.0 * a.B * a.heads * (double)a.Nq * keys * 64, 2.0 * ((double)a.B * a.Nq * a.heads * 64 * 2 + 2.0 * a.B * keys * a.heads * 64 + (double)a.B * G * a.Nq));
  CHECK_LAUNCH(c, ia2p_launch_attention_regions(a, region_w, G, c->stream), "regional cross-attention");
}

static void op_attn(RunCtx* c, const AttnArgs& a) {
  double keys = 0;
  for (int s = 0; s < a.nseg; ++s) keys += a.seg[s].nkeys;
  ProfScope ps(c, PK_ATTN, 4.0 * a.B * a.heads * (double)a.Nq * keys * 64, 2.0 * ((double)a.B * a.Nq * a.heads * 64 * 2 + 2.0 * a.B * keys * a.heads * 64));
  CHECK_LAUNCH(c, ia2p_launch_attention(a, c->stream), "attention");
}

// to_q projection + the cross-attention that consumes it in ONE launch (qxattn.hip); Q never leaves the CU
static void op_qxattn(RunCtx* c, const half_t* A, int lda, const half_t* W, const LnIn* ln, int M, int N, int K, const AttnArgs& x) {
  GemmArgs a = gemm_desc(zero_page(), A, lda, W, K, nullptr, nullptr, 0, nullptr, N, M, N, K);
  ln_attach(a, ln);
  set_prefetch(c, a, W, (size_t)N * K * sizeof(half_t));
  double keys = 0;
  for (int s = 0; s < x.nseg; ++s) keys += x.seg[s].nkeys;
  RoleScope role(c, ROLE_Q_XATTN);
#ifdef IA2P_CLOCK_STAMP
  if (c->stamp_buf && c->role == c->stamp_role && !c->dry && !c->tuning && c->stamp_n < c->stamp_cap && (M / 128) * (N / 64) <= RunCtx::STAMP_WG) {
    a.partial = (float*)(c->stamp_buf + (size_t)c->stamp_n * RunCtx::STAMP_WG * 8);
    c->stamp_meta.push_back({a.M, a.N, a.K, -5, (M / 128) * (N / 64)});      // (variant -5: the fused to_q + cross-attention tile, 128 x 64)
    ++c->stamp_n;
  }
#endif
  ProfScope ps(c, PK_QXATTN, 2.0 * M * N * K + 4.0 * x.B * x.heads * (double)x.Nq * keys * 64,
               2.0 * ((double)M * K + (double)N * K + (double)M * N + 2.0 * x.B * keys * x.heads * 64));
  CHECK_LAUNCH(c, ia2p_launch_qproj_xattn(a, x, c->stream), "to_q + cross-attention");
}

// context K/V of every cross-attention layer in one GEMM each (text rows / image-token rows of ctx); per layer: reference
// attention_processor.py:358-359 (to_k/to_v) and :379-380 (to_k_ip/to_v_ip). kv_text: [B*Lt, kv_rows], kv_ip: [B*Li, kv_rows].
// [col0, col0 + ncols): the layers whose columns are projected (ncols < 0: all). A column range runs on the plan of the whole projection -- same tile, same K split,
// hence the same bits whichever way the columns are cut (and no plan-table entries of its own).
static void project_context(ia2p_ctx* c, const half_t* context, int L, int B, half_t* kv_text, half_t* kv_ip, int col0 = 0, int ncols = -1) {
  RegionScope rs(c, PR_TRANSFORMER);
  RoleScope role(c, ROLE_CTX_KV);
  const int ctxd = c->cfg.cross_attention_dim;
  const int Lt = ctx_lt(c, L), Li = ctx_li(c);
  if (ncols < 0) ncols = c->kv_rows - col0;
  GemmOpt o;      // rows of the text / image tokens of every batch element; a column range on the whole projection's plan
  o.rpb = Lt; o.bstride = L; o.roff = 0; o.plan_n = ncols != c->kv_rows ? c->kv_rows : 0;
  op_gemm(c, context, ctxd, W_(c, c->kv_text_base + (size_t)col0 * ctxd), nullptr, nullptr, 0, kv_text ? kv_text + col0 : nullptr, c->kv_rows, B * Lt, ncols, ctxd, o);
  o.rpb = Li; o.roff = Lt;
  if (Li) op_gemm(c, context, ctxd, W_(c, c->kv_ip_base + (size_t)col0 * ctxd), nullptr, nullptr, 0, kv_ip ? kv_ip + col0 : nullptr, c->kv_rows, B * Li, ncols, ctxd, o);
}

// does transformer block b of t, at HW tokens per image, take the fused QKV + self-attention launch? (workspace and arena offsets are 256-byte aligned: the dry pass, with
// null pointers, decides the same way)
static bool sattn_fusable(Fwd& f, const Transformer& t, const TBlock& b, int HW, const half_t* tk, const float* st, int slots, half_t* O) {
#ifdef IA2P_NO_SATTN_FUSE      // A/B builds: projection and self-attention as two launches everywhere
  return false;
#else
  ia2p_ctx* c = f.c;
  const int C = t.c, M = f.B * HW;
  if (!(c->ln_fold && c->sattn_fuse && HW == 256 && C == t.heads * 64 && (long)f.B * t.heads >= c->xattn_min_tiles)) return false;
  GemmArgs g = qkv_desc(nullptr, tk, C, W_(c, b.fqkv), nullptr, M, 3 * C, C);
  const LnIn ln{st, slots, (const float*)(c->arena + b.cs1), (const float*)(c->arena + b.lb1), 0.f};
  ln_attach(g, &ln);
  return ia2p_qkv_sattn_ok(g, sattn_desc(O, C, f.B, t.heads, HW));
#endif
}
// the slice of the context projection that belongs to block b (columns [kv_col, kv_col + 2C) of kv_text / kv_ip)
static CtxKvSlice ctx_kv_slice(Fwd& f, const Transformer& t, const TBlock& b) {
  ia2p_ctx* c = f.c;
  const int ctxd = c->cfg.cross_attention_dim;
  const int Li = ctx_li(c), Lt = ctx_lt(c, f.L);
  CtxKvSlice k;
  memset(&k, 0, sizeof k);
  k.ctx = f.ctxp; k.lda = ctxd; k.L = f.L; k.Lt = Lt; k.Li = Li; k.B = f.B;
  k.Wt = W_(c, b.wkv2); k.Wi = Li ? W_(c, b.wkvip) : nullptr;
  k.Ct = f.kv_text.p ? f.kv_text.p + b.kv_col : nullptr; k.Ci = (Li && f.kv_ip.p) ? f.kv_ip.p + b.kv_col : nullptr;
  k.ldc = c->kv_rows; k.N = 2 * t.c; k.K = ctxd;
  return k;
}
// Which blocks' context K/V does their own fused QKV + self-attention launch project? Those that take the fused launch (sattn_fusable) with room for the slice's tiles
// beside the (image, head) tiles (ia2p_qkv_sattn_ctx_ok) -- and only while the whole projection's plans run without a K split: the in-launch tiles do not split, and a
// split changes the order of the sums. Fills f.kv_inlaunch and returns the column ranges [first, second) left for the head of the step, merged where adjacent.
static std::vector<std::pair<int, int>> plan_context_kv(Fwd& f, int h, int w) {
  ia2p_ctx* c = f.c;
  std::vector<std::pair<int, int>> up_front;
  f.kv_inlaunch.clear();
  const int ctxd = c->cfg.cross_attention_dim;
  const int Li = ctx_li(c), Lt = ctx_lt(c, f.L);
  bool on = c->ctx_kv_inlaunch && !c->ctx_drop && ia2p_gemm_plan(f.B * Lt, c->kv_rows, ctxd, false, false).splitk <= 1 && (!Li || ia2p_gemm_plan(f.B * Li, c->kv_rows, ctxd, false, false).splitk <= 1);
  std::vector<std::pair<int, int>> cols;      // every block's {column, width}
  auto visit = [&](const Transformer& t, int HW) {
    for (const TBlock& b : t.blocks) {
      cols.push_back({b.kv_col, 2 * t.c});
      if (!on || !sattn_fusable(f, t, b, HW, nullptr, c->dry ? nullptr : (const float*)16, 1, nullptr)) continue;
      if (ia2p_qkv_sattn_ctx_ok(sattn_desc(nullptr, t.c, f.B, t.heads, HW), ctx_kv_slice(f, t, b))) f.kv_inlaunch[b.kv_col] = 1;
    }
  };
  int H = h, Wd = w;
  for (const Stage& st : c->down) {
    for (const Transformer& t : st.att) visit(t, H * Wd);
    if (st.resample) { H = (H - 1) / 2 + 1; Wd = (Wd - 1) / 2 + 1; }
  }
  visit(c->mid_t, H * Wd);
  for (const Stage& st : c->up) {
    for (const Transformer& t : st.att) visit(t, H * Wd);
    if (st.resample) { H *= 2; Wd *= 2; }
  }
  std::sort(cols.begin(), cols.end());
  for (const auto& cw : cols) {
    if (f.kv_inlaunch.count(cw.first)) continue;
    if (!up_front.empty() && up_front.back().second == cw.first) up_front.back().second = cw.first + cw.second;
    else up_front.push_back({cw.first, cw.first + cw.second});
  }
  return up_front;
}

static T2 run_transformer(Fwd& f, const Transformer& t, T2 x, int H, int Wd, bool out_stats = false) {
  ia2p_ctx* c = f.c;
  RegionScope rs(c, PR_TRANSFORMER);
  const int HW = H * Wd, M = f.B * HW, C = t.c;
  const int Lt = ctx_lt(c, f.L);
  const int Li = ctx_li(c);
  T2 n = wsalloc(c, (size_t)M * C);
  op_gn(c, x.p, n.p, t.ng, t.nb, f.B, HW, C, 1e-6f, 0, f.gn_partial);
  // The three LayerNorms of a block never run as kernels: every GEMM that writes the token stream `tk` also emits per-row
  // {sum, sum of squares} partials of its fp16 output (`st`), and the GEMM that consumes LN(tk) reads raw `tk` against the
  // gamma-folded weights and finishes the normalisation in its epilogue (LnIn; GemmArgs.ln_* in common.h).
  T2 tk = wsalloc(c, (size_t)M * C);
  T2 stt = wsalloc(c, (size_t)M * ((C + 63) / 64) * 2 * 2);                // float2 per row and slot (one slot per tile column, tiles >= 64 wide)
  float* st = (float*)stt.p;
  int slots = 0;
  const float eps = 1e-5f;
  auto F_ = [&](size_t off) { return (const float*)(c->arena + off); };
  const bool fold = c->ln_fold;
  if (!fold) st = nullptr;
  GemmOpt to_tk;      // a GEMM that writes the token stream leaves the row statistics of its output
  to_tk.stats = st; to_tk.stat_slots = &slots;
  auto folded = [](const LnIn& ln) { GemmOpt o; o.ln = &ln; return o; };      // a GEMM that reads LN(tk) as raw tk against the folded weights
  { RoleScope role(c, ROLE_PROJ_IO); op_gemm(c, n.p, C, W_(c, t.win), W_(c, t.bin), nullptr, 0, tk.p, C, M, C, C, to_tk); }
  wsfree(c, n);
  T2 lnb = fold ? T2{(size_t)-1, nullptr} : wsalloc(c, (size_t)M * C);
  T2 qkv = wsalloc(c, (size_t)M * 3 * C), att = wsalloc(c, (size_t)M * C);
  T2 ff = wsalloc(c, (size_t)M * 4 * C);
  const int ldkv = c->kv_rows;
  for (const TBlock& b : t.blocks) {
    // self-attention (AttnProcessor2_0, reference attention_processor.py:205-279)
    // 256 tokens per image (the 16 x 16 level): the QKV tile of one image x one head holds everything that head's attention needs -- projection and attention
    // as ONE launch when there are enough (image, head) pairs to fill the chip (same threshold and switch as the fused cross-attention)
    {
    RoleScope role_sa(c, ROLE_QKV_SATTN);
    // (a site the fused tile does not take -- alignment of O / the folded constants, the 31-bit operand limit -- runs projection + attention as two launches)
    const bool fuse_sa = sattn_fusable(f, t, b, HW, tk.p, st, slots, att.p);
    const AttnArgs sa = sattn_desc(att.p, C, f.B, t.heads, HW);
    // this block's context K / V: left to this launch by plan_context_kv, on the CUs the (image, head) tiles leave empty
    auto kvi = f.kv_inlaunch.find(b.kv_col);
    const bool kv_mine = kvi != f.kv_inlaunch.end() && kvi->second == 1;
    const CtxKvSlice ck = ctx_kv_slice(f, t, b);
    const bool kv_here = kv_mine && fuse_sa && ia2p_qkv_sattn_ctx_ok(sa, ck);
    if (kv_mine && !kv_here) project_context(c, f.ctxp, f.L, f.B, f.kv_text.p, f.kv_ip.p, b.kv_col, 2 * C);      // (the site refused after all: today's route, for this block's columns)
    if (kv_mine) kvi->second = 2;
    if (fuse_sa) {
      const LnIn ln{st, slots, F_(b.cs1), F_(b.lb1), eps};
      op_qkv_sattn(c, tk.p, C, W_(c, b.fqkv), &ln, M, C, sa, kv_here ? &ck : nullptr);
    } else if (fold) {
      const LnIn ln{st, slots, F_(b.cs1), F_(b.lb1), eps};
      op_gemm(c, tk.p, C, W_(c, b.fqkv), nullptr, nullptr, 0, qkv.p, 3 * C, M, 3 * C, C, folded(ln));
    } else {
      op_ln(c, tk.p, lnb.p, b.ln1g, b.ln1b, M, C);
      op_gemm(c, lnb.p, C, W_(c, b.wqkv), nullptr, nullptr, 0, qkv.p, 3 * C, M, 3 * C, C);
    }
    if (!fuse_sa) {
      op_attn(c, attn_desc(qkv.p, 3 * C, att.p, C, f.B, t.heads, HW, 1, AttnSeg{c->dry ? nullptr : qkv.p + C, c->dry ? nullptr : qkv.p + 2 * C, HW, 3 * C, HW, 1.f}));
    }
    }
    { RoleScope role(c, ROLE_ATTN_OUT); op_gemm(c, att.p, C, W_(c, b.wo1), W_(c, b.bo1), tk.p, C, tk.p, C, M, C, C, to_tk); }
    // cross-attention (IPAttnProcessor2_0 :310-412 when the adapter is installed, else AttnProcessor2_0)
    {
      RoleScope role(c, ROLE_Q_XATTN);
      const half_t* kt = c->dry ? nullptr : f.kv_text.p + b.kv_col;
      const half_t* ki = (c->dry || !Li) ? nullptr : f.kv_ip.p + b.kv_col;
      AttnArgs a = attn_desc(qkv.p, C, att.p, C, f.B, t.heads, HW, Li ? 2 : 1, AttnSeg{kt, c->dry ? nullptr : kt + C, Lt, ldkv, Lt, 1.f}, AttnSeg{ki, ki ? ki + C : nullptr, Li, ldkv, Li, c->ip_scale});
      a.w1_b = Li ? f.ip_scales : nullptr;
      // a 128 x 64 tile of to_q is 128 queries x one head: projection and attention run as one launch when tiles do not straddle batch elements
      // (and the context fits 3 key tiles: its K / V ride in registers through the projection loop); small problems keep the finer 64 x 64 split
      // (a regional site -- ia2p_unet_forward_r -- always takes the q GEMM and the stand-alone regional launch)
      const half_t* rw = nullptr;
      for (int i = 0; i < f.n_rlev; ++i) if (f.rlev[i].HW == HW) rw = f.rlev[i].w.p;
      const bool regional = f.G > 0;
      const bool fuse = !regional && c->xattn_fuse && HW % 128 == 0 && C == t.heads * 64 && (Lt + 63) / 64 + (Li + 63) / 64 <= 3 && (long)(M / 128) * t.heads >= c->xattn_min_tiles;
      if (fold) {
        const LnIn ln{st, slots, F_(b.cs2), F_(b.lb2), eps};
        if (fuse) op_qxattn(c, tk.p, C, W_(c, b.fq2), &ln, M, C, C, a);
        else op_gemm(c, tk.p, C, W_(c, b.fq2), nullptr, nullptr, 0, qkv.p, C, M, C, C, folded(ln));
      } else {
        op_ln(c, tk.p, lnb.p, b.ln2g, b.ln2b, M, C);
        if (fuse) op_qxattn(c, lnb.p, C, W_(c, b.wq2), nullptr, M, C, C, a);
        else op_gemm(c, lnb.p, C, W_(c, b.wq2), nullptr, nullptr, 0, qkv.p, C, M, C, C);
      }
      if (regional) op_attn_regions(c, a, rw, f.G);
      else if (!fuse) op_attn(c, a);
    }
    { RoleScope role(c, ROLE_ATTN_OUT); op_gemm(c, att.p, C, W_(c, b.wo2), W_(c, b.bo2), tk.p, C, tk.p, C, M, C, C, to_tk); }
    // GEGLU feed-forward
    if (!fold) op_ln(c, tk.p, lnb.p, b.ln3g, b.ln3b, M, C);
    {
      const LnIn ln{st, slots, F_(b.cs3), F_(b.lb3), eps};
      GemmOpt o1, o2;
      o1.geglu = 1; o1.ln = fold ? &ln : nullptr;
      o2.stats = st;
      GemmArgs g1 = gemm_args(c, fold ? tk.p : lnb.p, C, W_(c, fold ? b.fff1 : b.wff1), W_(c, b.bff1), nullptr, 0, ff.p, 4 * C, M, 8 * C, C, o1);
      GemmArgs g2 = gemm_args(c, ff.p, 4 * C, W_(c, b.wff2), W_(c, b.bff2), tk.p, C, tk.p, C, M, C, 4 * C, o2);
      run_ffn(c, g1, g2, &slots);
    }
  }
  wsfree(c, stt); wsfree(c, lnb); wsfree(c, qkv); wsfree(c, att); wsfree(c, ff);
  T2 out = wsalloc(c, (size_t)M * C);
  GnWant gw{HW};
  const bool want = f.gn_on && out_stats && ia2p_plan_any_gn(M);
  GemmOpt po;
  po.gw = want ? &gw : nullptr;
  { RoleScope role(c, ROLE_PROJ_IO); op_gemm(c, tk.p, C, W_(c, t.wout), W_(c, t.bout), x.p, C, out.p, C, M, C, C, po); }
  wsfree(c, tk);
  if (want) gst_put(f, out, gw.out);
  return out;
}

// What a controlled pass carries on top of the plain one (diffusers UNet2DConditionModel.forward `down_block_additional_residuals` / `mid_block_additional_residual`, and
// ControlNetModel.forward). UNet side: one residual per skip (skip order) and one for the mid block's output, channels-last like the tensors they are added to.
// ControlNet side: the embedded condition [B*h*w, C0], the per-image conditioning scales, and the buffer the n_skips + 1 residuals are written to, back to back.
struct CtlIo {
  const half_t* const* down = nullptr; const half_t* mid = nullptr;
  const half_t* cond = nullptr; const float* scales = nullptr; half_t* res = nullptr;
};
// t += r in place ([M, C]); the statistics the tensor carries are taken again over the sum, in the slots its producer chose (a consumer that fuses its GroupNorm reads them
// from f.gst; without any, the consumer's own pass -- gn_ensure_stats, or a GroupNorm launch -- sees the sum in memory)
static void add_residual(Fwd& f, T2 t, const half_t* r, long M, int C) {
  ia2p_ctx* c = f.c;
  double* st = nullptr;
  int rows = 0;
  auto it = f.gst.find(t.off);
  if (it != f.gst.end()) {
    if (it->second.ok() && it->second.rows % 16 == 0 && M % it->second.rows == 0) { st = (double*)it->second.buf.p; rows = it->second.rows; }
    else { wsfree(c, it->second.buf); f.gst.erase(it); }
  }
  CHECK_LAUNCH(c, ia2p_launch_residual_add_gnstats(t.p, r, t.p, (int)M, C, rows, st, c->stream), "residual injection");
}
// a zero convolution: out[m, :] = fp16(scales[m / HW] * fp16(x[m, :] . W^T + bias)), no K split (the scaled epilogue has no reduce-launch form)
static void zero_conv(ia2p_ctx* c, const half_t* x, size_t w, size_t b, const float* scales, half_t* out, int M, int C, int HW) {
  GemmArgs a = gemm_args(c, x, C, W_(c, w), W_(c, b), nullptr, 0, out, C, M, C, C);
  a.act = 4; a.rscale = scales; a.rows_per_batch = HW;
  set_prefetch(c, a, W_(c, w), (size_t)C * C * sizeof(half_t));
  const GemmPlan pl = ia2p_gemm_plan(M, C, C, false, false);
  RoleScope role(c, ROLE_PROJ_IO);
  ProfScope ps(c, PK_GEMM0 + pl.variant, 2.0 * M * C * C, gemm_bytes(M, C, C, 0, false));
  CHECK_LAUNCH(c, ia2p_launch_gemm_variant(a, false, pl.variant, c->stream), "zero convolution");
}

// One evaluation as run_forward sees it, whichever entry point asked for it: the shape, the tensors, and what the pass carries on top of the plain one. A sizing or
// recording pass runs over a record that holds the shape and the option switches only (shape_only): no pointer is read there.
struct FwdCall {
  int B = 0, h = 0, w = 0, L = 0;
  const half_t *sample = nullptr, *context = nullptr, *kv = nullptr, *text_embeds = nullptr, *time_ids = nullptr;
  half_t* out = nullptr;
  float timestep = 0.f;                   // the one timestep of the batch, unless ...
  const float* timesteps = nullptr;       // ... device [B]: one per batch element
  const float* ip_scales = nullptr;       // device [B] or null: per-request IP-Adapter scale
  const half_t* region_masks = nullptr;   // fp16 [B, G, h, w] (regional image prompts), with ...
  int G = 0;                              // ... G token groups; 0: none
  bool kv_cached = false;                 // the context projections were computed before (ia2p_project_context) and are read from `kv`
  CtlIo io;
  static FwdCall shape(int B, int h, int w, int L, int G = 0, bool kv_cached = false) {
    FwdCall s;
    s.B = B; s.h = h; s.w = w; s.L = L; s.G = G; s.kv_cached = kv_cached;
    return s;
  }
  FwdCall shape_only() const { return shape(B, h, w, L, G, kv_cached); }
};

// gn_mode: the GroupNorm mode of the pass -- the context's gn_fuse (0 launches, 1 fused, 2 the unfused twin), or, from forward_workspace, every one of them and
// 3: the sizing pass of ia2p_autotune
static ia2p_status run_forward(ia2p_ctx* c, int gn_mode, const FwdCall& call) {
  const int B = call.B, h = call.h, w = call.w, L = call.L, G = call.G;
  const CtlIo& io = call.io;
  const ia2p_unet_config& g = c->cfg;
  const int n = g.n_blocks;
  const int T = g.time_embed_dim, Tp = g.time_proj_dim, Ain = g.projection_class_embeddings_input_dim, Ad = g.addition_time_embed_dim;
  const int pooled = Ain - g.num_time_ids * Ad;
  Fwd f{c, B, h, w, L, call.context, T2{(size_t)-1, nullptr}, nullptr, T2{(size_t)-1, nullptr}, T2{(size_t)-1, nullptr}};
  f.ip_scales = call.ip_scales;
  f.gn_mode = gn_mode;
  f.tune_like = c->gn_fuse != 0 && (c->dry && !c->record ? gn_mode == 3 : c->tuning);      // (a sizing pass takes its mode's word; a recording or real pass is what the context is doing)
  f.gn_on = gn_mode != 0 && gn_mode != 3 && !c->tuning;      // (the autotune pass measures the plain kernels: GroupNorm launches there)

  // regional image prompts: the mask pyramid, one launch per distinct attention resolution, FIRST in the workspace (a regional pass needs what the plain pass needs
  // plus exactly these tensors: ia2p_workspace_bytes_r)
  f.G = G;
  if (G > 0) {
    int H = h, Wd = w;
    auto level = [&](bool has_att) {
      if (!has_att) return;
      for (int i = 0; i < f.n_rlev; ++i) if (f.rlev[i].HW == H * Wd) return;
      auto& lv = f.rlev[f.n_rlev++];
      lv.HW = H * Wd;
      lv.w = wsalloc(c, (size_t)B * G * H * Wd);
      RoleScope role(c, ROLE_Q_XATTN);
      ProfScope ps(c, PK_EMBED, 0, 0);
      CHECK_LAUNCH(c, ia2p_launch_region_levels(call.region_masks, lv.w.p, B, G, h, w, h / H, c->stream), "region_levels");
    };
    for (const Stage& st : c->down) {
      level(!st.att.empty());
      if (st.resample) { H = (H - 1) / 2 + 1; Wd = (Wd - 1) / 2 + 1; }
    }
    level(!c->mid_t.blocks.empty());
    for (const Stage& st : c->up) {
      level(!st.att.empty());
      if (st.resample) { H *= 2; Wd *= 2; }
    }
  }
  // GroupNorm partial sums (fp32) live at the front of the workspace
  T2 gnp = wsalloc(c, (size_t)B * 64 * g.norm_num_groups * 2 * 2);
  f.gn_partial = (float*)gnp.p;
  // ---- embeddings
  T2 tsin = wsalloc(c, (size_t)B * Tp), addin = wsalloc(c, (size_t)B * Ain), e1 = wsalloc(c, (size_t)B * T), emb0 = wsalloc(c, (size_t)B * T);
  T2 a1 = wsalloc(c, (size_t)B * T), emb = wsalloc(c, (size_t)B * T);
  f.temb_all = wsalloc(c, (size_t)B * c->temb_total);
  {
    RoleScope role(c, ROLE_EMBED);
    ProfScope ps(c, PK_EMBED, 0, 0);
    CHECK_LAUNCH(c, ia2p_launch_embed(call.timestep, call.timesteps, call.text_embeds, call.time_ids, tsin.p, addin.p, B, Tp, pooled, Ad, g.num_time_ids, c->stream), "embed");
    // skinny linears hold <= 16 rows per launch: larger batches go in row chunks
    auto lin = [&](const half_t* X, int ldx, size_t w, size_t b, const half_t* add, int ldadd, half_t* o, int ldo, int N, int K, int si, int so, const char* what) {
      for (int r0 = 0; r0 < B; r0 += 16) {
        const int rows = std::min(16, B - r0);
        CHECK_LAUNCH(c, ia2p_launch_linear_small(c->dry ? nullptr : X + (size_t)r0 * ldx, ldx, W_(c, w), W_(c, b), (c->dry || !add) ? nullptr : add + (size_t)r0 * ldadd, ldadd,
                                                 c->dry ? nullptr : o + (size_t)r0 * ldo, ldo, rows, N, K, si, so, c->stream), what);
      }
    };
    lin(tsin.p, Tp, c->te1w, c->te1b, nullptr, 0, e1.p, T, T, Tp, 0, 1, "time_embedding.linear_1");
    lin(e1.p, T, c->te2w, c->te2b, nullptr, 0, emb0.p, T, T, T, 0, 0, "time_embedding.linear_2");
    lin(addin.p, Ain, c->ae1w, c->ae1b, nullptr, 0, a1.p, T, T, Ain, 0, 1, "add_embedding.linear_1");
    // `emb` is only ever consumed through SiLU (every ResnetBlock2D: time_emb_proj(nonlinearity(temb))), so the last embedding linear stores
    // SiLU(emb) -- applied to the fp32 sum, rounded once -- and the stacked projection reads it as is: the activation used to be recomputed inside that
    // kernel by every one of its 3 440 output-column waves (64 SiLUs per wave-iteration against 256 FMAs)
    lin(a1.p, T, c->ae2w, c->ae2b, emb0.p, T, emb.p, T, T, T, 0, 1, "add_embedding.linear_2 (+ SiLU)");
    lin(emb.p, T, c->tw_all, c->tb_all, nullptr, 0, f.temb_all.p, c->temb_total, c->temb_total, T, 0, 0, "time_emb_proj (stacked)");
  }
  wsfree(c, tsin); wsfree(c, addin); wsfree(c, e1); wsfree(c, emb0); wsfree(c, a1); wsfree(c, emb);

  // ---- context K/V for every cross-attention layer in one GEMM each (text rows / image-token rows of ctx);
  //      per layer: reference attention_processor.py:358-359 (to_k/to_v) and :379-380 (to_k_ip/to_v_ip)
  if (c->kv_rows > 0) {
    const int Lt = ctx_lt(c, L), Li = ctx_li(c);
    if (Lt < 1) return fail(c, IA2P_ERR_SHAPE, "context length %d leaves no text rows", L);
    if (call.kv_cached) {
      f.kv_text.p = const_cast<half_t*>(call.kv);
      if (Li && call.kv) f.kv_ip.p = const_cast<half_t*>(call.kv) + (size_t)B * Lt * c->kv_rows;
    } else {
      f.kv_text = wsalloc(c, (size_t)B * Lt * c->kv_rows);
      if (Li) f.kv_ip = wsalloc(c, (size_t)B * Li * c->kv_rows);
      // (On a low-priority side stream beside the start of the step -- round 3, docs/LOG.md -- the projection cost +0.7 ms per step: the work is conserved, the
      //  interleaving costs. The step belongs on ONE queue; the pipelines hoist the projection out of the loop anyway.)
      // Round 7: a block that takes the fused QKV + self-attention launch has its columns projected by extra workgroups of that launch (plan_context_kv); the head of the
      // step keeps the other blocks' column ranges. The autotune pass projects everything here as well -- the whole projection's plan is what every range runs on, and
      // it is measured on the whole projection -- and lets the fused launches rewrite their columns with the same bits.
      const std::vector<std::pair<int, int>> up_front = plan_context_kv(f, h, w);
      if (c->tuning || f.tune_like) project_context(c, call.context, L, B, f.kv_text.p, f.kv_ip.p);
      else for (const auto& r : up_front) project_context(c, call.context, L, B, f.kv_text.p, f.kv_ip.p, r.first, r.second - r.first);
    }
  }

  // ---- down path
  RegionScope rs_conv(c, PR_CONV_BLOCK);      // from here on everything outside run_transformer belongs to the conv blocks
  int H = h, Wd = w;
  std::vector<T2> skips;
  std::vector<int> skip_c;
  T2 x = wsalloc(c, (size_t)B * H * Wd * g.block_out_channels[0]);
  {
    RoleScope role(c, ROLE_CONV_IO);
    ProfScope ps(c, PK_CONV_IN, 2.0 * B * H * Wd * 9.0 * g.in_channels * g.block_out_channels[0],
                 2.0 * ((double)B * H * Wd * (g.in_channels + g.block_out_channels[0]) + 64.0 * g.block_out_channels[0]));
    CHECK_LAUNCH(c, ia2p_launch_conv_in(call.sample, W_(c, c->conv_in_w), W_(c, c->conv_in_b), x.p, B, g.in_channels, H, Wd, g.block_out_channels[0], c->stream), "conv_in");
  }
  // Every tensor below feeds a GroupNorm in front of a 3x3 convolution -- the next ResnetBlock2D's norm1, or (the skips) the norm1 of an up-path block much later --
  // and carries its producer's column sums with it (f.gst); conv_in is a direct kernel: the consumer that fuses runs the canonical statistics pass over its output
  // ControlNet: sample = conv_in(sample) + controlnet_cond (the embedded condition, on the latent grid)
  if (c->cn) CHECK_LAUNCH(c, ia2p_launch_residual_add_gnstats(x.p, io.cond, x.p, B * H * Wd, g.block_out_channels[0], 0, nullptr, c->stream), "condition embedding");
  std::vector<int> skip_hw;      // (ControlNet: pixels per image of every skip, for its zero convolution)
  skips.push_back(x); skip_c.push_back(g.block_out_channels[0]); skip_hw.push_back(H * Wd);
  for (int i = 0; i < n; ++i) {
    const Stage& st = c->down[i];
    for (size_t j = 0; j < st.res.size(); ++j) {
      const bool att = !st.att.empty();
      T2 r = run_resnet(f, st.res[j], x, H, Wd, nullptr, 0, !att);      // (with a transformer behind it the block's output only feeds that transformer's own GroupNorm)
      if (att) { T2 t = run_transformer(f, st.att[j], r, H, Wd, true); act_free(f, r); r = t; }
      x = r;
      skips.push_back(x); skip_c.push_back(st.res[j].cout); skip_hw.push_back(H * Wd);
    }
    if (st.resample) {
      const int Ho = (H - 1) / 2 + 1, Wo = (Wd - 1) / 2 + 1;
      T2 d = wsalloc(c, (size_t)B * Ho * Wo * st.rc);
      GnWant gw{Ho * Wo};
      const bool want = f.gn_on && ia2p_plan_any_gn(B * Ho * Wo);
      ConvOpt o;
      o.stride = 2; o.gw = want ? &gw : nullptr;
      op_conv3(c, x.p, B, H, Wd, st.rc, W_(c, st.rw), W_(c, st.rb), st.rc, d.p, o);
      if (want) gst_put(f, d, gw.out);
      H = Ho; Wd = Wo; x = d;
      skips.push_back(x); skip_c.push_back(st.rc); skip_hw.push_back(H * Wd);
    }
  }
  // ---- mid
  {
    T2 r0 = run_resnet(f, c->mid_r0, x, H, Wd);          // x stays alive: it is the top skip
    T2 t = run_transformer(f, c->mid_t, r0, H, Wd, true); act_free(f, r0);
    T2 r1 = run_resnet(f, c->mid_r1, t, H, Wd, nullptr, 0, !c->cn); act_free(f, t);
    x = r1;
  }
  if (c->cn) {
    // ---- ControlNet: no up path. Residual k = zero_conv_k(skip_k) * conditioning_scale, the mid residual likewise, back to back in the caller's buffer
    half_t* res = io.res;
    const float* scales = io.scales;
    size_t off = 0;
    for (size_t k = 0; k < skips.size(); ++k) {
      const int Mk = B * skip_hw[k];
      zero_conv(c, skips[k].p, c->zc_w[k], c->zc_b[k], scales, res ? res + off : nullptr, Mk, skip_c[k], skip_hw[k]);
      off += (size_t)Mk * skip_c[k];
    }
    zero_conv(c, x.p, c->zm_w, c->zm_b, scales, res ? res + off : nullptr, B * H * Wd, g.block_out_channels[n - 1], H * Wd);
    for (T2 s : skips) act_free(f, s);
    act_free(f, x);
    for (auto& kv : f.gst) wsfree(c, kv.second.buf);
    f.gst.clear();
    wsfree(c, f.temb_all); wsfree(c, gnp); wsfree(c, f.kv_text); wsfree(c, f.kv_ip);
    return c->failed ? IA2P_ERR_HIP : IA2P_OK;
  }
  // a controlled UNet pass: mid_out += mid_residual; every skip gets its residual where the up path pops it -- after the whole down path and the mid block have read
  // the unmodified tensors, which is diffusers' order (the residuals are added to the finished tuple of skips)
  if (io.mid) add_residual(f, x, io.mid, (long)B * H * Wd, g.block_out_channels[n - 1]);
  // ---- up path
  for (int i = 0; i < n; ++i) {
    const Stage& st = c->up[i];
    for (size_t j = 0; j < st.res.size(); ++j) {
      T2 sk = skips.back(); skips.pop_back();
      const int cs = skip_c.back(); skip_c.pop_back();
      const int cx = st.res[j].cin - cs;
      const long M = (long)B * H * Wd;
      if (io.down) add_residual(f, sk, io.down[skips.size()], M, cs);
      T2 r;
      const bool att = !st.att.empty();
      const bool last = i == n - 1 && j + 1 == st.res.size();      // (the last block's output feeds conv_norm_out: a GroupNorm launch of its own)
      if (c->sc_fuse && c->cat_free && st.res[j].shortcut && cx % 64 == 0 && cs % 64 == 0) {
        // torch.cat([hidden, skip]) never materialised: GroupNorm and the appended shortcut blocks of conv2 read the two tensors
        r = run_resnet(f, st.res[j], x, H, Wd, &sk, cx, !att && !last);
        act_free(f, x); act_free(f, sk);
      } else {
        T2 cat = wsalloc(c, (size_t)M * st.res[j].cin);
        {
          ProfScope ps(c, PK_CONCAT, 0, 4.0 * M * st.res[j].cin);
          CHECK_LAUNCH(c, ia2p_launch_concat(x.p, cx, cx, sk.p, cs, cs, cat.p, M, c->stream), "concat");
        }
        act_free(f, x); act_free(f, sk);
        r = run_resnet(f, st.res[j], cat, H, Wd, nullptr, 0, !att && !last);
        act_free(f, cat);      // (with whatever statistics a fusing consumer computed for it)
      }
      if (att) { T2 t = run_transformer(f, st.att[j], r, H, Wd, true); act_free(f, r); r = t; }
      x = r;
    }
    if (st.resample) {
      T2 u = wsalloc(c, (size_t)B * (2 * H) * (2 * Wd) * st.rc);
      GnWant gw{4 * H * Wd};
      const bool want = f.gn_on && ia2p_plan_any_gn(4 * B * H * Wd);
      ConvOpt o;
      o.up = 1; o.gw = want ? &gw : nullptr;
      op_conv3(c, x.p, B, H, Wd, st.rc, W_(c, st.rw), W_(c, st.rb), st.rc, u.p, o);
      if (want) gst_put(f, u, gw.out);
      act_free(f, x);
      H *= 2; Wd *= 2; x = u;
    }
  }
  if (H != h || Wd != w) return fail(c, IA2P_ERR_SHAPE, "latent %dx%d does not survive the down/up path (needs divisibility by 2^%d)", h, w, n - 1);
  // ---- out
  const int c0 = g.block_out_channels[0];
  T2 no = wsalloc(c, (size_t)B * H * Wd * c0);
  op_gn(c, x.p, no.p, c->ngo, c->nbo, B, H * Wd, c0, g.norm_eps, 1, f.gn_partial);
  act_free(f, x);
  {
    RoleScope role(c, ROLE_CONV_IO);
    ProfScope ps(c, PK_CONV_OUT, 2.0 * B * H * Wd * 9.0 * c0 * g.out_channels, 2.0 * ((double)B * H * Wd * (c0 + g.out_channels) + 9.0 * c0 * g.out_channels));
    CHECK_LAUNCH(c, ia2p_launch_conv_out(no.p, c0, W_(c, c->conv_out_w), W_(c, c->conv_out_b), call.out, B, c0, H, Wd, g.out_channels, c->stream), "conv_out");
  }
  for (auto& kv : f.gst) wsfree(c, kv.second.buf);      // (none left on a complete pass)
  f.gst.clear();
  wsfree(c, no); wsfree(c, f.temb_all); wsfree(c, gnp); wsfree(c, f.kv_text); wsfree(c, f.kv_ip);
  for (int i = 0; i < f.n_rlev; ++i) wsfree(c, f.rlev[i].w);
  return c->failed ? IA2P_ERR_HIP : IA2P_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
extern "C" {

ia2p_status ia2p_create(const ia2p_unet_config* cfg, ia2p_ctx** out) {
  return rc_create(cfg, out, "ia2p_create", [](ia2p_ctx* c) {
    const ia2p_status st = build_plan(c);
    if (st != IA2P_OK) return st;
    c->groups = c->cfg.norm_num_groups;
    ia2p_sk_counters_invalidate();      // a fresh context never trusts tickets an earlier (possibly failed) one left behind
    return IA2P_OK;
  });
}
void ia2p_destroy(ia2p_ctx* c) { delete c; }
const char* ia2p_last_error(ia2p_ctx* c) { return rc_last_error(c); }
size_t ia2p_arena_bytes(ia2p_ctx* c) { return rc_arena_bytes(c); }

ia2p_status ia2p_bind_arena(ia2p_ctx* c, void* dev, size_t bytes) { return rc_bind_arena(c, dev, bytes); }
ia2p_status ia2p_load_tensor(ia2p_ctx* c, const char* key, const void* src, const int64_t* shape, int ndim, void* stream) {
  return rc_load_tensor(c, key, src, shape, ndim, stream);
}
ia2p_status ia2p_read_tensor(ia2p_ctx* c, const char* key, void* dst, const int64_t* shape, int ndim, void* stream) {
  return rc_read_tensor(c, key, dst, shape, ndim, stream);
}
// LayerNorm folding pass over every transformer block (idempotent: reads the raw tensors, writes the folded copies)
static ia2p_status fold_all(ia2p_ctx* c, hipStream_t stream, bool sync) {
  std::vector<const Transformer*> ts;
  for (const Stage& s : c->down) for (const Transformer& t : s.att) ts.push_back(&t);
  ts.push_back(&c->mid_t);
  for (const Stage& s : c->up) for (const Transformer& t : s.att) ts.push_back(&t);
  hipError_t e = hipSuccess;
  auto H = [&](size_t off) { return c->arena + off; };
  auto F = [&](size_t off) { return (float*)(c->arena + off); };
  for (const Transformer* t : ts)
    for (const TBlock& b : t->blocks) {
      const int C = t->c;
      if (e == hipSuccess) e = ia2p_launch_fold_ln(H(b.wqkv), H(b.ln1g), H(b.ln1b), nullptr, H(b.fqkv), F(b.cs1), F(b.lb1), 3 * C, C, stream);
      if (e == hipSuccess) e = ia2p_launch_fold_ln(H(b.wq2), H(b.ln2g), H(b.ln2b), nullptr, H(b.fq2), F(b.cs2), F(b.lb2), C, C, stream);
      if (e == hipSuccess) e = ia2p_launch_fold_ln(H(b.wff1), H(b.ln3g), H(b.ln3b), H(b.bff1), H(b.fff1), F(b.cs3), F(b.lb3), 8 * C, C, stream);
    }
  // conv2 + conv_shortcut of a ResnetBlock2D as ONE implicit GEMM: weight rows concatenated along K, biases added
  std::vector<const Resnet*> rs;
  for (const Stage& s : c->down) for (const Resnet& r : s.res) rs.push_back(&r);
  rs.push_back(&c->mid_r0); rs.push_back(&c->mid_r1);
  for (const Stage& s : c->up) for (const Resnet& r : s.res) rs.push_back(&r);
  for (const Resnet* r : rs)
    if (r->shortcut && e == hipSuccess)
      e = ia2p_launch_cat_rows(H(r->w2), 9 * r->cout, H(r->wsc), r->cin, H(r->b2), H(r->bsc), H(r->wcat), H(r->bcat), r->cout, stream);
  if (e == hipSuccess && sync) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail_hip(c, e, "weight folding");
  c->fold_dirty = false;
  return IA2P_OK;
}
ia2p_status ia2p_finalize_weights(ia2p_ctx* c) {
  const ia2p_status st = rc_finalize(c, "UNet");
  return st == IA2P_OK ? fold_all(c, nullptr, true) : st;
}
size_t ia2p_arena_raw_bytes(ia2p_ctx* c) { return c ? c->arena_raw_elems * sizeof(half_t) : 0; }
// The head of the arena ([0, ia2p_arena_raw_bytes): parameters as loaded) was filled elsewhere -- an RCCL broadcast from the rank that read the
// checkpoint; the derived tail (LayerNorm folds) is recomputed here from it, so 2.5 GB of it never cross xGMI.
// The fold kernels must run AFTER the broadcast that filled the head: they are enqueued on the caller's stream (the one the collective was
// ordered on) and that stream is synchronised before returning, so forwards on any other stream afterwards see finished folds.
ia2p_status ia2p_adopt_arena_on(ia2p_ctx* c, int with_ip_adapter, void* stream) {
  const ia2p_status st = rc_adopt(c, with_ip_adapter != 0);
  return st == IA2P_OK ? fold_all(c, (hipStream_t)stream, true) : st;
}
ia2p_status ia2p_adopt_arena(ia2p_ctx* c, int with_ip_adapter) { return ia2p_adopt_arena_on(c, with_ip_adapter, nullptr); }

// ---- the one collective of the batch-data-parallel path, through the C ABI: RCCL broadcast of the arena head + local adoption -------------------------
// RCCL is bound late (dlopen / dlsym): the library has no link-time dependency on it, and a host that already carries an RCCL instance (PyTorch bundles its
// own librccl.so with SONAME librccl.so.1) must be served by THAT instance -- the communicator handed in was created by it. RTLD_NOLOAD first: whatever is
// already in the process; only a host without any RCCL gets the system one loaded for it.
namespace {
struct Rccl {
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool ok = false;
};
const Rccl& rccl() {
  static const Rccl r = [] {
    Rccl x;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so"})
      if (!h) h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
      if (!h) h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (!h) return x;
    x.Broadcast = (decltype(x.Broadcast))dlsym(h, "ncclBroadcast");
    x.CommUserRank = (decltype(x.CommUserRank))dlsym(h, "ncclCommUserRank");
    x.CommCount = (decltype(x.CommCount))dlsym(h, "ncclCommCount");
    x.GetErrorString = (decltype(x.GetErrorString))dlsym(h, "ncclGetErrorString");
    x.ok = x.Broadcast && x.CommUserRank && x.CommCount && x.GetErrorString;
    return x;
  }();
  return r;
}
}  // namespace
int ia2p_rccl_available(void) { return rccl().ok ? 1 : 0; }
ia2p_status ia2p_bcast_arena(ia2p_ctx* c, void* rccl_comm, int root, int with_ip_adapter, void* stream) {
  if (!c || !rccl_comm) return fail(c, IA2P_ERR_INVALID, "bcast_arena: null argument");
  if (!c->arena) return fail(c, IA2P_ERR_STATE, "bcast_arena before bind_arena");
  const Rccl& r = rccl();
  if (!r.ok) return fail(c, IA2P_ERR_STATE, "bcast_arena: no RCCL in this process and none could be loaded (librccl.so.1)");
  ncclComm_t comm = (ncclComm_t)rccl_comm;
  int rank = -1, n = 0;
  ncclResult_t e = r.CommUserRank(comm, &rank);
  if (e == ncclSuccess) e = r.CommCount(comm, &n);
  if (e != ncclSuccess) return fail(c, IA2P_ERR_INVALID, "bcast_arena: not a usable communicator (%s)", r.GetErrorString(e));
  if (root < 0 || root >= n) return fail(c, IA2P_ERR_INVALID, "bcast_arena: root %d outside a communicator of %d ranks", root, n);
  // a few large messages (ring broadcast over point-to-point xGMI is per-link bound: message COUNT is what to keep small), each below 2^31 bytes
  char* p = (char*)c->arena;
  const size_t total = c->arena_raw_elems * sizeof(half_t), piece = (size_t)1 << 30;
  for (size_t lo = 0; lo < total && e == ncclSuccess; lo += piece)
    e = r.Broadcast(p + lo, p + lo, std::min(piece, total - lo), ncclInt8, root, comm, (hipStream_t)stream);
  if (e != ncclSuccess) { ia2p_sk_counters_invalidate(); return fail(c, IA2P_ERR_HIP, "bcast_arena: ncclBroadcast: %s", r.GetErrorString(e)); }
  if (rank == root) {                  // the root keeps its own tail; its stream is synchronised like the receivers' (the call returns with the head sent)
    const hipError_t he = hipStreamSynchronize((hipStream_t)stream);
    return he == hipSuccess ? IA2P_OK : fail_hip(c, he, "bcast_arena");
  }
  return ia2p_adopt_arena_on(c, with_ip_adapter, stream);      // fold kernels ordered behind the broadcast on the same stream, which is synchronised before returning
}

ia2p_status ia2p_set_gn_fuse(ia2p_ctx* c, int mode) {
  if (!c || mode < 0 || mode > 2) return fail(c, IA2P_ERR_INVALID, "set_gn_fuse: mode %d (0 GroupNorm launches, 1 fused into the convolutions, 2 the fused path's unfused twin)", mode);
  c->gn_fuse = mode;
  c->wseq_key = -1;
  return IA2P_OK;
}
ia2p_status ia2p_set_ip_adapter(ia2p_ctx* c, int enabled, int num_tokens, float scale) {
  if (!c) return IA2P_ERR_INVALID;
  if (c->cn) return fail(c, IA2P_ERR_STATE, "set_ip_adapter on a ControlNet context (ia2p_controlnet_set_image_tokens: it sees the text rows only)");
  if (enabled) {
    if (num_tokens < 1 || num_tokens > 64) return fail(c, IA2P_ERR_INVALID, "num_tokens %d out of range", num_tokens);
    for (auto& kv : c->params)
      if (kv.second.optional && !kv.second.loaded) return fail(c, IA2P_ERR_KEY, "IP-Adapter enabled but '%s' was never loaded", kv.first.c_str());
  }
  c->ip_enabled = enabled ? 1 : 0; c->ip_tokens = num_tokens; c->ip_scale = scale;
  return IA2P_OK;
}

static ia2p_status check_fwd_shape(ia2p_ctx* c, int B, int h, int w, int L) {
  if (B < 1 || B > 1024) return fail(c, IA2P_ERR_SHAPE, "batch %d outside 1..1024", B);
  const int div = 1 << (c->cfg.n_blocks - 1);
  if (h < div || w < div || h % div || w % div) return fail(c, IA2P_ERR_SHAPE, "latent %dx%d must be divisible by %d", h, w, div);
  if (L < 1) return fail(c, IA2P_ERR_SHAPE, "context length %d", L);
  if (c->ip_enabled && L <= c->ip_tokens) return fail(c, IA2P_ERR_SHAPE, "context length %d must exceed the %d image tokens", L, c->ip_tokens);
  if (L <= c->ctx_drop) return fail(c, IA2P_ERR_SHAPE, "context length %d must exceed the %d image-token rows the ControlNet leaves out", L, c->ctx_drop);
  return IA2P_OK;
}

// the workspace of a pass: a dry pass per GroupNorm mode 0 .. n_modes - 1, the maximum (0: a mode failed). Modes 0 .. 2: the GroupNorms as launches of their own, inside
// their convolutions (the product path), the fused path's unfused twin -- a workspace sized here serves every ia2p_set_gn_fuse mode; mode 3: the autotune pass (GroupNorm
// launches + the statistics and live tensors its fused candidates need), which only the plain UNet pass runs (no regions, no ControlNet)
static size_t forward_workspace(ia2p_ctx* c, const FwdCall& shape, int n_modes) {
  size_t need = 0;
  for (int mode = 0; mode < n_modes; ++mode) {
    const size_t n = pass_dry(c, [&] { return run_forward(c, mode, shape); });
    if (!n) return 0;
    need = std::max(need, n);
  }
  return need;
}
// one evaluation, once its entry point's own checks passed. record_key names the weight launch sequence of the pass: when it is not the recorded one, a dry pass of the
// same code path over the shape-only record notes it.
static ia2p_status forward_pass(ia2p_ctx* c, void* stream, void* ws, size_t ws_bytes, int record_key, const FwdCall& call) {
  // a tensor was reloaded after finalize (hot swap, strict=False load): re-derive the folds on this stream and wait (rare; the wait keeps a following forward on
  // ANOTHER stream from reading half-written folds)
  ia2p_status st = pass_ready(c, [&] { return fold_all(c, (hipStream_t)stream, true); });
  if (st == IA2P_OK) st = pass_enter(c, stream, ws, ws_bytes);
  if (st != IA2P_OK) return st;
  pass_record(c, record_key, [&] { return run_forward(c, c->gn_fuse, call.shape_only()); });
  c->tail_pf = c->arena + c->embed_lo; c->tail_pf_bytes = (c->embed_hi - c->embed_lo) * sizeof(half_t);   // the next step starts with these
  return pass_leave(c, run_forward(c, c->gn_fuse, call));
}

// ---- the UNet callable: one record (ia2p_unet_call), one validator, and the legacy argument lists as thin callers of the record form
// the record as first published ends with mid_residual: a caller compiled against a later header may pass more, never less
static const size_t UNET_CALL_V1 = offsetof(ia2p_unet_call, mid_residual) + sizeof(const void*);
// Every rule on which fields of an ia2p_unet_call may meet (the table in include/ia2p.h), in the order the legacy exports applied them: what the options need, the
// tensors every pass needs, the context's kind and state, the shape. u: the caller's record, fields it did not know zeroed. sizing: a workspace query -- the shape,
// G and the presence of residuals count, no pointer is required and no adapter state (the query may come before ia2p_set_ip_adapter).
static ia2p_status check_call(ia2p_ctx* c, const ia2p_unet_call* in, const void* ws, bool sizing, ia2p_unet_call& u) {
  if (!c || !in) return fail(c, IA2P_ERR_INVALID, "unet_forward: null argument");
  if (in->struct_size < UNET_CALL_V1 || in->struct_size > sizeof u)
    return fail(c, IA2P_ERR_INVALID, "unet_forward: struct_size %u (this library reads records of %zu .. %zu bytes)", in->struct_size, UNET_CALL_V1, sizeof u);
  memset(&u, 0, sizeof u);
  memcpy(&u, in, in->struct_size);
  const bool regions = u.region_masks || u.G, residuals = u.down_residuals || u.mid_residual || u.n_down;
  if (!sizing) {
    if ((!u.context) == (!u.kv)) return fail(c, IA2P_ERR_INVALID, "unet_forward: exactly one of context / kv is required");
    if (!u.timesteps && (u.ip_scales || regions || residuals)) return fail(c, IA2P_ERR_INVALID, "unet_forward: ip_scales, region_masks and residuals need per-row timesteps");
  }
  if (regions && residuals) return fail(c, IA2P_ERR_INVALID, "unet_forward: residuals together with region_masks (the regional pass is not combined with a ControlNet)");
  if (regions) {
    if (!sizing && !u.region_masks) return fail(c, IA2P_ERR_INVALID, "unet_forward: G=%d without region_masks", u.G);
    if (u.G < 1 || u.G > 16) return fail(c, IA2P_ERR_SHAPE, "unet_forward: G=%d (1 .. 16)", u.G);
    if (!sizing && (!c->ip_enabled || c->ip_tokens != 4 * u.G))
      return fail(c, IA2P_ERR_STATE, "unet_forward: %d token groups need the IP-Adapter enabled with num_tokens = %d (ia2p_set_ip_adapter)", u.G, 4 * u.G);
  }
  if (residuals && !sizing) {
    if (!u.down_residuals || !u.mid_residual) return fail(c, IA2P_ERR_INVALID, "unet_forward: down_residuals and mid_residual come together");
    if (u.n_down != c->n_skips) return fail(c, IA2P_ERR_SHAPE, "unet_forward: %d down residuals, this UNet has %d skips", u.n_down, c->n_skips);
    for (int i = 0; i < u.n_down; ++i)
      if (!u.down_residuals[i] || (((uintptr_t)u.down_residuals[i]) & 15)) return fail(c, IA2P_ERR_INVALID, "unet_forward: down residual %d is null or not 16-byte aligned", i);
    if (((uintptr_t)u.mid_residual) & 15) return fail(c, IA2P_ERR_INVALID, "unet_forward: the mid residual is not 16-byte aligned");
  }
  if (!sizing) {
    if (u.ip_scales && !c->ip_enabled) return fail(c, IA2P_ERR_STATE, "unet_forward: per-request IP-Adapter scales without an installed adapter");
    if (!u.sample || !u.text_embeds || !u.time_ids || !u.out || !ws) return fail(c, IA2P_ERR_INVALID, "unet_forward: null argument");
  }
  if (c->cn) return fail(c, IA2P_ERR_STATE, "unet_forward on a ControlNet context (ia2p_controlnet_forward)");
  if (!sizing && !c->finalized) return fail(c, IA2P_ERR_STATE, "unet_forward before weights were finalized");
  return check_fwd_shape(c, u.B, u.h, u.w, u.L);
}
static FwdCall fwd_call(const ia2p_unet_call& u) {
  FwdCall f = FwdCall::shape(u.B, u.h, u.w, u.L);
  f.sample = (const half_t*)u.sample; f.context = (const half_t*)u.context; f.kv = (const half_t*)u.kv; f.kv_cached = u.kv != nullptr;
  f.text_embeds = (const half_t*)u.text_embeds; f.time_ids = (const half_t*)u.time_ids; f.out = (half_t*)u.out;
  f.timestep = u.timestep; f.timesteps = u.timesteps; f.ip_scales = u.ip_scales;
  f.region_masks = (const half_t*)u.region_masks; f.G = u.G;
  f.io.down = (const half_t* const*)u.down_residuals; f.io.mid = (const half_t*)u.mid_residual;
  return f;
}
// 0 on a refusal. A regional pass needs what the plain pass needs plus the mask pyramid in front of it (and the autotune pass runs no regions: three modes); residuals
// are added in place: no allocation beyond the plain pass's.
size_t ia2p_workspace_bytes_x(ia2p_ctx* c, const ia2p_unet_call* call) {
  ia2p_unet_call u;
  if (check_call(c, call, nullptr, true, u) != IA2P_OK) return 0;
  return forward_workspace(c, fwd_call(u).shape_only(), u.G ? 3 : 4);
}
ia2p_status ia2p_unet_forward_x(ia2p_ctx* c, void* stream, const ia2p_unet_call* call, void* ws, size_t ws_bytes) {
  ia2p_unet_call u;
  const ia2p_status st = check_call(c, call, ws, false, u);
  if (st != IA2P_OK) return st;
  return forward_pass(c, stream, ws, ws_bytes, (c->ip_enabled ? 1 + c->ip_tokens : 0) + (u.kv ? 1000 : 0) + (u.G ? 2000 : 0), fwd_call(u));
}

// ---- the legacy argument lists: each fills a record and calls the record form; its own checks are what makes it THIS form (the pointers it cannot do without)
static ia2p_unet_call unet_call(int B, int h, int w, int L, const void* sample = nullptr, const void* context = nullptr, const void* kv = nullptr,
                                const void* text_embeds = nullptr, const void* time_ids = nullptr, void* out = nullptr) {
  ia2p_unet_call u;
  memset(&u, 0, sizeof u);
  u.struct_size = sizeof u;
  u.B = B; u.h = h; u.w = w; u.L = L;
  u.sample = sample; u.context = context; u.kv = kv; u.text_embeds = text_embeds; u.time_ids = time_ids; u.out = out;
  return u;
}
size_t ia2p_workspace_bytes(ia2p_ctx* c, int B, int h, int w, int L) {
  const ia2p_unet_call u = unet_call(B, h, w, L);
  return ia2p_workspace_bytes_x(c, &u);
}
size_t ia2p_workspace_bytes_r(ia2p_ctx* c, int B, int h, int w, int L, int G) {
  if (G < 1) return 0;      // (G = 0 is the plain query in a record)
  ia2p_unet_call u = unet_call(B, h, w, L);
  u.G = G;
  return ia2p_workspace_bytes_x(c, &u);
}
size_t ia2p_workspace_bytes_c(ia2p_ctx* c, int B, int h, int w, int L) { return ia2p_workspace_bytes(c, B, h, w, L); }
int ia2p_unet_num_skips(ia2p_ctx* c) { return c ? c->n_skips : 0; }

ia2p_status ia2p_unet_forward(ia2p_ctx* c, void* stream, const void* sample, float timestep, const void* context, int L,
                              const void* text_embeds, const void* time_ids, void* out, int B, int h, int w, void* ws, size_t ws_bytes) {
  ia2p_unet_call u = unet_call(B, h, w, L, sample, context, nullptr, text_embeds, time_ids, out);
  u.timestep = timestep;
  return ia2p_unet_forward_x(c, stream, &u, ws, ws_bytes);
}
ia2p_status ia2p_unet_forward_kv(ia2p_ctx* c, void* stream, const void* sample, float timestep, const void* kv, int L, const void* text_embeds,
                                 const void* time_ids, void* out, int B, int h, int w, void* ws, size_t ws_bytes) {
  ia2p_unet_call u = unet_call(B, h, w, L, sample, nullptr, kv, text_embeds, time_ids, out);
  u.timestep = timestep;
  return ia2p_unet_forward_x(c, stream, &u, ws, ws_bytes);
}
// per-row timesteps and IP-Adapter scales: batch element b gets the bits of a uniform batch evaluated at (timesteps[b], ip_scales[b]) (tests/test_batch_gpu.py)
ia2p_status ia2p_unet_forward_v(ia2p_ctx* c, void* stream, const void* sample, const float* timesteps, const float* ip_scales, const void* context, const void* kv,
                                int L, const void* text_embeds, const void* time_ids, void* out, int B, int h, int w, void* ws, size_t ws_bytes) {
  if (!timesteps) return fail(c, IA2P_ERR_INVALID, "unet_forward_v: timesteps and exactly one of context / kv are required");
  ia2p_unet_call u = unet_call(B, h, w, L, sample, context, kv, text_embeds, time_ids, out);
  u.timesteps = timesteps; u.ip_scales = ip_scales;
  return ia2p_unet_forward_x(c, stream, &u, ws, ws_bytes);
}
// ... with regional image prompts: G token groups of four under region_masks [B, G, h, w] (run_forward builds the pyramid; run_transformer the regional sites)
ia2p_status ia2p_unet_forward_r(ia2p_ctx* c, void* stream, const void* sample, const float* timesteps, const float* ip_scales, const void* context, const void* kv,
                                int L, const void* text_embeds, const void* time_ids, void* out, int B, int h, int w, void* ws, size_t ws_bytes,
                                const void* region_masks, int G) {
  if (!c) return IA2P_ERR_INVALID;
  if (!timesteps || !region_masks) return fail(c, IA2P_ERR_INVALID, "unet_forward_r: timesteps, region_masks and exactly one of context / kv are required");
  ia2p_unet_call u = unet_call(B, h, w, L, sample, context, kv, text_embeds, time_ids, out);
  u.timesteps = timesteps; u.ip_scales = ip_scales; u.region_masks = region_masks; u.G = G;
  return ia2p_unet_forward_x(c, stream, &u, ws, ws_bytes);
}
// ... with a ControlNet's residuals, added in place where the up path pops each skip (add_residual)
ia2p_status ia2p_unet_forward_c(ia2p_ctx* c, void* stream, const void* sample, const float* timesteps, const float* ip_scales, const void* context, const void* kv,
                                int L, const void* text_embeds, const void* time_ids, void* out, int B, int h, int w, void* ws, size_t ws_bytes,
                                const void* const* down_residuals, int n_down, const void* mid_residual, const void* region_masks, int G) {
  if (!c) return IA2P_ERR_INVALID;
  if (!timesteps) return fail(c, IA2P_ERR_INVALID, "unet_forward_c: timesteps and exactly one of context / kv are required");
  if (!down_residuals || !mid_residual) return fail(c, IA2P_ERR_INVALID, "unet_forward_c: null residuals (the plain pass is ia2p_unet_forward_v)");
  ia2p_unet_call u = unet_call(B, h, w, L, sample, context, kv, text_embeds, time_ids, out);
  u.timesteps = timesteps; u.ip_scales = ip_scales; u.region_masks = region_masks; u.G = G;
  u.down_residuals = down_residuals; u.n_down = n_down; u.mid_residual = mid_residual;
  return ia2p_unet_forward_x(c, stream, &u, ws, ws_bytes);
}

// ---- the ControlNet executor (diffusers 0.26.3 ControlNetModel; the reference prepares its attention seam only: ip_adapter.py:143-148) -----------------------------------
ia2p_status ia2p_controlnet_create(const ia2p_controlnet_config* cfg, ia2p_ctx** out) {
  if (!cfg || !out) return fail(nullptr, IA2P_ERR_INVALID, "ia2p_controlnet_create: null argument");
  return rc_create(&cfg->unet, out, "ia2p_controlnet_create", [&](ia2p_ctx* c) {
    c->cn = true;
    c->ce_in_ch = cfg->conditioning_channels;
    for (int i = 0; i < 4; ++i) c->ce_ch[i] = cfg->conditioning_embedding_out_channels[i];
    if (c->ce_in_ch < 1 || c->ce_in_ch * 9 > 64) return fail(c, IA2P_ERR_SHAPE, "controlnet: conditioning_channels %d (1 .. 7: the first convolution takes Cin * 9 <= 64)", c->ce_in_ch);
    for (int i = 0; i < 4; ++i)
      if (c->ce_ch[i] < 16 || c->ce_ch[i] > 256 || c->ce_ch[i] % 16) return fail(c, IA2P_ERR_SHAPE, "controlnet: conditioning_embedding_out_channels[%d]=%d must be a multiple of 16 in 16 .. 256", i, c->ce_ch[i]);
    const ia2p_status st = build_plan(c);
    if (st != IA2P_OK) return st;
    c->groups = c->cfg.norm_num_groups;
    ia2p_sk_counters_invalidate();
    return IA2P_OK;
  });
}
void ia2p_controlnet_destroy(ia2p_ctx* c) { delete c; }
const char* ia2p_controlnet_last_error(ia2p_ctx* c) { return rc_last_error(c); }
size_t ia2p_controlnet_arena_bytes(ia2p_ctx* c) { return rc_arena_bytes(c); }
ia2p_status ia2p_controlnet_bind_arena(ia2p_ctx* c, void* dev, size_t bytes) { return rc_bind_arena(c, dev, bytes); }
ia2p_status ia2p_controlnet_load_tensor(ia2p_ctx* c, const char* key, const void* src, const int64_t* shape, int ndim, void* stream) { return rc_load_tensor(c, key, src, shape, ndim, stream); }
ia2p_status ia2p_controlnet_finalize_weights(ia2p_ctx* c) {
  if (!c || !c->cn) return fail(c, IA2P_ERR_STATE, "controlnet_finalize_weights: not a ControlNet context");
  const ia2p_status st = rc_finalize(c, "ControlNet");
  return st == IA2P_OK ? fold_all(c, nullptr, true) : st;
}
// the ControlNet's contexts carry `num_tokens` trailing image-token rows it must not see (0: none): it attends to rows [0, L - num_tokens) of every context
ia2p_status ia2p_controlnet_set_image_tokens(ia2p_ctx* c, int num_tokens) {
  if (!c || !c->cn) return fail(c, IA2P_ERR_STATE, "controlnet_set_image_tokens: not a ControlNet context");
  if (num_tokens < 0 || num_tokens > 64) return fail(c, IA2P_ERR_INVALID, "controlnet_set_image_tokens: num_tokens %d out of range", num_tokens);
  c->ctx_drop = num_tokens;
  c->wseq_key = -1;
  return IA2P_OK;
}
int ia2p_controlnet_num_residuals(ia2p_ctx* c) { return c && c->cn ? c->n_skips + 1 : 0; }
// does this ControlNet fit a UNet? (block_out_channels, layers_per_block and cross_attention_dim must match: the residuals are added to that UNet's skips)
ia2p_status ia2p_controlnet_check_unet(ia2p_ctx* c, ia2p_ctx* unet) {
  if (!c || !c->cn || !unet || unet->cn) return fail(c, IA2P_ERR_INVALID, "controlnet_check_unet: a ControlNet context and a UNet context are required");
  const ia2p_unet_config &a = c->cfg, &b = unet->cfg;
  bool same = a.n_blocks == b.n_blocks && a.layers_per_block == b.layers_per_block && a.cross_attention_dim == b.cross_attention_dim && a.in_channels == b.in_channels;
  for (int i = 0; same && i < a.n_blocks; ++i) same = a.block_out_channels[i] == b.block_out_channels[i];
  if (!same) return fail(c, IA2P_ERR_SHAPE, "controlnet: block_out_channels, layers_per_block, in_channels and cross_attention_dim must match the UNet's");
  return IA2P_OK;
}
// the residual buffer of a forward at (B, h, w): total bytes (0 on a bad shape); per residual k < n_skips + 1 (the mid residual last) its element offset, channels and grid
size_t ia2p_controlnet_residual_layout(ia2p_ctx* c, int B, int h, int w, int64_t* offsets, int* channels, int* hs, int* ws) {
  if (!c || !c->cn || check_fwd_shape(c, B, h, w, c->ctx_drop + 1) != IA2P_OK) return 0;
  const ia2p_unet_config& g = c->cfg;
  size_t off = 0;
  int k = 0, H = h, Wd = w;
  auto put = [&](int ch) {
    if (offsets) offsets[k] = (int64_t)off;
    if (channels) channels[k] = ch;
    if (hs) hs[k] = H;
    if (ws) ws[k] = Wd;
    off += (size_t)B * H * Wd * ch; ++k;
  };
  put(g.block_out_channels[0]);
  for (int i = 0; i < g.n_blocks; ++i) {
    for (int j = 0; j < g.layers_per_block; ++j) put(g.block_out_channels[i]);
    if (i != g.n_blocks - 1) { H = (H - 1) / 2 + 1; Wd = (Wd - 1) / 2 + 1; put(g.block_out_channels[i]); }
  }
  put(g.block_out_channels[g.n_blocks - 1]);
  return off * sizeof(half_t);
}
// condition embedding: image [B, conditioning_channels, 8 h, 8 w] NCHW fp16 in [0, 1] -> [B * h * w, block_out_channels[0]] channels-last. Depends on the image and the
// weights only: once per request, not per step.
static ia2p_status run_embed(ia2p_ctx* c, const half_t* image, half_t* out, int B, int h, int w) {
  RoleScope role(c, ROLE_CONV_IO);
  int H = 8 * h, Wd = 8 * w;
  T2 cur = wsalloc(c, (size_t)B * H * Wd * c->ce_ch[0]);
  CHECK_LAUNCH(c, ia2p_launch_conv_in(image, W_(c, c->ce_in_w), W_(c, c->ce_in_b), cur.p, B, c->ce_in_ch, H, Wd, c->ce_ch[0], c->stream, 1.0f, 1), "controlnet_cond_embedding.conv_in");
  for (int i = 0; i < 3; ++i) {
    T2 t = wsalloc(c, (size_t)B * H * Wd * c->ce_ch[i]);
    CHECK_LAUNCH(c, ia2p_launch_conv3x3_narrow(cur.p, W_(c, c->ce_w[2 * i]), W_(c, c->ce_b[2 * i]), t.p, B, H, Wd, c->ce_ch[i], c->ce_ch[i], 1, 1, c->stream), "controlnet_cond_embedding.blocks (stride 1)");
    wsfree(c, cur);
    const int Ho = (H - 1) / 2 + 1, Wo = (Wd - 1) / 2 + 1;
    T2 u = wsalloc(c, (size_t)B * Ho * Wo * c->ce_ch[i + 1]);
    CHECK_LAUNCH(c, ia2p_launch_conv3x3_narrow(t.p, W_(c, c->ce_w[2 * i + 1]), W_(c, c->ce_b[2 * i + 1]), u.p, B, H, Wd, c->ce_ch[i], c->ce_ch[i + 1], 2, 1, c->stream), "controlnet_cond_embedding.blocks (stride 2)");
    wsfree(c, t);
    cur = u; H = Ho; Wd = Wo;
  }
  const int C0 = c->cfg.block_out_channels[0];
  if (c->ce_ch[3] % 64 == 0) op_conv3(c, cur.p, B, H, Wd, c->ce_ch[3], W_(c, c->ce_out_w), W_(c, c->ce_out_b), C0, out);
  else CHECK_LAUNCH(c, ia2p_launch_conv3x3_narrow(cur.p, W_(c, c->ce_out_w), W_(c, c->ce_out_b), out, B, H, Wd, c->ce_ch[3], C0, 1, 0, c->stream), "controlnet_cond_embedding.conv_out");
  wsfree(c, cur);
  return c->failed ? IA2P_ERR_HIP : IA2P_OK;
}
static bool embed_shape_ok(ia2p_ctx* c, int B, int h, int w) { return c && c->cn && B >= 1 && B <= 1024 && h >= 1 && w >= 1 && (int64_t)B * 64 * h * w <= (int64_t)1 << 30; }
size_t ia2p_controlnet_embed_bytes(ia2p_ctx* c, int B, int h, int w) { return embed_shape_ok(c, B, h, w) ? (size_t)B * h * w * c->cfg.block_out_channels[0] * sizeof(half_t) : 0; }
size_t ia2p_controlnet_embed_workspace_bytes(ia2p_ctx* c, int B, int h, int w) {
  if (!embed_shape_ok(c, B, h, w)) return 0;
  return pass_dry(c, [&] { return run_embed(c, nullptr, nullptr, B, h, w); });
}
ia2p_status ia2p_controlnet_embed(ia2p_ctx* c, void* stream, const void* image, int B, int h, int w, void* out, size_t out_bytes, void* ws, size_t ws_bytes) {
  if (!c || !c->cn) return fail(c, IA2P_ERR_STATE, "controlnet_embed: not a ControlNet context");
  if (!image || !out || !ws) return fail(c, IA2P_ERR_INVALID, "controlnet_embed: null argument");
  if (!c->finalized) return fail(c, IA2P_ERR_STATE, "controlnet_embed before weights were finalized");
  if (!embed_shape_ok(c, B, h, w)) return fail(c, IA2P_ERR_SHAPE, "controlnet_embed: B=%d h=%d w=%d", B, h, w);
  if (out_bytes < ia2p_controlnet_embed_bytes(c, B, h, w)) return fail(c, IA2P_ERR_NOMEM, "controlnet_embed: the output holds %zu bytes, needs %zu", out_bytes, ia2p_controlnet_embed_bytes(c, B, h, w));
  ia2p_status st = pass_ready(c, [&] { return fold_all(c, (hipStream_t)stream, true); });
  if (st == IA2P_OK) st = pass_enter(c, stream, ws, ws_bytes);
  if (st != IA2P_OK) return st;
  const bool pf = c->prefetch;
  c->prefetch = false;               // a stand-alone call: no "next launch" to stream weights for
  st = run_embed(c, (const half_t*)image, (half_t*)out, B, h, w);
  c->prefetch = pf;
  c->wseq_key = -1;
  return pass_leave(c, st);
}
size_t ia2p_controlnet_workspace_bytes(ia2p_ctx* c, int B, int h, int w, int L) {
  if (!c || !c->cn || check_fwd_shape(c, B, h, w, L) != IA2P_OK) return 0;
  return forward_workspace(c, FwdCall::shape(B, h, w, L), 3);
}
size_t ia2p_controlnet_context_kv_bytes(ia2p_ctx* c, int B, int L) { return c && c->cn && L > c->ctx_drop ? ia2p_context_kv_bytes(c, B, L) : 0; }
ia2p_status ia2p_controlnet_project_context(ia2p_ctx* c, void* stream, const void* context, int L, int B, void* kv, size_t kv_bytes, void* ws, size_t ws_bytes) {
  if (!c || !c->cn) return fail(c, IA2P_ERR_STATE, "controlnet_project_context: not a ControlNet context");
  if (L <= c->ctx_drop) return fail(c, IA2P_ERR_SHAPE, "controlnet_project_context: context length %d must exceed the %d image-token rows", L, c->ctx_drop);
  return ia2p_project_context(c, stream, context, L, B, kv, kv_bytes, ws, ws_bytes);
}
// One ControlNet evaluation: the `_v` argument shape (per-row timesteps, `context` or cached `kv`) plus the embedded condition (ia2p_controlnet_embed) and the per-image
// conditioning scales (device float [B]). Writes the n_skips + 1 residuals channels-last into `residuals` (ia2p_controlnet_residual_layout).
ia2p_status ia2p_controlnet_forward(ia2p_ctx* c, void* stream, const void* sample, const float* timesteps, const void* context, const void* kv, int L,
                                    const void* text_embeds, const void* time_ids, const void* cond, const float* scales, void* residuals, size_t residual_bytes,
                                    int B, int h, int w, void* ws, size_t ws_bytes) {
  if (!c || !c->cn) return fail(c, IA2P_ERR_STATE, "controlnet_forward: not a ControlNet context");
  if (!sample || !timesteps || (!context) == (!kv) || !text_embeds || !time_ids || !cond || !scales || !residuals || !ws)
    return fail(c, IA2P_ERR_INVALID, "controlnet_forward: null argument (exactly one of context / kv)");
  if ((((uintptr_t)cond) | ((uintptr_t)residuals)) & 15) return fail(c, IA2P_ERR_INVALID, "controlnet_forward: cond and residuals must be 16-byte aligned");
  if (!c->finalized) return fail(c, IA2P_ERR_STATE, "controlnet_forward before weights were finalized");
  ia2p_status st = check_fwd_shape(c, B, h, w, L);
  if (st != IA2P_OK) return st;
  const size_t need = ia2p_controlnet_residual_layout(c, B, h, w, nullptr, nullptr, nullptr, nullptr);
  if (residual_bytes < need) return fail(c, IA2P_ERR_NOMEM, "controlnet_forward: the residual buffer holds %zu bytes, needs %zu", residual_bytes, need);
  FwdCall f = FwdCall::shape(B, h, w, L);
  f.sample = (const half_t*)sample; f.context = (const half_t*)context; f.kv = (const half_t*)kv; f.kv_cached = kv != nullptr;
  f.text_embeds = (const half_t*)text_embeds; f.time_ids = (const half_t*)time_ids; f.timesteps = timesteps;
  f.io.cond = (const half_t*)cond; f.io.scales = scales; f.io.res = (half_t*)residuals;
  return forward_pass(c, stream, ws, ws_bytes, (kv ? 1000 : 0) + c->ctx_drop, f);
}

// ---- context K/V hoisted out of the step: the projections depend on (context, weights) only, constant over a request's steps
size_t ia2p_context_kv_bytes(ia2p_ctx* c, int B, int L) {
  if (!c || B < 1 || L < 1 || (c->ip_enabled && L <= c->ip_tokens)) return 0;
  return (size_t)B * L * c->kv_rows * sizeof(half_t);
}
ia2p_status ia2p_project_context(ia2p_ctx* c, void* stream, const void* context, int L, int B, void* kv, size_t kv_bytes, void* ws, size_t ws_bytes) {
  if (!c || !context || !kv || !ws) return fail(c, IA2P_ERR_INVALID, "project_context: null argument");
  if (!c->finalized) return fail(c, IA2P_ERR_STATE, "project_context before weights were finalized");
  const size_t need = ia2p_context_kv_bytes(c, B, L);
  if (!need) return fail(c, IA2P_ERR_SHAPE, "project_context: B=%d L=%d", B, L);
  if (kv_bytes < need) return fail(c, IA2P_ERR_NOMEM, "project_context: kv buffer holds %zu bytes, needs %zu", kv_bytes, need);
  ia2p_status st = pass_ready(c, [&] { return fold_all(c, (hipStream_t)stream, true); });
  if (st == IA2P_OK) st = pass_enter(c, stream, ws, ws_bytes);
  if (st != IA2P_OK) return st;
  const bool pf = c->prefetch;
  c->prefetch = false;               // a stand-alone call: no "next launch" to stream weights for
  const int Lt = c->ip_enabled ? L - c->ip_tokens : L;
  project_context(c, (const half_t*)context, L, B, (half_t*)kv, (half_t*)kv + (size_t)B * Lt * c->kv_rows);
  c->prefetch = pf;
  c->wseq_key = -1;                  // the launch sequence of the next forward is rebuilt
  return pass_leave(c, IA2P_OK);
}
// Measure-and-pick pass: one forward in which every GEMM / conv site whose shape has no measured plan yet times its
// candidate tile / K-split plans in place (tune_site) and records the fastest in the process-wide plan table.
// Re-query ia2p_workspace_bytes afterwards: K-split choices change the slab sizes.
ia2p_status ia2p_autotune(ia2p_ctx* c, void* stream, const void* sample, float timestep, const void* context, int L, const void* text_embeds,
                          const void* time_ids, void* out, int B, int h, int w, void* ws, size_t ws_bytes, int reps, int* sites) {
  if (!c) return fail(c, IA2P_ERR_INVALID, "autotune: null context");
  const bool prof = c->prof;
  c->prof = false;
  ia2p_status st = tune_begin(c, reps);
  if (st != IA2P_OK) return st;
  st = ia2p_unet_forward(c, stream, sample, timestep, context, L, text_embeds, time_ids, out, B, h, w, ws, ws_bytes);
  tune_end(c, (hipStream_t)stream);
  c->prof = prof;
  if (sites) *sites = c->tune_sites;
  return st;
}

#ifdef IA2P_CLOCK_STAMP
// Diagnostic builds only (IA2P_EXTRA_FLAGS=-DIA2P_CLOCK_STAMP; not declared in the headers, not part of the product library): in-kernel s_memrealtime stamps of the
// launches of one layer role INSIDE a step. buf: device memory, `launch_slots` x STAMP_WG x 8 u64, zeroed by the caller; role: ROLE_* index (ia2p_profile_read_role).
int ia2p_debug_stamp_begin(ia2p_ctx* c, int role, void* buf, int launch_slots) {
  if (!c) return -1;
  c->stamp_buf = (unsigned long long*)buf; c->stamp_role = role; c->stamp_cap = buf ? launch_slots : 0; c->stamp_n = 0; c->stamp_meta.clear();
  return RunCtx::STAMP_WG;
}
// launches stamped since begin; meta (optional): 5 ints per launch {M, N, K, variant, tiles}
int ia2p_debug_stamp_read(ia2p_ctx* c, int* meta, int max_launches) {
  if (!c) return -1;
  for (int i = 0; meta && i < (int)c->stamp_meta.size() && i < max_launches; ++i) {
    const auto& m = c->stamp_meta[i];
    meta[5 * i] = m.M; meta[5 * i + 1] = m.N; meta[5 * i + 2] = m.K; meta[5 * i + 3] = m.variant; meta[5 * i + 4] = m.tiles;
  }
  return (int)c->stamp_meta.size();
}
#endif
ia2p_status ia2p_profile_enable(ia2p_ctx* c, int on) {
  if (!c) return IA2P_ERR_INVALID;
  for (auto& r : c->recs) { c->evpool.push_back(r.e0); c->evpool.push_back(r.e1); }
  c->recs.clear();
  c->prof_zero();
  c->prof = on != 0;
  return IA2P_OK;
}
int ia2p_profile_classes(void) { return PK_NCLASS; }
static void prof_fold(ia2p_ctx* c) {
  for (auto& r : c->recs) {     // fold finished records (synchronises on their stop events)
    float t = 0.f;
    (void)hipEventSynchronize(r.e1);
    (void)hipEventElapsedTime(&t, r.e0, r.e1);
    c->p_ms[r.k] += t; c->p_fl[r.k] += r.flops; c->p_by[r.k] += r.bytes; c->p_pf[r.k] += r.pf; c->p_n[r.k] += 1;
    const int g = r.region >= 0 && r.region < PR_NREGION ? r.region : PR_OTHER;
    c->r_ms[g] += t; c->r_fl[g] += r.flops; c->r_by[g] += r.bytes; c->r_n[g] += 1;
    const int o = r.role >= 0 && r.role < ROLE_NROLE ? r.role : ROLE_OTHER;
    c->o_ms[o] += t; c->o_fl[o] += r.flops; c->o_by[o] += r.bytes; c->o_n[o] += 1;
    c->oc_ms[o][r.k] += t; c->oc_n[o][r.k] += 1;
    c->evpool.push_back(r.e0); c->evpool.push_back(r.e1);
  }
  c->recs.clear();
}
ia2p_status ia2p_profile_read_region(ia2p_ctx* c, int region, int64_t* launches, double* ms, double* flops, double* bytes) {
  if (!c || region < 0 || region >= PR_NREGION) return IA2P_ERR_INVALID;
  prof_fold(c);
  if (launches) *launches = c->r_n[region];
  if (ms) *ms = c->r_ms[region];
  if (flops) *flops = c->r_fl[region];
  if (bytes) *bytes = c->r_by[region];
  return IA2P_OK;
}
// per-ROLE sums (engine_rt.h ROLE_*): the layer a launch implements, whatever kernel instantiation the plan table picked for it
int ia2p_profile_roles(void) { return ROLE_NROLE; }
ia2p_status ia2p_profile_read_role(ia2p_ctx* c, int role, char* name, int name_len, int64_t* launches, double* ms, double* flops, double* bytes) {
  if (!c || role < 0 || role >= ROLE_NROLE) return IA2P_ERR_INVALID;
  prof_fold(c);
  if (name && name_len > 0) { strncpy(name, role_name(role), name_len - 1); name[name_len - 1] = 0; }
  if (launches) *launches = c->o_n[role];
  if (ms) *ms = c->o_ms[role];
  if (flops) *flops = c->o_fl[role];
  if (bytes) *bytes = c->o_by[role];
  return IA2P_OK;
}
// ... and the share of kernel class k in it (which instantiations carried the role on this plan table)
ia2p_status ia2p_profile_read_role_class(ia2p_ctx* c, int role, int k, int64_t* launches, double* ms) {
  if (!c || role < 0 || role >= ROLE_NROLE || k < 0 || k >= PK_NCLASS) return IA2P_ERR_INVALID;
  prof_fold(c);
  if (launches) *launches = c->oc_n[role][k];
  if (ms) *ms = c->oc_ms[role][k];
  return IA2P_OK;
}
// bytes of next-contraction weights that the launches of class k streamed with their trailing prefetch workgroups (part of the class's HBM-side
// traffic that is NOT its own operands: bench.py separates the two when it prices the PMC figure)
ia2p_status ia2p_profile_read_prefetch(ia2p_ctx* c, int k, double* bytes) {
  if (!c || k < 0 || k >= PK_NCLASS || !bytes) return IA2P_ERR_INVALID;
  prof_fold(c);
  *bytes = c->p_pf[k];
  return IA2P_OK;
}
ia2p_status ia2p_profile_read(ia2p_ctx* c, int k, char* name, int name_len, int64_t* launches, double* ms, double* flops, double* bytes) {
  if (!c || k < 0 || k >= PK_NCLASS) return IA2P_ERR_INVALID;
  prof_fold(c);
  if (name && name_len > 0) { strncpy(name, prof_name(k), name_len - 1); name[name_len - 1] = 0; }
  if (launches) *launches = c->p_n[k];
  if (ms) *ms = c->p_ms[k];
  if (flops) *flops = c->p_fl[k];
  if (bytes) *bytes = c->p_by[k];
  return IA2P_OK;
}

}  // extern "C"
