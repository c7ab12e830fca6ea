// LLaMA decoder executor (the instruction LLM) and its C ABI (ia2p_llm_*): see include/ia2p.h and DESIGN.md §10. Runtime and operator wrappers: engine_rt.h / engine_rt.hip.
// Kernels and their launchers: llm_kernels.h (fp16 GEMVs, attention, prefill row kernels), llm_q4.h (the 4-bit format). Here: the context, planning, the prefill and
// decode drivers, the C ABI.
#include "engine_rt.h"
#include "llm_kernels.h"
#include "llm_q4.h"

// =====================================================================================================================
// transformers LlamaModel + lm_head (reference instructany2pix/pipeline.py:201-211 `any2pix_lm.generate`, a Vicuna-7B shaped model):
// pre-RMSNorm blocks, rotary embeddings in the rotate_half convention, multi-head attention at head dim 128, SwiGLU MLP, final norm, untied head.
// Two paths over one fp16 KV cache [slot][layer][k|v][max_positions][hidden]:
//   prefill (T rows of one slot): op_gemm projections + row kernels (RMSNorm, RoPE + cache write, SiLU-multiply) + causal attention against the cache
//   decode (one row of each of 1 to 8 slots): five weight-streaming launches per layer -- QKV GEMV (RMSNorm in, RoPE + cache write out), attention, o_proj
//                     GEMV (+ residual), gate/up GEMV (RMSNorm in, silu(gate) * up out), down_proj GEMV (+ residual); the residual stream of a row stays fp32.
//                     One driver (llm_run_decode_rows): one row runs the single-row GEMV kernels, several the rows kernels.
// The projections of the layers are fp16, or 4-bit codes (ia2p_llm_set_weight_format): decode then runs the same five launches on the 4-bit GEMV kernels and
// prefill dequantises one projection at a time in front of its op_gemm.
// =====================================================================================================================

struct LLayer { size_t ln1, ln2, wqkv, wo, wgu, wd; size_t aqkv, ao, agu, ad; };      // a*: the absmax arrays of the 4-bit format (w*: the packed codes then)
struct ia2p_llm : RunCtx {
  ia2p_llm_config cfg;
  size_t tok, normf, head, invf;
  std::vector<LLayer> layers;
  half_t* kv = nullptr;                                // [slot][layer][k|v][max_pos][hidden]
  int max_pos = 0, n_slots = 0, cur = 0;               // cur: the slot a prefill acts on
  std::vector<int> spos{0};                            // position of every slot
  int wbits = 16;                                      // 16: fp16 projections; 4: codes of `codebook`, block 64, fp32 absmax (ia2p_llm_set_weight_format)
  float codebook[16] = {};
  std::unordered_map<std::string, size_t> q4_absmax;   // projection key -> offset of its absmax rows (arena elements)
};
// arena elements (2 bytes each) of a quantised [N, K]: packed codes, absmax
static size_t q4_code_elems(size_t nk) { return nk / 4; }
static size_t q4_absmax_elems(size_t nk) { return nk / 64 * 2; }

static ia2p_status llm_plan(ia2p_llm* c) {
  const ia2p_llm_config& g = c->cfg;
  const int H = g.hidden_size, I = g.intermediate_size;
  if (g.num_layers < 1 || g.num_heads < 1 || g.vocab_size < 1 || H < 128 || I < 64)
    return fail(c, IA2P_ERR_INVALID, "llm: layers %d, heads %d, vocabulary %d, hidden %d, intermediate %d", g.num_layers, g.num_heads, g.vocab_size, H, I);
  if (H % 64 || g.num_heads * 128 != H) return fail(c, IA2P_ERR_SHAPE, "llm: hidden %d must be a multiple of 64 and heads (%d) * 128 (head dim 128 only)", H, g.num_heads);
  if (g.num_kv_heads != g.num_heads) return fail(c, IA2P_ERR_SHAPE, "llm: %d key/value heads for %d heads (grouped-query attention is not built)", g.num_kv_heads, g.num_heads);
  if (I % 64) return fail(c, IA2P_ERR_SHAPE, "llm: intermediate %d must be a multiple of 64", I);
  const bool q4 = c->wbits == 4;
  if (q4 && (H > Q4_MAX_K || I > Q4_MAX_K)) return fail(c, IA2P_ERR_SHAPE, "llm: 4-bit weights serve rows of up to %d (hidden %d, intermediate %d)", Q4_MAX_K, H, I);
  c->params.clear(); c->layers.clear(); c->q4_absmax.clear();
  ArenaPlan A{c};
  c->tok = A.par("model.embed_tokens.weight", (size_t)g.vocab_size * H);
  for (int i = 0; i < g.num_layers; ++i) {
    const std::string p = "model.layers." + std::to_string(i) + ".";
    LLayer l;
    l.ln1 = A.par(p + "input_layernorm.weight", H);
    // a projection of `parts` equal [rows, K] tensors stacked as rows (blocks never cross a row, so in 4 bits the codes and the absmax rows stack the same way)
    auto proj = [&](size_t* w, size_t* am, const std::vector<std::string>& keys, size_t rows, size_t K) {
      const size_t nk = rows * K, parts = keys.size();
      *w = A.take(q4 ? q4_code_elems(parts * nk) : parts * nk);
      *am = q4 ? A.take(q4_absmax_elems(parts * nk)) : 0;
      for (size_t j = 0; j < parts; ++j) {
        if (!q4) { A.reg(p + keys[j], *w + j * nk, nk); continue; }
        c->params[p + keys[j]] = Param{*w + j * q4_code_elems(nk), nk, PK_Q4, (int)rows, (int)K, false, false};
        c->q4_absmax[p + keys[j]] = *am + j * q4_absmax_elems(nk);
      }
    };
    proj(&l.wqkv, &l.aqkv, {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"}, H, H);     // q | k | v rows stacked: one projection
    proj(&l.wo, &l.ao, {"self_attn.o_proj.weight"}, H, H);
    l.ln2 = A.par(p + "post_attention_layernorm.weight", H);
    proj(&l.wgu, &l.agu, {"mlp.gate_proj.weight", "mlp.up_proj.weight"}, I, H);                                              // gate | up rows stacked
    proj(&l.wd, &l.ad, {"mlp.down_proj.weight"}, H, I);
    c->layers.push_back(l);
  }
  c->normf = A.par("model.norm.weight", H);
  c->head = A.par("lm_head.weight", (size_t)g.vocab_size * H);
  c->invf = A.take(128);                                      // 64 fp32 rotary frequencies (derived at finalize)
  c->arena_elems = A.cur;
  return IA2P_OK;
}

static half_t* KCS(ia2p_llm* c, int slot, int layer) { return c->kv + ((size_t)slot * c->cfg.num_layers + layer) * 2 * c->max_pos * c->cfg.hidden_size; }
static half_t* VCS(ia2p_llm* c, int slot, int layer) { return KCS(c, slot, layer) + (size_t)c->max_pos * c->cfg.hidden_size; }
static half_t* KC(ia2p_llm* c, int layer) { return KCS(c, c->cur, layer); }
static half_t* VC(ia2p_llm* c, int layer) { return VCS(c, c->cur, layer); }
static int& POS(ia2p_llm* c) { return c->spos[c->cur]; }

// final norm + lm_head of the fp32 row xf: hidden_out [H] fp32, logits_out [vocab] fp32
static void llm_head(ia2p_llm* c, const float* xf, float* hidden_out, float* logits_out) {
  LlmGemv a{};
  a.W = W_(c, c->head); a.X = xf; a.gamma = W_(c, c->normf); a.eps = c->cfg.rms_norm_eps; a.N = c->cfg.vocab_size; a.K = c->cfg.hidden_size;
  a.out = logits_out; a.hid = hidden_out;
  CHECK_LAUNCH(c, llm_launch_gemv(a, EPI_PLAIN, c->stream), "llm lm_head");
}

// a prefill projection's fp16 weights: the arena's, or (4 bits) dequantised into `scratch` in front of the GEMM that reads them
static const half_t* llm_proj_f16(ia2p_llm* c, size_t w, size_t am, size_t elems, T2 scratch, const char* what) {
  if (c->wbits != 4) return W_(c, w);
  CHECK_LAUNCH(c, llm_launch_dequantize_q4(W_(c, w), (const float*)W_(c, am), elems, c->codebook, scratch.p, c->stream), what);
  return scratch.p;
}

// one decode projection for the rows of `b`, on the context's weight format
static hipError_t llm_proj_gemv_rows(ia2p_llm* c, LlmGemv& a, const LlmRows& b, size_t w, size_t am, int epi) {
  if (c->wbits != 4) { a.W = W_(c, w); return llm_launch_gemv_rows(a, b, epi, c->stream); }
  return llm_launch_gemv_q4_rows(a, llm_q4(W_(c, w), W_(c, am), c->codebook), b, epi, c->stream);
}

// n rows, row r = token tokens[r] (dev_tokens == nullptr: host ids) or dev_tokens[tokens[r]] (ids in device memory, `tokens` the host indices into them) at
// the position of slot slots[r]: per layer five GEMV launches and one attention launch, each once for all rows
static ia2p_status llm_run_decode_rows(ia2p_llm* c, const int32_t* slots, const int32_t* tokens, const int32_t* dev_tokens, int n, float* hidden_out,
                                       float* logits_out) {
  const ia2p_llm_config& g = c->cfg;
  const int H = g.hidden_size, I = g.intermediate_size;
  T2 xt = wsalloc(c, (size_t)2 * n * H), qt = wsalloc(c, (size_t)2 * n * H), at = wsalloc(c, (size_t)2 * n * H), ft = wsalloc(c, (size_t)2 * n * I);
  float *xf = (float*)xt.p, *qf = (float*)qt.p, *af = (float*)at.p, *ff = (float*)ft.p;
  if (!c->dry && !c->failed) {
    LlmTokRows ids{};
    int longest = 0;
    for (int r = 0; r < n; ++r) { ids.id[r] = tokens[r]; longest = std::max(longest, c->spos[slots[r]] + 1); }
    if (dev_tokens) hipLaunchKernelGGL(llm_rows_dev_f32_kernel, dim3((H + 255) / 256, n), dim3(256), 0, c->stream, W_(c, c->tok), (const int*)dev_tokens, ids, xf, H, g.vocab_size);
    else hipLaunchKernelGGL(llm_rows_f32_kernel, dim3((H + 255) / 256, n), dim3(256), 0, c->stream, W_(c, c->tok), ids, xf, H);
    CHECK_LAUNCH(c, hipGetLastError(), "llm embedding rows");
    auto rows = [&](const float* x, size_t xs, float* out, size_t os) {
      LlmRows b{};
      b.M = n;
      for (int r = 0; r < n; ++r) { b.X[r] = x + r * xs; b.out[r] = out ? out + r * os : nullptr; }
      return b;
    };
    for (int i = 0; i < g.num_layers && !c->failed; ++i) {
      const LLayer& l = c->layers[i];
      LlmGemv a{};
      a.gamma = W_(c, l.ln1); a.eps = g.rms_norm_eps; a.N = 3 * H; a.K = H; a.H = H; a.inv_freq = (const float*)W_(c, c->invf);
      LlmRows b = rows(xf, H, nullptr, 0);
      LlmAttnRows ar{};
      for (int r = 0; r < n; ++r) {
        b.q[r] = qf + (size_t)r * H; b.kc[r] = KCS(c, slots[r], i); b.vc[r] = VCS(c, slots[r], i); b.pos[r] = c->spos[slots[r]];
        ar.kc[r] = b.kc[r]; ar.vc[r] = b.vc[r]; ar.pos[r] = b.pos[r];
      }
      CHECK_LAUNCH(c, llm_proj_gemv_rows(c, a, b, l.wqkv, l.aqkv, EPI_QKV), "llm qkv rows");
      hipLaunchKernelGGL(llm_attn_rows_kernel, dim3(g.num_heads, n), dim3(256), attn_lds(longest), c->stream, (const float*)qf, ar, af, H, 0.08838834764831845f);
      CHECK_LAUNCH(c, hipGetLastError(), "llm attention rows");
      LlmGemv o{};
      o.N = H; o.K = H;
      CHECK_LAUNCH(c, llm_proj_gemv_rows(c, o, rows(af, H, xf, H), l.wo, l.ao, EPI_RESID), "llm o_proj rows");
      LlmGemv u{};
      u.gamma = W_(c, l.ln2); u.eps = g.rms_norm_eps; u.N = 2 * I; u.K = H;
      CHECK_LAUNCH(c, llm_proj_gemv_rows(c, u, rows(xf, H, ff, I), l.wgu, l.agu, EPI_SWIGLU), "llm gate/up rows");
      LlmGemv d{};
      d.N = H; d.K = I;
      CHECK_LAUNCH(c, llm_proj_gemv_rows(c, d, rows(ff, I, xf, H), l.wd, l.ad, EPI_RESID), "llm down_proj rows");
    }
    LlmGemv h{};          // final norm + lm_head of every row
    h.W = W_(c, c->head); h.gamma = W_(c, c->normf); h.eps = g.rms_norm_eps; h.N = g.vocab_size; h.K = H;
    LlmRows hb = rows(xf, H, logits_out, g.vocab_size);
    for (int r = 0; r < n; ++r) hb.hid[r] = hidden_out + (size_t)r * H;
    CHECK_LAUNCH(c, llm_launch_gemv_rows(h, hb, EPI_PLAIN, c->stream), "llm lm_head rows");
  }
  wsfree(c, ft); wsfree(c, at); wsfree(c, qt); wsfree(c, xt);
  return c->failed ? IA2P_ERR_HIP : IA2P_OK;
}

static ia2p_status llm_run_prefill(ia2p_llm* c, const half_t* embeds, int T, float* hidden_out, float* logits_out) {
  const ia2p_llm_config& g = c->cfg;
  const int H = g.hidden_size, I = g.intermediate_size, p0 = POS(c);
  T2 x = wsalloc(c, (size_t)T * H), xn = wsalloc(c, (size_t)T * H), qkv = wsalloc(c, (size_t)T * 3 * H), qt = wsalloc(c, (size_t)T * H * 2);
  T2 att = wsalloc(c, (size_t)T * H), gu = wsalloc(c, (size_t)T * 2 * I), act = wsalloc(c, (size_t)T * I), xt = wsalloc(c, (size_t)2 * H);
  T2 wq{(size_t)-1, nullptr};           // 4 bits: one projection at a time as fp16 (the largest: gate | up)
  if (c->wbits == 4) wq = wsalloc(c, std::max((size_t)3 * H * H, (size_t)2 * I * H));
  float *qf = (float*)qt.p, *xf = (float*)xt.p;
  if (!c->dry && !c->failed) {
    hipError_t e = hipMemcpyAsync(x.p, embeds, (size_t)T * H * sizeof(half_t), hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) fail_hip(c, e, "llm prefill");
  }
  for (int i = 0; i < g.num_layers; ++i) {
    const LLayer& l = c->layers[i];
    if (!c->dry && !c->failed) {
      hipLaunchKernelGGL(llm_rmsnorm_rows_kernel, dim3(T), dim3(256), 0, c->stream, (const half_t*)x.p, xn.p, W_(c, l.ln1), H, g.rms_norm_eps);
      CHECK_LAUNCH(c, hipGetLastError(), "llm input_layernorm");
    }
    op_gemm(c, xn.p, H, llm_proj_f16(c, l.wqkv, l.aqkv, (size_t)3 * H * H, wq, "llm dequantize qkv"), nullptr, nullptr, 0, qkv.p, 3 * H, T, 3 * H, H);
    if (!c->dry && !c->failed) {
      hipLaunchKernelGGL(llm_rope_cache_rows_kernel, dim3(T), dim3(256), 0, c->stream, (const half_t*)qkv.p, qf, KC(c, i), VC(c, i), (const float*)W_(c, c->invf), H, p0);
      CHECK_LAUNCH(c, hipGetLastError(), "llm rope");
      hipLaunchKernelGGL(llm_attn_kernel<half_t>, dim3(g.num_heads, T), dim3(256), attn_lds(p0 + T), c->stream, (const float*)qf, (const half_t*)KC(c, i), (const half_t*)VC(c, i), att.p, H, p0,
                         0.08838834764831845f);
      CHECK_LAUNCH(c, hipGetLastError(), "llm attention");
    }
    op_gemm(c, att.p, H, llm_proj_f16(c, l.wo, l.ao, (size_t)H * H, wq, "llm dequantize o_proj"), nullptr, x.p, H, x.p, H, T, H, H);
    if (!c->dry && !c->failed) {
      hipLaunchKernelGGL(llm_rmsnorm_rows_kernel, dim3(T), dim3(256), 0, c->stream, (const half_t*)x.p, xn.p, W_(c, l.ln2), H, g.rms_norm_eps);
      CHECK_LAUNCH(c, hipGetLastError(), "llm post_attention_layernorm");
    }
    op_gemm(c, xn.p, H, llm_proj_f16(c, l.wgu, l.agu, (size_t)2 * I * H, wq, "llm dequantize gate/up"), nullptr, nullptr, 0, gu.p, 2 * I, T, 2 * I, H);
    if (!c->dry && !c->failed) {
      hipLaunchKernelGGL(llm_silu_mul_rows_kernel, dim3(T), dim3(256), 0, c->stream, (const half_t*)gu.p, act.p, I);
      CHECK_LAUNCH(c, hipGetLastError(), "llm silu-multiply");
    }
    op_gemm(c, act.p, I, llm_proj_f16(c, l.wd, l.ad, (size_t)H * I, wq, "llm dequantize down_proj"), nullptr, x.p, H, x.p, H, T, H, I);
  }
  if (!c->dry && !c->failed) {          // only the last row goes through model.norm and lm_head
    hipLaunchKernelGGL(llm_row_f32_kernel, dim3((H + 255) / 256), dim3(256), 0, c->stream, (const half_t*)(x.p + (size_t)(T - 1) * H), xf, H);
    CHECK_LAUNCH(c, hipGetLastError(), "llm last row");
    llm_head(c, xf, hidden_out, logits_out);
  }
  if (c->wbits == 4) wsfree(c, wq);
  wsfree(c, xt); wsfree(c, act); wsfree(c, gu); wsfree(c, att); wsfree(c, qt); wsfree(c, qkv); wsfree(c, xn); wsfree(c, x);
  return c->failed ? IA2P_ERR_HIP : IA2P_OK;
}

// workspace need of a prefill of T rows (T > 0) or of a decode step of n rows: a host dry run
static size_t llm_dry(ia2p_llm* c, int T, int n = 1) {
  return pass_dry(c, [&] { return T > 0 ? llm_run_prefill(c, nullptr, T, nullptr, nullptr) : llm_run_decode_rows(c, nullptr, nullptr, nullptr, n, nullptr, nullptr); });
}
static ia2p_status llm_ready(ia2p_llm* c, const char* what) {
  if (!c->finalized) return fail(c, IA2P_ERR_STATE, "%s before weights were finalized", what);
  if (!c->kv) return fail(c, IA2P_ERR_STATE, "%s before ia2p_llm_bind_kv", what);
  return IA2P_OK;
}
// exact: the batched decode takes `need` as the least size of an aligned workspace (the earlier entry points allow the alignment slack to be missing)
static ia2p_status llm_enter(ia2p_llm* c, void* stream, void* ws, size_t ws_bytes, size_t need, bool exact = false) {
  const size_t lost = (size_t)(-(uintptr_t)ws & 255);      // what aligning ws to 256 bytes costs
  if (need == 0 || ws_bytes < lost || ws_bytes - lost + (exact ? 0 : 256) < need) return fail(c, IA2P_ERR_NOMEM, "llm: workspace of %zu bytes, %zu needed", ws_bytes, need);
  c->wseq.clear();      // (no prefetch plan: the decode launches stream their own weights)
  return pass_enter(c, stream, ws, ws_bytes);
}

// transformers LlamaRotaryEmbedding: inv_freq[i] = 1 / theta^(2 i / 128), fp32 (the table ia2p_llm_finalize_weights uploads and ia2p_llm_rope_inv_freq returns)
static void llm_rope_inv_freq(float theta, float* f) {
  for (int i = 0; i < 64; ++i) f[i] = 1.0f / powf(theta, (float)(2 * i) / 128.0f);
}

extern "C" {

ia2p_status ia2p_llm_create(const ia2p_llm_config* cfg, ia2p_llm** out) {
  return rc_create(cfg, out, "ia2p_llm_create", [](ia2p_llm* c) {
    if (c->cfg.rms_norm_eps <= 0.f) c->cfg.rms_norm_eps = 1e-5f;
    if (c->cfg.rope_theta <= 0.f) c->cfg.rope_theta = 10000.f;
    return llm_plan(c);
  });
}
void ia2p_llm_destroy(ia2p_llm* c) { delete c; }
const char* ia2p_llm_last_error(ia2p_llm* c) { return rc_last_error(c); }
size_t ia2p_llm_arena_bytes(ia2p_llm* c) { return rc_arena_bytes(c); }
ia2p_status ia2p_llm_bind_arena(ia2p_llm* c, void* dev, size_t bytes) { return rc_bind_arena(c, dev, bytes); }
ia2p_status ia2p_llm_load_tensor(ia2p_llm* c, const char* key, const void* src, const int64_t* shape, int ndim, void* stream) {
  if (!c || !key || !src || !shape || !c->arena) return rc_load_tensor(c, key, src, shape, ndim, stream);      // (its refusals)
  auto it = c->params.find(key);
  if (it == c->params.end() || it->second.kind != PK_Q4) return rc_load_tensor(c, key, src, shape, ndim, stream);
  Param& p = it->second;              // a 4-bit projection: quantised from the fp16 tensor into the arena
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  if (n != p.elems) return fail(c, IA2P_ERR_SHAPE, "parameter '%s': expected %zu elements, got %zu", key, p.elems, n);
  hipError_t e = llm_launch_quantize_q4((const half_t*)src, n, c->codebook, c->arena + p.off, (float*)(c->arena + c->q4_absmax[key]), (hipStream_t)stream);
  if (e != hipSuccess) return fail_hip(c, e, (std::string("quantize '") + key + "'").c_str());
  p.loaded = true;
  return IA2P_OK;
}
ia2p_status ia2p_llm_set_weight_format(ia2p_llm* c, int bits, const float* codebook) {
  if (!c) return fail(nullptr, IA2P_ERR_INVALID, "llm_set_weight_format: null argument");
  if (bits != 16 && bits != 4) return fail(c, IA2P_ERR_INVALID, "llm_set_weight_format: %d bits (16 or 4)", bits);
  if (bits == 4 && !codebook) return fail(c, IA2P_ERR_INVALID, "llm_set_weight_format: 4 bits need a codebook of 16 values");
  if (c->arena) return fail(c, IA2P_ERR_STATE, "llm_set_weight_format after ia2p_llm_bind_arena");
  const int old = c->wbits;
  c->wbits = bits;
  if (bits == 4) memcpy(c->codebook, codebook, sizeof c->codebook);
  const ia2p_status st = llm_plan(c);
  if (st != IA2P_OK) { c->wbits = old; (void)llm_plan(c); c->failed = false; }
  return st;
}
int ia2p_llm_weight_bits(ia2p_llm* c) { return c ? c->wbits : 0; }
size_t ia2p_llm_q4_packed_bytes(int64_t N, int64_t K) { return N < 1 || K < 64 || K % 64 ? 0 : (size_t)N * (size_t)K / 2; }
ia2p_status ia2p_llm_quantize_q4(void* stream, const void* W, int64_t N, int64_t K, const float* codebook, void* packed, float* absmax) {
  const ia2p_status st = q4_op_args("llm_quantize_q4", W, packed, absmax, codebook, N, K);
  if (st != IA2P_OK) return st;
  hipError_t e = llm_launch_quantize_q4((const half_t*)W, (size_t)(N * K), codebook, packed, absmax, (hipStream_t)stream);
  RET_HIP(e, "llm_quantize_q4");
}
ia2p_status ia2p_llm_dequantize_q4(void* stream, const void* packed, const float* absmax, int64_t N, int64_t K, const float* codebook, void* W) {
  const ia2p_status st = q4_op_args("llm_dequantize_q4", packed, absmax, W, codebook, N, K);
  if (st != IA2P_OK) return st;
  hipError_t e = llm_launch_dequantize_q4(packed, absmax, (size_t)(N * K), codebook, (half_t*)W, (hipStream_t)stream);
  RET_HIP(e, "llm_dequantize_q4");
}
ia2p_status ia2p_llm_gemv_q4(void* stream, const void* packed, const float* absmax, const float* codebook, const float* x, float* out, int N, int K) {
  if (!out) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv_q4: null argument");
  const ia2p_status st = llm_gemv_q4_check(packed, absmax, codebook, x, N, K, 0, 1, EPI_PLAIN);
  if (st != IA2P_OK) return llm_refuse("llm_gemv_q4", st, N, K, 64, Q4_MAX_K, 1);
  LlmGemv a{};
  a.X = x; a.N = N; a.K = K; a.out = out;
  hipError_t e = llm_launch_gemv_q4(a, llm_q4(packed, absmax, codebook), EPI_PLAIN, (hipStream_t)stream);
  RET_HIP(e, "llm_gemv_q4");
}
ia2p_status ia2p_llm_finalize_weights(ia2p_llm* c) {
  const ia2p_status st = rc_finalize(c, "LLM");
  if (st != IA2P_OK) return st;
  float f[64];
  llm_rope_inv_freq(c->cfg.rope_theta, f);
  hipError_t e = hipMemcpy(c->arena + c->invf, f, sizeof f, hipMemcpyHostToDevice);
  if (e != hipSuccess) { c->finalized = false; return fail_hip(c, e, "llm rotary table"); }
  return IA2P_OK;
}
size_t ia2p_llm_kv_slots_bytes(ia2p_llm* c, int max_positions, int n_slots) {
  if (!c || n_slots < 1 || max_positions < 1 || max_positions > LLM_MAX_POSITIONS) return 0;
  return (size_t)n_slots * c->cfg.num_layers * 2 * (size_t)max_positions * c->cfg.hidden_size * sizeof(half_t);
}
size_t ia2p_llm_kv_bytes(ia2p_llm* c, int max_positions) { return ia2p_llm_kv_slots_bytes(c, max_positions, 1); }
static ia2p_status llm_bind_slots(ia2p_llm* c, const char* what, void* dev, size_t bytes, int max_positions, int n_slots) {
  if (!c || !dev) return fail(c, IA2P_ERR_INVALID, "%s: null argument", what);
  if (n_slots < 1) return fail(c, IA2P_ERR_INVALID, "%s: %d slots", what, n_slots);
  if (max_positions < 1 || max_positions > LLM_MAX_POSITIONS) return fail(c, IA2P_ERR_SHAPE, "%s: %d positions (1..%d)", what, max_positions, LLM_MAX_POSITIONS);
  if (((uintptr_t)dev) & 15) return fail(c, IA2P_ERR_INVALID, "%s: the cache must be 16-byte aligned", what);
  const size_t need = ia2p_llm_kv_slots_bytes(c, max_positions, n_slots);
  if (bytes < need) return fail(c, IA2P_ERR_NOMEM, "%s: %zu bytes, %zu needed", what, bytes, need);
  c->kv = (half_t*)dev; c->max_pos = max_positions; c->n_slots = n_slots; c->cur = 0;
  c->spos.assign((size_t)n_slots, 0);
  return IA2P_OK;
}
ia2p_status ia2p_llm_bind_kv(ia2p_llm* c, void* dev, size_t bytes, int max_positions) { return llm_bind_slots(c, "llm_bind_kv", dev, bytes, max_positions, 1); }
ia2p_status ia2p_llm_bind_kv_slots(ia2p_llm* c, void* dev, size_t bytes, int max_positions, int n_slots) {
  return llm_bind_slots(c, "llm_bind_kv_slots", dev, bytes, max_positions, n_slots);
}
int ia2p_llm_slots(ia2p_llm* c) { return c ? c->n_slots : 0; }
size_t ia2p_llm_workspace_bytes(ia2p_llm* c, int max_T) {
  if (!c || max_T < 1) return 0;
  const size_t a = llm_dry(c, max_T), b = llm_dry(c, 0);
  return a && b ? std::max(a, b) : 0;
}
size_t ia2p_llm_batch_workspace_bytes(ia2p_llm* c, int max_T, int max_rows) {
  if (!c || max_T < 0 || max_rows < 1 || max_rows > LLM_MAX_ROWS) return 0;
  size_t a = 1;       // every T up to max_T: a prefill's need is not monotone in T (the K-split of its GEMMs changes with the row count)
  for (int T = 1; T <= max_T && a; ++T) { const size_t t = llm_dry(c, T); a = t ? std::max(a, t) : 0; }
  const size_t b = llm_dry(c, 0, max_rows);
  return a && b ? std::max(a, b) : 0;
}
ia2p_status ia2p_llm_reset(ia2p_llm* c) {
  if (!c) return fail(nullptr, IA2P_ERR_INVALID, "llm_reset: null argument");
  c->spos[0] = 0;
  return IA2P_OK;
}
int ia2p_llm_position(ia2p_llm* c) { return c ? c->spos[0] : -1; }
ia2p_status ia2p_llm_reset_slot(ia2p_llm* c, int slot) {
  if (!c) return fail(nullptr, IA2P_ERR_INVALID, "llm_reset_slot: null argument");
  if (slot < 0 || slot >= c->n_slots) return fail(c, IA2P_ERR_INVALID, "llm_reset_slot: slot %d of %d", slot, c->n_slots);
  c->spos[slot] = 0;
  return IA2P_OK;
}
int ia2p_llm_slot_position(ia2p_llm* c, int slot) { return c && slot >= 0 && slot < c->n_slots ? c->spos[slot] : -1; }
ia2p_status ia2p_llm_embed(ia2p_llm* c, void* stream, const int32_t* ids, int T, void* out) {
  if (!c || !ids || !out) return fail(c, IA2P_ERR_INVALID, "llm_embed: null argument");
  if (T < 1) return fail(c, IA2P_ERR_SHAPE, "llm_embed: T=%d", T);
  if (!c->finalized) return fail(c, IA2P_ERR_STATE, "llm_embed before weights were finalized");
  hipLaunchKernelGGL(llm_gather_rows_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream, (const int*)ids, W_(c, c->tok), (half_t*)out, c->cfg.hidden_size, c->cfg.vocab_size);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? IA2P_OK : fail_hip(c, e, "llm_embed");
}
static ia2p_status llm_prefill_at(ia2p_llm* c, const char* what, int slot, void* stream, const void* inputs_embeds, int T, float* hidden_out, float* logits_out, void* ws,
                                  size_t ws_bytes) {
  if (!c || !inputs_embeds || !hidden_out || !logits_out || !ws) return fail(c, IA2P_ERR_INVALID, "%s: null argument", what);
  ia2p_status st = llm_ready(c, what);
  if (st != IA2P_OK) return st;
  if (slot < 0 || slot >= c->n_slots) return fail(c, IA2P_ERR_INVALID, "%s: slot %d of %d", what, slot, c->n_slots);
  const int pos = c->spos[slot];
  if (T < 1 || pos + T > c->max_pos) return fail(c, IA2P_ERR_SHAPE, "%s: %d rows at position %d, the cache holds %d", what, T, pos, c->max_pos);
  if (!zero_page()) return fail(c, IA2P_ERR_HIP, "cannot allocate zero page");
  c->cur = slot;
  st = llm_enter(c, stream, ws, ws_bytes, llm_dry(c, T));
  if (st == IA2P_OK) st = pass_leave(c, llm_run_prefill(c, (const half_t*)inputs_embeds, T, hidden_out, logits_out));
  c->cur = 0;
  if (st == IA2P_OK) c->spos[slot] += T;
  return st;
}
ia2p_status ia2p_llm_prefill(ia2p_llm* c, void* stream, const void* inputs_embeds, int T, float* hidden_out, float* logits_out, void* ws, size_t ws_bytes) {
  return llm_prefill_at(c, "llm_prefill", 0, stream, inputs_embeds, T, hidden_out, logits_out, ws, ws_bytes);
}
ia2p_status ia2p_llm_prefill_slot(ia2p_llm* c, void* stream, int slot, const void* inputs_embeds, int T, float* hidden_out, float* logits_out, void* ws, size_t ws_bytes) {
  return llm_prefill_at(c, "llm_prefill_slot", slot, stream, inputs_embeds, T, hidden_out, logits_out, ws, ws_bytes);
}
ia2p_status ia2p_llm_decode(ia2p_llm* c, void* stream, int token_id, float* hidden_out, float* logits_out, void* ws, size_t ws_bytes) {
  if (!c || !hidden_out || !logits_out || !ws) return fail(c, IA2P_ERR_INVALID, "llm_decode: null argument");
  ia2p_status st = llm_ready(c, "llm_decode");
  if (st != IA2P_OK) return st;
  const int pos = c->spos[0];
  if (pos < 1) return fail(c, IA2P_ERR_STATE, "llm_decode before a prefill (position 0)");
  if (pos >= c->max_pos) return fail(c, IA2P_ERR_SHAPE, "llm_decode: position %d is past the cache (%d positions)", pos, c->max_pos);
  if (token_id < 0 || token_id >= c->cfg.vocab_size) return fail(c, IA2P_ERR_SHAPE, "llm_decode: token %d outside the vocabulary (%d)", token_id, c->cfg.vocab_size);
  st = llm_enter(c, stream, ws, ws_bytes, llm_dry(c, 0));
  if (st != IA2P_OK) return st;
  const int32_t slot = 0, token = token_id;
  st = pass_leave(c, llm_run_decode_rows(c, &slot, &token, nullptr, 1, hidden_out, logits_out));
  if (st == IA2P_OK) c->spos[0] += 1;
  return st;
}
// the batched decode step behind both entry points: `tokens` are host ids (dev_tokens == nullptr; checked against the vocabulary) or host indices into dev_tokens
static ia2p_status llm_decode_rows_at(ia2p_llm* c, const char* what, void* stream, const int32_t* slots, const int32_t* tokens, const int32_t* dev_tokens, int n,
                                      float* hidden_out, float* logits_out, void* ws, size_t ws_bytes) {
  if (!c || !slots || !tokens || !hidden_out || !logits_out || !ws) return fail(c, IA2P_ERR_INVALID, "%s: null argument", what);
  ia2p_status st = llm_ready(c, what);
  if (st != IA2P_OK) return st;
  if (n < 1 || n > LLM_MAX_ROWS) return fail(c, IA2P_ERR_INVALID, "%s: %d rows (1..%d)", what, n, LLM_MAX_ROWS);
  for (int r = 0; r < n; ++r) {
    if (slots[r] < 0 || slots[r] >= c->n_slots) return fail(c, IA2P_ERR_INVALID, "%s: row %d names slot %d, the cache has %d", what, r, slots[r], c->n_slots);
    for (int p = 0; p < r; ++p)
      if (slots[p] == slots[r]) return fail(c, IA2P_ERR_INVALID, "%s: slot %d is named twice (rows %d and %d)", what, slots[r], p, r);
  }
  for (int r = 0; r < n; ++r) {
    const int pos = c->spos[slots[r]];
    if (pos < 1) return fail(c, IA2P_ERR_STATE, "%s: slot %d before a prefill (position 0)", what, slots[r]);
    if (pos >= c->max_pos) return fail(c, IA2P_ERR_SHAPE, "%s: slot %d at position %d is past the cache (%d positions)", what, slots[r], pos, c->max_pos);
    if (dev_tokens) {
      if (tokens[r] < 0) return fail(c, IA2P_ERR_INVALID, "%s: token index %d of row %d", what, tokens[r], r);
    } else if (tokens[r] < 0 || tokens[r] >= c->cfg.vocab_size) {
      return fail(c, IA2P_ERR_SHAPE, "%s: token %d of row %d outside the vocabulary (%d)", what, tokens[r], r, c->cfg.vocab_size);
    }
  }
  st = llm_enter(c, stream, ws, ws_bytes, llm_dry(c, 0, n), true);
  if (st != IA2P_OK) return st;
  st = pass_leave(c, llm_run_decode_rows(c, slots, tokens, dev_tokens, n, hidden_out, logits_out));
  if (st == IA2P_OK)
    for (int r = 0; r < n; ++r) c->spos[slots[r]] += 1;
  return st;
}
ia2p_status ia2p_llm_decode_batch(ia2p_llm* c, void* stream, const int32_t* slots, const int32_t* token_ids, int n, float* hidden_out, float* logits_out, void* ws,
                                  size_t ws_bytes) {
  return llm_decode_rows_at(c, "llm_decode_batch", stream, slots, token_ids, nullptr, n, hidden_out, logits_out, ws, ws_bytes);
}
ia2p_status ia2p_llm_decode_batch_dev(ia2p_llm* c, void* stream, const int32_t* slots, const int32_t* dev_tokens, const int32_t* token_index, int n, float* hidden_out,
                                      float* logits_out, void* ws, size_t ws_bytes) {
  if (!dev_tokens) return fail(c, IA2P_ERR_INVALID, "llm_decode_batch_dev: null argument");
  if (((uintptr_t)dev_tokens) & 3) return fail(c, IA2P_ERR_INVALID, "llm_decode_batch_dev: the token buffer must be 4-byte aligned");
  static const int32_t in_order[LLM_MAX_ROWS] = {0, 1, 2, 3, 4, 5, 6, 7};
  return llm_decode_rows_at(c, "llm_decode_batch_dev", stream, slots, token_index ? token_index : in_order, dev_tokens, n, hidden_out, logits_out, ws, ws_bytes);
}
static LlmRows gemv_rows_args(const float* x, float* out, int N, int K, int M) {
  LlmRows b{};
  b.M = M;
  for (int m = 0; m < M; ++m) { b.X[m] = x + (size_t)m * K; b.out[m] = out + (size_t)m * N; }
  return b;
}
ia2p_status ia2p_llm_gemv_rows(void* stream, const void* W, const float* x, float* out, int N, int K, int M) {
  if (!out) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv_rows: null argument");
  const ia2p_status st = llm_gemv_check(W, x, N, K, 0, M, EPI_PLAIN);
  if (st != IA2P_OK) return llm_refuse("llm_gemv_rows", st, N, K, 8, 0, M);
  LlmGemv a{};
  a.W = (const half_t*)W; a.N = N; a.K = K;
  hipError_t e = llm_launch_gemv_rows(a, gemv_rows_args(x, out, N, K, M), EPI_PLAIN, (hipStream_t)stream);
  RET_HIP(e, "llm_gemv_rows");
}
ia2p_status ia2p_llm_gemv_q4_rows(void* stream, const void* packed, const float* absmax, const float* codebook, const float* x, float* out, int N, int K, int M) {
  if (!out) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv_q4_rows: null argument");
  const ia2p_status st = llm_gemv_q4_check(packed, absmax, codebook, x, N, K, 0, M, EPI_PLAIN);
  if (st != IA2P_OK) return llm_refuse("llm_gemv_q4_rows", st, N, K, 64, Q4_MAX_K, M);
  LlmGemv a{};
  a.N = N; a.K = K;
  hipError_t e = llm_launch_gemv_q4_rows(a, llm_q4(packed, absmax, codebook), gemv_rows_args(x, out, N, K, M), EPI_PLAIN, (hipStream_t)stream);
  RET_HIP(e, "llm_gemv_q4_rows");
}
ia2p_status ia2p_llm_gemv(void* stream, const void* W, const float* x, float* out, int N, int K) {
  if (!out) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv: null argument");
  const ia2p_status st = llm_gemv_check(W, x, N, K, 0, 1, EPI_PLAIN);
  if (st != IA2P_OK) return llm_refuse("llm_gemv", st, N, K, 8, 0, 1);
  LlmGemv a{};
  a.W = (const half_t*)W; a.X = x; a.N = N; a.K = K; a.out = out;
  hipError_t e = llm_launch_gemv(a, EPI_PLAIN, (hipStream_t)stream);
  RET_HIP(e, "llm_gemv");
}
// ---- the remaining launches of the decode and prefill paths on their own: the launchers and kernels the drivers run, every refusal made here on the host ----
// fp16 weights (absmax and codebook both null) or 4-bit codes (both given); the shared refusals of the two GEMV entry points below
static ia2p_status llm_gemv_op_check(const char* what, const void* W, const float* absmax, const float* codebook, const float* x, const void* gamma, float eps, int N, int K,
                                     int H, int M, int epi) {
  if ((absmax == nullptr) != (codebook == nullptr)) return fail(nullptr, IA2P_ERR_INVALID, "%s: absmax and codebook go together (both: 4-bit codes, neither: fp16 weights)", what);
  if (gamma && !(eps >= 0.f && eps < INFINITY)) return fail(nullptr, IA2P_ERR_INVALID, "%s: eps=%g", what, (double)eps);
  const bool q4 = absmax != nullptr;
  const ia2p_status st = q4 ? llm_gemv_q4_check(W, absmax, codebook, x, N, K, H, M, epi) : llm_gemv_check(W, x, N, K, H, M, epi);
  if (st == IA2P_ERR_SHAPE && N >= 1 && !llm_epi_shape_ok(epi, N, H)) return fail(nullptr, st, "%s: N=%d H=%d (SwiGLU: N even; QKV: N = 3 H, H = heads * 128)", what, N, H);
  return st == IA2P_OK ? st : q4 ? llm_refuse(what, st, N, K, 64, Q4_MAX_K, M) : llm_refuse(what, st, N, K, 8, 0, M);
}
static bool llm_positions_ok(const int32_t* pos, int M) {
  for (int m = 0; m < M; ++m)
    if (pos[m] < 0 || pos[m] >= LLM_MAX_POSITIONS) return false;
  return true;
}
ia2p_status ia2p_llm_gemv_epi(void* stream, const void* W, const float* absmax, const float* codebook, const float* x, const void* gamma, float eps, int epi, float* out,
                              float* hid, int N, int K, int M) {
  static const int epis[3] = {EPI_PLAIN, EPI_RESID, EPI_SWIGLU};
  if (!out) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv_epi: null argument");
  if (epi < 0 || epi > 2) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv_epi: epilogue %d (0 plain, 1 residual, 2 SwiGLU)", epi);
  if (hid && (epi != IA2P_LLM_EPI_PLAIN || !gamma)) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv_epi: hid goes with the plain epilogue and a gamma");
  const ia2p_status st = llm_gemv_op_check("llm_gemv_epi", W, absmax, codebook, x, gamma, eps, N, K, 0, M, epis[epi]);
  if (st != IA2P_OK) return st;
  LlmGemv a{};
  a.W = absmax ? nullptr : (const half_t*)W; a.gamma = (const half_t*)gamma; a.eps = eps; a.N = N; a.K = K;
  LlmRows b = gemv_rows_args(x, out, epi == IA2P_LLM_EPI_SWIGLU ? N / 2 : N, K, M);
  for (int m = 0; m < M; ++m) b.hid[m] = hid ? hid + (size_t)m * K : nullptr;
  hipError_t e = absmax ? llm_launch_gemv_q4_rows(a, llm_q4(W, absmax, codebook), b, epis[epi], (hipStream_t)stream) : llm_launch_gemv_rows(a, b, epis[epi], (hipStream_t)stream);
  RET_HIP(e, "llm_gemv_epi");
}
ia2p_status ia2p_llm_gemv_qkv(void* stream, const void* W, const float* absmax, const float* codebook, const float* x, const void* gamma, float eps, const float* inv_freq,
                              const int32_t* pos, float* q, void* const* k_cache, void* const* v_cache, int H, int K, int M) {
  if (!inv_freq || !pos || !q || !k_cache || !v_cache) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv_qkv: null argument");
  if (H < 128 || H > (1 << 20)) return fail(nullptr, IA2P_ERR_SHAPE, "llm_gemv_qkv: H=%d (heads * 128)", H);
  const ia2p_status st = llm_gemv_op_check("llm_gemv_qkv", W, absmax, codebook, x, gamma, eps, 3 * H, K, H, M, EPI_QKV);
  if (st != IA2P_OK) return st;
  for (int m = 0; m < M; ++m)
    if (!k_cache[m] || !v_cache[m]) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv_qkv: null cache of row %d", m);
  if (!llm_positions_ok(pos, M)) return fail(nullptr, IA2P_ERR_SHAPE, "llm_gemv_qkv: a position outside 0..%d", LLM_MAX_POSITIONS - 1);
  LlmGemv a{};
  a.W = absmax ? nullptr : (const half_t*)W; a.gamma = (const half_t*)gamma; a.eps = eps; a.N = 3 * H; a.K = K; a.H = H; a.inv_freq = inv_freq;
  LlmRows b{};
  b.M = M;
  for (int m = 0; m < M; ++m) { b.X[m] = x + (size_t)m * K; b.q[m] = q + (size_t)m * H; b.kc[m] = (half_t*)k_cache[m]; b.vc[m] = (half_t*)v_cache[m]; b.pos[m] = pos[m]; }
  hipError_t e = absmax ? llm_launch_gemv_q4_rows(a, llm_q4(W, absmax, codebook), b, EPI_QKV, (hipStream_t)stream) : llm_launch_gemv_rows(a, b, EPI_QKV, (hipStream_t)stream);
  RET_HIP(e, "llm_gemv_qkv");
}
// heads and H of an attention entry point
static ia2p_status llm_attn_shape(const char* what, int heads, int H) {
  if (heads < 1 || heads > 65535 || H != heads * 128) return fail(nullptr, IA2P_ERR_SHAPE, "%s: H=%d for %d heads (head dim 128 only)", what, H, heads);
  return IA2P_OK;
}
ia2p_status ia2p_llm_attention_rows(void* stream, const float* q, const void* const* k_cache, const void* const* v_cache, const int32_t* pos, float* out, int heads, int H,
                                    int M) {
  if (!q || !k_cache || !v_cache || !pos || !out) return fail(nullptr, IA2P_ERR_INVALID, "llm_attention_rows: null argument");
  const ia2p_status st = llm_attn_shape("llm_attention_rows", heads, H);
  if (st != IA2P_OK) return st;
  if (M < 1 || M > LLM_MAX_ROWS) return fail(nullptr, IA2P_ERR_SHAPE, "llm_attention_rows: M=%d (1..%d)", M, LLM_MAX_ROWS);
  LlmAttnRows ar{};
  int longest = 0;
  for (int m = 0; m < M; ++m) {
    if (!k_cache[m] || !v_cache[m]) return fail(nullptr, IA2P_ERR_INVALID, "llm_attention_rows: null cache of row %d", m);
    if ((((uintptr_t)k_cache[m]) | ((uintptr_t)v_cache[m])) & 15) return fail(nullptr, IA2P_ERR_INVALID, "llm_attention_rows: the caches must be 16-byte aligned");
    ar.kc[m] = (const half_t*)k_cache[m]; ar.vc[m] = (const half_t*)v_cache[m]; ar.pos[m] = pos[m];
  }
  if (!llm_positions_ok(pos, M)) return fail(nullptr, IA2P_ERR_SHAPE, "llm_attention_rows: a position outside 0..%d", LLM_MAX_POSITIONS - 1);
  for (int m = 0; m < M; ++m) longest = std::max(longest, pos[m] + 1);
  hipLaunchKernelGGL(llm_attn_rows_kernel, dim3(heads, M), dim3(256), attn_lds(longest), (hipStream_t)stream, q, ar, out, H, 0.08838834764831845f);
  hipError_t e = hipGetLastError();
  RET_HIP(e, "llm_attention_rows");
}
// T rows at positions p0 .. p0 + T - 1 of one cache
static ia2p_status llm_rows_span(const char* what, int p0, int T) {
  if (T < 1 || p0 < 0 || p0 >= LLM_MAX_POSITIONS || T > LLM_MAX_POSITIONS - p0)
    return fail(nullptr, IA2P_ERR_SHAPE, "%s: %d rows at position %d (positions 0..%d)", what, T, p0, LLM_MAX_POSITIONS - 1);
  return IA2P_OK;
}
ia2p_status ia2p_llm_attention_prefill(void* stream, const float* q, const void* k_cache, const void* v_cache, void* out, int heads, int H, int p0, int T) {
  if (!q || !k_cache || !v_cache || !out) return fail(nullptr, IA2P_ERR_INVALID, "llm_attention_prefill: null argument");
  if ((((uintptr_t)k_cache) | ((uintptr_t)v_cache)) & 15) return fail(nullptr, IA2P_ERR_INVALID, "llm_attention_prefill: the caches must be 16-byte aligned");
  ia2p_status st = llm_attn_shape("llm_attention_prefill", heads, H);
  if (st == IA2P_OK) st = llm_rows_span("llm_attention_prefill", p0, T);
  if (st != IA2P_OK) return st;
  hipLaunchKernelGGL(llm_attn_kernel<half_t>, dim3(heads, T), dim3(256), attn_lds(p0 + T), (hipStream_t)stream, q, (const half_t*)k_cache, (const half_t*)v_cache, (half_t*)out, H,
                     p0, 0.08838834764831845f);
  hipError_t e = hipGetLastError();
  RET_HIP(e, "llm_attention_prefill");
}
ia2p_status ia2p_llm_rmsnorm_rows(void* stream, const void* x, const void* gamma, float eps, void* y, int T, int H) {
  if (!x || !gamma || !y) return fail(nullptr, IA2P_ERR_INVALID, "llm_rmsnorm_rows: null argument");
  if (!(eps >= 0.f && eps < INFINITY)) return fail(nullptr, IA2P_ERR_INVALID, "llm_rmsnorm_rows: eps=%g", (double)eps);
  if (T < 1 || H < 1) return fail(nullptr, IA2P_ERR_SHAPE, "llm_rmsnorm_rows: T=%d H=%d", T, H);
  hipLaunchKernelGGL(llm_rmsnorm_rows_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, (half_t*)y, (const half_t*)gamma, H, eps);
  hipError_t e = hipGetLastError();
  RET_HIP(e, "llm_rmsnorm_rows");
}
ia2p_status ia2p_llm_rope_cache_rows(void* stream, const void* qkv, const float* inv_freq, float* q, void* k_cache, void* v_cache, int H, int p0, int T) {
  if (!qkv || !inv_freq || !q || !k_cache || !v_cache) return fail(nullptr, IA2P_ERR_INVALID, "llm_rope_cache_rows: null argument");
  if (H < 128 || H % 128) return fail(nullptr, IA2P_ERR_SHAPE, "llm_rope_cache_rows: H=%d (heads * 128)", H);
  const ia2p_status st = llm_rows_span("llm_rope_cache_rows", p0, T);
  if (st != IA2P_OK) return st;
  hipLaunchKernelGGL(llm_rope_cache_rows_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream, (const half_t*)qkv, q, (half_t*)k_cache, (half_t*)v_cache, inv_freq, H, p0);
  hipError_t e = hipGetLastError();
  RET_HIP(e, "llm_rope_cache_rows");
}
ia2p_status ia2p_llm_silu_mul_rows(void* stream, const void* gate_up, void* act, int T, int I) {
  if (!gate_up || !act) return fail(nullptr, IA2P_ERR_INVALID, "llm_silu_mul_rows: null argument");
  if (T < 1 || I < 1 || I > (1 << 30)) return fail(nullptr, IA2P_ERR_SHAPE, "llm_silu_mul_rows: T=%d I=%d", T, I);
  hipLaunchKernelGGL(llm_silu_mul_rows_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream, (const half_t*)gate_up, (half_t*)act, I);
  hipError_t e = hipGetLastError();
  RET_HIP(e, "llm_silu_mul_rows");
}
ia2p_status ia2p_llm_rope_inv_freq(float rope_theta, float* inv_freq) {
  if (!inv_freq) return fail(nullptr, IA2P_ERR_INVALID, "llm_rope_inv_freq: null argument");
  if (!(rope_theta > 0.f && rope_theta < INFINITY)) return fail(nullptr, IA2P_ERR_INVALID, "llm_rope_inv_freq: rope_theta=%g", (double)rope_theta);
  llm_rope_inv_freq(rope_theta, inv_freq);
  return IA2P_OK;
}
ia2p_status ia2p_gelu(void* stream, void* x, int64_t n) {
  if (!x) return fail(nullptr, IA2P_ERR_INVALID, "gelu: null argument");
  if (n < 1 || n > ((int64_t)1 << 31)) return fail(nullptr, IA2P_ERR_SHAPE, "gelu: n=%lld", (long long)n);
  hipLaunchKernelGGL(llm_gelu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (half_t*)x, (long)n);
  hipError_t e = hipGetLastError();
  RET_HIP(e, "gelu");
}

}  // extern "C"
