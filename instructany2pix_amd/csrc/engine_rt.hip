// Definitions of the runtime engine_rt.h declares: error state, workspace and event pool, the pass protocol's enter / leave, weight prefetch, the in-place autotuner, the
// operator wrappers (plan, K-split slabs, profiling class, launch) and the weight-arena plumbing. Host code only; every executor (engine.hip, vae_engine.hip,
// clip_engine.hip, vit_engine.hip, llm_engine.hip) and the per-operator C ABI (ops_abi.hip) link against this file and need nothing from each other.
#include "engine_rt.h"

thread_local std::string g_err;

const half_t* zero_page() {
  static thread_local void* z[16] = {nullptr};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  if (!z[dev]) {
    if (hipMalloc(&z[dev], 256) != hipSuccess) return nullptr;
    (void)hipMemset(z[dev], 0, 256);
  }
  return (const half_t*)z[dev];
}

static int g_xattn_min_tiles = -1;      // test hook: fusion threshold of contexts created from now on (< 0: the built-in 128)
int ia2p_default_xattn_min_tiles() { return g_xattn_min_tiles; }
extern "C" void ia2p_debug_set_xattn_min_tiles(int tiles) { g_xattn_min_tiles = tiles; }

const char* prof_name(int k) {
  static char buf[PK_NCLASS][64];
  static const char* const other[] = {"attention_f16_kernel", "gn_stats_kernel+gn_apply_kernel", "layernorm_kernel",
                                      "embed_kernel+linear_small_kernel", "conv_in_kernel", "conv_out_kernel", "concat_kernel", "splitk_reduce_kernel", "qproj_xattn_kernel", "qkv_sattn_kernel"};
  if (k >= PK_HALO_GN0) { snprintf(buf[k], sizeof buf[k], "conv_halo_f16_kernel<%d, 1>", IA2P_GEMM_TILES[24 + k - PK_HALO_GN0].bn); return buf[k]; }
  if (k >= PK_ATTN) return other[k - PK_ATTN];
  const GemmTile t = IA2P_GEMM_TILES[(k % PK_CONV0) % IA2P_GEMM_NVARIANT];
  if (t.halo) snprintf(buf[k], sizeof buf[k], "conv_halo_f16_kernel<%d, 0>", t.bn);
  else if (t.pp == 4) snprintf(buf[k], sizeof buf[k], "gemm_geglu_f16_kernel");
  else if (t.pp == 2) snprintf(buf[k], sizeof buf[k], "gemm_f16_kernel<%d, %d, %d, %s, 2, 64, 2, 4>", t.bm, t.bn, t.stages, k >= PK_CONV0 ? "true" : "false");
  else if (t.pp) snprintf(buf[k], sizeof buf[k], "gemm_f16_kernel<%d, %d, %d, %s, 4, 64, 1, 2>", t.bm, t.bn, t.stages, k >= PK_CONV0 ? "true" : "false");
  else if (t.bn == 80) snprintf(buf[k], sizeof buf[k], "gemm_f16_kernel<%d, %d, %d, %s, 4, 64, 0, 1>", t.bm, t.bn, t.stages, k >= PK_CONV0 ? "true" : "false");
  else snprintf(buf[k], sizeof buf[k], "gemm_f16_kernel<%d, %d, %d, %s, 2, 64, 0, 2>", t.bm, t.bn, t.stages, k >= PK_CONV0 ? "true" : "false");
  return buf[k];
}

const char* role_name(int r) {
  static const char* const names[ROLE_NROLE] = {"other", "ff_in (GEGLU projection, norm3 folded)", "ff_out", "qkv + self-attention (norm1 folded)", "attention out-projections (attn1 / attn2 to_out)",
                                                "to_q + cross-attention (norm2 folded)", "conv3x3 (ResnetBlock2D convs incl. fused shortcut, resample convs)", "groupnorm (+SiLU)",
                                                "proj_in / proj_out", "context K/V projection", "time / add embeddings", "conv_in / conv_out"};
  return r >= 0 && r < ROLE_NROLE ? names[r] : "?";
}

ia2p_status fail(RunCtx* c, ia2p_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) { c->err = buf; c->failed = true; }
  g_err = buf;
  return st;      // (K-split tickets: invalidated where a launch / sync error is seen -- CHECK_LAUNCH, RET_HIP, fail_hip -- not for argument refusals)
}
ia2p_status fail_hip(RunCtx* c, hipError_t e, const char* what) {
  if (e != hipErrorInvalidValue) ia2p_sk_counters_invalidate();
  return fail(c, IA2P_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

T2 wsalloc(RunCtx* c, size_t elems) {
  const size_t off = c->ws.alloc(elems * sizeof(half_t));
  if (off == (size_t)-1) { if (!c->failed) { fail(c, IA2P_ERR_NOMEM, "workspace too small"); c->ws_full = true; } return T2{off, nullptr}; }
  return T2{off, c->dry ? nullptr : (half_t*)(c->ws_base + off)};
}
void wsfree(RunCtx* c, T2 t) {
  if (t.off == (size_t)-1) return;
  c->ws.release(t.off);
}

ia2p_status pass_enter(RunCtx* c, void* stream, void* ws, size_t ws_bytes) {
  const uintptr_t base = ((uintptr_t)ws + 255) & ~(uintptr_t)255;
  const size_t lost = base - (uintptr_t)ws;
  if (ws_bytes < lost) return fail(c, IA2P_ERR_NOMEM, "workspace too small");      // (caller-supplied values: the difference below must not wrap)
  c->widx = 0; c->dry = false; c->failed = c->ws_full = false; c->stream = (hipStream_t)stream;
  c->ws.reset(ws_bytes - lost); c->ws_base = (char*)base;
  return IA2P_OK;
}
ia2p_status pass_leave(RunCtx* c, ia2p_status st) {
  if (!c->failed) return st;
  return c->ws_full ? IA2P_ERR_NOMEM : st == IA2P_OK ? IA2P_ERR_HIP : st;
}

hipEvent_t get_event(RunCtx* c) {
  if (!c->evpool.empty()) { hipEvent_t e = c->evpool.back(); c->evpool.pop_back(); return e; }
  hipEvent_t e; (void)hipEventCreate(&e); return e;
}
void set_prefetch(RunCtx* c, GemmArgs& a, const half_t* W, size_t bytes) {
  if (c->dry) { if (c->record) c->wseq.push_back({W, bytes}); return; }
  if (!c->prefetch || c->widx + 1 > c->wseq.size()) { ++c->widx; return; }
  const bool last = c->widx + 1 == c->wseq.size();
  if (last && !c->tail_pf) { ++c->widx; return; }
  const std::pair<const half_t*, size_t> nx = last ? std::make_pair(c->tail_pf, c->tail_pf_bytes) : c->wseq[c->widx + 1];
  ++c->widx;
  if (nx.second > ((size_t)96 << 20)) return;           // larger than the Infinity Cache can usefully hold
  a.pf = nx.first; a.pf_bytes = (long)nx.second;
  static const size_t pf_cap = ia2p_exp_env("IA2P_PF_BLOCKS") ? (size_t)atoi(ia2p_exp_env("IA2P_PF_BLOCKS")) : 128;            // tuning hooks: most prefetch workgroups per launch,
  static const size_t pf_per = ia2p_exp_env("IA2P_PF_BLOCK_BYTES") ? (size_t)atol(ia2p_exp_env("IA2P_PF_BLOCK_BYTES")) : 131072;   // bytes per workgroup below that
  a.pf_blocks = (int)std::max<size_t>(1, std::min<size_t>(pf_cap, (nx.second + pf_per - 1) / pf_per));
}

// One measurement of a candidate list (tune_site's protocol): rounds over all candidates, round -1 untimed, so that clock / cache drift during the measurement hits every
// candidate alike; a candidate's score is its FASTEST round (launch-time noise only ever adds). Before every launch the L2s are flushed (a memset over the flush region)
// and `warm` is read back in: what the launch just before the site wrote in the real sequence (its activations, its residual), while the weights sit in the Infinity Cache
// (prefetched by the previous launch), not in L2. ok[i] == 0 on entry: not a candidate of this site; cleared where a step of the protocol fails.
struct TuneWarm { const void* p; size_t bytes; };
static std::vector<float> time_candidates(RunCtx* c, const GemmArgs& a, bool conv, const std::vector<GemmPlan>& cands, const std::vector<TuneWarm>& warm, std::vector<char>& ok) {
  std::vector<float> best_ms(cands.size(), 1e30f);
  hipEvent_t e0 = get_event(c), e1 = get_event(c);
  for (int r = -1; r < c->tune_reps; ++r)
    for (size_t i = 0; i < cands.size(); ++i) {
      if (!ok[i]) continue;
      GemmArgs b = a;
      b.splitk = cands[i].splitk > 1 ? cands[i].splitk : 0;
      b.partial = cands[i].splitk > 1 ? (float*)c->tune_scratch : nullptr;
      bool good = hipMemsetAsync(c->tune_scratch + c->tune_slab_bytes, r & 1, c->tune_flush_bytes, c->stream) == hipSuccess;
      for (const TuneWarm& w : warm) good = good && ia2p_launch_touch(w.p, std::min<size_t>(w.bytes, (size_t)64 << 20), (unsigned*)c->tune_scratch, c->stream) == hipSuccess;
      good = good && hipEventRecord(e0, c->stream) == hipSuccess;
      good = good && ia2p_launch_gemm_variant(b, conv, cands[i].variant, c->stream) == hipSuccess;
      good = good && hipEventRecord(e1, c->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess;
      float ms = 0.f;
      good = good && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
      if (!good) { (void)hipGetLastError(); ok[i] = 0; continue; }
      if (r >= 0 && ms < best_ms[i]) best_ms[i] = ms;
    }
  c->evpool.push_back(e0); c->evpool.push_back(e1);
  return best_ms;
}
// In-place measurement of the candidate plans of one GEMM / conv site (autotune pass): time_candidates over the plain candidates -- the prefetch workgroups of the site
// are part of every candidate launch -- and, behind a GroupNorm, over the fused ones. The fastest goes into the plan table. Re-running a site is harmless: outputs are
// rewritten (in-place residuals only drift).
static void tune_site(RunCtx* c, const GemmArgs& a, bool conv, const GemmArgs* fa, float gn_ms) {
  if (ia2p_plan_lookup(a.M, a.N, a.K, conv, a.geglu != 0, nullptr)) return;
  std::vector<GemmPlan> cands;
  ia2p_gemm_candidates(a.M, a.N, a.K, conv, a.geglu != 0, c->tune_slab_bytes, ia2p_exp_env("IA2P_TUNE_SLACK") ? atof(ia2p_exp_env("IA2P_TUNE_SLACK")) : 2.5, &cands);      // (2.5 x the modelled best: -0.04 ms per step against 1.7 on the same box, profiles/r05t_slack_ab.txt; 4.0 measures 4 x the candidates for the same picks)
  static const bool tune_log = getenv("IA2P_TUNE_LOG") != nullptr;      // every candidate's time, for calibrating the cost model
  std::vector<char> ok(cands.size(), 1);
  for (size_t i = 0; i < cands.size(); ++i)
    if (IA2P_GEMM_TILES[cands[i].variant].halo && !(conv && ia2p_conv_halo_ok(a) && cands[i].splitk <= a.Cin / 64)) ok[i] = 0;      // (this site is not one for the halo-staged kernel: its twin tile is in the list anyway)
  const size_t imgs = conv ? (size_t)(a.M / std::max(1, a.Ho * a.Wo)) : 0;
  std::vector<TuneWarm> warm{{a.A, conv ? imgs * a.Hs * a.Ws * a.Cin * sizeof(half_t) : (a.rpb ? 0 : (size_t)a.M * a.lda * sizeof(half_t))}};
  if (a.residual) warm.push_back({a.residual, (size_t)a.M * a.ldr * sizeof(half_t)});
  const std::vector<float> best_ms = time_candidates(c, a, conv, cands, warm, ok);
  float fastest = 1e30f;
  for (size_t i = 0; i < cands.size(); ++i) {
    if (!ok[i]) continue;
    if (tune_log) fprintf(stderr, "[ia2p tune] %d %d %d conv=%d geglu=%d variant=%d splitk=%d us=%.2f\n", a.M, a.N, a.K, (int)conv, a.geglu, cands[i].variant, cands[i].splitk, 1e3 * best_ms[i]);
    fastest = std::min(fastest, best_ms[i]);
  }
  // candidates come best-modelled first: among those within 2 % of the fastest measurement the model's favourite wins (stable picks)
  GemmPlan best{-1, 1};
  for (size_t i = 0; i < cands.size() && best.variant < 0; ++i)
    if (ok[i] && best_ms[i] <= 1.02f * fastest) best = cands[i];
  // A site behind a GroupNorm (fa: the site's GroupNorm-FUSED form -- raw operand, producer statistics --, gn_ms: what the GroupNorm launch in front of it just
  // took; RunOpt): the fused launch on every halo-staged tile / K split it may run on is timed the same way, and taken when it beats
  // GroupNorm launch + best plain plan. The fused kernel normalises every halo image in LDS beside its MFMAs (+15 ... 25 % per launch): it pays where the norm's
  // launch is expensive against the convolution (few input channels on the large maps), not everywhere.
  if (fa && conv && best.variant >= 0 && gn_ms > 0.f) {
    std::vector<GemmPlan> fc;
    ia2p_conv_gn_candidates(*fa, c->tune_slab_bytes, &fc);
    std::vector<TuneWarm> fwarm{{fa->A, imgs * fa->Hs * fa->Ws * fa->gn.C0 * sizeof(half_t)}};
    if (fa->A1b) fwarm.push_back({fa->A1b, (size_t)fa->M * fa->lda1b * sizeof(half_t)});
    if (fa->residual) fwarm.push_back({fa->residual, (size_t)fa->M * fa->ldr * sizeof(half_t)});
    std::vector<char> fok(fc.size(), 1);
    const std::vector<float> fms = time_candidates(c, *fa, true, fc, fwarm, fok);
    const float unfused = fastest + gn_ms;
    int bi = -1;
    for (size_t i = 0; i < fc.size(); ++i) {
      if (!fok[i]) continue;
      if (tune_log) fprintf(stderr, "[ia2p tune] %d %d %d conv=1 FUSED groupnorm variant=%d splitk=%d us=%.2f (groupnorm launch %.2f us + best plain plan = %.2f us)\n", fa->M, fa->N, fa->K, fc[i].variant, fc[i].splitk,
                            1e3 * fms[i], 1e3 * gn_ms, 1e3 * unfused);
      if (fms[i] < 1e29f && (bi < 0 || fms[i] < fms[bi])) bi = (int)i;
    }
    if (bi >= 0 && fms[bi] < 0.97f * unfused) best = fc[bi];      // (3 % margin: the fused form also pays for the statistics in its producers' epilogues)
  }
  if (best.variant < 0) { fail(c, IA2P_ERR_HIP, "autotune: no candidate plan ran for %d x %d x %d", a.M, a.N, a.K); return; }
  ia2p_plan_set(a.M, a.N, a.K, conv, a.geglu != 0, best);
  ++c->tune_sites;
}

// rows per slot of the stand-alone statistics pass over an image of HW rows: the largest multiple of 16 that divides HW and is <= 1024 (0: none)
int gn_fallback_rows(int HW) {
  for (int k = 1; k <= HW / 16; ++k)
    if (HW % k == 0 && (HW / k) % 16 == 0 && HW / k <= 1024) return HW / k;
  return 0;
}
// rows per slot of the column sums a launch's own epilogue leaves (0: it cannot): whole 16-row runs, whole tiles per image, 16-byte epilogue routes, at most
// IA2P_GN_MAX_SLOTS slots per image; a K split only when it combines inside the launch
int gn_epilogue_rows(const GemmArgs& a, bool conv, int variant, int splitk, bool combined, int HW) {
  const int bm = IA2P_GEMM_TILES[ia2p_gemm_variant_ran(a, conv, variant)].bm;
  return (!a.geglu && !a.act && a.ldc % 8 == 0 && a.N % 8 == 0 && bm % 16 == 0 && HW % bm == 0 && a.M % HW == 0 && HW / bm <= IA2P_GN_MAX_SLOTS && (splitk <= 1 || combined)) ? bm : 0;
}
// plan, K-split slabs, profiling class and launch of one GEMM / implicit-GEMM conv
// gw != nullptr: the launch also leaves the GroupNorm statistics of its output (gn_fold.h) -- from its own epilogue when the tile allows, else from a gn_colstats_kernel pass
void run_gemm(RunCtx* c, GemmArgs& a, bool conv, const char* what, double flops, double bytes, const RunOpt& r) {
  int* const stat_slots = r.stat_slots; GnWant* const gw = r.gw;
  const int plan_n = r.plan_n > 0 ? r.plan_n : a.N;      // (a column range of a stacked projection: the whole projection's plan -- project_context)
  if (c->tuning && !c->dry && !c->failed && plan_n == a.N) tune_site(c, a, conv, r.tune_fused, r.tune_gn_ms);
  const GemmPlan pl = ia2p_gemm_plan(a.M, plan_n, a.K, conv, a.geglu != 0);
  if (pl.variant < 0 || pl.variant >= IA2P_GEMM_NVARIANT) { fail(c, IA2P_ERR_INVALID, "%s: tile variant %d out of range", what, pl.variant); return; }
  if (c->tuning && !c->dry && pl.splitk > 1 && (size_t)pl.splitk * a.M * a.N * sizeof(float) > c->tune_slab_bytes) {
    fail(c, IA2P_ERR_NOMEM, "%s: plan (variant %d, K split %d) needs %zu bytes of slabs, the autotune scratch holds %zu", what, pl.variant, pl.splitk,
         (size_t)pl.splitk * a.M * a.N * sizeof(float), c->tune_slab_bytes);
    return;
  }
  T2 slab{(size_t)-1, nullptr};
  if (pl.splitk > 1) {
    a.splitk = pl.splitk;
    if (c->tuning && !c->dry) a.partial = (float*)c->tune_scratch;      // plans change during the pass: slabs live outside the workspace
    else { slab = wsalloc(c, (size_t)pl.splitk * a.M * a.N * 2); a.partial = (float*)slab.p; }
  }
  struct Rel { RunCtx* c; T2 t; ~Rel() { wsfree(c, t); } } rel{c, slab};
  int combined = pl.splitk > 1 && ia2p_splitk_inkernel(a.M, a.N, pl.splitk);     // (dry pass: the policy's answer; the launcher reports what it really did)
  int gn_rows_epi = 0;
  if (gw) {      // (a launch whose tile cannot take the sums leaves none: the consumer that wants them runs the canonical pass itself, gn_ensure_stats)
    gw->out = GnStats{};
    gn_rows_epi = gn_epilogue_rows(a, conv, pl.variant, pl.splitk, combined != 0, gw->HW);
    if (gn_rows_epi) {
      gw->out.buf = wsalloc(c, (size_t)(a.M / gn_rows_epi) * a.N * 8);      // double2 per slot and column
      a.gn_out = (double*)gw->out.buf.p;
    }
  }
#ifdef IA2P_CLOCK_STAMP
  if (c->stamp_buf && c->role == c->stamp_role && (pl.splitk <= 1 || combined) && !c->dry && !c->tuning && c->stamp_n < c->stamp_cap) {
    const GemmTile& t = IA2P_GEMM_TILES[pl.variant];
    const int tiles = ((a.M + t.bm - 1) / t.bm) * ((a.N + t.bn - 1) / t.bn) * (pl.splitk > 1 ? pl.splitk : 1);      // (workgroups: a K split launches one per tile and slice)
    if (tiles <= RunCtx::STAMP_WG && !t.halo) {
      unsigned long long* rec = c->stamp_buf + (size_t)c->stamp_n * RunCtx::STAMP_WG * 8;
      if (pl.splitk > 1) a.stamp = rec;
      else a.partial = (float*)rec;
      c->stamp_meta.push_back({a.M, a.N, a.K, pl.splitk > 1 ? -100 * pl.splitk - pl.variant : pl.variant, tiles});
      ++c->stamp_n;
    }
  }
#endif
  {
    ProfScope ps(c, (conv ? PK_CONV0 : PK_GEMM0) + pl.variant, flops, bytes);
    ps.pf = a.pf ? (double)a.pf_bytes : 0.0;
    int ran = pl.variant;
    CHECK_LAUNCH(c, ia2p_launch_gemm_variant(a, conv, pl.variant, c->stream, false, &combined, &ran), what);
    ps.set_class(conv && a.gn.st0 && ran >= 24 && ran <= 26 ? PK_HALO_GN0 + ran - 24 : (conv ? PK_CONV0 : PK_GEMM0) + ran);      // (a halo-staged plan runs its gathered twin at a site it does not take: booked under the kernel that ran)
  }
  if (pl.splitk > 1 && !combined) {
    ProfScope ps(c, PK_REDUCE, 0, (double)pl.splitk * a.M * a.N * 4 + 2.0 * a.M * a.N);
    CHECK_LAUNCH(c, ia2p_launch_splitk_reduce(a, c->stream), what);
  }
  if (gw && gw->out.buf.off != (size_t)-1) {
    if (gn_rows_epi && (pl.splitk <= 1 || combined)) gw->out.rows = gn_rows_epi;
    else { wsfree(c, gw->out.buf); gw->out = GnStats{}; }      // (the launcher finished the K split with a reduce launch after all)
  }
  // row-statistics slots of this launch's output: one per tile column, or ONE when a reduce launch wrote it
  if (stat_slots) *stat_slots = (pl.splitk > 1 && !combined) ? 1 : (a.N + IA2P_GEMM_TILES[pl.variant].bn - 1) / IA2P_GEMM_TILES[pl.variant].bn;
}

// the descriptor of an executor's linear layer: gemm_desc + the folded LayerNorm in front, the row statistics behind, and the epilogue scales
GemmArgs gemm_args(RunCtx*, const half_t* A, int lda, const half_t* W, const half_t* bias, const half_t* residual, int ldr,
                   half_t* C, int ldc, int M, int N, int K, const GemmOpt& o) {
  GemmArgs a = gemm_desc(zero_page(), A, lda, W, o.ldw ? o.ldw : K, bias, residual, ldr, C, ldc, M, N, K, o.geglu, o.rpb, o.bstride, o.roff, o.act);
  ln_attach(a, o.ln);
  a.stats_out = o.stats;
  a.acc_scale = o.acc_scale; a.bias_scale = o.bias_scale;
  return a;
}
double gemm_bytes(int M, int N, int K, int geglu, bool residual) { return 2.0 * ((double)M * K + (double)N * K + (double)M * (geglu ? N / 2 : N) + (residual ? (double)M * N : 0)); }
void op_gemm(RunCtx* c, const half_t* A, int lda, const half_t* W, const half_t* bias, const half_t* residual, int ldr,
             half_t* C, int ldc, int M, int N, int K, const GemmOpt& o) {
  GemmArgs a = gemm_args(c, A, lda, W, bias, residual, ldr, C, ldc, M, N, K, o);
  set_prefetch(c, a, W, (size_t)N * K * sizeof(half_t));
  RunOpt r; r.stat_slots = o.stat_slots; r.gw = o.gw; r.plan_n = o.plan_n;
  run_gemm(c, a, false, "gemm", 2.0 * M * N * K, gemm_bytes(M, N, K, o.geglu, residual != nullptr), r);
}
// the GroupNorm-fused form of a convolution descriptor: the operand is the norm's RAW input X [| gn.X1b], with its producers' statistics
static void conv_gn_attach(GemmArgs& a, const ConvGn& gn, const half_t* X) {
  a.A = X; a.lda = gn.C0; a.A1b = gn.X1b; a.lda1b = a.Cin - gn.C0;
  a.gn = gn_in_desc((const double*)gn.s0.buf.p, gn.s0.rows, gn.X1b ? (const double*)gn.s1.buf.p : nullptr, gn.s1.rows, gn.C0, a.Cin, gn.gamma, gn.beta, gn.groups, gn.eps, 1);
}
void op_conv3(RunCtx* c, const half_t* X, int B, int Hs, int Ws, int Cin, const half_t* W, const half_t* bias, int Co, half_t* Y, const ConvOpt& o) {
  const int Cin2 = o.Cin2, Cin3 = o.Cin3; const half_t *X2 = o.X2, *X3 = o.X3; const ConvGn* gn = o.gn;
  // (appended blocks are described by their channel counts: in a dry pass the pointers are null, the shapes -- hence plans and slabs -- must not change)
  if ((Cin2 > 0 && (o.stride != 1 || o.up || o.pad_lo != 1 || Cin2 % 64)) || (Cin3 > 0 && (Cin2 <= 0 || Cin3 % 64)) || Cin2 < 0 || Cin3 < 0 ||
      (!c->dry && ((Cin2 > 0) != (X2 != nullptr) || (Cin3 > 0) != (X3 != nullptr)))) { fail(c, IA2P_ERR_SHAPE, "conv3x3 with appended 1x1 blocks: stride 1, no upsampling, Cin2 / Cin3 %% 64 == 0 (stride %d up %d pad %d Cin %d Cin2 %d Cin3 %d, X2 %s, X3 %s)", o.stride, o.up, o.pad_lo, Cin, Cin2, Cin3, X2 ? "set" : "null", X3 ? "set" : "null"); return; }
  GemmArgs a = conv3_desc(zero_page(), X, B, Hs, Ws, Cin, W, bias, Co, o.stride, o.up, o.pad_lo, o.rowvec, o.rowvec_ld, o.residual, Y, X2, Cin2, X3, Cin3);
  if (gn && gn->fused) conv_gn_attach(a, *gn, X);      // GroupNorm + SiLU applied inside the convolution (the caller asked ia2p_conv_gn_fusable)
  a.acc_scale = o.acc_scale; a.bias_scale = o.bias_scale;
  set_prefetch(c, a, W, (size_t)Co * a.K * sizeof(half_t));
  RunOpt r; r.gw = o.gw;
  GemmArgs fa;      // autotune pass: the site's GroupNorm-fused form, for tune_site to time against GroupNorm launch + plain plan
  if (gn && gn->tune && !gn->fused && c->tuning && !c->dry && gn->s0.ok() && gn->Xraw) {
    fa = a;
    conv_gn_attach(fa, *gn, gn->Xraw);
    if (ia2p_conv_gn_ok(fa)) { r.tune_fused = &fa; r.tune_gn_ms = gn->gn_ms; }
  }
  RoleScope role(c, ROLE_CONV3X3);
  run_gemm(c, a, true, "conv3x3", 2.0 * a.M * (double)Co * a.K, 2.0 * ((double)B * Hs * Ws * Cin + (double)Co * a.K + (double)a.M * Co + (o.residual ? (double)a.M * Co : 0) + (double)a.M * (Cin2 + Cin3)), r);
}
void op_gn(RunCtx* c, const half_t* x, half_t* y, size_t g, size_t b, int B, int HW, int C, float eps, int silu, float* partial, const half_t* x2, int Ca) {
  RoleScope role(c, ROLE_GROUPNORM);
  ProfScope ps(c, PK_GN, 8.0 * B * HW * C, 4.0 * B * HW * C);
  if (x2) CHECK_LAUNCH(c, ia2p_launch_groupnorm(x, Ca, y, C, W_(c, g), W_(c, b), partial, B, HW, C, c->groups, eps, silu, c->stream, x2, C - Ca, Ca), "groupnorm");
  else CHECK_LAUNCH(c, ia2p_launch_groupnorm(x, C, y, C, W_(c, g), W_(c, b), partial, B, HW, C, c->groups, eps, silu, c->stream), "groupnorm");
}
void op_ln(RunCtx* c, const half_t* x, half_t* y, size_t g, size_t b, int M, int C) {
  ProfScope ps(c, PK_LN, 8.0 * M * C, 4.0 * M * C);
  CHECK_LAUNCH(c, ia2p_launch_layernorm(x, C, y, C, W_(c, g), W_(c, b), M, C, 1e-5f, c->stream), "layernorm");
}

// ---- weight arena plumbing shared by the six contexts
ia2p_status rc_bind_arena(RunCtx* c, void* dev, size_t bytes) {
  if (!c || !dev) return fail(c, IA2P_ERR_INVALID, "bind_arena: null argument");
  if (bytes < c->arena_elems * sizeof(half_t)) return fail(c, IA2P_ERR_NOMEM, "arena needs %zu bytes, got %zu", c->arena_elems * sizeof(half_t), bytes);
  if (((uintptr_t)dev) & 255) return fail(c, IA2P_ERR_INVALID, "arena must be 256-byte aligned");
  c->arena = (half_t*)dev;
  c->finalized = false;
  c->wseq_key = -1;
  return IA2P_OK;
}
ia2p_status rc_load_tensor(RunCtx* c, const char* key, const void* src, const int64_t* shape, int ndim, void* stream) {
  if (!c || !key || !src || !shape) return fail(c, IA2P_ERR_INVALID, "load_tensor: null argument");
  if (!c->arena) return fail(c, IA2P_ERR_STATE, "load_tensor before bind_arena");
  auto it = c->params.find(key);
  if (it == c->params.end()) return fail(c, IA2P_ERR_KEY, "unknown parameter key '%s'", key);
  Param& p = it->second;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  if (n != p.elems) return fail(c, IA2P_ERR_SHAPE, "parameter '%s': expected %zu elements, got %zu", key, p.elems, n);
  hipStream_t s = (hipStream_t)stream;
  half_t* dst = c->arena + p.off;
  hipError_t e = hipSuccess;
  switch (p.kind) {
    case PK_COPY: e = hipMemcpyAsync(dst, src, n * sizeof(half_t), hipMemcpyDeviceToDevice, s); break;
    case PK_CONV: e = ia2p_launch_pack_conv((const half_t*)src, dst, p.d0, p.d1, s); break;
    case PK_CONV_TAP: e = ia2p_launch_pack_conv((const half_t*)src, dst, p.d0, p.d1, s); break;
    case PK_GEGLU_W: case PK_GEGLU_B: e = ia2p_launch_pack_geglu((const half_t*)src, dst, p.d0, p.d1, s); break;
    case PK_PAD_CONV_IN: e = ia2p_launch_pack_conv_in((const half_t*)src, dst, p.d0, p.d1, s); break;
  }
  if (e != hipSuccess) return fail_hip(c, e, (std::string("load '") + key + "'").c_str());
  p.loaded = true;
  c->fold_dirty = true;     // data derived from the parameters at finalize (LayerNorm folds) is stale until the owner re-derives it
  return IA2P_OK;
}
// the inverse of rc_load_tensor for the kinds the UNet family registers: the parameter back in the checkpoint's layout (the re-layouts are permutations: the loaded bits)
ia2p_status rc_read_tensor(RunCtx* c, const char* key, void* dst, const int64_t* shape, int ndim, void* stream) {
  if (!c || !key || !dst || !shape) return fail(c, IA2P_ERR_INVALID, "read_tensor: null argument");
  if (!c->arena) return fail(c, IA2P_ERR_STATE, "read_tensor before bind_arena");
  auto it = c->params.find(key);
  if (it == c->params.end()) return fail(c, IA2P_ERR_KEY, "unknown parameter key '%s'", key);
  const Param& p = it->second;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  if (n != p.elems) return fail(c, IA2P_ERR_SHAPE, "parameter '%s': expected %zu elements, got %zu", key, p.elems, n);
  if (!p.loaded) return fail(c, IA2P_ERR_STATE, "parameter '%s' was never loaded", key);
  hipStream_t s = (hipStream_t)stream;
  const half_t* src = c->arena + p.off;
  hipError_t e = hipSuccess;
  switch (p.kind) {
    case PK_COPY: e = hipMemcpyAsync(dst, src, n * sizeof(half_t), hipMemcpyDeviceToDevice, s); break;
    case PK_CONV: case PK_CONV_TAP: e = ia2p_launch_unpack_conv(src, (half_t*)dst, p.d0, p.d1, s); break;
    case PK_GEGLU_W: case PK_GEGLU_B: e = ia2p_launch_unpack_geglu(src, (half_t*)dst, p.d0, p.d1, s); break;
    case PK_PAD_CONV_IN: e = ia2p_launch_unpack_conv_in(src, (half_t*)dst, p.d0, p.d1, s); break;
    default: return fail(c, IA2P_ERR_INVALID, "parameter '%s': kind %d cannot be read back", key, p.kind);
  }
  if (e != hipSuccess) return fail_hip(c, e, (std::string("read '") + key + "'").c_str());
  return IA2P_OK;
}
ia2p_status rc_load_padded_rows(RunCtx* c, const char* key, size_t off, int rows, int Kraw, int Kpad, const void* src, const int64_t* shape, int ndim, void* stream) {
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  if (n != (size_t)rows * Kraw) return fail(c, IA2P_ERR_SHAPE, "parameter '%s': expected %zu elements, got %zu", key, (size_t)rows * Kraw, n);
  half_t* dst = c->arena + off;
  hipError_t e = hipMemsetAsync(dst, 0, (size_t)rows * Kpad * sizeof(half_t), (hipStream_t)stream);
  if (e == hipSuccess) e = hipMemcpy2DAsync(dst, Kpad * sizeof(half_t), src, Kraw * sizeof(half_t), Kraw * sizeof(half_t), rows, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e != hipSuccess) return fail_hip(c, e, (std::string("load '") + key + "'").c_str());
  c->params[key].loaded = true;
  return IA2P_OK;
}
ia2p_status rc_finalize(RunCtx* c, const char* what) {
  if (!c) return IA2P_ERR_INVALID;
  if (!c->arena) return fail(c, IA2P_ERR_STATE, "finalize before bind_arena");
  int missing = 0;
  std::string first;
  for (auto& kv : c->params)
    if (!kv.second.loaded && !kv.second.optional) { if (!missing) first = kv.first; ++missing; }
  if (missing) return fail(c, IA2P_ERR_KEY, "%d %s parameters not loaded (e.g. '%s')", missing, what, first.c_str());
  c->finalized = true;
  return IA2P_OK;
}
ia2p_status rc_adopt(RunCtx* c, bool with_optional) {
  if (!c || !c->arena) return fail(c, IA2P_ERR_STATE, "adopt_arena before bind_arena");
  for (auto& kv : c->params)
    if (with_optional || !kv.second.optional) kv.second.loaded = true;
  c->finalized = true;
  return IA2P_OK;
}

// ---- scratch of an autotune pass (ia2p_autotune, engine.hip): [slabs of the K-split candidates | flush region]
ia2p_status tune_begin(RunCtx* c, int reps) {
  c->tune_slab_bytes = (size_t)256 << 20; c->tune_flush_bytes = (size_t)48 << 20;
  if (hipMalloc((void**)&c->tune_scratch, c->tune_slab_bytes + c->tune_flush_bytes) != hipSuccess) {
    (void)hipGetLastError();
    c->tune_scratch = nullptr;
    return fail(c, IA2P_ERR_NOMEM, "autotune: cannot allocate %zu MiB of scratch", (c->tune_slab_bytes + c->tune_flush_bytes) >> 20);
  }
  c->tuning = true; c->tune_reps = reps < 1 ? 5 : reps; c->tune_sites = 0;
  return IA2P_OK;
}
void tune_end(RunCtx* c, hipStream_t s) {
  c->tuning = false;
  (void)hipStreamSynchronize(s);
  (void)hipFree(c->tune_scratch);
  c->tune_scratch = nullptr;
}
