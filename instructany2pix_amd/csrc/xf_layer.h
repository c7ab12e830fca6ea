// One pre-LayerNorm transformer block on op_gemm, shared by the CLIP text executor (clip_engine.hip) and the ViT executor (vit_engine.hip):
// QKV GEMM with the first LayerNorm folded, the caller's attention launch, out-proj + residual, fc1 with the second LayerNorm folded + activation,
// fc2 + residual. No LayerNorm launches: row statistics travel from each residual GEMM's epilogue to the next folded GEMM (as in the UNet).
#pragma once
#include "engine_rt.h"

// arena offsets of a block: parameters as loaded (wqkv / bqkv: q, k, v rows stacked) and what xf_refold derives from them
struct CLayer { size_t ln1g, ln1b, wqkv, bqkv, wo, bo, ln2g, ln2b, w1, b1, w2, b2, fqkv, cs1, lb1, f1, cs2, lb2; };

// room for what xf_refold derives, behind the block's parameters
inline void xf_take_folds(ArenaPlan& a, CLayer& l, int H, int I) {
  l.fqkv = a.take((size_t)3 * H * H); l.cs1 = a.take((size_t)2 * 3 * H); l.lb1 = a.take((size_t)2 * 3 * H);
  l.f1 = a.take((size_t)I * H); l.cs2 = a.take((size_t)2 * I); l.lb2 = a.take((size_t)2 * I);
}

// gamma-folded copies of the two LayerNorm-consuming weights of every block (+ column sums and folded biases). At finalize: null stream, sync. Before a pass that
// finds fold_dirty set (a tensor was reloaded after finalize): on the pass's stream without a wait, so the pass's launches are ordered behind the new folds.
inline ia2p_status xf_refold(RunCtx* c, const std::vector<CLayer>& layers, int H, int I, hipStream_t stream, bool sync, const char* what) {
  hipError_t e = hipSuccess;
  auto Hp = [&](size_t off) { return c->arena + off; };
  auto Fp = [&](size_t off) { return (float*)(c->arena + off); };
  for (const CLayer& l : layers) {
    if (e == hipSuccess) e = ia2p_launch_fold_ln(Hp(l.wqkv), Hp(l.ln1g), Hp(l.ln1b), Hp(l.bqkv), Hp(l.fqkv), Fp(l.cs1), Fp(l.lb1), 3 * H, H, stream);
    if (e == hipSuccess) e = ia2p_launch_fold_ln(Hp(l.w1), Hp(l.ln2g), Hp(l.ln2b), Hp(l.b1), Hp(l.f1), Fp(l.cs2), Fp(l.lb2), I, H, stream);
  }
  if (e == hipSuccess && sync) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail_hip(c, e, (std::string(what) + " LayerNorm folding").c_str());
  c->fold_dirty = false;
  return IA2P_OK;
}

// x [M, H] is updated in place; st holds its row statistics in `slots` slots on entry and on exit. attn(): qkv [M, 3H] -> att [M, H].
template <class Attn>
inline void xf_layer(RunCtx* c, const CLayer& l, half_t* x, half_t* qkv, half_t* att, half_t* ff, float* st, int& slots, int M, int H, int I, float eps, int act, Attn&& attn) {
  auto Fp = [&](size_t off) { return (const float*)(c->arena + off); };
  GemmOpt to_x;      // a GEMM that writes x leaves the row statistics of its output
  to_x.stats = st; to_x.stat_slots = &slots;
  {
    const LnIn ln{st, slots, Fp(l.cs1), Fp(l.lb1), eps};
    GemmOpt o;
    o.ln = &ln;
    op_gemm(c, x, H, W_(c, l.fqkv), nullptr, nullptr, 0, qkv, 3 * H, M, 3 * H, H, o);
  }
  attn();
  op_gemm(c, att, H, W_(c, l.wo), W_(c, l.bo), x, H, x, H, M, H, H, to_x);
  {
    const LnIn ln{st, slots, Fp(l.cs2), Fp(l.lb2), eps};
    GemmOpt o;
    o.ln = &ln; o.act = act;
    op_gemm(c, x, H, W_(c, l.f1), nullptr, nullptr, 0, ff, I, M, I, H, o);
  }
  op_gemm(c, ff, I, W_(c, l.w2), W_(c, l.b2), x, H, x, H, M, H, I, to_x);
}
