"""Context K/V projected inside the fused QKV + self-attention launch (qkv_sattn_kernel, csrc/qxattn.hip): the (image, head) tiles of that launch number
B * heads -- 160 on 256 compute units at batch 8 -- and the layer's slice of the context projection (reference attention_processor.py:358-359 `to_k` / `to_v`,
:379-380 `to_k_ip` / `to_v_ip`) rides along as 128 x 160 GEMM tiles on the units they leave empty.

What is checked is bits, not tolerances: the tiles are the GEMM family's own body and epilogue, whose sums run over k in one order whatever the tile, so
  * O of the launch == O of the plain fused launch (ia2p_qkv_self_attention),
  * the K/V columns written == the stand-alone projection of the same rows (ia2p_gemm_ex, on several tiles), and nothing outside them is touched,
  * a whole UNet evaluation == the same evaluation with IA2P_CTX_KV_INLAUNCH=0 == the per-request route (ia2p_project_context + ia2p_unet_forward_kv).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    from instructany2pix_amd import _ffi
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib = _ffi.lib()
    assert lib.ia2p_device_is_gfx950() == 1
    return lib


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().cuda()


def _run(L, name, *args):
    from instructany2pix_amd import _ffi as f
    f.check(getattr(L, name)(f.current_stream(), *args))
    torch.cuda.synchronize()


# cfg 3's shape (batch 8, 20 heads: 160 fused tiles + 80 + 16 context tiles = the chip's 256 units) and batch 4, each with 77 + 4 tokens and text-only;
# batch 16: 320 fused tiles alone exceed the units -- the rule refuses and the projections run as launches of their own in front
@pytest.mark.parametrize("B,Lc,Li,inl", [(8, 81, 4, 1), (8, 77, 0, 1), (4, 81, 4, 1), (4, 77, 0, 1), (16, 81, 4, 0), (16, 77, 0, 0)])
def test_fused_launch_with_context_tiles(L, B, Lc, Li, inl):
    from instructany2pix_amd import _ffi as f
    heads, K, ctxd = 20, 1280, 2048
    C_, N, M, Lt = heads * 64, 2 * heads * 64, B * 256, Lc - Li
    g = torch.Generator().manual_seed(1000 + B + Lc)
    t = (torch.randn(M, K, generator=g) * 1.5 + 0.3).half().cuda()
    gamma, beta = (1.0 + 0.3 * torch.randn(K, generator=g)).half().cuda(), (0.2 * torch.randn(K, generator=g)).half().cuda()
    W = (torch.randn(3 * C_, K, generator=g) * K ** -0.5).half().cuda()
    Wf = torch.empty_like(W)
    cs, fb = torch.empty(3 * C_, dtype=torch.float32, device="cuda"), torch.empty(3 * C_, dtype=torch.float32, device="cuda")
    _run(L, "ia2p_fold_layernorm", f.ptr(W), f.ptr(gamma), f.ptr(beta), None, f.ptr(Wf), f.ptr(cs), f.ptr(fb), 3 * C_, K)
    tf = t.float()
    slots = K // 64
    st = torch.stack([tf.view(M, slots, 64).sum(2), (tf * tf).view(M, slots, 64).sum(2)], dim=2).permute(1, 0, 2).contiguous()
    ln = f.LnFoldC(st.data_ptr(), slots, cs.data_ptr(), fb.data_ptr(), 1e-5)
    ctx = _rnd(B, Lc, ctxd, seed=7 + B)
    Wt, Wi = _rnd(N, ctxd, seed=8, scale=ctxd ** -0.5), _rnd(N, ctxd, seed=9, scale=ctxd ** -0.5)
    # the layer's columns sit inside a wider buffer, as in the executor ([rows, kv_rows], column kv_col): canaries around them
    ldkv, col = N + 768, 256
    kv_t = torch.full((B * Lt, ldkv), float("nan"), dtype=torch.half, device="cuda")
    kv_i = torch.full((max(B * Li, 1), ldkv), float("nan"), dtype=torch.half, device="cuda")
    at = lambda buf: C.c_void_p(buf.data_ptr() + 2 * col)
    plain = torch.full((B, 256, C_), float("nan"), dtype=torch.half, device="cuda")
    one = torch.full((B, 256, C_), float("nan"), dtype=torch.half, device="cuda")
    _run(L, "ia2p_qkv_self_attention", f.ptr(t), f.ptr(Wf), None, C.addressof(ln), f.ptr(plain), C_, B, heads, K)
    went = C.c_int(-1)
    _run(L, "ia2p_qkv_self_attention_ctx", f.ptr(t), f.ptr(Wf), None, C.addressof(ln), f.ptr(one), C_, B, heads, K,
         f.ptr(ctx), Lc, Li, ctxd, f.ptr(Wt), f.ptr(Wi) if Li else None, at(kv_t), at(kv_i) if Li else None, ldkv, N, C.addressof(went))
    assert went.value == inl, went.value
    assert torch.equal(one, plain), float((one.float() - plain.float()).abs().max())
    # K / V: the stand-alone projection of the same rows, whatever tile it runs on (8: the committed plan of the whole projection at batch 8; 19: the tile the launch carries; 5)
    rows_t = ctx[:, :Lt].reshape(B * Lt, ctxd).contiguous()
    ref = torch.empty(B * Lt, N, dtype=torch.half, device="cuda")
    for tile in (8, 19, 5):
        L.ia2p_debug_set_gemm_tile(tile)
        try:
            _run(L, "ia2p_gemm_ex", f.ptr(rows_t), f.ptr(Wt), None, None, f.ptr(ref), B * Lt, N, ctxd, 0, None, None, None, 1, None)
        finally:
            L.ia2p_debug_set_gemm_tile(-1)
        assert torch.equal(kv_t[:, col:col + N], ref), (tile, float((kv_t[:, col:col + N].float() - ref.float()).abs().max()))
    assert torch.isnan(kv_t[:, :col]).all() and torch.isnan(kv_t[:, col + N:]).all()
    if Li:
        rows_i = ctx[:, Lt:].reshape(B * Li, ctxd).contiguous()
        refi = torch.empty(B * Li, N, dtype=torch.half, device="cuda")
        _run(L, "ia2p_gemm_ex", f.ptr(rows_i), f.ptr(Wi), None, None, f.ptr(refi), B * Li, N, ctxd, 0, None, None, None, 1, None)
        assert torch.equal(kv_i[:, col:col + N], refi), float((kv_i[:, col:col + N].float() - refi.float()).abs().max())
        assert torch.isnan(kv_i[:, :col]).all() and torch.isnan(kv_i[:, col + N:]).all()
    else:
        assert torch.isnan(kv_i).all()
    # bad arguments are refused, not mis-computed
    s = f.current_stream()
    assert L.ia2p_qkv_self_attention_ctx(s, f.ptr(t), f.ptr(Wf), None, C.addressof(ln), f.ptr(one), C_, B, heads, K, None, Lc, Li, ctxd, f.ptr(Wt), None, at(kv_t), None, ldkv, N, None) != 0
    assert L.ia2p_qkv_self_attention_ctx(s, f.ptr(t), f.ptr(Wf), None, C.addressof(ln), f.ptr(one), C_, B, heads, K, f.ptr(ctx), Lc, Lc, ctxd, f.ptr(Wt), f.ptr(Wi), at(kv_t), at(kv_i), ldkv, N, None) != 0
    assert L.ia2p_qkv_self_attention_ctx(s, f.ptr(t), f.ptr(Wf), None, C.addressof(ln), f.ptr(one), C_, B, heads, K, f.ptr(ctx), Lc, 0, ctxd, f.ptr(Wt), None, at(kv_t), None, N - 8, N, None) != 0


def _roles(m, run):
    m.profile(True)
    out = run(m)
    torch.cuda.synchronize()
    r = m.profile_read_roles()
    m.profile(False)
    pick = lambda name: [v for k, v in r.items() if k.startswith(name)][0]
    return out, pick("context K/V"), pick("qkv + self-attention")


def _three_routes(on, off, x, ctx, te, tid, t=321):
    """evaluation with the switch on / off on the reference's per-step schedule, and the per-request route; returns (outputs, role records)"""
    kw = dict(encoder_hidden_states=ctx, added_cond_kwargs=dict(text_embeds=te, time_ids=tid))
    call = lambda m: m(x, t, **kw)[0].clone()
    for m in (on, off):
        m.cache_context_kv = False
    try:
        a, kv_a, sa_a = _roles(on, call)
        b, kv_b, sa_b = _roles(off, call)
        on.cache_context_kv = True
        on.invalidate_context_kv()
        first = call(on)             # projects once (ia2p_project_context), then ia2p_unet_forward_kv
        again = call(on)
    finally:
        for m in (on, off):
            m.cache_context_kv = True
            m.invalidate_context_kv()
    return (a, b, first, again), (kv_a, kv_b, sa_a, sa_b)


@pytest.mark.parametrize("Lc,ip", [(81, True), (77, False)])
def test_unet_reduced_config_three_routes_agree(monkeypatch, Lc, ip):
    """The tiny topology at a 64 x 64 latent: its 256-channel level is 16 x 16 (256 tokens per image, 4 heads), the blocks there take the fused launch and carry their
    context K/V; the 128-channel blocks (1024 tokens) keep the projection at the head of the step."""
    from instructany2pix_amd import _ffi
    from instructany2pix_amd.attention_processor import AttnProcessor2_0
    from instructany2pix_amd.config import tiny
    from instructany2pix_amd.unet import HipUNet2DConditionModel, clear_plans
    from instructany2pix_amd.weights import unet_param_specs, ip_adapter_specs, synthetic_state_dict
    from tests.test_unet_gpu import _inputs, _install_ip
    cfg = tiny()
    sd = synthetic_state_dict(unet_param_specs(cfg), seed=7)
    ipsd = synthetic_state_dict(ip_adapter_specs(cfg, 64)["ip_adapter"], seed=7)
    clear_plans()
    _ffi.lib().ia2p_debug_set_xattn_min_tiles(1)           # (by default only launches of >= 128 tiles are fused: the tiny model has fewer)
    try:
        on = HipUNet2DConditionModel(cfg, DEV)
        monkeypatch.setenv("IA2P_CTX_KV_INLAUNCH", "0")
        off = HipUNet2DConditionModel(cfg, DEV)
        monkeypatch.delenv("IA2P_CTX_KV_INLAUNCH")
    finally:
        _ffi.lib().ia2p_debug_set_xattn_min_tiles(-1)
    for m in (on, off):
        m.load_state_dict(sd)
        if ip:
            _install_ip(m, cfg, ipsd, 0.8)
        else:
            m.set_attn_processor(AttnProcessor2_0())
    x, ctx, te, tid = (t.to(DEV) for t in _inputs(cfg, 2, 64, 64, Lc, seed=77))
    (a, b, first, again), (kv_a, kv_b, sa_a, sa_b) = _three_routes(on, off, x, ctx, te, tid)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), float((a.float() - b.float()).abs().max())
    assert torch.equal(a, first) and torch.equal(a, again)
    # the 12 blocks of the 256-channel level are projected inside their launches: their flops moved from the head-of-step role to the launches' role
    moved = 2.0 * 2 * Lc * (12 * 512) * cfg.cross_attention_dim
    assert kv_b["flops"] - kv_a["flops"] == pytest.approx(moved, rel=1e-6), (kv_a, kv_b)
    assert sa_a["flops"] - sa_b["flops"] == pytest.approx(moved, rel=1e-6) and sa_a["launches"] == sa_b["launches"]
    assert kv_a["launches"] >= 1 and kv_b["launches"] == (2 if ip else 1)


def test_unet_cfg3_three_routes_agree():
    """cfg 3 (batch 8, 64 x 64 latent, 77 + 4 tokens) at full size under the committed plan table -- the configuration bench.py times: the 60 blocks of the 1280-channel
    level carry their context K/V (160 + 96 workgroups per launch), the ten 640-channel blocks keep theirs at the head of the step, in two column ranges."""
    import os
    os.environ["IA2P_CTX_KV_INLAUNCH"] = "0"
    try:
        from instructany2pix_amd.config import sdxl_base
        from instructany2pix_amd.unet import HipUNet2DConditionModel, clear_plans, import_plans
        from instructany2pix_amd.weights import unet_param_specs, ip_adapter_specs, iter_synthetic
        cfg = sdxl_base()
        off = HipUNet2DConditionModel(cfg, DEV)
    finally:
        del os.environ["IA2P_CTX_KV_INLAUNCH"]
    on = HipUNet2DConditionModel(cfg, DEV)
    us, ips = unet_param_specs(cfg), ip_adapter_specs(cfg)["ip_adapter"]
    for m in (on, off):
        m.load_state_dict(iter_synthetic(us, 7, DEV, torch.float16))
        m.load_ip_adapter_weights(iter_synthetic(ips, 7, DEV, torch.float16), scale=1.0, num_tokens=4)
    from bench import make_inputs, DEFAULT_PLANS
    clear_plans()
    try:
        text = "".join(l for l in open(DEFAULT_PLANS).read().splitlines() if not l.startswith("#")).strip()
        assert import_plans(text) >= 100
        lat, ctx, pooled, tid = make_inputs(cfg, 8, 64, 81, DEV, cfg_id=3)
        (a, b, first, again), (kv_a, kv_b, sa_a, sa_b) = _three_routes(on, off, lat, ctx, pooled, tid, t=981)
    finally:
        clear_plans()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), float((a.float() - b.float()).abs().max())
    assert torch.equal(a, first) and torch.equal(a, again)
    moved = 2.0 * 8 * 81 * (60 * 2560) * 2048
    assert kv_b["launches"] == 2 and kv_a["launches"] == 4, (kv_a, kv_b)
    assert kv_b["flops"] - kv_a["flops"] == pytest.approx(moved, rel=1e-6)
    # (the role also holds the projection + attention launches of the ten 640-channel blocks; the fused launches are the 60 of the 1280-channel level)
    assert sa_a["launches"] == sa_b["launches"] and sa_a["kernels"]["qkv_sattn_kernel"]["launches"] == sa_b["kernels"]["qkv_sattn_kernel"]["launches"] == 60, (sa_a, sa_b)
    assert sa_a["flops"] - sa_b["flops"] == pytest.approx(moved, rel=1e-6)
