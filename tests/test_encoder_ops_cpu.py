"""The references of tests/encoder_ops_ref.py against independent torch code in fp64 (a wrong reference cannot bless a wrong kernel), the host-side refusals of the
entry points tests/test_encoder_ops_gpu.py goes through (none reaches a HIP call), and the condition under which the modelled accuracy of the native exponential
may stand in a bound: below a tenth of it, for every case the GPU tests use."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_ops_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def _close(a, b, tol=1e-12):
    a, b = R.f64(a), R.f64(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ---- the references against torch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,Hi,Wi,ps,stride", [(3, 28, 42, 14, 14), (1, 32, 50, 16, 10), (3, 32, 32, 16, 16)])
def test_patch_gather_is_unfold(C_, Hi, Wi, ps, stride):
    gh, gw = (Hi - ps) // stride + 1, (Wi - ps) // stride + 1
    px = torch.randn(2, C_, Hi, Wi, generator=R.gen(1), dtype=torch.float64)
    Kraw = C_ * ps * ps
    want = F.unfold(px, kernel_size=ps, stride=stride).transpose(1, 2).reshape(2 * gh * gw, Kraw)
    got = R.patch_gather(px, ps, stride, gh, gw, Kraw + 40)
    assert torch.equal(got[:, :Kraw], want) and not got[:, Kraw:].any()
    if stride < ps:
        assert torch.equal(got[0, stride:ps], got[1, :ps - stride])      # neighbouring patches overlap


@pytest.mark.parametrize("B,Hs,Ws,Ci,Co", [(1, 1, 1, 8, 8), (2, 5, 7, 24, 16)])
def test_pixel_shuffle_of_the_gemm_is_conv_transpose(B, Hs, Ws, Ci, Co):
    ct = torch.nn.ConvTranspose2d(Ci, Co, kernel_size=2, stride=2).double()
    x = torch.randn(B, Ci, Hs, Ws, generator=R.gen(2), dtype=torch.float64)
    Wg = ct.weight.detach().permute(2, 3, 1, 0).reshape(4 * Co, Ci)          # rows (ky, kx, co)
    g = x.permute(0, 2, 3, 1).reshape(B * Hs * Ws, Ci) @ Wg.t() + ct.bias.detach().repeat(4)
    _close(R.pixel_shuffle2(g, B, Hs, Ws, Co), ct(x).detach().permute(0, 2, 3, 1))


@pytest.mark.parametrize("T,heads", [(1, 1), (65, 3), (128, 1)])
def test_causal_attention_is_sdpa(T, heads):
    qkv = R.attention_case("diffuse", T, heads, 5)
    out, bound, _ = R.causal_attention(qkv, 2, T, heads)
    q, k, v = R.f64(qkv).reshape(2, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    want = F.scaled_dot_product_attention(q, k, v, is_causal=True).permute(0, 2, 1, 3).reshape(2 * T, heads * 64)
    _close(out, want)
    assert bool((bound > 0).all()) and float((bound / out.abs().clamp_min(1e-3)).max()) < 4e-3      # about an fp16 ulp, not a tolerance


def test_planted_attention_rows_are_their_key():
    for edge in R.ATTN_EDGES:
        T = 128
        qkv = R.attention_case("planted", T, 1, 9, edge)
        out, bound, _ = R.causal_attention(qkv, 2, T, 1)
        v = R.f64(qkv).reshape(2, T, 3, 64)[:, :, 2]
        tgt = R.planted_target(T, edge)
        rows = (tgt >= 0).nonzero().flatten()
        assert len(rows) >= T - 64
        got = out.reshape(2, T, 64)[:, rows]
        assert float((got - v[:, tgt[rows]]).abs().max()) < 1e-5, edge


def _clip_eos_transformers(ids, last, eos_token_id):
    """the two pooling rules of transformers' CLIPTextTransformer.forward, restated"""
    if eos_token_id == 2:
        return last[torch.arange(last.shape[0]), ids.to(torch.int).argmax(dim=-1)]
    return last[torch.arange(last.shape[0]), (ids.to(torch.int) == eos_token_id).int().argmax(dim=-1)]


@pytest.mark.parametrize("eos_id", [2, 49407])
def test_clip_pool_is_transformers_rule_and_layer_norm(eos_id):
    T, H = 20, 100
    ids = torch.randint(3, 49000, (6, T), generator=R.gen(3))
    ids[0, 7] = ids[0, 12] = 49407      # a tie: the first wins
    ids[1, 0] = 49407
    ids[2, T - 1] = 49407
    ids[3, 5] = 49407                   # row 4, 5: absent (largest id under the legacy rule)
    x = torch.randn(6, T, H, generator=R.gen(4)).half()
    g, b = (1 + 0.2 * torch.randn(H, generator=R.gen(5))).half(), (0.1 * torch.randn(H, generator=R.gen(6))).half()
    y, bound, pos = R.clip_pool(ids, x, g, b, eos_id, 1e-5)
    want = F.layer_norm(_clip_eos_transformers(ids, x.double(), eos_id), (H,), g.double(), b.double(), float(torch.tensor(1e-5, dtype=torch.float32)))
    _close(y, want)
    if eos_id != 2:
        assert pos.tolist()[:6] == [7, 0, T - 1, 5, 0, 0]
    assert float((bound / y.abs().clamp_min(0.05)).max()) < 0.02


@pytest.mark.parametrize("stem,pre", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_vit_embed_is_layer_norm_composition(stem, pre):
    B, T, H = 2, 5, 64
    g = R.gen(7)
    patches, cls, pos = torch.randn(B * (T - 1), H, generator=g).half(), torch.randn(H, generator=g).half(), torch.randn(T, H, generator=g).half()
    sg, sb, pg, pb = [(1 + 0.2 * torch.randn(H, generator=g)).half() for _ in range(4)]
    (x, xb), (st, sb_) = R.vit_embed(patches, cls, pos, sg if stem else None, sb if stem else None, pg if pre else None, pb if pre else None, 1e-6, B, T)
    eps = float(torch.tensor(1e-6, dtype=torch.float32))
    tok = patches.double().reshape(B, T - 1, H)
    if stem:
        tok = F.layer_norm(tok, (H,), sg.double(), sb.double(), eps)
    want = torch.cat([cls.double().expand(B, 1, H), tok], 1) + pos.double()
    if pre:
        want = F.layer_norm(want, (H,), pg.double(), pb.double(), eps)
    _close(x, want.reshape(B * T, H))
    xr = R.round16(x)
    _close(st, torch.stack([xr.sum(-1), (xr * xr).sum(-1)], -1))
    assert float((xb / x.abs().clamp_min(0.05)).max()) < 0.02 and bool((sb_ > 0).all())


def test_row_stats_allow_for_the_neighbouring_fp16_value_only_near_a_boundary():
    ref = torch.tensor([[1.0 + 2.0 ** -11 + 1e-9, 0.5, 3.0, 1.0]], dtype=torch.float64)      # the first entry sits on a rounding boundary
    _, tight = R.row_stats(ref, torch.zeros_like(ref))
    _, loose = R.row_stats(ref, torch.full_like(ref, 1e-8))
    assert float(tight[0, 0]) < 1e-5 and 2.0 ** -10 <= float(loose[0, 0]) < 2.0 ** -10 + 1e-5


@pytest.mark.parametrize("width", [8, 256, 320])
def test_embed_is_the_diffusers_formula(width):
    vals = torch.tensor([0.0, 1.0, 500.5, 999.0, 1024.0, 2047.0])
    ref, bound = R.sinusoid(vals, width)
    want = R.sinusoid_diffusers(vals, width)
    assert want.dtype == torch.float32 and want.shape == ref.shape
    assert R.ratio(want, ref, bound) <= 1.0                        # torch's fp32 evaluation meets the bound counted for an fp32 evaluation
    half = width // 2
    a = vals.double()[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    _close(ref, torch.cat([a.cos(), a.sin()], -1))
    assert float(bound.max()) < 2047 * 40 * R.U + 1e-6


def test_ip_attn_map_is_the_reference_expression():
    """attn_map = query @ ip_key.transpose(-2, -1).softmax(dim=-1): the softmax runs over the tokens"""
    Q, K = R.ip_map_case("diffuse", 4, 7, 3, 11)
    out, _, _ = R.ip_attn_map(Q, K, 3)
    query = Q.double()[..., :192].reshape(2, 7, 3, 64).transpose(1, 2)
    ip_key = K.double()[..., :192].reshape(2, 4, 3, 64).transpose(1, 2)
    _close(out, query @ ip_key.transpose(-2, -1).softmax(dim=-1))
    Q, K = R.ip_map_case("planted", 16, 3, 1, 12)
    out, _, _ = R.ip_attn_map(Q, K, 1)
    lead = K.double()[..., :64].argmax(1)                                  # [2, 64]
    want = torch.stack([(Q.double()[..., :64] * (lead == t).double()[:, None, :]).sum(-1) for t in range(16)], -1)
    assert float((out[:, 0] - want).abs().max()) < 1e-5


def test_softmax_reference_and_conv1x1_and_dots():
    x = R.softmax_case("diffuse", 2056, 2080, 1)
    p, bound, _ = R.softmax_rows(x, 2056, 0.125)
    _close(p, torch.softmax(x.double()[:, :2056] * 0.125, -1))
    xx, w, b = torch.randn(2, 3, 50, generator=R.gen(1)).half(), torch.randn(8, 3, generator=R.gen(2)).half(), torch.randn(8, generator=R.gen(3)).half()
    y, _ = R.conv1x1_nchw(xx, w, b)
    _close(y, F.conv2d(xx.double().reshape(2, 3, 5, 10), w.double().reshape(8, 3, 1, 1), b.double()).reshape(2, 8, 50))
    h, u = torch.randn(3, 16, generator=R.gen(4)).half(), torch.randn(3, 9, 16, generator=R.gen(5)).half()
    _close(R.hyper_dot(h, u)[0], torch.bmm(u.double(), h.double()[:, :, None])[:, :, 0])


def test_gelu_polynomial_error_is_the_recorded_one():
    e = R.gelu_erf_cpu_error()
    print(f"[encoder-ops] erf polynomial in numpy fp32 over every fp16 x in [-8, 8]: max |error| {e:.3e}")
    assert 1e-7 < e <= R.GELU_ERF_CPU
    x = R.all_fp16(-8, 8)
    assert x.numel() == 2 * (0x4800 + 1)      # 0 .. 8.0 and their negatives
    y, bound = R.gelu(x)
    _close(y, F.gelu(x.double()), 1e-9)
    assert float(bound.max()) < 4e-3 and bool((bound <= 2 * R.half_ulp16(y.abs()) + 8e-6).all())      # the store's half ulp and, in the tail, the polynomial


# ---- the modelled exponential stays below a tenth of every bound -----------------------------------------------------------------------------------------
def test_exponential_share_of_every_gpu_case():
    worst = {"attention": 0.0, "softmax": 0.0, "ip_attn_map": 0.0}
    for fam, T, heads, edge in R.attention_cases():
        worst["attention"] = max(worst["attention"], R.causal_attention(R.attention_case(fam, T, heads, 100 + T, edge), 2, T, heads)[2])
    for n in R.SOFTMAX_N:
        for fam, ld, scale, at in R.softmax_cases(n):
            worst["softmax"] = max(worst["softmax"], R.softmax_rows(R.softmax_case(fam, n, ld, n + ld, at), n, scale)[2])
    for fam, ntok, Nq, heads in R.ip_map_cases():
        Q, K = R.ip_map_case(fam, ntok, Nq, heads, ntok + Nq)
        worst["ip_attn_map"] = max(worst["ip_attn_map"], R.ip_attn_map(Q, K, heads)[2])
    print(f"[encoder-ops] largest share of the modelled exponential in a bound: {worst}")
    assert max(worst.values()) <= 0.1      # (each reference asserts it as well)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch(lib):
    """every call below is refused on the host: the pointers are never dereferenced and no GPU is needed"""
    INVALID, SHAPE = 1, 2
    p = C.c_void_p(256)
    L = lib
    cases = [
        # clip_embed: ids, tok, embeds, pos, x, stats, rows, T, H, vocab
        (L.ia2p_clip_embed(None, None, p, None, p, p, p, 4, 4, 64, 10), INVALID),        # ids without embeds
        (L.ia2p_clip_embed(None, p, None, None, p, p, p, 4, 4, 64, 10), INVALID),        # no table
        (L.ia2p_clip_embed(None, p, p, None, None, p, p, 4, 4, 64, 10), INVALID),        # pos
        (L.ia2p_clip_embed(None, p, p, None, p, None, p, 4, 4, 64, 10), INVALID),        # x
        (L.ia2p_clip_embed(None, None, None, p, p, p, None, 4, 4, 64, 10), INVALID),     # stats
        (L.ia2p_clip_embed(None, p, p, None, p, p, p, 0, 4, 64, 10), SHAPE),
        (L.ia2p_clip_embed(None, p, p, None, p, p, p, 4, 0, 64, 10), SHAPE),
        (L.ia2p_clip_embed(None, p, p, None, p, p, p, 4, 4, 60, 10), SHAPE),
        (L.ia2p_clip_embed(None, p, p, None, p, p, p, 4, 4, 0, 10), SHAPE),
        (L.ia2p_clip_embed(None, p, p, None, p, p, p, 4, 4, 64, 0), SHAPE),
        # causal_attention_small: qkv, out, B, T, heads, D
        (L.ia2p_causal_attention_small(None, None, p, 1, 8, 1, 64), INVALID),
        (L.ia2p_causal_attention_small(None, p, None, 1, 8, 1, 64), INVALID),
        (L.ia2p_causal_attention_small(None, p, p, 1, 0, 1, 64), SHAPE),
        (L.ia2p_causal_attention_small(None, p, p, 1, 129, 1, 64), SHAPE),
        (L.ia2p_causal_attention_small(None, p, p, 1, 8, 1, 80), SHAPE),                 # the kernel's head dimension is fixed
        (L.ia2p_causal_attention_small(None, p, p, 1, 8, 1, 32), SHAPE),
        (L.ia2p_causal_attention_small(None, p, p, 0, 8, 1, 64), SHAPE),
        (L.ia2p_causal_attention_small(None, p, p, 1, 8, 0, 64), SHAPE),
        # clip_pool: ids, x, gamma, beta, out, B, T, H, eos_id, eps
        (L.ia2p_clip_pool(None, None, p, p, p, p, 1, 8, 64, 2, 1e-5), INVALID),
        (L.ia2p_clip_pool(None, p, None, p, p, p, 1, 8, 64, 2, 1e-5), INVALID),
        (L.ia2p_clip_pool(None, p, p, None, p, p, 1, 8, 64, 2, 1e-5), INVALID),
        (L.ia2p_clip_pool(None, p, p, p, None, p, 1, 8, 64, 2, 1e-5), INVALID),
        (L.ia2p_clip_pool(None, p, p, p, p, None, 1, 8, 64, 2, 1e-5), INVALID),
        (L.ia2p_clip_pool(None, p, p, p, p, p, 1, 8, 64, 2, -1.0), INVALID),
        (L.ia2p_clip_pool(None, p, p, p, p, p, 0, 8, 64, 2, 1e-5), SHAPE),
        (L.ia2p_clip_pool(None, p, p, p, p, p, 1, 0, 64, 2, 1e-5), SHAPE),
        (L.ia2p_clip_pool(None, p, p, p, p, p, 1, 8, 0, 2, 1e-5), SHAPE),
        # softmax_rows: x, ld, rows, n, scale
        (L.ia2p_softmax_rows(None, None, 64, 1, 64, 1.0), INVALID),
        (L.ia2p_softmax_rows(None, p, 64, 0, 64, 1.0), SHAPE),
        (L.ia2p_softmax_rows(None, p, 56, 1, 64, 1.0), SHAPE),                           # ld < n
        (L.ia2p_softmax_rows(None, p, 68, 1, 64, 1.0), SHAPE),                           # rows not 16-byte aligned
        (L.ia2p_softmax_rows(None, p, 64, 1, 60, 1.0), SHAPE),
        (L.ia2p_softmax_rows(None, p, 64, 1, 0, 1.0), SHAPE),
        (L.ia2p_softmax_rows(None, p, 16392, 1, 16392, 1.0), SHAPE),
        # conv1x1_nchw: x, w, bias, y, B, Ci, Co, HW
        (L.ia2p_conv1x1_nchw(None, None, p, p, p, 1, 4, 4, 16), INVALID),
        (L.ia2p_conv1x1_nchw(None, p, None, p, p, 1, 4, 4, 16), INVALID),
        (L.ia2p_conv1x1_nchw(None, p, p, None, p, 1, 4, 4, 16), INVALID),
        (L.ia2p_conv1x1_nchw(None, p, p, p, None, 1, 4, 4, 16), INVALID),
        (L.ia2p_conv1x1_nchw(None, p, p, p, p, 1, 0, 4, 16), SHAPE),
        (L.ia2p_conv1x1_nchw(None, p, p, p, p, 1, 4, 0, 16), SHAPE),
        (L.ia2p_conv1x1_nchw(None, p, p, p, p, 1, 9, 4, 16), SHAPE),
        (L.ia2p_conv1x1_nchw(None, p, p, p, p, 1, 4, 9, 16), SHAPE),
        (L.ia2p_conv1x1_nchw(None, p, p, p, p, 0, 4, 4, 16), SHAPE),
        (L.ia2p_conv1x1_nchw(None, p, p, p, p, 1, 4, 4, 0), SHAPE),
        # patch_gather: px, cols, B, C, Hi, Wi, ps, stride, gh, gw, Kpad
        (L.ia2p_patch_gather(None, None, p, 1, 3, 28, 28, 14, 14, 2, 2, 588), INVALID),
        (L.ia2p_patch_gather(None, p, None, 1, 3, 28, 28, 14, 14, 2, 2, 588), INVALID),
        (L.ia2p_patch_gather(None, p, p, 1, 3, 28, 28, 14, 14, 3, 2, 588), SHAPE),       # a third patch row is outside the image
        (L.ia2p_patch_gather(None, p, p, 1, 3, 28, 28, 14, 14, 2, 3, 588), SHAPE),
        (L.ia2p_patch_gather(None, p, p, 1, 3, 28, 28, 14, 14, 2, 2, 587), SHAPE),       # Kpad < C ps ps
        (L.ia2p_patch_gather(None, p, p, 1, 3, 28, 28, 14, 0, 2, 2, 588), SHAPE),
        (L.ia2p_patch_gather(None, p, p, 0, 3, 28, 28, 14, 14, 2, 2, 588), SHAPE),
        (L.ia2p_patch_gather(None, p, p, 1, 0, 28, 28, 14, 14, 2, 2, 588), SHAPE),
        # vit_embed: patches, cls, pos, stem_g, stem_b, pre_g, pre_b, x, stats, B, T, H, eps
        (L.ia2p_vit_embed(None, None, p, p, None, None, None, None, p, p, 1, 5, 64, 1e-6), INVALID),
        (L.ia2p_vit_embed(None, p, None, p, None, None, None, None, p, p, 1, 5, 64, 1e-6), INVALID),
        (L.ia2p_vit_embed(None, p, p, None, None, None, None, None, p, p, 1, 5, 64, 1e-6), INVALID),
        (L.ia2p_vit_embed(None, p, p, p, None, None, None, None, None, p, 1, 5, 64, 1e-6), INVALID),
        (L.ia2p_vit_embed(None, p, p, p, None, None, None, None, p, None, 1, 5, 64, 1e-6), INVALID),
        (L.ia2p_vit_embed(None, p, p, p, p, None, None, None, p, p, 1, 5, 64, 1e-6), INVALID),      # a gamma without its beta
        (L.ia2p_vit_embed(None, p, p, p, None, p, None, None, p, p, 1, 5, 64, 1e-6), INVALID),
        (L.ia2p_vit_embed(None, p, p, p, None, None, p, None, p, p, 1, 5, 64, 1e-6), INVALID),
        (L.ia2p_vit_embed(None, p, p, p, None, None, None, p, p, p, 1, 5, 64, 1e-6), INVALID),
        (L.ia2p_vit_embed(None, p, p, p, None, None, None, None, p, p, 1, 5, 64, -1.0), INVALID),
        (L.ia2p_vit_embed(None, p, p, p, None, None, None, None, p, p, 0, 5, 64, 1e-6), SHAPE),
        (L.ia2p_vit_embed(None, p, p, p, None, None, None, None, p, p, 1, 1, 64, 1e-6), SHAPE),
        (L.ia2p_vit_embed(None, p, p, p, None, None, None, None, p, p, 1, 5, 96, 1e-6), SHAPE),
        (L.ia2p_vit_embed(None, p, p, p, None, None, None, None, p, p, 1, 5, 2112, 1e-6), SHAPE),
        # vit_project: X, W, out, B, N, K
        (L.ia2p_vit_project(None, None, p, p, 1, 4, 64), INVALID),
        (L.ia2p_vit_project(None, p, None, p, 1, 4, 64), INVALID),
        (L.ia2p_vit_project(None, p, p, None, 1, 4, 64), INVALID),
        (L.ia2p_vit_project(None, p, p, p, 0, 4, 64), SHAPE),
        (L.ia2p_vit_project(None, p, p, p, 65536, 4, 64), SHAPE),
        (L.ia2p_vit_project(None, p, p, p, 1, 0, 64), SHAPE),
        (L.ia2p_vit_project(None, p, p, p, 1, 4, 60), SHAPE),
        (L.ia2p_vit_project(None, p, p, p, 1, 4, 0), SHAPE),
        # embed: t, ts, text_embeds, time_ids, tsin, addin, B, Tp, P, Ad, nids
        (L.ia2p_embed(None, 1.0, None, p, p, None, p, 1, 320, 1280, 256, 6), INVALID),
        (L.ia2p_embed(None, 1.0, None, p, p, p, None, 1, 320, 1280, 256, 6), INVALID),
        (L.ia2p_embed(None, 1.0, None, None, p, p, p, 1, 320, 1280, 256, 6), INVALID),   # P > 0 without text_embeds
        (L.ia2p_embed(None, 1.0, None, p, None, p, p, 1, 320, 1280, 256, 6), INVALID),   # nids > 0 without time_ids
        (L.ia2p_embed(None, 1.0, None, p, p, p, p, 1, 321, 1280, 256, 6), SHAPE),        # an odd width makes i % half wrap
        (L.ia2p_embed(None, 1.0, None, p, p, p, p, 1, 320, 1280, 255, 6), SHAPE),
        (L.ia2p_embed(None, 1.0, None, p, p, p, p, 1, 0, 1280, 256, 6), SHAPE),
        (L.ia2p_embed(None, 1.0, None, p, p, p, p, 1, 320, 1280, 0, 6), SHAPE),
        (L.ia2p_embed(None, 1.0, None, p, p, p, p, 0, 320, 1280, 256, 6), SHAPE),
        (L.ia2p_embed(None, 1.0, None, p, p, p, p, 1, 320, -1, 256, 6), SHAPE),
        (L.ia2p_embed(None, 1.0, None, p, p, p, p, 1, 320, 1280, 256, -1), SHAPE),
        # concat: a, lda, Ca, b, ldb, Cb, y, M
        (L.ia2p_concat(None, None, 8, 8, p, 8, 8, p, 1), INVALID),
        (L.ia2p_concat(None, p, 8, 8, None, 8, 8, p, 1), INVALID),
        (L.ia2p_concat(None, p, 8, 8, p, 8, 8, None, 1), INVALID),
        (L.ia2p_concat(None, p, 8, 12, p, 8, 8, p, 1), SHAPE),
        (L.ia2p_concat(None, p, 8, 8, p, 8, 0, p, 1), SHAPE),
        (L.ia2p_concat(None, p, 8, 16, p, 8, 8, p, 1), SHAPE),                           # lda < Ca
        (L.ia2p_concat(None, p, 8, 8, p, 12, 8, p, 1), SHAPE),                           # rows of b not 16-byte aligned
        (L.ia2p_concat(None, p, 8, 8, p, 8, 8, p, 0), SHAPE),
        # cat_rows: a, Ka, b, Kb, bias_a, bias_b, dst, bias_dst, rows
        (L.ia2p_cat_rows(None, None, 8, p, 8, p, p, p, p, 1), INVALID),
        (L.ia2p_cat_rows(None, p, 8, None, 8, p, p, p, p, 1), INVALID),
        (L.ia2p_cat_rows(None, p, 8, p, 8, None, p, p, p, 1), INVALID),
        (L.ia2p_cat_rows(None, p, 8, p, 8, p, None, p, p, 1), INVALID),
        (L.ia2p_cat_rows(None, p, 8, p, 8, p, p, None, p, 1), INVALID),
        (L.ia2p_cat_rows(None, p, 8, p, 8, p, p, p, None, 1), INVALID),
        (L.ia2p_cat_rows(None, p, 12, p, 8, p, p, p, p, 1), SHAPE),
        (L.ia2p_cat_rows(None, p, 8, p, 0, p, p, p, p, 1), SHAPE),
        (L.ia2p_cat_rows(None, p, 8, p, 8, p, p, p, p, 0), SHAPE),
        # pixel_shuffle2: g, y, B, Hs, Ws, Co
        (L.ia2p_pixel_shuffle2(None, None, p, 1, 2, 2, 8), INVALID),
        (L.ia2p_pixel_shuffle2(None, p, None, 1, 2, 2, 8), INVALID),
        (L.ia2p_pixel_shuffle2(None, p, p, 0, 2, 2, 8), SHAPE),
        (L.ia2p_pixel_shuffle2(None, p, p, 1, 0, 2, 8), SHAPE),
        (L.ia2p_pixel_shuffle2(None, p, p, 1, 2, 0, 8), SHAPE),
        (L.ia2p_pixel_shuffle2(None, p, p, 1, 2, 2, 12), SHAPE),
        (L.ia2p_pixel_shuffle2(None, p, p, 1, 2, 2, 0), SHAPE),
        # hyper_dot: hyper, hyper_stride, up, mask, n, P, C
        (L.ia2p_hyper_dot(None, None, 32, p, p, 1, 4, 32), INVALID),
        (L.ia2p_hyper_dot(None, p, 32, None, p, 1, 4, 32), INVALID),
        (L.ia2p_hyper_dot(None, p, 32, p, None, 1, 4, 32), INVALID),
        (L.ia2p_hyper_dot(None, p, 24, p, p, 1, 4, 32), SHAPE),                          # stride < C
        (L.ia2p_hyper_dot(None, p, 36, p, p, 1, 4, 32), SHAPE),
        (L.ia2p_hyper_dot(None, p, 32, p, p, 0, 4, 32), SHAPE),
        (L.ia2p_hyper_dot(None, p, 32, p, p, 65536, 4, 32), SHAPE),
        (L.ia2p_hyper_dot(None, p, 32, p, p, 1, 0, 32), SHAPE),
        (L.ia2p_hyper_dot(None, p, 32, p, p, 1, 4, 12), SHAPE),
        # sam_act: x, n, kind;  sam_add_rows: a, b, out, n, period;  sam_take_col: src, ld, dst, n
        (L.ia2p_sam_act(None, None, 8, 0), INVALID),
        (L.ia2p_sam_act(None, p, 0, 0), SHAPE),
        (L.ia2p_sam_act(None, p, 8, 2), SHAPE),
        (L.ia2p_sam_act(None, p, 8, -1), SHAPE),
        (L.ia2p_sam_add_rows(None, None, p, p, 16, 8), INVALID),
        (L.ia2p_sam_add_rows(None, p, None, p, 16, 8), INVALID),
        (L.ia2p_sam_add_rows(None, p, p, None, 16, 8), INVALID),
        (L.ia2p_sam_add_rows(None, p, p, p, 0, 8), SHAPE),
        (L.ia2p_sam_add_rows(None, p, p, p, 20, 8), SHAPE),
        (L.ia2p_sam_add_rows(None, p, p, p, 16, 4), SHAPE),
        (L.ia2p_sam_add_rows(None, p, p, p, 24, 16), SHAPE),                             # the period does not divide n
        (L.ia2p_sam_take_col(None, None, 4, p, 8), INVALID),
        (L.ia2p_sam_take_col(None, p, 4, None, 8), INVALID),
        (L.ia2p_sam_take_col(None, p, 4, p, 0), SHAPE),
        (L.ia2p_sam_take_col(None, p, 0, p, 8), SHAPE),
    ]
    wrong = [(i, got, want) for i, (got, want) in enumerate(cases) if got != want]
    assert not wrong, wrong
    assert b"sam_take_col" in lib.ia2p_last_error(None)
