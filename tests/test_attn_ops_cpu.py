"""The references of tests/attn_ops_ref.py against independent code in fp64 (a wrong reference cannot bless a wrong kernel), the two conditions under which a
model may stand in a bound (the native exponential and the 2 u per MFMA addition: a tenth of the bound each, for every case the GPU tests use), the planted cases
(the reference output is the planted value row), the resize cases' excluded share, and the host-side refusals of the six entry points (none reaches a HIP call)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ops_ref as R  # noqa: E402
from tests import sam_ref  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def _close(a, b, tol=1e-11):
    a, b = R.f64(a), R.f64(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ---- the references against independent ones ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,bias,D", [(17, 0, 64), (65, 1, 80), (272, 0, 80)])
def test_full_attention_is_sdpa(T, bias, D):
    qkv, bk, bv, _ = R.full_case("diffuse", T, bias, D)
    B, heads = R.FULL_B, R.FULL_HEADS
    x = qkv.double().reshape(B, T, 3, heads, D).permute(2, 0, 3, 1, 4)
    k, v = x[1], x[2]
    if bias:
        k = torch.cat([k, bk.double().reshape(1, heads, 1, D).expand(B, heads, 1, D)], 2)
        v = torch.cat([v, bv.double().reshape(1, heads, 1, D).expand(B, heads, 1, D)], 2)
    want = F.scaled_dot_product_attention(x[0], k, v).permute(0, 2, 1, 3).reshape(B * T, heads * D)
    _close(R.full_ref("diffuse", T, bias, D)[0], want)


@pytest.mark.parametrize("family,window,gh,gw,D", [("diffuse", 14, 20, 33, 80), ("pad", 7, 20, 20, 64), ("diffuse", 16, 32, 20, 80), ("diffuse", 1, 3, 5, 80),
                                                   ("diffuse", 0, 13, 5, 80), ("late", 0, 28, 12, 64), ("tables", 0, 1, 70, 80), ("planted", 0, 70, 1, 64)])
def test_relpos_attention_is_sam_ref(family, window, gh, gw, D):
    qkv, bias, rh, rw, _ = R.relpos_case(family, window, gh, gw, D)
    B, heads = R.relpos_dims(gh, gw, window)
    _close(R.relpos_ref(family, window, gh, gw, D)[0], sam_ref.relpos_attention_ref(qkv, bias, rh, rw, B, gh, gw, heads, D, window))


@pytest.mark.parametrize("shape", [(2, 7, 65, 8), (1, 3, 64, 1)])
def test_small_head_attention_is_sam_ref_and_sdpa(shape):
    B, Tq, Tk, heads = shape
    q, k, v, _ = R.small_case("diffuse", *shape, 32)
    ref = R.small_ref("diffuse", *shape, 32)[0]
    _close(ref, sam_ref.small_head_attention_ref(q, k, v, heads))
    f = lambda t: t.double().reshape(B, -1, heads, 32).transpose(1, 2)      # noqa: E731
    _close(ref, F.scaled_dot_product_attention(f(q), f(k), f(v)).transpose(1, 2).reshape(B, Tq, heads * 32))


@pytest.mark.parametrize("name", [c[0] for c in R.UPSAMPLE_CASES])
def test_resize_is_interpolate(name):
    _, n, sh, sw, rows, ld, H, W = next(c for c in R.UPSAMPLE_CASES if c[0] == name)
    x = R.upsample_case(name)
    ref, bound = R.bilinear_resize(x, sh, sw, H, W)
    _close(ref, F.interpolate(x.double()[None, :, :sh, :sw], size=(H, W), mode="bilinear", align_corners=False)[0])
    assert float(bound.max()) < 2e-4      # a coordinate error of 3 u (sh + 1) on slopes of a few units, seven roundings of values of a few units
    for thr in R.UPSAMPLE_THR:            # the excluded share of every case
        share = 1.0 - float(R.sure_pixels(ref, bound, thr).double().mean())
        print(f"[attn-ops] resize {name} thr {thr}: {share:.4%} of the pixels within the bound of the threshold")
        assert share <= 0.01
    if name == "80to320":                 # the exact-threshold block is decided, not excluded
        inner = R.sure_pixels(ref, bound, 0.0)[0, 136:168, 96:128]
        assert bool(inner.all()) and bool((ref[0, 136:168, 96:128] == 0).all())


@pytest.mark.parametrize("k", [1, 2, 7, 10, 40, 700])
def test_morph_is_scipy(k):
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for m in R.morph_masks(37, 257, 5)[:6] + R.morph_masks(1, 600, 6)[:4]:
        H, W = m.shape
        if ndimage is not None:
            er, di = ndimage.minimum_filter(m, size=k, mode="constant", cval=255), ndimage.maximum_filter(m, size=k, mode="constant", cval=0)
        else:      # pixel by pixel over the header's window
            er, di = np.empty_like(m), np.empty_like(m)
            for y in range(H):
                for x in range(W):
                    win = m[max(y - k // 2, 0):y + k - k // 2, max(x - k // 2, 0):x + k - k // 2]
                    er[y, x], di[y, x] = win.min(), win.max()
        assert np.array_equal(R.morph(m, k, False), er) and np.array_equal(R.morph(m, k, True), di)


# ---- the two models stay below a tenth of every bound, and every planted row is its key's value row -------------------------------------------------------
def _planted(ref, bound, want, tag):
    if want is None:
        return 0
    rows = ~torch.isnan(want)
    assert bool(((ref - want).abs()[rows] <= bound[rows]).all()), f"{tag}: the reference of a planted row is not its key's value row"
    return int(rows.sum())


def _fold(worst, shares):
    return max(worst[0], shares[0]), max(worst[1], shares[1])


def test_shares_and_planted_rows_full():
    worst, n = (0.0, 0.0), 0
    for case in R.full_cases():
        ref, bound, shares = R.full_ref(*case)
        worst, n = _fold(worst, shares), n + _planted(ref, bound, R.full_case(*case)[3], f"full {case}")
    print(f"[attn-ops] full_attention: largest share of the exponential / MFMA model in a bound {worst[0]:.4f} / {worst[1]:.4f}; {n} planted outputs")
    assert max(worst) <= 0.1 and n > 0


def test_shares_and_planted_rows_global():
    worst, n = (0.0, 0.0), 0
    for family, gh, gw, D in R.global_cases():
        ref, bound, shares = R.relpos_ref(family, 0, gh, gw, D)
        worst, n = _fold(worst, shares), n + _planted(ref, bound, R.relpos_case(family, 0, gh, gw, D)[4], f"global {family} {gh}x{gw} D={D}")
    print(f"[attn-ops] global relpos: largest share of the exponential / MFMA model in a bound {worst[0]:.4f} / {worst[1]:.4f}; {n} planted outputs")
    assert max(worst) <= 0.1 and n > 0


def test_shares_and_planted_rows_window():
    worst, n = (0.0, 0.0), 0
    for case in R.window_cases():
        ref, bound, shares = R.relpos_ref(*case)
        worst, n = _fold(worst, shares), n + _planted(ref, bound, R.relpos_case(*case)[4], f"window {case}")
    print(f"[attn-ops] window relpos: largest share of the exponential / MFMA model in a bound {worst[0]:.4f} / {worst[1]:.4f}; {n} planted outputs")
    assert max(worst) <= 0.1 and n > 0


def test_shares_and_planted_rows_small_head():
    worst, n = (0.0, 0.0), 0
    for case in R.small_cases():
        ref, bound, shares = R.small_ref(*case)
        worst, n = _fold(worst, shares), n + _planted(ref, bound, R.small_case(*case)[3], f"small head {case}")
    print(f"[attn-ops] small head: largest share of the exponential model in a bound {worst[0]:.4f} (no MFMA: {worst[1]})")
    assert max(worst) <= 0.1 and worst[1] == 0.0 and n > 0


def test_thin_grid_is_the_lds_limit_of_the_formula():
    for D, total in ((80, 169), (64, 186)):
        gh, gw = R.thin_grid(D)
        assert gh + gw == total and R.relpos_lds_bytes(D, gh, gw) <= 65536 < R.relpos_lds_bytes(D, gh, gw + 1) and gh * gw < 2000


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch(lib):
    """every call below is refused on the host: the pointers are never dereferenced and no GPU is needed"""
    INVALID, SHAPE = 1, 2
    p, p2 = C.c_void_p(256), C.c_void_p(4096)
    L = lib
    thin80, thin64 = R.thin_grid(80), R.thin_grid(64)
    cases = [
        # attention_full: qkv, out, bias_k, bias_v, B, T, heads, D
        (L.ia2p_attention_full(None, None, p, None, None, 1, 8, 1, 64), INVALID),
        (L.ia2p_attention_full(None, p, None, None, None, 1, 8, 1, 64), INVALID),
        (L.ia2p_attention_full(None, p, p, p, None, 1, 8, 1, 64), INVALID),                      # bias_k without bias_v
        (L.ia2p_attention_full(None, p, p, None, p, 1, 8, 1, 64), INVALID),
        (L.ia2p_attention_full(None, p, p, None, None, 0, 8, 1, 64), INVALID),
        (L.ia2p_attention_full(None, p, p, None, None, 1, 0, 1, 64), INVALID),
        (L.ia2p_attention_full(None, p, p, None, None, 1, 8, 0, 64), INVALID),
        (L.ia2p_attention_full(None, p, p, None, None, 1, 8, 1, 96), SHAPE),
        (L.ia2p_attention_full(None, p, p, None, None, 1, 8, 1, 16), SHAPE),
        (L.ia2p_attention_full(None, p, p, None, None, 1, 273, 1, 80), SHAPE),                   # 273 keys
        (L.ia2p_attention_full(None, p, p, p, p, 1, 272, 1, 64), SHAPE),                         # 272 and the bias row
        (L.ia2p_attention_full(None, p, p, None, None, 65536, 8, 1, 64), SHAPE),
        # attention_window_relpos: qkv, out, qkv_bias, rel_h, rel_w, B, gh, gw, heads, D, window
        (L.ia2p_attention_window_relpos(None, None, p, p, p, p, 1, 4, 4, 1, 80, 14), INVALID),
        (L.ia2p_attention_window_relpos(None, p, None, p, p, p, 1, 4, 4, 1, 80, 14), INVALID),
        (L.ia2p_attention_window_relpos(None, p, p, None, p, p, 1, 4, 4, 1, 80, 14), INVALID),
        (L.ia2p_attention_window_relpos(None, p, p, p, None, p, 1, 4, 4, 1, 80, 14), INVALID),
        (L.ia2p_attention_window_relpos(None, p, p, p, p, None, 1, 4, 4, 1, 80, 14), INVALID),
        (L.ia2p_attention_window_relpos(None, p, p, p, p, p, 0, 4, 4, 1, 80, 14), INVALID),
        (L.ia2p_attention_window_relpos(None, p, p, p, p, p, 1, 0, 4, 1, 80, 14), INVALID),
        (L.ia2p_attention_window_relpos(None, p, p, p, p, p, 1, 4, 0, 1, 80, 14), INVALID),
        (L.ia2p_attention_window_relpos(None, p, p, p, p, p, 1, 4, 4, 0, 80, 14), INVALID),
        (L.ia2p_attention_window_relpos(None, p, p, p, p, p, 1, 4, 4, 1, 96, 14), SHAPE),
        (L.ia2p_attention_window_relpos(None, p, p, p, p, p, 1, 4, 4, 1, 32, 14), SHAPE),
        (L.ia2p_attention_window_relpos(None, p, p, p, p, p, 1, 4, 4, 1, 80, 0), SHAPE),
        (L.ia2p_attention_window_relpos(None, p, p, p, p, p, 1, 4, 4, 1, 80, 17), SHAPE),
        (L.ia2p_attention_window_relpos(None, p, p, p, p, p, 1, 4, 4, 1, 80, -1), SHAPE),
        (L.ia2p_attention_window_relpos(None, p, p, p, p, p, 4, 64, 64, 16, 80, 1), SHAPE),      # 262144 (image, window, head) triples
        # attention_global_relpos: qkv, out, rel_h, rel_w, B, gh, gw, heads, D
        (L.ia2p_attention_global_relpos(None, None, p, p, p, 1, 4, 4, 1, 80), INVALID),
        (L.ia2p_attention_global_relpos(None, p, None, p, p, 1, 4, 4, 1, 80), INVALID),
        (L.ia2p_attention_global_relpos(None, p, p, None, p, 1, 4, 4, 1, 80), INVALID),
        (L.ia2p_attention_global_relpos(None, p, p, p, None, 1, 4, 4, 1, 80), INVALID),
        (L.ia2p_attention_global_relpos(None, p, p, p, p, 0, 4, 4, 1, 80), INVALID),
        (L.ia2p_attention_global_relpos(None, p, p, p, p, 1, 0, 4, 1, 80), INVALID),
        (L.ia2p_attention_global_relpos(None, p, p, p, p, 1, 4, 4, 0, 80), INVALID),
        (L.ia2p_attention_global_relpos(None, p, p, p, p, 1, 4, 4, 1, 96), SHAPE),
        (L.ia2p_attention_global_relpos(None, p, p, p, p, 1, 128, 128, 1, 80), SHAPE),
        (L.ia2p_attention_global_relpos(None, p, p, p, p, 1, thin80[0], thin80[1] + 1, 1, 80), SHAPE),      # one past the LDS limit, both head dims and both axes
        (L.ia2p_attention_global_relpos(None, p, p, p, p, 1, thin80[1] + 1, thin80[0], 1, 80), SHAPE),
        (L.ia2p_attention_global_relpos(None, p, p, p, p, 1, thin64[0], thin64[1] + 1, 1, 64), SHAPE),
        (L.ia2p_attention_global_relpos(None, p, p, p, p, 1, thin64[1] + 1, thin64[0], 1, 64), SHAPE),
        (L.ia2p_attention_global_relpos(None, p, p, p, p, 1, 40000, 1, 1, 80), SHAPE),
        (L.ia2p_attention_global_relpos(None, p, p, p, p, 65536, 4, 4, 1, 80), SHAPE),
        # attention_small_head: q, k, v, out, B, Tq, Tk, heads, D
        (L.ia2p_attention_small_head(None, None, p, p, p, 1, 7, 7, 8, 16), INVALID),
        (L.ia2p_attention_small_head(None, p, None, p, p, 1, 7, 7, 8, 16), INVALID),
        (L.ia2p_attention_small_head(None, p, p, None, p, 1, 7, 7, 8, 16), INVALID),
        (L.ia2p_attention_small_head(None, p, p, p, None, 1, 7, 7, 8, 16), INVALID),
        (L.ia2p_attention_small_head(None, p, p, p, p, 0, 7, 7, 8, 16), INVALID),
        (L.ia2p_attention_small_head(None, p, p, p, p, 1, 0, 7, 8, 16), INVALID),
        (L.ia2p_attention_small_head(None, p, p, p, p, 1, 7, 0, 8, 16), INVALID),
        (L.ia2p_attention_small_head(None, p, p, p, p, 1, 7, 7, 0, 16), INVALID),
        (L.ia2p_attention_small_head(None, p, p, p, p, 1, 7, 7, 8, 64), SHAPE),
        (L.ia2p_attention_small_head(None, p, p, p, p, 1, 7, 7, 8, 8), SHAPE),
        # mask_upsample_threshold: logits, n, src_h, src_w, src_ld, src_image_stride, H, W, threshold, out_logits, out_mask
        (L.ia2p_mask_upsample_threshold(None, None, 1, 8, 8, 8, 64, 16, 16, 0.0, p, p), INVALID),
        (L.ia2p_mask_upsample_threshold(None, p, 1, 8, 8, 8, 64, 16, 16, 0.0, None, None), INVALID),      # neither output
        (L.ia2p_mask_upsample_threshold(None, p, 0, 8, 8, 8, 64, 16, 16, 0.0, p, p), SHAPE),
        (L.ia2p_mask_upsample_threshold(None, p, 65536, 8, 8, 8, 64, 16, 16, 0.0, p, p), SHAPE),
        (L.ia2p_mask_upsample_threshold(None, p, 1, 0, 8, 8, 64, 16, 16, 0.0, p, p), SHAPE),
        (L.ia2p_mask_upsample_threshold(None, p, 1, 8, 0, 8, 64, 16, 16, 0.0, p, p), SHAPE),
        (L.ia2p_mask_upsample_threshold(None, p, 1, 8, 8, 7, 64, 16, 16, 0.0, p, p), SHAPE),               # ld < src_w
        (L.ia2p_mask_upsample_threshold(None, p, 2, 8, 8, 8, 63, 16, 16, 0.0, p, p), SHAPE),               # src_image_stride too small
        (L.ia2p_mask_upsample_threshold(None, p, 2, 8, 6, 8, 61, 16, 16, 0.0, p, p), SHAPE),               # (7 rows of 8 and 6 more are 62)
        (L.ia2p_mask_upsample_threshold(None, p, 1, 8, 8, 8, 64, 0, 16, 0.0, p, p), SHAPE),
        (L.ia2p_mask_upsample_threshold(None, p, 1, 8, 8, 8, 64, 65536, 16, 0.0, p, p), SHAPE),
        (L.ia2p_mask_upsample_threshold(None, p, 1, 8, 8, 8, 64, 16, 0, 0.0, p, p), SHAPE),
        # mask_morph: src, dst, tmp, H, W, k, is_dilate
        (L.ia2p_mask_morph(None, None, p, p2, 8, 8, 3, 0), INVALID),
        (L.ia2p_mask_morph(None, p, None, p2, 8, 8, 3, 0), INVALID),
        (L.ia2p_mask_morph(None, p, p, None, 8, 8, 3, 0), INVALID),
        (L.ia2p_mask_morph(None, p, p2, p, 8, 8, 3, 0), INVALID),                                # tmp aliases src
        (L.ia2p_mask_morph(None, p, p2, p2, 8, 8, 3, 0), INVALID),                               # tmp aliases dst
        (L.ia2p_mask_morph(None, p, p, p, 8, 8, 3, 1), INVALID),
        (L.ia2p_mask_morph(None, p, p, p2, 0, 8, 3, 0), SHAPE),
        (L.ia2p_mask_morph(None, p, p, p2, 65536, 8, 3, 0), SHAPE),
        (L.ia2p_mask_morph(None, p, p, p2, 8, 0, 3, 0), SHAPE),
        (L.ia2p_mask_morph(None, p, p, p2, 8, 8, 0, 0), SHAPE),
        (L.ia2p_mask_morph(None, p, p, p2, 8, 8, -2, 1), SHAPE),
    ]
    for i, (got, want) in enumerate(cases):
        assert got == want, f"case {i}: status {got}, expected {want}"
