"""Editing inside a mask on the MI355X (C ABI: ia2p_known_blend_v, ia2p_mask_to_latent, ia2p_mask_feather_u8, ia2p_image_composite_u8).

Every comparison is an exact integer or bit comparison: the selection copies bits, the image kernels are integer arithmetic (references: tests/edit_mask_ref.py),
and what the loops promise is bit identity -- an all-ones mask changes nothing, an all-zeros mask returns the base latents, a half mask leaves its outside at the
base latents / the base image's bytes. Tiny configs, 16 x 16 latents, synthetic weights, 3 to 5 step loops (tests/test_edit_batch_gpu.py's models)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edit_mask_ref as R                                  # noqa: E402
from unet_ops_ref import EW_SIZES                          # noqa: E402  ((1,1,1), (1,1,63), (1,1,64), (1,1,65), (4,3,33*33))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- 1. the selection -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 4])
@pytest.mark.parametrize("B,C,HW", list(EW_SIZES) + [(3, 4, 256)])
def test_known_blend_v_is_a_selection_on_the_bits(B, C, HW, levels):
    from instructany2pix_amd.scheduler import known_blend_v, mask_blend_v
    g = torch.Generator().manual_seed(B * 1000 + HW + levels)
    h, w = (33, 33) if HW == 33 * 33 else (1, HW) if HW < 256 else (16, 16)
    # every 16-bit pattern may occur (NaNs, infinities, -0): the selection copies bits
    x = torch.randint(-32768, 32768, (B, C, h, w), generator=g, dtype=torch.int32).to(torch.int16).view(torch.float16).to(DEV)
    known = torch.randint(-32768, 32768, (levels, B, C, h, w), generator=g, dtype=torch.int32).to(torch.int16).view(torch.float16).to(DEV)
    mask = (torch.rand(B, 1, h, w, generator=g) > 0.5).half()
    mask.view(-1)[::7] *= -1.0                                                       # -0.0 where it was 0 (still "outside"), -1 where it was 1 (still "inside")
    mask = mask.to(DEV)
    level = torch.tensor([(b * 3 + 1) % levels for b in range(B)], dtype=torch.int32, device=DEV)      # a different level per row
    n, pad = x.numel(), 96
    bufs = [torch.full((n + pad,), -77.0, dtype=torch.float16, device=DEV) for _ in range(2)]
    out, out2 = (b[:n].view(B, C, h, w) for b in bufs)
    known_blend_v(x, known, level, mask, out, out2)
    gathered = torch.stack([known[int(level[b]), b] for b in range(B)])
    want = torch.where((mask != 0).expand(B, C, h, w), _bits(x), _bits(gathered))
    assert torch.equal(_bits(out), want) and torch.equal(_bits(out2), _bits(out))
    assert all(bool((b[n:] == -77.0).all()) for b in bufs)                          # nothing past B * C * HW is written
    only = torch.empty_like(x)
    known_blend_v(x, known, level, mask, only)                                      # out2 is optional
    assert torch.equal(_bits(only), want)
    inplace = x.clone()
    known_blend_v(inplace, known, level, mask, inplace, out2)                       # out may alias x
    assert torch.equal(_bits(inplace), want) and torch.equal(_bits(out2), want)
    # on finite values it is the existing blend with (1, 0) on the gathered rows
    xf, kf = torch.randn(B, C, h, w, generator=g).half().to(DEV), torch.randn(levels, B, C, h, w, generator=g).half().to(DEV)
    m01 = (mask != 0).half()
    sel, via = torch.empty_like(xf), torch.empty_like(xf)
    known_blend_v(xf, kf, level, m01, sel)
    gf = torch.stack([kf[int(level[b]), b] for b in range(B)]).contiguous()
    mask_blend_v(xf, gf, torch.zeros_like(xf), m01, torch.tensor([[1.0, 0.0]] * B, device=DEV), via)
    assert torch.equal(sel, via)
    # an unaligned view takes the scalar path and gives the same bits
    if HW % 8 == 0:
        off = torch.empty(n + 1, dtype=torch.float16, device=DEV)[1:].view(B, C, h, w)
        off.copy_(x)
        res = torch.empty(n + 1, dtype=torch.float16, device=DEV)[1:].view(B, C, h, w)
        known_blend_v(off, known, level, mask, res)
        assert torch.equal(_bits(res), want)


# ---- 2. the image kernels against the numpy references ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", R.SIZES)
def test_mask_to_latent_and_feather_equal_the_references(H, W, B):
    from instructany2pix_amd.image_processor import mask_feather, mask_to_latent
    g = np.random.default_rng(H * 100 + W + B)
    cases = R.masks(B, H, W, H + W + B)
    cases["sparse"] = np.where(g.random((B, H, W)) < 0.02, 255, 0).astype(np.uint8)
    for name, m in cases.items():
        dm = torch.from_numpy(m).to(DEV)
        for f in (8, 4, 1):                  # 8: two cells per thread on R.VECTOR_SIZES (W / 8 even), one cell per thread on the others; 4 and 1: one cell per thread
            got = mask_to_latent(dm, f)
            assert got.dtype == torch.float16 and tuple(got.shape) == (B, 1, H // f, W // f)
            assert np.array_equal(got.cpu().numpy(), R.mask_to_latent_ref(m, f)), (name, f)
        for r in R.RADII:
            got = mask_feather(dm, r).cpu().numpy()
            assert np.array_equal(got, R.mask_feather_ref(m, r)), (name, r)
            assert (got[m < 128] == 0).all()                                         # the ramp falls inside the mask only
        assert np.array_equal(mask_feather(dm, 0).cpu().numpy(), np.where(m >= 128, 255, 0))
    assert (mask_feather(torch.from_numpy(cases["ones"]).to(DEV), 9) == 255).all()
    assert ((W % 16 == 0 and (W // 8) % 2 == 0) == ((H, W) in R.VECTOR_SIZES)) and len(R.VECTOR_SIZES) == 2      # which sizes take the 16-byte paths
    # an unaligned mask (a view one byte in) takes the scalar paths: same results
    m = cases["random"]
    buf = torch.empty(m.size + 1, dtype=torch.uint8, device=DEV)
    off = buf[1:].view(B, H, W)
    off.copy_(torch.from_numpy(m))
    assert np.array_equal(mask_feather(off, 3).cpu().numpy(), R.mask_feather_ref(m, 3))
    assert np.array_equal(mask_to_latent(off, 8).cpu().numpy(), R.mask_to_latent_ref(m, 8))


@pytest.mark.parametrize("H,W", [(40, 56), (24, 64)])                                # the scalar and the 16-byte path
def test_mask_feather_at_the_largest_radius(H, W):
    from instructany2pix_amd.image_processor import mask_feather
    m = R.masks(1, H, W, 5)["random"]
    m[0, H // 4:3 * H // 4, 5:W - 6] = 255
    assert np.array_equal(mask_feather(torch.from_numpy(m).to(DEV), 64).cpu().numpy(), R.mask_feather_ref(m, 64))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", R.COMPOSITE_SIZES)
def test_image_composite_equals_the_reference(H, W, B, C):
    from instructany2pix_amd.image_processor import image_composite, mask_feather
    g = np.random.default_rng(H + W * 7 + B * 3 + C)
    e, b = g.integers(0, 256, (B, H, W, C), dtype=np.uint8), g.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    de, db = torch.from_numpy(e).to(DEV), torch.from_numpy(b).to(DEV)
    alphas = {"random": g.integers(0, 256, (B, H, W), dtype=np.uint8), "zeros": np.zeros((B, H, W), np.uint8), "ones": np.full((B, H, W), 255, np.uint8),
              "feathered": R.mask_feather_ref(R.masks(B, H, W, 9)["stripe"], 3)}
    for name, a in alphas.items():
        da = torch.from_numpy(a).to(DEV)
        buf = torch.full((e.size + 64,), 7, dtype=torch.uint8, device=DEV)
        out = buf[:e.size].view(B, H, W, C)
        image_composite(de, db, da, out=out)
        assert np.array_equal(out.cpu().numpy(), R.image_composite_ref(e, b, a)), name
        assert bool((buf[e.size:] == 7).all())
        assert np.array_equal(image_composite(de, db, da).cpu().numpy(), R.image_composite_ref(e, b, a))
    assert np.array_equal(image_composite(de, db, torch.from_numpy(alphas["ones"]).to(DEV)).cpu().numpy(), e)
    assert np.array_equal(image_composite(de, db, torch.from_numpy(alphas["zeros"]).to(DEV)).cpu().numpy(), b)
    inplace = de.clone()
    image_composite(inplace, db, torch.from_numpy(alphas["random"]).to(DEV), out=inplace)          # out may alias edited
    assert np.array_equal(inplace.cpu().numpy(), R.image_composite_ref(e, b, alphas["random"]))
    # views one byte into their buffers take the scalar path: the same bytes, nothing written before or behind the output
    def off(a):
        buf = torch.full((a.size + 2,), 7, dtype=torch.uint8, device=DEV)
        buf[1:-1].copy_(torch.from_numpy(a).reshape(-1))
        return buf, buf[1:-1].view(a.shape)
    (_, oe), (_, ob), (_, oa), (obuf, oo) = off(e), off(b), off(alphas["random"]), off(np.zeros_like(e))
    image_composite(oe, ob, oa, out=oo)
    assert np.array_equal(oo.cpu().numpy(), R.image_composite_ref(e, b, alphas["random"])) and int(obuf[0]) == 7 and int(obuf[-1]) == 7
    # the feathered alpha of the device equals the reference's
    assert np.array_equal(mask_feather(torch.from_numpy(R.masks(B, H, W, 9)["stripe"]).to(DEV), 3).cpu().numpy(), alphas["feathered"])


@pytest.mark.parametrize("C", [1, 3])
def test_image_composite_endpoints_over_all_pairs(C):
    """a in {0, 255} over all 256 x 256 (e, b) pairs: exactly e, exactly b"""
    from instructany2pix_amd.image_processor import image_composite
    e, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    e, b = np.repeat(e[None, ..., None], C, axis=-1).copy(), np.repeat(b[None, ..., None], C, axis=-1).copy()
    de, db = torch.from_numpy(e).to(DEV), torch.from_numpy(b).to(DEV)
    for a, want in ((255, e), (0, b)):
        got = image_composite(de, db, torch.full((1, 256, 256), a, dtype=torch.uint8, device=DEV)).cpu().numpy()
        assert np.array_equal(got, want), a
    for a in (1, 127, 128, 254):
        al = np.full((1, 256, 256), a, np.uint8)
        assert np.array_equal(image_composite(de, db, torch.from_numpy(al).to(DEV)).cpu().numpy(), R.image_composite_ref(e, b, al)), a


def test_refusals_come_before_any_launch():
    from instructany2pix_amd import _ffi
    L, s, p = _ffi.lib(), _ffi.current_stream(), _ffi.ptr
    INVALID, SHAPE = 1, 2
    x = torch.zeros(2, 4, 8, 8, dtype=torch.float16, device=DEV)
    known, level = torch.zeros(3, 2, 4, 8, 8, dtype=torch.float16, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    mask, out = torch.zeros(2, 1, 8, 8, dtype=torch.float16, device=DEV), torch.full_like(x, 5.0)
    good = [p(x), p(known), p(level), p(mask), p(out)]
    for i in range(5):                                                               # x, known, level, mask, out: none may be null (out2 may)
        a = list(good)
        a[i] = None
        assert L.ia2p_known_blend_v(s, *a, None, 2, 4, 64, 3) == INVALID, i
    for B, C, HW, lv in ((0, 4, 64, 3), (2, 0, 64, 3), (2, 4, 0, 3), (2, 4, 64, 0), (-1, 4, 64, 3)):
        assert L.ia2p_known_blend_v(s, *good, None, B, C, HW, lv) == SHAPE, (B, C, HW, lv)
    m8, o8 = torch.zeros(1, 16, 24, dtype=torch.uint8, device=DEV), torch.full((1, 16, 24), 9, dtype=torch.uint8, device=DEV)
    lat, ws = torch.full((1, 1, 2, 3), 5.0, dtype=torch.float16, device=DEV), torch.zeros(1, 16, 24, dtype=torch.int16, device=DEV)
    assert L.ia2p_mask_to_latent(s, None, p(lat), 1, 16, 24, 8) == INVALID and L.ia2p_mask_to_latent(s, p(m8), None, 1, 16, 24, 8) == INVALID
    assert L.ia2p_mask_to_latent(s, p(m8), p(lat), 1, 16, 24, 0) == INVALID
    for H, W, f in ((16, 24, 5), (12, 24, 8), (16, 20, 8)):                          # H % f or W % f non-zero
        assert L.ia2p_mask_to_latent(s, p(m8), p(lat), 1, H, W, f) == SHAPE, (H, W, f)
    assert L.ia2p_mask_to_latent(s, p(m8), p(lat), 0, 16, 24, 8) == SHAPE
    for a in ((None, p(o8), p(ws)), (p(m8), None, p(ws)), (p(m8), p(o8), None), (p(m8), p(m8), p(ws))):      # (the last: out may not alias the mask)
        assert L.ia2p_mask_feather_u8(s, *a, 1, 16, 24, 3) == INVALID
    for r in (65, -1, 1000):
        assert L.ia2p_mask_feather_u8(s, p(m8), p(o8), p(ws), 1, 16, 24, r) == INVALID, r
    assert L.ia2p_mask_feather_u8(s, p(m8), p(o8), p(ws), 1, 0, 24, 3) == SHAPE
    e3 = torch.zeros(1, 16, 24, 3, dtype=torch.uint8, device=DEV)
    o3 = torch.full_like(e3, 9)
    for i in range(4):
        a = [p(e3), p(e3), p(m8), p(o3)]
        a[i] = None
        assert L.ia2p_image_composite_u8(s, *a, 1, 16, 24, 3) == INVALID, i
    for C in (2, 0, 4):
        assert L.ia2p_image_composite_u8(s, p(e3), p(e3), p(m8), p(o3), 1, 16, 24, C) == SHAPE, C
    with pytest.raises(ValueError, match="SHAPE"):
        _ffi.check(L.ia2p_image_composite_u8(s, p(e3), p(e3), p(m8), p(o3), 1, 16, 24, 2))
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((o8 == 9).all()) and bool((lat == 5.0).all()) and bool((o3 == 9).all())      # no refused call launched anything
    assert L.ia2p_known_blend_v(s, *good, None, 2, 4, 64, 3) == 0 and L.ia2p_mask_feather_u8(s, p(m8), p(o8), p(ws), 1, 16, 24, 64) == 0


# ---- the loops --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    from test_edit_batch_gpu import Models
    return Models()


def _cond(m, seed, n_subjects=0):
    from test_edit_batch_gpu import _cond
    return _cond(m, seed, n_subjects)


def _half(px=128, cols=60):
    """a pixel mask whose edge cuts a latent cell: columns < cols may change; at 8 (4) pixels per cell the latent mask covers cells 0 .. (cols - 1) // f"""
    m = np.zeros((px, px), np.uint8)
    m[:, :cols] = 255
    return m


def _explicit(c):
    from instructany2pix_amd.pipeline import EMBED_KEYS, fuse_instruction_embedding
    la = fuse_instruction_embedding(c["base_embed"], c["image_embeds"], c["y"], [0.0, 0.4, 1.0], 20.0).reshape(1, -1)[0]
    return la, {k: c[k] for k in EMBED_KEYS}


def _f16(t):
    return t.to(DEV, torch.float16)


# 5. the inversion records its trajectory
def test_inversion_trajectory_is_what_the_callback_sees(models):
    from instructany2pix_amd.batch import invert_batch
    pipe = models.pipeline()
    c = _cond(models, 200)
    seen = []
    kw = dict(num_inference_steps=4, latents=c["base_latents"], prompt_embeds=c["negative_prompt_embeds"], pooled_prompt_embeds=c["negative_pooled_prompt_embeds"])
    plain = pipe.pipe_inversion.inverse(**kw, callback=lambda i, t, x: seen.append(x.clone()))
    assert not hasattr(plain, "trajectory")
    rec = pipe.pipe_inversion.inverse(**kw, return_trajectory=True)
    assert torch.equal(rec.images, plain.images)                                     # the same final latents, bit for bit
    traj = rec.trajectory
    assert tuple(traj.shape) == (5, 1, 4, 16, 16) and traj.dtype == torch.float16
    assert torch.equal(traj[0], _f16(c["base_latents"]))                             # I_0: the base latents as the loop holds them
    for j in range(1, 5):
        assert torch.equal(traj[j], seen[j - 1]), j                                  # level j: what the callback sees at iteration j - 1
    assert torch.equal(traj[4], rec.images)
    # the joint loop: steps (3, 5, 4); a request's levels 0 .. N_r are its own trajectory, the final latents are unchanged
    cs = [_cond(models, 201 + i) for i in range(3)]
    args = (models.base, pipe.pipe.scheduler.config, torch.cat([c["base_latents"] for c in cs]), torch.cat([c["negative_prompt_embeds"] for c in cs]),
            torch.cat([c["negative_pooled_prompt_embeds"] for c in cs]), (3, 5, 4))
    x_plain = invert_batch(*args)
    x_rec, tj = invert_batch(*args, return_trajectory=True)
    assert torch.equal(x_plain, x_rec) and tuple(tj.shape) == (6, 3, 4, 16, 16)
    for r, n in enumerate((3, 5, 4)):
        assert torch.equal(tj[0, r], _f16(cs[r]["base_latents"])[0]) and torch.equal(tj[n, r], x_rec[r])
        assert all(torch.equal(tj[k, r], x_rec[r]) for k in range(n, 6))             # held: the levels above N_r repeat x_T
        assert not torch.equal(tj[1, r], tj[0, r])


# 1 + 2 + 3. denoise
def test_denoise_under_all_ones_all_zeros_and_half_masks(models):
    pipe = models.pipeline()
    c = _cond(models, 210)
    la, emb = _explicit(c)
    kw = dict(**emb, num_inference_steps=4, cfg=4.0, noise=c["polar_noise"])
    base = _f16(c["base_latents"])
    plain, inv = pipe.denoise(c["base_latents"], la, **kw)
    ones, inv1 = pipe.denoise(c["base_latents"], la, **kw, edit_mask=np.full((128, 128), 255, np.uint8))
    assert torch.equal(ones, plain) and torch.equal(inv1, inv)                       # an all-ones mask: the same latents, bit for bit
    zeros, _ = pipe.denoise(c["base_latents"], la, **kw, edit_mask=np.zeros((128, 128), bool))
    assert torch.equal(zeros, base) and not torch.equal(plain, base)                 # an all-zeros mask: the base latents, bit for bit
    half, _ = pipe.denoise(c["base_latents"], la, **kw, edit_mask=_half())
    inside = torch.zeros(1, 4, 16, 16, dtype=torch.bool, device=DEV)
    inside[..., :8] = True                                                           # pixel column 59 lies in cell 7: the whole cell may change
    assert torch.equal(half[~inside], base[~inside]) and not torch.equal(half[inside], base[inside])
    assert not torch.equal(half[inside], plain[inside])                              # (the inside is not the unmasked edit either: its surroundings differ)
    lat_mask = torch.zeros(1, 1, 16, 16)
    lat_mask[..., :8] = 1
    again, _ = pipe.denoise(c["base_latents"], la, **kw, edit_mask=lat_mask)         # the latent mask itself
    assert torch.equal(again, half)
    with pytest.raises(ValueError, match="edit_mask is 64 x 64: expected 128 x 128"):
        pipe.denoise(c["base_latents"], la, **kw, edit_mask=np.zeros((64, 64), np.uint8))


# 1 + 2 + 3. __call__ and edit_batch, latents out
@pytest.mark.parametrize("refinement", [0.0, 0.5])
def test_call_and_edit_batch_keep_the_outside_at_the_base_latents(models, refinement):
    conds = {f"edit {i}": _cond(models, 220 + i) for i in range(2)}
    pipe = models.pipeline(conds, refiner_handoff="latent")
    kw = dict(num_inference_steps=3, cfg=4.0, refinement=refinement, seed=5)
    c = conds["edit 0"]
    base = _f16(c["base_latents"])
    plain = pipe("edit 0", [], **kw)
    ones = pipe("edit 0", [], **kw, edit_mask=np.full((128, 128), 255, np.uint8))
    assert torch.equal(ones[0], plain[0]) and torch.equal(ones[1], plain[1])
    zeros = pipe("edit 0", [], **kw, edit_mask=np.zeros((128, 128), np.uint8))
    assert torch.equal(zeros[0], base) and torch.equal(zeros[1], base)               # `non_refined` and `oo`
    half = pipe("edit 0", [], **kw, edit_mask=_half(), debug=True)
    m = half[2]["edit_mask_latent"]
    assert tuple(m.shape) == (1, 1, 16, 16) and m[..., :8].eq(1).all() and m[..., 8:].eq(0).all()
    inside = (m != 0).expand(1, 4, 16, 16)
    for x in half[:2]:
        assert torch.equal(x[~inside], base[~inside]) and not torch.equal(x[inside], base[inside])
    if refinement > 0:
        assert not torch.equal(half[1][inside], half[0][inside])                     # the refiner pass did repaint the inside
    # edit_batch: the same three, one mask for all requests and a list with None entries
    bkw = dict(num_inference_steps=3, cfg=4.0, refinement=refinement, seeds=[5, 6], group=2)
    insts = list(conds)
    bplain = pipe.edit_batch(insts, [[], []], **bkw)
    bones = pipe.edit_batch(insts, [[], []], **bkw, edit_masks=np.full((128, 128), 255, np.uint8))
    bzeros = pipe.edit_batch(insts, [[], []], **bkw, edit_masks=[np.zeros((128, 128), np.uint8), None])
    for i in range(2):
        assert torch.equal(bones[i][0], bplain[i][0]) and torch.equal(bones[i][1], bplain[i][1]), i
    assert torch.equal(bzeros[0][0], base) and torch.equal(bzeros[0][1], base)
    assert torch.equal(bzeros[1][0], bplain[1][0]) and torch.equal(bzeros[1][1], bplain[1][1])      # the request without a mask: its unmasked bits
    bhalf = pipe.edit_batch(insts, [[], []], **bkw, edit_masks=[_half(), _half(cols=100)], debug=True)
    for i, cols in enumerate((8, 13)):
        b_i = _f16(conds[insts[i]]["base_latents"])
        mi = bhalf[i][2]["edit_mask_latent"]
        assert mi[..., :cols].eq(1).all() and mi[..., cols:].eq(0).all()
        ins = (mi != 0).expand(1, 4, 16, 16)
        for x in bhalf[i][:2]:
            assert torch.equal(x[~ins], b_i[~ins]) and not torch.equal(x[ins], b_i[ins])
    with pytest.raises(ValueError, match='must be "pil" or "latent"'):
        models.pipeline(conds, vae=models.vae)("edit 0", [], **kw, edit_mask=_half(64, 30), output_type="np")


# 4. a mixed group
def test_a_group_of_three_with_two_masks_and_its_stages_by_hand(models):
    from instructany2pix_amd.batch import EditRequest, RefineRequest, refine_batch
    from instructany2pix_amd.pipeline import EMBED_KEYS
    conds = {f"edit {i}": _cond(models, 230 + i) for i in range(3)}
    pipe = models.pipeline(conds, refiner_handoff="latent")
    cs, steps = list(conds.values()), (3, 5, 4)
    masks = [_half(), None, _half(cols=20)]
    lat_masks = [torch.zeros(1, 1, 16, 16) for _ in range(3)]
    lat_masks[0][..., :8], lat_masks[2][..., :3] = 1, 1

    def reqs(ms):
        return [EditRequest(base_latents=c["base_latents"], latent_la=_explicit(c)[0], **_explicit(c)[1], num_inference_steps=n, cfg=4.0 + i, noise=c["polar_noise"],
                            edit_mask=m) for i, (c, n, m) in enumerate(zip(cs, steps, ms))]
    out, inv = pipe.denoise_batch(reqs(masks), group=4)
    plain, inv_plain = pipe.denoise_batch(reqs([None] * 3), group=4)
    assert torch.equal(inv, inv_plain)
    assert torch.equal(out[1], plain[1])                                             # the row without a mask: its row of the all-unmasked group, bit for bit
    for r in (0, 2):                                                                 # each masked row's outside is its OWN base, at its own step count
        ins = (lat_masks[r] != 0).expand(1, 4, 16, 16)[0].to(DEV)
        b = _f16(cs[r]["base_latents"])[0]
        assert torch.equal(out[r][~ins], b[~ins]) and not torch.equal(out[r][ins], b[ins]) and not torch.equal(out[r], plain[r])
    # edit_batch equals the loops called by hand (denoise_batch, then refine_batch on the requests that ask for it)
    refinement = [0.1, 0.1, 0.0]
    got = pipe.edit_batch(list(conds), [[]] * 3, num_inference_steps=list(steps), cfg=[4.0, 5.0, 6.0], refinement=refinement, group=4, edit_masks=masks)
    # (`edit_batch` hands `polar_noise` / `refiner_noise` of the conditioner over, as the requests above do)
    rr = [RefineRequest(latents=out[i:i + 1], **{k: cs[i]["refiner_" + k] for k in EMBED_KEYS}, strength=refinement[i], noise=cs[i]["refiner_noise"],
                        known_latents=cs[i]["base_latents"] if masks[i] is not None else None, edit_mask=lat_masks[i] if masks[i] is not None else None) for i in (0, 1)]
    refined = refine_batch(pipe.piperf, rr, group=4)
    for i in range(3):
        assert torch.equal(got[i][0], out[i:i + 1]), i
        assert torch.equal(got[i][1], refined[i:i + 1] if i < 2 else out[i:i + 1]), i
    ins = (lat_masks[0] != 0).expand(1, 4, 16, 16).to(DEV)
    assert torch.equal(got[0][1][~ins], _f16(cs[0]["base_latents"])[~ins]) and not torch.equal(got[0][1][ins], got[0][0][ins])
    # the serial refiner pass under the same mask keeps the same outside
    serial = pipe.piperf(latents=out[0:1], **{k: cs[0]["refiner_" + k] for k in EMBED_KEYS}, strength=0.1, noise=cs[0]["refiner_noise"], output_type="latent",
                         known_latents=cs[0]["base_latents"], edit_mask=lat_masks[0]).images
    assert torch.equal(serial[~ins], _f16(cs[0]["base_latents"])[~ins])


# 6. a subject pass under an edit mask
def test_a_subject_pass_under_an_edit_mask_stays_inside_it(models):
    conds = {"edit 0": _cond(models, 240, n_subjects=1)}
    pipe = models.pipeline(conds, refiner_handoff="latent")
    c = conds["edit 0"]
    base = _f16(c["base_latents"])
    sub = torch.nn.functional.interpolate(c["subject_data"][0][0][None, None], size=(16, 16))[0, 0] >= 0.5
    assert sub[:, :8].any() and sub[:, 8:].any()                                     # the subject's mask reaches across the edit mask's edge
    kw = dict(num_inference_steps=3, cfg=4.0, refinement=0.0, subject_strength=0.1, seed=3)
    nr, oo, _ = pipe("edit 0", [], **kw, edit_mask=_half())
    inside = torch.zeros(1, 4, 16, 16, dtype=torch.bool, device=DEV)
    inside[..., :8] = True
    assert torch.equal(nr[~inside], base[~inside]) and torch.equal(oo[~inside], base[~inside])      # everything outside the edit mask: the base latents
    both = (sub.to(DEV) & inside[0, 0])[None, None].expand(1, 4, 16, 16)
    assert not torch.equal(oo[both], nr[both])                                       # inside both masks the pass repainted
    only_edit = inside & ~both
    assert torch.equal(oo[only_edit], nr[only_edit])                                 # inside the edit mask but outside the subject's: the inpaint loop keeps it
    got = pipe.edit_batch(["edit 0"], [[]], num_inference_steps=3, cfg=4.0, refinement=0.0, subject_strength=0.1, seeds=[3], edit_masks=[_half()])
    assert torch.equal(got[0][1][~inside], base[~inside]) and not torch.equal(got[0][1][both], got[0][0][both])
    pipe.ip_adapter_xl.set_scale(1.0)


# 1 + 3. images out: the 8-bit composite
def test_pil_output_composites_with_the_base_image_in_8_bits(models):
    """tiny VAE (factor 4: 64 x 64 images over 16 x 16 latents), the reference's image hand-off to the refiner, feather radius 3"""
    conds = {f"edit {i}": _cond(models, 250 + i) for i in range(2)}
    pipe = models.pipeline(conds, vae=models.vae)
    post = lambda lat: np.asarray(pipe.pipe.image_processor.postprocess(models.vae.decode_from_latents(_f16(lat)), output_type="pil")[0])
    kw = dict(num_inference_steps=3, cfg=4.0, refinement=0.1, seed=9)
    mask = _half(64, 30)                                                             # pixel columns < 30; latent cells 0 .. 7
    base_img = post(conds["edit 0"]["base_latents"])                                 # no image from the conditioner: the 8-bit decode of the base latents
    plain = pipe("edit 0", [], **kw, output_type="pil")
    ones = pipe("edit 0", [], **kw, output_type="pil", edit_mask=np.full((64, 64), 255, np.uint8))
    assert ones[0][0].tobytes() == plain[0][0].tobytes() and ones[1][0].tobytes() == plain[1][0].tobytes()      # an all-ones mask: the same bytes
    lat = pipe("edit 0", [], **kw, edit_mask=mask)
    pil = pipe("edit 0", [], **kw, edit_mask=mask, edit_feather=3, output_type="pil")
    assert pil[2] == "SUCCESS!" and pil[0][0].size == (64, 64) and pil[1][0].size == (64, 64) and pil[1] is not pil[0]
    for img, latents in ((pil[0][0], lat[0]), (pil[1][0], lat[1])):
        a, edited = np.asarray(img), post(latents)
        assert np.array_equal(a[:, 30:], base_img[:, 30:])                           # every pixel outside the pixel mask: the base image's byte
        assert np.array_equal(a[:, :27], edited[:, :27])                             # every pixel whose 7 x 7 window lies inside the mask: the edited byte
        assert not np.array_equal(a[:, :27], base_img[:, :27])
    hard = pipe("edit 0", [], **kw, edit_mask=mask, edit_feather=0, output_type="pil")
    a = np.asarray(hard[1][0])
    assert np.array_equal(a[:, 30:], base_img[:, 30:]) and np.array_equal(a[:, :30], post(lat[1])[:, :30])      # r = 0: a hard seam at the mask's edge
    zeros = pipe("edit 0", [], **kw, edit_mask=np.zeros((64, 64), np.uint8), output_type="pil")
    assert np.array_equal(np.asarray(zeros[0][0]), base_img) and np.array_equal(np.asarray(zeros[1][0]), base_img)
    # edit_batch: the masked request composited, the other one postprocessed as ever
    insts = list(conds)
    bkw = dict(num_inference_steps=3, cfg=4.0, refinement=0.1, seeds=[9, 10], group=2)
    bplain = pipe.edit_batch(insts, [[], []], **bkw, output_type="pil")
    blat = pipe.edit_batch(insts, [[], []], **bkw, edit_masks=[mask, None])
    bpil = pipe.edit_batch(insts, [[], []], **bkw, edit_masks=[mask, None], edit_feather=3, output_type="pil")
    assert bpil[1][1][0].tobytes() == bplain[1][1][0].tobytes() and bpil[1][0][0].tobytes() == bplain[1][0][0].tobytes()
    for k in (0, 1):
        a, edited = np.asarray(bpil[0][k][0]), post(blat[0][k])
        assert np.array_equal(a[:, 30:], base_img[:, 30:]) and np.array_equal(a[:, :27], edited[:, :27])
    bones = pipe.edit_batch(insts, [[], []], **bkw, edit_masks=np.full((64, 64), 255, np.uint8), output_type="pil")
    assert all(bones[i][k][0].tobytes() == bplain[i][k][0].tobytes() for i in range(2) for k in range(2))


def test_a_loaded_base_image_is_the_composite_background(models):
    """the conditioner hands a PIL base image over: it is encoded as ever, and outside the mask the result carries ITS bytes"""
    import PIL.Image
    g = np.random.default_rng(4)
    img = PIL.Image.fromarray(g.integers(0, 256, (64, 64, 3), dtype=np.uint8))
    c = _cond(models, 260)
    del c["base_latents"]
    c["base_image"] = img
    pipe = models.pipeline({"edit 0": c}, vae=models.vae)
    mask = _half(64, 30)
    nr, oo, _ = pipe("edit 0", [], num_inference_steps=3, cfg=4.0, refinement=0.0, seed=2, edit_mask=mask, edit_feather=3, output_type="pil")
    a = np.asarray(nr[0])
    assert oo is nr and np.array_equal(a[:, 30:], np.asarray(img)[:, 30:]) and not np.array_equal(a[:, :27], np.asarray(img)[:, :27])
    got = pipe.edit_batch(["edit 0"], [[]], num_inference_steps=3, cfg=4.0, refinement=0.0, seeds=[2], edit_masks=[mask], edit_feather=3, output_type="pil")
    assert np.array_equal(np.asarray(got[0][0][0])[:, 30:], np.asarray(img)[:, 30:])
    with pytest.raises(ValueError, match="edit_mask is 32 x 32: expected 64 x 64"):
        pipe("edit 0", [], num_inference_steps=3, cfg=4.0, refinement=0.0, seed=2, edit_mask=np.zeros((32, 32), np.uint8), output_type="pil")
