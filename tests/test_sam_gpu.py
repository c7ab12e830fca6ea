"""SAM on the MI355X (csrc/sam.hip, csrc/sam_engine.hip, instructany2pix_amd/sam.py) against `transformers.SamModel` (tests/sam_ref.py) and fp64 restatements
of the attention launches.

Tolerances.
  Attention launches alone: rel-L2 < 2e-3 against the fp64 arithmetic on the same fp16 inputs (the bound `ia2p_attention_full` is held to, test_imagebind_gpu.py).
  The per-launch fp64 bounds of the three attention launches, the resize and the morphology live in tests/attn_ops_ref.py / tests/test_attn_ops_gpu.py.
  Encoder and box-to-mask: 3 x the error of the ORACLE ITSELF run in fp16 (`model.half()` on the CPU, same fp16-rounded weights) against fp64, measured on the
  CPU at exactly these shapes and seeds (tiny config, head dim 80, image 320, seed 0, the two boxes of sam_ref.BOXES); the margin is for reduction order and for
  the fp16 probability / activation stores the HIP path has and torch's CPU fp16 has not. Measured -> bound:
      embeddings   rel-L2 9.05e-4 -> 2.72e-3     max-abs 4.36e-3 -> 1.31e-2
      mask logits  rel-L2 1.55e-3 -> 4.64e-3     max-abs 7.06e-3 -> 2.12e-2
      IoU          max-abs 6.54e-4 -> 1.96e-3
  (fp32 against fp64: 1.1e-6 / 1.2e-6; logit std 0.95, max |logit| 3.47). test_sam_cpu.py re-measures the fp16 figures and fails if they leave these bounds' third.
  Binary masks must equal the oracle's wherever |oracle logit after resize| exceeds the band = the logits' max-abs bound (2.12e-2); the excluded share is capped at
  10 % (2.9 % of the pixels lie within 1 % of max |logit| = 3.5e-2 here).
"""
import numpy as np
import pytest
import torch

from tests import sam_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMB_REL, EMB_MAX, LOGIT_REL, LOGIT_MAX, IOU_MAX = 2.72e-3, 1.31e-2, 4.64e-3, 2.12e-2, 1.96e-3
BAND, BAND_CAP = LOGIT_MAX, 0.10


@pytest.fixture(scope="module")
def L():
    from instructany2pix_amd import _ffi
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib = _ffi.lib()
    assert lib.ia2p_device_is_gfx950() == 1
    return lib


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


# ---- the attention launches alone ------------------------------------------------------------------------------------------------------------------
def _relpos(L, qkv, bias, rh, rw, B, gh, gw, heads, D, window):
    from instructany2pix_amd import _ffi
    dq, db, dh, dw = qkv.to(DEV), bias.to(DEV), rh.to(DEV), rw.to(DEV)
    out = torch.full((B * gh * gw, heads * D), float("nan"), dtype=torch.half, device=DEV)
    if window:
        _ffi.check(L.ia2p_attention_window_relpos(_ffi.current_stream(), _ffi.ptr(dq), _ffi.ptr(out), _ffi.ptr(db), _ffi.ptr(dh), _ffi.ptr(dw), B, gh, gw, heads, D, window))
    else:
        _ffi.check(L.ia2p_attention_global_relpos(_ffi.current_stream(), _ffi.ptr(dq), _ffi.ptr(out), _ffi.ptr(dh), _ffi.ptr(dw), B, gh, gw, heads, D))
    torch.cuda.synchronize()
    return out.cpu()


def _relpos_inputs(B, gh, gw, heads, D, Sh, Sw, seed):
    H = heads * D
    return rnd(B * gh * gw, 3 * H, seed=seed), rnd(3 * H, seed=seed + 1, scale=0.5), rnd(2 * Sh - 1, D, seed=seed + 2, scale=0.1), rnd(2 * Sw - 1, D, seed=seed + 3, scale=0.1)


@pytest.mark.parametrize("D", [80, 64])
def test_window_attention_vs_fp64(L, D):
    """20 x 20 grid under 14 x 14 windows: padded to 28, so the right / bottom windows are partial and hold pad keys"""
    B, g, heads, S = 2, 20, 2, 14
    qkv, bias, rh, rw = _relpos_inputs(B, g, g, heads, D, S, S, seed=D)
    out = _relpos(L, qkv, bias, rh, rw, B, g, g, heads, D, S)
    ref = R.relpos_attention_ref(qkv, bias, rh, rw, B, g, g, heads, D, S)
    assert torch.isfinite(out).all()
    r = R.rel_l2(out, ref)
    print(f"window attention D={D}: rel-L2 {r:.3e}")
    assert r < 2e-3, r


def _dominant_case(L, gh, gw, window, D=80):
    """One relative-position entry dominant: rel_h[dh0 + Sh - 1] and rel_w[dw0 + Sw - 1] point along a direction every query has a large component in, so a query
    at (qh, qw) must return the value row of the key at (qh - dh0, qw - dw0) of its window. dh0 != dw0 and neither is 0: an h / w swap, a sign flip or an offset
    off by one lands on another key."""
    heads, B = 1, 1
    Sh, Sw = (window, window) if window else (gh, gw)
    dh0, dw0 = 2, -3
    qkv = rnd(gh * gw, 3 * D, seed=5, scale=0.1)
    qkv[:, 0] = 8.0                                                   # every q has component 8 along axis 0
    rh, rw = torch.zeros(2 * Sh - 1, D).half(), torch.zeros(2 * Sw - 1, D).half()
    rh[dh0 + Sh - 1, 0] = 4.0                                         # +32 on the logit of keys with qh - kh == dh0
    rw[dw0 + Sw - 1, 0] = 4.0
    bias = torch.zeros(3 * D).half()
    out = _relpos(L, qkv, bias, rh, rw, B, gh, gw, heads, D, window)
    checked = 0
    for qh, qw in [(5, 4), (7, 9), (2, 0), (gh - 1, 3)]:
        wy, wx = (qh // Sh, qw // Sw) if window else (0, 0)
        kh, kw = qh - dh0, qw - dw0
        if kh < wy * Sh or kw < wx * Sw or kh >= min((wy + 1) * Sh, gh) or kw >= min((wx + 1) * Sw, gw):
            continue                                                  # the favoured key is outside this query's window / the grid
        want = qkv[kh * gw + kw, 2 * D:].float()
        got = out[qh * gw + qw].float()
        assert (got - want).abs().max() < 2e-3, (qh, qw, (got - want).abs().max())
        checked += 1
    assert checked >= 2


def test_window_attention_dominant_entry(L):
    _dominant_case(L, 20, 20, 14)


def test_window_attention_pad_keys_take_part(L):
    """A large value in the bias' v rows and a k row aligned with every q: queries of the partial windows (whose pad keys carry the bias) are pulled to the bias'
    value row, queries of the full window are not"""
    B, g, heads, D, S = 1, 20, 1, 80, 14
    qkv, _, rh, rw = _relpos_inputs(B, g, g, heads, D, S, S, seed=9)
    qkv = (qkv.float() * 0.1).half()
    qkv[:, 0] = 6.0
    bias = torch.zeros(3 * D).half()
    bias[D] = 6.0                        # k of a pad token: logit 36 / sqrt(80) = 4 above the others
    bias[2 * D:] = 3.0                   # v of a pad token
    out = _relpos(L, qkv, bias, rh, rw, B, g, g, heads, D, S)
    ref = R.relpos_attention_ref(qkv, bias, rh, rw, B, g, g, heads, D, S)
    assert R.rel_l2(out, ref) < 2e-3
    o = out.float().reshape(g, g, D)
    assert o[:14, :14].abs().max() < 0.5          # the full window has no pad key
    assert o[14:, :].mean() > 1.5 and o[:, 14:].mean() > 1.5      # 132 (36) pad keys of 196 with e^4 the weight: the output sits near the bias' 3.0


@pytest.mark.parametrize("D", [80, 64])
@pytest.mark.parametrize("gh,gw", [(20, 20), (28, 12)])
def test_global_attention_vs_fp64(L, gh, gw, D):
    """28 x 12 = 336 keys: non-square, five full key tiles and a ragged sixth; two runs agree to the bit"""
    B, heads = 2, 2
    qkv, bias, rh, rw = _relpos_inputs(B, gh, gw, heads, D, gh, gw, seed=gh + D)
    out = _relpos(L, qkv, bias, rh, rw, B, gh, gw, heads, D, 0)
    ref = R.relpos_attention_ref(qkv, bias, rh, rw, B, gh, gw, heads, D, 0)
    assert torch.isfinite(out).all()
    r = R.rel_l2(out, ref)
    print(f"global attention {gh}x{gw} D={D}: rel-L2 {r:.3e}")
    assert r < 2e-3, r
    again = _relpos(L, qkv, bias, rh, rw, B, gh, gw, heads, D, 0)
    assert torch.equal(out, again)


@pytest.mark.parametrize("gh,gw", [(20, 20), (28, 12)])
def test_global_attention_dominant_entry(L, gh, gw):
    _dominant_case(L, gh, gw, 0)


@pytest.mark.parametrize("D", [16, 32])
@pytest.mark.parametrize("Tq,Tk", [(7, 400), (400, 7), (7, 7)])
def test_small_head_attention_vs_fp64(L, Tq, Tk, D):
    from instructany2pix_amd import _ffi
    B, heads = 2, 8
    q, k, v = rnd(B, Tq, heads * D, seed=1), rnd(B, Tk, heads * D, seed=2), rnd(B, Tk, heads * D, seed=3)
    out = torch.full((B, Tq, heads * D), float("nan"), dtype=torch.half, device=DEV)
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    _ffi.check(L.ia2p_attention_small_head(_ffi.current_stream(), _ffi.ptr(dq), _ffi.ptr(dk), _ffi.ptr(dv), _ffi.ptr(out), B, Tq, Tk, heads, D))
    torch.cuda.synchronize()
    r = R.rel_l2(out.cpu(), R.small_head_attention_ref(q, k, v, heads))
    print(f"small-head attention {Tq}x{Tk} D={D}: rel-L2 {r:.3e}")
    assert r < 2e-3, r


def test_attention_shape_errors(L):
    from instructany2pix_amd import _ffi
    t = torch.zeros(1 << 16, dtype=torch.half, device=DEV)
    p, s = _ffi.ptr(t), _ffi.current_stream()
    with pytest.raises(ValueError, match="SHAPE"):
        _ffi.check(L.ia2p_attention_window_relpos(s, p, p, p, p, p, 1, 4, 4, 1, 96, 14))      # head dim
    with pytest.raises(ValueError, match="SHAPE"):
        _ffi.check(L.ia2p_attention_window_relpos(s, p, p, p, p, p, 1, 4, 4, 1, 80, 17))      # window
    with pytest.raises(ValueError, match="SHAPE"):
        _ffi.check(L.ia2p_attention_global_relpos(s, p, p, p, p, 1, 128, 128, 1, 80))         # 256 bias rows of 64 queries do not fit
    with pytest.raises(ValueError, match="SHAPE"):
        _ffi.check(L.ia2p_attention_small_head(s, p, p, p, p, 1, 7, 7, 8, 64))


# ---- morphology and resize ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob_mask():
    """96 x 80 uint8 mask with blobs touching all four borders"""
    rng = np.random.default_rng(3)
    m = np.zeros((96, 80), np.uint8)
    for cy, cx, r in [(0, 20, 14), (95, 50, 17), (40, 0, 12), (60, 79, 15), (48, 40, 11), (20, 60, 6)]:
        yy, xx = np.mgrid[0:96, 0:80]
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255
    m[rng.random(m.shape) < 0.01] ^= 255
    assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    return m


@pytest.mark.parametrize("k", [10, 40, 7])
def test_morphology_equals_scipy(L, blob_mask, k):
    from scipy import ndimage
    from instructany2pix_amd.sam import morph
    d = torch.from_numpy(blob_mask).to(DEV)
    er, di = morph(d, k, dilate=False).cpu().numpy(), morph(d, k, dilate=True).cpu().numpy()
    assert np.array_equal(er, ndimage.minimum_filter(blob_mask, size=k, mode="constant", cval=255))
    assert np.array_equal(di, ndimage.maximum_filter(blob_mask, size=k, mode="constant", cval=0))


def test_upsample_threshold_equals_torch(L):
    from instructany2pix_amd.sam import upsample_threshold
    low = rnd(2, 80, 80, seed=4).float()
    mask, up = upsample_threshold(low.to(DEV), (320, 320), want_logits=True)
    ref = torch.nn.functional.interpolate(low[None], size=(320, 320), mode="bilinear", align_corners=False)[0]
    assert (up.cpu() - ref).abs().max() < 1e-5
    sure = ref.abs() > 1e-4
    assert torch.equal((mask.cpu() > 0)[sure], (ref > 0)[sure])
    # a cropped source to a non-square target (the second step of SAM's post-processing)
    m2, u2 = upsample_threshold(low.to(DEV), (50, 90), crop=(40, 72), want_logits=True)
    ref2 = torch.nn.functional.interpolate(low[None, :, :40, :72], size=(50, 90), mode="bilinear", align_corners=False)[0]
    assert (u2.cpu() - ref2).abs().max() < 1e-5


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_sam(L):
    from instructany2pix_amd.sam import HipSamModel, HipSamPredictor, sam_tiny_config
    model = HipSamModel(sam_tiny_config(), DEV).load_state_dict(R.oracle_model().state_dict())
    pred = HipSamPredictor(model)
    pred.set_image(R.sample_image())
    return model, pred


def test_encoder_vs_oracle(tiny_sam):
    model, pred = tiny_sam
    e64 = R.oracle_outputs()["fp64"][0]
    emb = pred.features.cpu()
    assert emb.shape == (1, 400, 256) and torch.isfinite(emb).all()
    r, m = R.rel_l2(emb, e64), R.max_abs(emb, e64)
    print(f"encoder: rel-L2 {r:.3e} (bound {EMB_REL:.2e}), max-abs {m:.3e} (bound {EMB_MAX:.2e})")
    assert r < EMB_REL and m < EMB_MAX, (r, m)


def test_box_to_mask_vs_oracle(tiny_sam):
    model, pred = tiny_sam
    _, l64, i64 = R.oracle_outputs()["fp64"]
    low, iou = model.predict_boxes(pred.features, R.BOXES)
    torch.cuda.synchronize()
    r, m, mi = R.rel_l2(low.cpu(), l64), R.max_abs(low.cpu(), l64), R.max_abs(iou.cpu(), i64)
    print(f"logits: rel-L2 {r:.3e} (bound {LOGIT_REL:.2e}), max-abs {m:.3e} (bound {LOGIT_MAX:.2e}); IoU max-abs {mi:.3e} (bound {IOU_MAX:.2e})")
    assert r < LOGIT_REL and m < LOGIT_MAX and mi < IOU_MAX, (r, m, mi)
    for j in range(2):                                                # one box at a time through the predictor gives the batch's rows
        masks, iou1, low1 = pred.predict(box=R.BOXES[j:j + 1], multimask_output=False)
        assert masks.shape == (1, 320, 320) and masks.dtype == np.bool_ and low1.shape == (1, 80, 80)
        assert R.max_abs(low1[0], l64[j]) < LOGIT_MAX and abs(float(iou1[0]) - float(i64[j])) < IOU_MAX
        big = R.resize_logits(l64[j:j + 1], (320, 320))[0]
        sure = big.abs() > BAND
        share = 1.0 - float(sure.float().mean())
        print(f"box {j}: {share:.3%} of the pixels inside the band")
        assert share < BAND_CAP
        assert torch.equal(torch.from_numpy(masks[0])[sure], (big > 0)[sure])
    with pytest.raises(NotImplementedError):
        pred.predict(point_coords=np.zeros((1, 2)), point_labels=np.ones(1))
    with pytest.raises(NotImplementedError):
        pred.predict(box=R.BOXES[:1], multimask_output=True)
    with pytest.raises(ValueError, match="SHAPE"):
        model.predict_boxes(pred.features, np.array([[10.0, 10.0, 400.0, 100.0]], np.float32))      # outside the 320 x 320 input


def _oracle_get_mask(box_xyxy, e, d, b, size):
    """the oracle chain: transformers (fp64) -> scipy min / max filters -> PIL blur"""
    from PIL import Image, ImageFilter
    from scipy import ndimage
    model = R.oracle_model()
    px = R.pixels_of(R.sample_image())
    _, low, _ = R.run_model(model, px, np.asarray(box_xyxy, np.float32).reshape(1, 4), torch.float64, embeddings=R.oracle_outputs()["fp64"][0])
    m = (R.resize_logits(low, (size, size))[0] > 0).numpy().astype(np.uint8) * 255
    m = ndimage.minimum_filter(m, size=e, mode="constant", cval=255)
    m = ndimage.maximum_filter(m, size=d, mode="constant", cval=0)
    img = Image.fromarray(m)
    return img.filter(ImageFilter.GaussianBlur(radius=b)) if b > 0 else img


def test_get_mask_end_to_end(tiny_sam):
    from instructany2pix_amd.inpaint import prepare_mask
    from instructany2pix_amd.sam import get_mask, select_box
    model, pred = tiny_sam
    boxes = torch.tensor([[0.40, 0.45, 0.50, 0.60], [0.70, 0.30, 0.40, 0.50]])      # cxcywh in [0, 1]
    phrases = ["a brown dog", "cat"]
    # (the reference's e = 10 erodes this random-weight model's speckled masks to nothing: the first two cases keep something to compare, the third is the default)
    inside = []
    for ph, kw in [("dog", dict(d=40, e=4, b=20)), ("the cat", dict(d=12, e=5, b=0)), ("dog", dict(d=40, b=20))]:
        got = get_mask(ph, boxes, phrases, pred, size=320, **kw)
        want = _oracle_get_mask(select_box(ph, boxes, phrases, 0, 320), kw.get("e", 10), kw["d"], kw["b"], 320)
        assert got.size == (320, 320) and got.mode == "L"
        a = prepare_mask(torch.from_numpy(np.array(got)), 40, 40, "cpu")
        w = prepare_mask(torch.from_numpy(np.array(want)), 40, 40, "cpu")
        diff = float((a != w).float().mean())
        print(f"get_mask {ph!r}: {diff:.3%} of the latent cells differ, {float(w.mean()):.1%} inside")
        inside.append(float(w.mean()))
        assert diff <= 0.01, diff
    assert 0.5 < inside[0] < 0.95 and 0.01 < inside[1] < 0.2      # (the oracle's masks, measured on the CPU: 78 % and 2.8 % inside)


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------------------------
def test_pipeline_subjects_by_phrase(L):
    """(phrase, embedding) subjects: detector boxes -> SAM masks -> the inpaint pass; equals `subject_consistency` on the masks `get_mask` returns, differs from
    subject_strength=0; (mask, embedding) subjects give what they gave before"""
    from instructany2pix_amd.config import tiny, tiny_vae
    from instructany2pix_amd.inpaint import subject_consistency
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    from instructany2pix_amd.sam import get_mask
    from instructany2pix_amd.unet import HipUNet2DConditionModel
    from instructany2pix_amd.vae import HipAutoencoderKL
    from instructany2pix_amd.weights import ip_adapter_specs, synthetic_state_dict, unet_param_specs, vae_param_specs
    # a SAM whose masks survive the reference's 10 x 10 erosion: positive biases on the upscaled features and on the hypernetwork's output make every logit
    # positive (a random-weight model's speckles erode to an empty mask, and an empty mask re-paints nothing); box-to-mask values are tested above
    from instructany2pix_amd.sam import HipSamModel, HipSamPredictor, sam_tiny_config
    sd = {k: v.clone() for k, v in R.oracle_model().state_dict().items()}
    sd["mask_decoder.upscale_conv2.bias"] += 2.0
    sd["mask_decoder.output_hypernetworks_mlps.0.proj_out.bias"] += 1.0
    pred = HipSamPredictor(HipSamModel(sam_tiny_config(), DEV).load_state_dict(sd))
    cfg, vcfg = tiny(), tiny_vae()
    base = HipUNet2DConditionModel(cfg, DEV)
    base.load_state_dict(synthetic_state_dict(unet_param_specs(cfg), seed=7))
    vae = HipAutoencoderKL(vcfg, DEV)
    vae.load_state_dict(synthetic_state_dict(vae_param_specs(vcfg), seed=7))
    specs = ip_adapter_specs(cfg, 64)
    ck = {"image_proj": synthetic_state_dict(specs["image_proj"], seed=7), "ip_adapter": synthetic_state_dict(specs["ip_adapter"], seed=7)}
    g = torch.Generator().manual_seed(8)
    rn = lambda *s: torch.randn(*s, generator=g)
    emb = dict(prompt_embeds=rn(1, 77, cfg.cross_attention_dim).half(), pooled_prompt_embeds=rn(1, cfg.pooled_dim).half(),
               negative_prompt_embeds=rn(1, 77, cfg.cross_attention_dim).half(), negative_pooled_prompt_embeds=rn(1, cfg.pooled_dim).half())
    subjects = [("the dog.", rn(64)), ("cat's", rn(64))]
    cond = dict(image_embeds=rn(1, 64), base_embed=rn(1, 64), y=rn(1, 64), caption="a photo", base_latents=rn(1, 4, 16, 16).half(), **emb,
                subject_data=subjects, subject_noise=rn(1, 4, 16, 16).half(), **{"subject_" + k: v for k, v in emb.items()})
    boxes, phrases = torch.tensor([[0.35, 0.40, 0.40, 0.50], [0.70, 0.60, 0.45, 0.55]]), ["dog", "a cat"]
    seen = []

    def detector(image, text_prompt):
        seen.append((image.shape, image.dtype, text_prompt))
        return boxes, phrases

    pipe = InstructAny2PixPipeline(unet=base, ip_ckpt=ck, device=DEV, clip_embeddings_dim=64, conditioner=lambda inst, mm, use_cache=False: cond, vae=vae,
                                   segmenter=pred, detector=detector)
    run = lambda s: pipe("add the dog", [], num_inference_steps=5, cfg=4.0, refinement=0.0, subject_strength=s)
    torch.manual_seed(3)
    non_refined, out, msg = run(0.7)
    assert msg == "SUCCESS!" and torch.isfinite(out).all() and not torch.equal(non_refined, out)
    assert seen == [((64, 64, 3), np.uint8, "the dog.. cat's")]
    # by hand: the segmenter's image is the decoded result, masks from get_mask with the stripped phrases, then the loop on masks
    masks = [get_mask(ph, boxes, phrases, pred, i=0, d=40, b=20, size=64) for ph in ("the dog", "cat")]
    assert all(np.array_equal(np.array(a), np.array(b)) for a, b in zip(masks, pipe.subject_masks)) and all(np.array(m).max() == 255 for m in masks)
    pairs = [(torch.from_numpy(np.array(m)), e) for m, (_, e) in zip(masks, subjects)]
    by_hand = subject_consistency(pairs, non_refined, pipe.ip_adapter_xl_inpaint, 0.7, output_type="latent", noise=cond["subject_noise"], **emb)
    assert torch.equal(by_hand, out)
    pipe.ip_adapter_xl.set_scale(1.0)
    torch.manual_seed(3)
    a, b, _ = run(0.0)
    assert torch.equal(a, b) and torch.equal(a, non_refined)
    # (mask, embedding) entries: exactly today's route
    cond["subject_data"] = pairs
    pipe.ip_adapter_xl.set_scale(1.0)
    torch.manual_seed(3)
    _, out2, _ = run(0.7)
    assert torch.equal(out2, out)
    # missing pieces are named
    cond["subject_data"] = subjects
    pipe.gdino = None
    pipe.ip_adapter_xl.set_scale(1.0)
    with pytest.raises(KeyError, match="subject_boxes"):
        run(0.7)
    cond["subject_boxes"] = (boxes, phrases)
    pipe.sam = None
    pipe.ip_adapter_xl.set_scale(1.0)
    with pytest.raises(ValueError, match="segmenter="):
        run(0.7)
    pipe.sam = pred
    pipe.ip_adapter_xl.set_scale(1.0)
    torch.manual_seed(3)
    _, out3, _ = run(0.7)
    assert torch.equal(out3, out)
