"""The HIP image codec (csrc/image.hip) against numpy restatements of diffusers 0.26.3's image arithmetic, exhaustively over 8-bit codes and fp16
bit patterns, and images through the public pipeline surface (`vae=`, PIL `image=` / `mask_image=`, `output_type`, base images)."""
import numpy as np
import PIL.Image
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- numpy restatements of the diffusers formulas ---------------------------------------------------------------------------------------------
def ref_from_u8(u8_bhwc, normalize=True):
    """pil_to_numpy (np.float32 / 255.0) -> numpy_to_pt -> normalize (2 x - 1, fp32) -> .to(float16)"""
    v = u8_bhwc.astype(np.float32) / 255.0
    if normalize:
        v = 2.0 * v - 1.0
    return torch.from_numpy(v.transpose(0, 3, 1, 2).astype(np.float16))


def ref_unit(x_f16):
    """denormalize of the fp32 image: (x / 2 + 0.5).clamp(0, 1)"""
    with np.errstate(invalid="ignore"):                                     # (NaN inputs: compared on their own)
        return np.clip(x_f16.astype(np.float32) / 2 + np.float32(0.5), 0, 1)


def ref_to_u8(x_bchw_f16):
    """postprocess -> numpy_to_pil: (v * 255).round().astype(uint8), NHWC (finite and infinite inputs; NaN has no defined result there)"""
    with np.errstate(invalid="ignore"):
        return (ref_unit(x_bchw_f16) * np.float32(255)).round().astype(np.uint8).transpose(0, 2, 3, 1)


def all_fp16():
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)


@pytest.fixture(scope="module")
def codec():
    from instructany2pix_amd import build
    build.build(verbose=False)
    from instructany2pix_amd import image_processor
    return image_processor


# ---- exhaustive bit-exactness ------------------------------------------------------------------------------------------------------------------
def test_to_u8_every_fp16_pattern(codec):
    x = all_fp16()
    nan = torch.isnan(x)
    got = codec.image_to_u8(x.reshape(1, 1, 256, 256).to(DEV).contiguous()).cpu().reshape(-1)
    want = torch.from_numpy(ref_to_u8(x.reshape(1, 1, 256, 256).numpy().copy()).reshape(-1).copy())
    assert torch.equal(got[~nan], want[~nan])
    assert int(nan.sum()) == 2046 and bool((got[nan] == 0).all())           # NaN -> 0
    # the same through torch on the GPU (what the pipelines' eager path computed)
    t = ((x[~nan].to(DEV).float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).cpu()
    assert torch.equal(got[~nan], t)


def test_requantize_every_fp16_pattern_equals_to_8bit_image(codec):
    from instructany2pix_amd.pipeline import to_8bit_image
    x = all_fp16().to(DEV)
    nan = torch.isnan(x)
    got = codec.requantize(x.contiguous())
    want = to_8bit_image(x)
    assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))
    assert bool((got[nan] == -1).all())                                      # NaN -> code 0 -> -1
    y = x.clone()
    codec.requantize(y, out=y)                                               # in place
    assert torch.equal(y.view(torch.int16), got.view(torch.int16))


def test_to_f32_every_fp16_pattern(codec):
    x = all_fp16()
    nan = torch.isnan(x).numpy()
    want = ref_unit(x.numpy())
    for nhwc in (True, False):
        got = codec.image_to_f32(x.reshape(1, 1, 256, 256).to(DEV).contiguous(), nhwc=nhwc).cpu().numpy().reshape(-1)
        assert np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))
        assert np.isnan(got[nan]).all()


@pytest.mark.parametrize("C", [1, 3])
def test_from_u8_every_code(codec, C):
    codes = np.arange(256, dtype=np.uint8)
    for H, W in ((256, 1), (16, 16), (1, 256)):
        u8 = np.stack([np.roll(codes, 7 * c) for c in range(C)], -1).reshape(1, H, W, C)
        for normalize in (True, False):
            got = codec.image_from_u8(torch.from_numpy(u8).to(DEV), normalize=normalize).cpu()
            assert torch.equal(got.view(torch.int16), ref_from_u8(u8, normalize).view(torch.int16))


def test_eight_bit_round_trip_is_lossless(codec):
    codes = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1).to(DEV)
    lut = codec.image_from_u8(codes)
    assert torch.equal(codec.image_to_u8(lut), codes)
    q = torch.arange(256, dtype=torch.float32)
    assert torch.equal((((lut.cpu().reshape(-1).float() / 2) + 0.5) * 255).round(), q)
    assert torch.equal(codec.requantize(lut), lut)


# ---- shapes, tails, streams --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(1, 61, 67), (3, 61, 67), (3, 64, 64), (1, 1, 5), (2, 32, 40)])
@pytest.mark.parametrize("C", [1, 3])
def test_codec_shapes_and_side_stream(codec, B, H, W, C):
    g = np.random.default_rng(B * 1000 + H * W + C)
    u8 = g.integers(0, 256, size=(B, H, W, C), dtype=np.uint8)
    x = torch.from_numpy((g.standard_normal((B, C, H, W)) * 0.8).astype(np.float16))
    u8_d, x_d = torch.from_numpy(u8).to(DEV), x.to(DEV)

    def run():
        return (codec.image_from_u8(u8_d), codec.image_from_u8(u8_d, normalize=False), codec.image_to_u8(x_d),
                codec.image_to_f32(x_d, nhwc=True), codec.image_to_f32(x_d, nhwc=False), codec.requantize(x_d))
    outs = run()
    torch.cuda.synchronize()
    assert torch.equal(outs[0].cpu().view(torch.int16), ref_from_u8(u8).view(torch.int16))
    assert torch.equal(outs[1].cpu().view(torch.int16), ref_from_u8(u8, False).view(torch.int16))
    assert np.array_equal(outs[2].cpu().numpy(), ref_to_u8(x.numpy()))
    assert np.array_equal(outs[3].cpu().numpy(), ref_unit(x.numpy()).transpose(0, 2, 3, 1))
    assert np.array_equal(outs[4].cpu().numpy(), ref_unit(x.numpy()))
    from instructany2pix_amd.pipeline import to_8bit_image
    assert torch.equal(outs[5].view(torch.int16), to_8bit_image(x_d).view(torch.int16))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = run()
    side.synchronize()
    for a, b in zip(outs, again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_processor_round_trip_pil(codec):
    from instructany2pix_amd.image_processor import VaeImageProcessor
    p = VaeImageProcessor(vae_scale_factor=4, device=DEV)
    a = np.random.default_rng(0).integers(0, 256, size=(48, 40, 3), dtype=np.uint8)
    t = p.preprocess([PIL.Image.fromarray(a), PIL.Image.fromarray(a).convert("RGBA")])   # non-RGB modes are converted
    assert t.dtype == torch.float16 and tuple(t.shape) == (2, 3, 48, 40) and t.is_cuda
    assert torch.equal(t[0], t[1]) and torch.equal(p.preprocess(a), t[:1])  # uint8 HWC ndarray
    assert torch.equal(t.cpu().view(torch.int16), ref_from_u8(np.stack([a, a])).view(torch.int16))
    out = p.postprocess(t, output_type="pil")
    assert len(out) == 2 and np.array_equal(np.asarray(out[0]), a)
    f = a.astype(np.float32) / 255.0                                          # diffusers' float [0, 1] convention
    assert torch.equal(p.preprocess(f[None]), (2.0 * torch.from_numpy(f[None].transpose(0, 3, 1, 2)) - 1.0).half().to(DEV))
    assert p.preprocess(t) is not None and torch.equal(p.preprocess(t), t)   # [-1, 1] tensors pass through
    np_out = p.postprocess(t, output_type="np")
    assert np_out.dtype == np.float32 and np_out.shape == (2, 48, 40, 3)
    pt_out = p.postprocess(t, output_type="pt")
    assert pt_out.dtype == torch.float32 and tuple(pt_out.shape) == (2, 3, 48, 40)
    mp = VaeImageProcessor(vae_scale_factor=4, do_normalize=False, do_binarize=True, do_convert_grayscale=True, device=DEV)
    m = mp.preprocess(PIL.Image.fromarray(a))
    gray = np.asarray(PIL.Image.fromarray(a).convert("L"))
    assert tuple(m.shape) == (1, 1, 48, 40) and torch.equal(m[0, 0].cpu(), torch.from_numpy((gray >= 128).astype(np.float16)))


# ---- pipelines ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    from instructany2pix_amd.config import tiny, tiny_refiner, tiny_vae
    from instructany2pix_amd.unet import HipUNet2DConditionModel
    from instructany2pix_amd.vae import HipAutoencoderKL
    from instructany2pix_amd.weights import unet_param_specs, ip_adapter_specs, vae_param_specs, synthetic_state_dict
    bcfg, rcfg, vcfg = tiny(), tiny_refiner(), tiny_vae()
    base = HipUNet2DConditionModel(bcfg, DEV)
    base.load_state_dict(synthetic_state_dict(unet_param_specs(bcfg), seed=7))
    ref = HipUNet2DConditionModel(rcfg, DEV)
    ref.load_state_dict(synthetic_state_dict(unet_param_specs(rcfg), seed=11))
    vae = HipAutoencoderKL(vcfg, DEV)
    vae.load_state_dict(synthetic_state_dict(vae_param_specs(vcfg), seed=7))
    specs = ip_adapter_specs(bcfg, 64)
    ck = {"image_proj": synthetic_state_dict(specs["image_proj"], seed=7), "ip_adapter": synthetic_state_dict(specs["ip_adapter"], seed=7)}
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g)
    cond = dict(image_embeds=rn(1, 64), base_embed=rn(1, 64), y=rn(1, 64), caption="a photo",
                prompt_embeds=rn(1, 77, bcfg.cross_attention_dim).half(), pooled_prompt_embeds=rn(1, bcfg.pooled_dim).half(),
                negative_prompt_embeds=rn(1, 77, bcfg.cross_attention_dim).half(), negative_pooled_prompt_embeds=rn(1, bcfg.pooled_dim).half(),
                refiner_prompt_embeds=rn(1, 77, rcfg.cross_attention_dim).half(), refiner_pooled_prompt_embeds=rn(1, rcfg.pooled_dim).half(),
                refiner_negative_prompt_embeds=rn(1, 77, rcfg.cross_attention_dim).half(), refiner_negative_pooled_prompt_embeds=rn(1, rcfg.pooled_dim).half(),
                refiner_noise=rn(1, 4, 16, 16).half())
    return dict(base=base, ref=ref, vae=vae, ck=ck, cond=cond)


def _image(w=64, h=64, seed=0):
    return PIL.Image.fromarray(np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8))


def _top(models, cond):
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    return InstructAny2PixPipeline(unet=models["base"], ip_ckpt=models["ck"], device=DEV, clip_embeddings_dim=64,
                                   conditioner=lambda inst, mm, use_cache=False: cond, refiner_unet=models["ref"], vae=models["vae"])


def _count_decodes(vae):
    calls = []
    inner = vae.decode

    def decode(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    vae.decode = decode
    return calls, lambda: vars(vae).pop("decode")


def test_call_pil_output_equals_codec_on_the_decoded_latents(models, codec):
    vae = models["vae"]
    pipe = _top(models, dict(models["cond"], base_image=_image()))
    for refinement in (0.5, 0.0):
        torch.manual_seed(3)
        nr_l, oo_l, msg = pipe("make it blue", [], num_inference_steps=4, cfg=4.0, refinement=refinement)
        assert msg == "SUCCESS!" and tuple(nr_l.shape) == (1, 4, 16, 16)
        calls, restore = _count_decodes(vae)
        try:
            torch.manual_seed(3)
            nr_p, oo_p, _ = pipe("make it blue", [], num_inference_steps=4, cfg=4.0, refinement=refinement, output_type="pil")
        finally:
            restore()
        assert len(calls) == (2 if refinement > 0 else 1)                    # one decode per returned image (the hand-over decode is re-used)
        for lat, pil in ((nr_l, nr_p), (oo_l, oo_p)):
            assert isinstance(pil, list) and len(pil) == 1 and pil[0].size == (64, 64) and pil[0].mode == "RGB"
            want = codec.image_to_u8(vae.decode_from_latents(lat))[0].cpu().numpy()
            assert np.array_equal(np.asarray(pil[0]), want)
        if refinement == 0:
            assert oo_p is nr_p
        else:
            assert not np.array_equal(np.asarray(nr_p[0]), np.asarray(oo_p[0]))
    torch.manual_seed(3)
    nr_n, _, _ = pipe("make it blue", [], num_inference_steps=4, cfg=4.0, refinement=0.0, output_type="np")
    assert nr_n.dtype == np.float32 and nr_n.shape == (1, 64, 64, 3)


def test_base_img_path_route_equals_the_pil_route(models, tmp_path):
    from instructany2pix_amd.pipeline import loas_base_img
    path = str(tmp_path / "base.png")
    _image(80, 64, seed=4).save(path)
    by_path = _top(models, dict(models["cond"], base_img_path=path))
    by_path.base_image_size = 64
    by_pil = _top(models, dict(models["cond"], base_image=loas_base_img(path, 64)))
    outs = []
    for pipe in (by_path, by_pil):
        torch.manual_seed(3)
        outs.append(pipe("make it blue", [], num_inference_steps=4, cfg=4.0, refinement=0.0))
    assert torch.equal(outs[0][0], outs[1][0])
    # base_latents wins when present
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(9)).half()
    both = _top(models, dict(models["cond"], base_image=_image(), base_latents=lat))
    only = _top(models, dict(models["cond"], base_latents=lat))
    r = []
    for pipe in (both, only):
        torch.manual_seed(3)
        r.append(pipe("make it blue", [], num_inference_steps=4, cfg=4.0, refinement=0.0)[0])
    assert torch.equal(r[0], r[1])


def test_sub_pipelines_accept_pil_images(models):
    from instructany2pix_amd.ddim import SDXLDDIMPipeline, StableDiffusionXLPipeline
    from instructany2pix_amd.img2img import StableDiffusionXLImg2ImgPipeline
    from instructany2pix_amd.inpaint import StableDiffusionXLInpaintPipeline
    vae, c = models["vae"], models["cond"]
    img = _image(seed=6)
    inv = SDXLDDIMPipeline(models["base"], vae=vae)
    t = inv.image_processor.preprocess(img)
    emb = dict(prompt_embeds=c["prompt_embeds"], pooled_prompt_embeds=c["pooled_prompt_embeds"])
    neg = dict(negative_prompt_embeds=c["negative_prompt_embeds"], negative_pooled_prompt_embeds=c["negative_pooled_prompt_embeds"])
    runs = []
    for image in (img, t):
        torch.manual_seed(1)
        runs.append(inv.inverse(image=image, num_inference_steps=3, **emb).images)
    assert torch.equal(runs[0], runs[1]) and tuple(runs[0].shape) == (1, 4, 16, 16)

    rf = StableDiffusionXLImg2ImgPipeline(models["ref"], vae=vae)
    remb = dict(prompt_embeds=c["refiner_prompt_embeds"], pooled_prompt_embeds=c["refiner_pooled_prompt_embeds"],
                negative_prompt_embeds=c["refiner_negative_prompt_embeds"], negative_pooled_prompt_embeds=c["refiner_negative_pooled_prompt_embeds"])
    runs = []
    for image, ot in ((img, "latent"), (t, "latent"), (img, "pil")):
        torch.manual_seed(1)
        runs.append(rf(image=image, strength=0.5, num_inference_steps=4, noise=c["refiner_noise"], output_type=ot, **remb).images)
    assert torch.equal(runs[0], runs[1])
    assert np.array_equal(np.asarray(runs[2][0]), np.asarray(rf.image_processor.postprocess(vae.decode_from_latents(runs[0]))[0]))

    ip = StableDiffusionXLInpaintPipeline(models["base"], vae=vae)
    m = np.zeros((64, 64), dtype=np.uint8)
    m[8:40, 16:56] = 200
    mask = PIL.Image.fromarray(m)
    mt = ip.mask_processor.preprocess(mask)
    noise = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(2)).half()
    runs = []
    for image, mk in ((img, mask), (t, mt)):
        torch.manual_seed(1)
        runs.append(ip(image=image, mask_image=mk, strength=0.7, num_inference_steps=4, guidance_scale=4.0, noise=noise, output_type="latent",
                       **emb, **neg).images)
    assert torch.equal(runs[0], runs[1])

    sd = StableDiffusionXLPipeline(models["base"], vae=vae)
    xT = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3)).half()
    lat = sd(latents=xT, num_inference_steps=3, guidance_scale=4.0, output_type="latent", **emb, **neg).images
    pt = sd(latents=xT, num_inference_steps=3, guidance_scale=4.0, output_type="pt", **emb, **neg).images
    assert pt.dtype == torch.float32 and torch.equal(pt, sd.image_processor.postprocess(vae.decode_from_latents(lat), output_type="pt"))
