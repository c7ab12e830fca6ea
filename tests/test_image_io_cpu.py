"""Image input / output without a GPU: the reference's base-image loader (`resize_and_crop`, `loas_base_img`), the host half of the image
processor, the argument checks of the pipelines' new keywords, and the HIP image codec's refusals (made before any HIP call)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import PIL.Image
import pytest
import torch


def _noise_image(w, h, seed=0, mode="RGB"):
    a = np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return PIL.Image.fromarray(a).convert(mode)


# ---- resize_and_crop / loas_base_img -------------------------------------------------------------------------------------------------------
# (input size, target (w, h), size after the resize, crop box by hand (PIL rounds .5 edges half to even) per crop type)
CASES = [
    ((150, 100), (64, 64), (96, 64), {"top": (0, 0, 64, 64), "middle": (16, 0, 80, 64), "bottom": (32, 0, 96, 64)}),          # landscape
    ((155, 100), (64, 64), (99, 64), {"top": (0, 0, 64, 64), "middle": (18, 0, 82, 64), "bottom": (35, 0, 99, 64)}),          # odd excess: 17.5 .. 81.5
    ((100, 150), (64, 64), (64, 96), {"top": (0, 0, 64, 64), "middle": (0, 16, 64, 80), "bottom": (0, 32, 64, 96)}),          # portrait
    ((100, 157), (64, 64), (64, 100), {"top": (0, 0, 64, 64), "middle": (0, 18, 64, 82), "bottom": (0, 36, 64, 100)}),        # odd excess: 18 .. 82
    ((100, 100), (64, 64), (64, 64), {"top": (0, 0, 64, 64), "middle": (0, 0, 64, 64), "bottom": (0, 0, 64, 64)}),             # square
    ((120, 90), (48, 32), (48, 36), {"top": (0, 0, 48, 32), "middle": (0, 2, 48, 34), "bottom": (0, 4, 48, 36)}),              # non-square target
]


@pytest.mark.parametrize("src,size,scaled,boxes", CASES)
@pytest.mark.parametrize("crop_type", ["top", "middle", "bottom"])
def test_resize_and_crop_boxes(src, size, scaled, boxes, crop_type):
    from instructany2pix_amd.pipeline import resize_and_crop
    img = _noise_image(*src, seed=sum(src))
    out = resize_and_crop(img, size, crop_type=crop_type)
    assert out.size == size
    x0, y0, x1, y1 = boxes[crop_type]
    want = np.asarray(img.resize(scaled))[y0:y1, x0:x1]           # PIL's default resampling, as the reference calls it
    assert np.array_equal(np.asarray(out), want)


def test_resize_and_crop_rejects_unknown_crop_type():
    from instructany2pix_amd.pipeline import resize_and_crop
    for src in ((150, 100), (100, 100)):
        with pytest.raises(ValueError):
            resize_and_crop(_noise_image(*src), (64, 64), crop_type="left")


def test_loas_base_img_loads_crops_and_resizes(tmp_path):
    from instructany2pix_amd.pipeline import loas_base_img, resize_and_crop
    img = _noise_image(155, 100, seed=3)
    path = str(tmp_path / "base.png")
    img.save(path)
    out = loas_base_img(path, size=64)
    assert out.size == (64, 64)
    assert np.array_equal(np.asarray(out), np.asarray(resize_and_crop(img, (64, 64), "middle")))


# ---- image processor, host side --------------------------------------------------------------------------------------------------------------
def test_default_height_width_rounds_down_to_the_vae_factor():
    from instructany2pix_amd.image_processor import VaeImageProcessor
    p8 = VaeImageProcessor(vae_scale_factor=8, device="cpu")
    assert p8.get_default_height_width(_noise_image(1023, 517)) == (512, 1016)
    assert p8.get_default_height_width(_noise_image(64, 64)) == (64, 64)
    assert p8.get_default_height_width(torch.zeros(1, 3, 70, 33)) == (64, 32)
    assert p8.get_default_height_width(np.zeros((1, 70, 33, 3))) == (64, 32)
    assert p8.get_default_height_width(_noise_image(100, 100), height=77, width=90) == (72, 88)
    p4 = VaeImageProcessor(vae_scale_factor=4, device="cpu")
    assert p4.get_default_height_width(_noise_image(67, 61)) == (60, 64)


def test_pil_host_half_resizes_converts_and_keeps_codes():
    from instructany2pix_amd.image_processor import VaeImageProcessor
    p = VaeImageProcessor(vae_scale_factor=8, device="cpu")
    rgba = _noise_image(70, 45, seed=1, mode="RGBA")
    u8, normalize = p.pil_to_u8([rgba])
    assert normalize and u8.dtype == np.uint8 and u8.shape == (1, 40, 64, 3) and u8.flags.c_contiguous
    want = np.asarray(rgba.resize((64, 40), resample=PIL.Image.Resampling.LANCZOS).convert("RGB"))
    assert np.array_equal(u8[0], want)
    img = _noise_image(64, 32, seed=2)
    u8, _ = p.pil_to_u8([img, img], height=32, width=64)              # no resize at the image's own size
    assert np.array_equal(u8[1], np.asarray(img))


def test_mask_grayscale_and_binarise_at_half():
    from instructany2pix_amd.image_processor import VaeImageProcessor
    mp = VaeImageProcessor(vae_scale_factor=8, do_normalize=False, do_binarize=True, do_convert_grayscale=True, device="cpu")
    ramp = np.tile(np.arange(256, dtype=np.uint8), (16, 1))           # 16 x 256, every code
    rgb = PIL.Image.fromarray(np.stack([ramp] * 3, -1))
    u8, normalize = mp.pil_to_u8([rgb])
    assert not normalize and u8.shape == (1, 16, 256, 1)
    gray = np.asarray(rgb.convert("L"))
    assert np.array_equal(u8[0, ..., 0], np.where(gray >= 128, 255, 0))
    # the same decision as diffusers' float path: binarize(pil_to_numpy(mask)) with q / 255 in fp32
    ref = VaeImageProcessor.binarize(VaeImageProcessor.pil_to_numpy([rgb.convert("L")]))
    assert np.array_equal(u8[0, ..., 0] // 255, ref[0].astype(np.uint8))
    with pytest.raises(ValueError):
        VaeImageProcessor(do_convert_rgb=True, do_convert_grayscale=True, device="cpu")


def test_postprocess_rejects_unknown_output_type():
    from instructany2pix_amd.image_processor import VaeImageProcessor
    p = VaeImageProcessor(device="cpu")
    with pytest.raises(ValueError):
        p.postprocess(torch.zeros(1, 3, 8, 8), output_type="jpeg")
    with pytest.raises(ValueError):
        p.postprocess(np.zeros((1, 8, 8, 3)), output_type="pil")
    z = torch.zeros(1, 4, 8, 8)
    assert p.postprocess(z, output_type="latent") is z


# ---- pipeline keywords -------------------------------------------------------------------------------------------------------------------------
def _fake_vae(blocks=(64, 128, 128)):
    """what the pipelines read from a HipAutoencoderKL at construction (no GPU needed for the checks below)"""
    return SimpleNamespace(config=SimpleNamespace(block_out_channels=blocks), device=torch.device("cpu"),
                           encode_to_latents=lambda image, generator=None: image, decode_from_latents=lambda z: z)


def test_vae_and_hooks_are_exclusive_and_the_scale_factor_follows_the_vae():
    from instructany2pix_amd.ddim import SDXLDDIMPipeline, StableDiffusionXLPipeline
    from instructany2pix_amd.img2img import StableDiffusionXLImg2ImgPipeline
    from instructany2pix_amd.inpaint import StableDiffusionXLInpaintPipeline
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    for cls in (SDXLDDIMPipeline, StableDiffusionXLPipeline, StableDiffusionXLImg2ImgPipeline, StableDiffusionXLInpaintPipeline):
        with pytest.raises(ValueError):
            cls(object(), vae=_fake_vae(), vae_encode=lambda x: x)
        with pytest.raises(ValueError):
            cls(object(), vae=_fake_vae(), vae_decode=lambda x: x)
        assert cls(object(), vae=_fake_vae()).vae_scale_factor == 4
        assert cls(object(), vae=_fake_vae((128, 256, 512, 512))).vae_scale_factor == 8
        hooks_only = cls(object(), vae_decode=lambda x: x)
        assert hooks_only.vae_scale_factor == 8 and hooks_only.vae is None and hooks_only.image_processor is None
    with pytest.raises(ValueError):
        InstructAny2PixPipeline(unet=object(), vae=_fake_vae(), vae_decode=lambda x: x)


def test_output_type_is_checked_before_any_work():
    from instructany2pix_amd.ddim import StableDiffusionXLPipeline
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline

    def conditioner(*a, **k):
        raise AssertionError("reached the conditioner")
    pipe = StableDiffusionXLPipeline(object(), vae=_fake_vae())
    with pytest.raises(ValueError, match="output_type"):
        pipe(prompt_embeds=torch.zeros(1, 77, 8), pooled_prompt_embeds=torch.zeros(1, 8), guidance_scale=1.0, output_type="jpeg")
    top = InstructAny2PixPipeline(unet=object(), conditioner=conditioner, vae=_fake_vae())
    with pytest.raises(ValueError, match="output_type"):
        top("x", [], output_type="jpeg")
    hooks = InstructAny2PixPipeline(unet=object(), conditioner=conditioner, vae_decode=lambda z: z)
    with pytest.raises(ValueError, match="vae="):
        hooks("x", [], output_type="pil")


# ---- HIP codec refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def test_codec_refuses_bad_arguments_before_any_hip_call(lib):
    from instructany2pix_amd import _ffi
    INVALID, SHAPE = 1, 2
    p = C.c_void_p(4096)            # never dereferenced: every call below is refused on its arguments
    n = None
    err = lambda: lib.ia2p_last_error(None)
    for call in (lambda s, d, B, H, W, Ch: lib.ia2p_image_from_u8(n, s, d, B, H, W, Ch, 1),
                 lambda s, d, B, H, W, Ch: lib.ia2p_image_to_u8(n, s, d, B, H, W, Ch),
                 lambda s, d, B, H, W, Ch: lib.ia2p_image_to_f32(n, s, d, B, H, W, Ch, 1)):
        assert call(None, p, 1, 8, 8, 3) == INVALID and b"null" in err()
        assert call(p, None, 1, 8, 8, 3) == INVALID
        assert call(p, p, 1, 8, 8, 2) == SHAPE and b"C=2" in err()
        assert call(p, p, 1, 8, 8, 4) == SHAPE
        assert call(p, p, 0, 8, 8, 3) == SHAPE
        assert call(p, p, 1, 0, 8, 3) == SHAPE
        assert call(p, p, 1, 8, 0, 1) == SHAPE
        assert call(p, p, -1, 8, 8, 3) == INVALID
        assert call(p, p, 16, 8192, 8192, 3) == SHAPE and b"32-bit" in err()      # 3 * 2^30 elements > 2^31 - 1
    assert lib.ia2p_image_from_u8(n, p, p, 1, 8, 8, 3, 2) == INVALID
    assert lib.ia2p_image_to_f32(n, p, p, 1, 8, 8, 3, 7) == INVALID
    assert lib.ia2p_image_requantize(n, None, p, 16) == INVALID
    assert lib.ia2p_image_requantize(n, p, None, 16) == INVALID
    assert lib.ia2p_image_requantize(n, p, p, 0) == SHAPE
    assert lib.ia2p_image_requantize(n, p, p, -5) == INVALID
    assert lib.ia2p_image_requantize(n, p, p, 1 << 31) == SHAPE
    with pytest.raises(ValueError, match="SHAPE"):
        _ffi.check(lib.ia2p_image_to_u8(n, p, p, 1, 8, 8, 2))
