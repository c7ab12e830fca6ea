"""`control_from=` at the top level on the MI355X: the condition map made on the device from the base image the pipeline holds drives the edit exactly as the
same map brought as `control_image=` does (latents compared with torch.equal), `debug` returns the map and it is tests/canny_ref.py's of the base image,
`control_from=None` is the plain call, the refusals, and the composition with the LCM sampler and with an edit mask."""
import os
import sys

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import canny_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANNY = {"kind": "canny", "low": 100, "high": 300}


def base_picture():
    """128 x 128 RGB: soft noise over blocks and a disc, so that the Canny map has strong, weak-kept and weak-dropped pixels"""
    g = np.random.default_rng(12)
    y, x = np.mgrid[0:128, 0:128]
    img = np.stack([40 + 60 * ((x // 32 + y // 32) % 2), 90 + 100 * (((x - 70) ** 2 + (y - 60) ** 2) < 900), 30 + x], -1).astype(np.float64)
    img += g.normal(0, 14, img.shape)
    return PIL.Image.fromarray(np.clip(np.rint(img), 0, 255).astype(np.uint8))


class Setup:
    def __init__(self):
        from test_controlnet_gpu import Models
        from instructany2pix_amd.config import VAEConfig
        from instructany2pix_amd.pipeline import InstructAny2PixPipeline
        from instructany2pix_amd.vae import HipAutoencoderKL
        from instructany2pix_amd.weights import synthetic_state_dict, vae_param_specs
        self.m = m = Models()
        vcfg = VAEConfig(block_out_channels=(64, 128, 128, 128), layers_per_block=1).validate()     # four levels: 8 pixels per latent cell, as the ControlNet's embedding assumes
        self.vae = HipAutoencoderKL(vcfg, DEV)
        self.vae.load_state_dict(synthetic_state_dict(vae_param_specs(vcfg), seed=7))
        g = torch.Generator().manual_seed(31)
        rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        b = m.ucfg
        self.image = base_picture()
        self.c = dict(image_embeds=rn(1, 64), base_embed=rn(1, 64), y=rn(1, 64), caption="a photo", base_image=self.image,
                      prompt_embeds=rn(1, 77, b.cross_attention_dim).half(), pooled_prompt_embeds=rn(1, b.pooled_dim).half(),
                      negative_prompt_embeds=rn(1, 77, b.cross_attention_dim).half(), negative_pooled_prompt_embeds=rn(1, b.pooled_dim).half())
        self.c_latents = dict(self.c, base_latents=rn(1, 4, 16, 16).half())
        del self.c_latents["base_image"]
        mk = lambda c, **kw: InstructAny2PixPipeline(unet=m.unet, ip_ckpt=m.ck, device=DEV, clip_embeddings_dim=64, vae=self.vae,      # noqa: E731
                                                     conditioner=lambda inst, mm, use_cache=False: c, **kw)
        self.pipe, self.pipe_latents, self.bare = mk(self.c, controlnet=m.cn), mk(self.c_latents, controlnet=m.cn), mk(self.c)
        for p in (self.bare, self.pipe_latents, self.pipe):
            p.ip_adapter_xl.set_scale(1.0)
        self.kw = dict(num_inference_steps=3, refinement=0, seed=11, control_scale=0.9)

    def close(self):
        for p in (self.pipe, self.pipe_latents, self.bare):
            p.ip_adapter_xl.disable()
        from instructany2pix_amd import _ffi
        _ffi.lib().ia2p_debug_set_gn_plan(-1)


@pytest.fixture(scope="module")
def s():
    st = Setup()
    yield st
    st.close()


@pytest.fixture(scope="module")
def plain(s):
    return s.pipe("edit", [], **s.kw)[0].clone()


def rel(a, b):
    a, b = a.float().cpu().reshape(-1), b.float().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("kind", ["canny", "blur", "grey", "canny_dict", "blur_dict"])
def test_control_from_is_the_control_image_of_its_own_map(s, plain, kind):
    from instructany2pix_amd.condition import Condition
    spec = {"canny": "canny", "blur": "blur", "grey": "grey", "canny_dict": CANNY, "blur_dict": Condition(kind="blur", sigma=1.2)}[kind]
    made = s.pipe("edit", [], control_from=spec, **s.kw)[0].clone()
    picture = s.pipe.make_control_image(spec, base_image=s.image)
    assert isinstance(picture, PIL.Image.Image) and picture.size == (128, 128) and picture.mode == ("RGB" if kind.startswith("blur") else "L")
    brought = s.pipe("edit", [], control_image=picture, **s.kw)[0]
    assert bool(torch.isfinite(made.float()).all()) and torch.equal(made, brought)
    assert rel(made, plain) > 1e-2, "the condition map does not change the result"
    if kind == "canny":
        assert np.array_equal(np.asarray(s.pipe.make_control_image(spec)), np.asarray(picture))     # base_image=None: the image of the last request


def test_debug_returns_the_map_and_it_is_the_reference_of_the_base_image(s):
    px = np.asarray(s.image)
    grey = R.grey_ref(px)
    state = R.canny_state_ref(grey, CANNY["low"], CANNY["high"])
    want = R.hysteresis_ref(state)
    strong, kept, dropped = int((state == 2).sum()), int(((state == 1) & (want > 0)).sum()), int(((state == 1) & (want == 0)).sum())
    print(f"[condition] base picture census: strong {strong}, weak kept {kept}, weak dropped {dropped}")
    assert strong > 50 and kept > 50 and dropped > 50
    msg = s.pipe("edit", [], control_from=CANNY, debug=True, **s.kw)[2]
    cm = msg["control_map"]
    assert cm.dtype == torch.uint8 and cm.is_cuda and tuple(cm.shape) == (1, 128, 128) and np.array_equal(cm[0].cpu().numpy(), want)
    assert np.array_equal(s.pipe("edit", [], control_from="grey", debug=True, **s.kw)[2]["control_map"][0].cpu().numpy(), grey)
    blur = s.pipe("edit", [], control_from={"kind": "blur", "sigma": 2.0}, debug=True, **s.kw)[2]["control_map"]
    from instructany2pix_amd.condition import gauss_taps
    assert tuple(blur.shape) == (1, 128, 128, 3) and np.array_equal(blur.cpu().numpy(), R.gauss_ref(px[None], gauss_taps(2.0)))
    assert "control_map" not in s.pipe("edit", [], debug=True, **s.kw)[2]


def test_control_from_none_is_the_plain_call(s, plain):
    assert torch.equal(s.pipe("edit", [], control_from=None, **s.kw)[0], plain)
    assert torch.equal(s.pipe("edit", [], control_from="canny", **dict(s.kw, control_scale=0.0))[0], plain)      # a scale of 0 is the plain call, as with control_image
    assert torch.equal(s.bare("edit", [], **s.kw)[0], plain)                                       # ... and so is a pipeline that has no ControlNet at all


def test_refusals(s):
    with pytest.raises(ValueError, match="one of the two"):
        s.pipe("edit", [], control_from="canny", control_image=s.image, **s.kw)
    with pytest.raises(ValueError, match="controlnet="):
        s.bare("edit", [], control_from="canny", **s.kw)
    with pytest.raises(ValueError, match="controlnet="):
        s.bare("edit", [], control_image=s.image, **s.kw)                                          # the error control_image gives
    with pytest.raises(ValueError, match="kind"):
        s.pipe("edit", [], control_from="depth", **s.kw)
    with pytest.raises(ValueError, match="base latents only"):
        s.pipe_latents("edit", [], control_from="canny", **s.kw)                                   # the conditioner brought latents: no 8-bit pixels to make the map from
    with pytest.raises(ValueError, match="8 x the latent grid"):
        s.pipe.control_map(CANNY, s.image.resize((64, 64)), torch.zeros(1, 4, 16, 16))
    with pytest.raises(TypeError):
        s.pipe.edit_batch(["edit"], [[]], control_from="canny")                                    # control is not in the batch paths


def test_denoise_takes_the_base_pixels(s):
    from instructany2pix_amd.pipeline import embeds
    g = torch.Generator().manual_seed(5)
    lat, la = torch.randn(1, 4, 16, 16, generator=g).half(), torch.randn(64, generator=g)
    kw = dict(**embeds(s.c), num_inference_steps=3, seed=3, control_scale=0.8)
    a = s.pipe.denoise(lat, la, control_from=CANNY, control_base=s.image, **kw)[0].clone()
    b = s.pipe.denoise(lat, la, control_image=s.pipe.make_control_image(CANNY, s.image), **kw)[0]
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="base latents only"):
        s.pipe.denoise(lat, la, control_from=CANNY, **kw)
    with pytest.raises(ValueError, match="one of the two"):
        s.pipe.denoise(lat, la, control_from=CANNY, control_base=s.image, control_image=s.image, **kw)


def test_composes_with_the_lcm_sampler_and_an_edit_mask(s, plain):
    picture = s.pipe.make_control_image(CANNY, base_image=s.image)
    lcm = dict(s.kw, sampler="lcm", sample_steps=3)
    a = s.pipe("edit", [], control_from=CANNY, **lcm)[0].clone()
    assert torch.equal(a, s.pipe("edit", [], control_image=picture, **lcm)[0]) and rel(a, s.pipe("edit", [], **lcm)[0]) > 1e-2
    mask = torch.zeros(1, 1, 16, 16)
    mask[..., 4:12, 4:12] = 1.0
    a = s.pipe("edit", [], control_from=CANNY, edit_mask=mask, **s.kw)[0].clone()
    b = s.pipe("edit", [], control_image=picture, edit_mask=mask, **s.kw)[0].clone()
    free = s.pipe("edit", [], edit_mask=mask, **s.kw)[0]
    assert torch.equal(a, b)
    keep = (mask == 0).expand_as(a).to(a.device)
    assert torch.equal(a[keep], free[keep]) and not torch.equal(a[~keep], free[~keep])             # outside the mask: the base latents, control or not
