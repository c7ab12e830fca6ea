"""`InstructAny2PixPipeline` call surface for the denoise hot path (reference instructany2pix/pipeline.py).

The reference's `__call__` (:303-386) does, in order: LLM + ImageBind (`forward_llm`, off-path), the GPT-2 prior
(off-path), then THE HOT SEGMENT
    :306-307  share one UNet between the pipelines, fresh DDIM scheduler
    :322-324  fuse base / instruction / prior embeddings into `latent_la` and renormalise to `norm`
    :330      latent_inv = pipe_inversion.inverse(num_inference_steps=N, prompt='', image=img_base)
    :331-337  polar interpolation with fresh noise (CPU, fp16, global torch RNG)
    :342-354  ip_adapter_xl.generate(prompt=..., clip_image_embeds=latent_la[0], latents=latent_inv, guidance_scale=cfg, scale=scale)
followed by the refiner pass (:358-361; `self.piperf`, img2img.py — SURVEY.md §8f rank 2, built; with a VAE attached the base result
reaches it the reference's way: decoded, quantised to 8 bits, re-encoded) and the subject-consistency
pass (:363-368; `self.pipe_inpainting` / `ip_adapter_xl_inpaint`, inpaint.py — rank 3, built; its masks come from SAM / GroundingDINO,
which stay outside).

This class keeps the constructor attributes other code touches (`.pipe`, `.pipe_inversion`, `.ip_adapter_xl`,
`.cache`; serve.py:9 assigns `.pipe.scheduler`) and the `__call__` keyword surface. The off-path stages are
injected as callables (`conditioner`, `text_encoder`, `vae`); `denoise()` is the hot segment itself on
already-computed conditioning and is what bench.py and the parity tests drive.
"""
from __future__ import annotations

import contextlib
import os
from typing import Any, Callable, Optional

import numpy as np
import PIL.Image
import torch

from . import noise as _noise
from .config import UNetConfig, sdxl_base
from .ddim import SDXLDDIMPipeline, StableDiffusionXLControlNetPipeline, StableDiffusionXLPipeline
from .img2img import StableDiffusionXLImg2ImgPipeline
from .inpaint import StableDiffusionXLInpaintPipeline, subject_consistency, subject_consistency_from_boxes
from .image_processor import OUTPUT_TYPES, requantize
from .ip_adapter import IPAdapterXL
from .prior import MODALITY
from .scheduler import DDIMScheduler, LCMScheduler, check_step_noise, resolve_sampler
from .unet import HipUNet2DConditionModel


def polar_intrtpolate(x, y, alpha):
    """reference pipeline.py:295-300 (name kept, typo included); runs where its inputs live (CPU fp16 in the reference)."""
    n0 = x.norm()
    n1 = y.norm()
    ll = x * alpha + y * (1 - alpha)
    n = n0 * alpha + n1 * (1 - alpha)
    return ll / ll.norm() * n


def to_8bit_image(image):
    """What the reference's hand-over between its pipelines does to an image TENSOR IN [-1, 1] (what `vae_decode` hooks return here; a hook that
    returns PIL images or [0, 1] tensors is rejected): `postprocess(output_type="pil")`
    (`(x / 2 + 0.5).clamp(0, 1)`, `* 255`, round, uint8) followed by the img2img pipeline's `preprocess` (`/ 255`, `2 x - 1`)."""
    if not torch.is_tensor(image) or not image.is_floating_point():
        raise TypeError("to_8bit_image expects the decode hook's float tensor in [-1, 1]")
    q = ((image.float() / 2 + 0.5).clamp(0, 1) * 255.0).round()
    return (q / 255.0 * 2.0 - 1.0).to(image.dtype)


def resize_and_crop(img, size, crop_type="middle"):
    """Scale a PIL image so that it covers `size` = (width, height) and cut the excess along the longer relative side (reference
    pipeline.py:39-83). The scaled side is truncated to an int; crop_type "top" keeps the top / left part, "middle" the centre (the box is
    in floats and may have .5 edges, which PIL's `crop` rounds), "bottom" the bottom / right part. Same PIL calls as the reference: `resize`
    with its default resampling, `crop` with the float box. An unknown crop_type raises ValueError (the reference only notices it when
    the aspect ratios differ)."""
    if crop_type not in ("top", "middle", "bottom"):
        raise ValueError(f"invalid crop_type {crop_type!r}: 'top', 'middle' or 'bottom'")
    img_ratio = img.size[0] / float(img.size[1])
    ratio = size[0] / float(size[1])
    if ratio > img_ratio:                           # relatively taller than the target: fit the width, crop rows
        img = img.resize((size[0], int(size[0] * img.size[1] / img.size[0])))
        lo = {"top": 0, "middle": (img.size[1] - size[1]) / 2, "bottom": img.size[1] - size[1]}[crop_type]
        return img.crop((0, lo, img.size[0], lo + size[1]))
    if ratio < img_ratio:                           # relatively wider: fit the height, crop columns
        img = img.resize((int(size[1] * img.size[0] / img.size[1]), size[1]))
        lo = {"top": 0, "middle": (img.size[0] - size[0]) / 2, "bottom": img.size[0] - size[0]}[crop_type]
        return img.crop((lo, 0, lo + size[0], img.size[1]))
    return img.resize((int(size[0]), int(size[1])))


def loas_base_img(base_img_path, size: int = 1024):
    """reference pipeline.py:289-293 (name kept, typo included): open the file, `resize_and_crop` to size x size (middle), resize to size x size."""
    img = PIL.Image.open(base_img_path)
    img = resize_and_crop(img, (size, size), crop_type="middle")
    return img.resize((size, size))


def _need(c, keys, stage):
    missing = [k for k in keys if k not in c]
    if missing:
        raise KeyError(f"the conditioner returned no {missing} (needed by the {stage}; pass refinement=0 / subject_strength=0 to skip that stage)")


# ---- what `__call__` and `batch.edit_batch` share, request by request (functions of the pipeline object) -----------------------------------------------
EMBED_KEYS = ("prompt_embeds", "pooled_prompt_embeds", "negative_prompt_embeds", "negative_pooled_prompt_embeds")
REFINER_KEYS, SUBJECT_KEYS = tuple("refiner_" + k for k in EMBED_KEYS), tuple("subject_" + k for k in EMBED_KEYS)      # what `_need` asks of a conditioner per stage
# the prompts around the LLM's caption (reference :342-345, :358-361); the inpaint pass runs IPAdapterXL.generate without a prompt: its defaults (ip_adapter.py)
INVERSION_PROMPT, NEGATIVE_PROMPT = "", ""
CAPTION_PREFIX = SUBJECT_PROMPT = "best quality, high quality"
SUBJECT_NEGATIVE_PROMPT = "monochrome, lowres, bad anatomy, worst quality, low quality"
REFINER_CAPTION_SUFFIX = ",high quality,well-formed,award-winning"


def embeds(c, stage: str = "") -> dict:
    """the four text embeddings of a stage ("", "refiner_", "subject_") of a conditioning dict, under the keyword names every loop takes them by"""
    return {k: c[stage + k] for k in EMBED_KEYS}


def check_output_type(pipeline, output_type):
    if output_type not in OUTPUT_TYPES:
        raise ValueError(f"output_type must be one of {OUTPUT_TYPES}, got {output_type!r}")
    if output_type != "latent" and pipeline.vae is None:
        raise ValueError(f"output_type={output_type!r} needs the pipeline built with vae=<HipAutoencoderKL>")


def prior_y0(pipeline, c):
    """the conditioner's `y`, else the prior's one live call on the instruction embedding (reference :313-317)"""
    if c.get("y") is not None:
        return c["y"]
    if pipeline.model is None:
        raise NotImplementedError("the conditioner returned no `y` and no prior= was attached")
    ie = c["image_embeds"]
    y = pipeline.model.generate_diffusion(MODALITY.VIDEO, MODALITY.IMAGE, ie / ie.norm() * 100, device="cpu", no_diffusion=True,
                                          num_inference_steps=25, image_bind_overwrite=None, dtype=torch.float32, guidance_scale=10,
                                          force_guidence_t0=True, do_classifier_free_guidance=True, score=6.5)
    return y[0].to(device=c["base_embed"].device, dtype=c["base_embed"].dtype)


def base_image(pipeline, c, who: str = ""):
    """the base image of a conditioning dict that carries no `base_latents`, not yet encoded: its `base_image` (PIL), else its `base_img_path` loaded by
    `loas_base_img`; `who` names the request where several share a call"""
    img = c.get("base_image")
    if img is None and c.get("base_img_path") is not None:
        img = pipeline.loas_base_img(c["base_img_path"])
    if img is None:
        raise KeyError(f"the conditioner returned none of base_latents / base_image / base_img_path{who}")
    if pipeline.vae is None:
        raise ValueError("a base_image / base_img_path needs the pipeline built with vae=<HipAutoencoderKL>")
    return img


def check_control_from(pipeline, control_from, control_image):
    """the refusals of `control_from=` that need no device: together with `control_image`, without a ControlNet, an unknown kind or knob -> the `Condition`"""
    from .condition import resolve
    if control_image is not None:
        raise ValueError("control_from makes the condition map from the base image; control_image brings one: give one of the two")
    if pipeline.controlnet is None:
        raise ValueError("control_from needs the pipeline built with controlnet=<HipControlNetModel>")
    return resolve(control_from)


def refiner_handoff_by_image(pipeline) -> bool:
    """whether the base result reaches the refiner the reference's way (decode, 8-bit image, VAE re-encode with a posterior SAMPLE). Where that route was
    asked for but cannot be taken, say so once: the latent route has different numerics and draws nothing from the RNG"""
    vae_route = pipeline.refiner_handoff == "image" and pipeline.pipe._vae_decode is not None and pipeline.piperf._vae_encode is not None
    if pipeline.refiner_handoff == "image" and not vae_route and not pipeline._warned_handoff:
        import warnings
        warnings.warn("refiner_handoff='image' needs vae_decode= on the base pipeline and vae_encode= on the refiner pipeline; handing the "
                      "latents over directly instead (pass refiner_handoff='latent' to choose this route explicitly)", RuntimeWarning, stacklevel=3)
        pipeline._warned_handoff = True
    return vae_route


# ---- editing inside a mask: what `__call__` and `batch.edit_batch` share --------------------------------------------------------------
def check_edit_output_type(output_type):
    if output_type not in ("pil", "latent"):
        raise ValueError(f"an edit_mask composites in 8 bits: output_type must be \"pil\" or \"latent\", got {output_type!r} (a float composite is not built)")


def edit_mask_file_size(c):
    """(width, height) of the base image FILE where the request's base image is loaded from it (a mask of that size is then accepted too), else None"""
    if c.get("base_latents") is None and c.get("base_image") is None and c.get("base_img_path") is not None:
        with PIL.Image.open(c["base_img_path"]) as im:
            return im.size
    return None


def resolve_edit_mask(pipeline, mask, base_latents, file_size=None, pixels: bool = True):
    """-> (pixel mask uint8 [1, H, W] in {0, 255}, latent mask fp16 [1, 1, h, w] in {0, 1}), both on the UNet's device. `mask`: anything
    `image_processor.load_edit_mask` takes, at H x W = vae_scale_factor x the latent grid (or `file_size`); a latent cell is 1 if any of its pixels is in
    the mask (`ia2p_mask_to_latent`). A torch tensor [1, 1, h, w] is a latent mask already; its pixel mask is each cell repeated, and is only built when
    `pixels` asks for it (the loops need the latent mask alone: `denoise` and `denoise_batch` pass False, so a mask their caller resolved costs nothing more)."""
    from .image_processor import load_edit_mask, mask_to_latent
    dev, f = pipeline.pipe.unet.device, int(pipeline.pipe.vae_scale_factor)
    h, w = int(base_latents.shape[-2]), int(base_latents.shape[-1])
    if torch.is_tensor(mask):
        if tuple(mask.shape) != (1, 1, h, w):
            raise ValueError(f"a tensor edit_mask is a latent mask [1, 1, {h}, {w}], got {tuple(mask.shape)} (pixel masks: PIL, numpy or a file path, {f * h} x {f * w})")
        m = (mask.to(dev) != 0).to(torch.float16).contiguous()
        if not pixels:
            return None, m
        px = (m[0] * 255).to(torch.uint8).repeat_interleave(f, dim=-2).repeat_interleave(f, dim=-1).contiguous()
        return px, m
    px = torch.from_numpy(load_edit_mask(mask, f * h, f * w, file_size))[None].to(dev).contiguous()
    return px, mask_to_latent(px, f)


def intersect_subject_mask(mask, edit_px):
    """a subject mask ([H, W] / [1, H, W] / [B, 1, H, W] in [0, 1], uint8 0..255 or PIL) times the edit mask (uint8 [1, H', W'] in {0, 255}; resized NEAREST
    where the sizes differ), before `inpaint.prepare_mask`: a subject pass under an edit mask repaints inside both"""
    if isinstance(mask, PIL.Image.Image):
        import numpy as np
        mask = torch.from_numpy(np.asarray(mask.convert("L")).copy())
    m = torch.as_tensor(mask)
    m = m.float() / 255.0 if m.dtype == torch.uint8 else m.float()
    e = (edit_px.to(m.device).float() / 255.0)[None]
    if tuple(e.shape[-2:]) != tuple(m.shape[-2:]):
        e = torch.nn.functional.interpolate(e, size=tuple(m.shape[-2:]))
    return m * e.reshape((1,) * (m.ndim - 2) + tuple(e.shape[-2:]))


def composite_edit(pipeline, decoded, base_u8, alpha):
    """decoded image fp16 [1, 3, H, W] in [-1, 1] -> the list of PIL images `postprocess(output_type="pil")` gives, composited in 8 bits with the base image
    through the feathered mask: every pixel outside the user's mask carries the base image's byte"""
    from .image_processor import image_composite, image_to_u8
    u8 = image_to_u8(decoded.to(device=base_u8.device, dtype=torch.float16).contiguous())
    u8 = image_composite(u8, base_u8, alpha, out=u8).cpu().numpy()
    return [PIL.Image.fromarray(a[..., 0] if a.shape[-1] == 1 else a) for a in u8]


def condition_from_llm_output(out, mm_data) -> dict:
    """`forward_llm`'s five-tuple -> the LLM's part of the conditioning dict a `conditioner=` would return; without an `<im_gen>` only the caption counts.
    `base_image`: the PIL image an mm_data entry carries for the base image's file; `subject_data`: the subjects that are image entries (:363-366)"""
    image_embeds, base_embed, caption, base_img_path, extra_data = out
    c = dict(image_embeds=image_embeds, base_embed=base_embed, caption=caption, base_img_path=base_img_path, extra_data=extra_data)
    if image_embeds is None:
        return c
    c["image_embeds"], c["base_embed"] = image_embeds.reshape(1, -1), base_embed.reshape(1, -1)      # host fp32, as the reference holds them (:236, :253)
    for e in mm_data:
        if e.get("fname") == base_img_path and e.get("image") is not None:
            c["base_image"] = e["image"]
    if extra_data is not None and len(extra_data.get("extra_idx", [])) > 0:
        c["subject_data"] = [(k, v) for (k, v, i) in zip(extra_data["all_objs"], extra_data["extra_embeds"], extra_data["extra_idx"])
                             if mm_data[int(i)]["type"] == "image"]
    return c


def fuse_instruction_embedding(base_embed, image_embeds, y0, h, norm):
    """reference pipeline.py:322-324"""
    latent_la = base_embed * h[0] + image_embeds * h[1] + y0 / y0.norm() * 20.0 * h[2]
    latent_la = latent_la.detach().clone()
    return latent_la / latent_la.norm() * norm


class InstructAny2PixPipeline:
    def __init__(self, ckpt: str = "ckpts", llm_folder: str = "llm-retrained", *, unet: Optional[HipUNet2DConditionModel] = None,
                 unet_config: Optional[UNetConfig] = None, unet_state_dict=None, ip_ckpt=None, device: str = "cuda:0",
                 conditioner: Optional[Callable] = None, text_encoder: Optional[Callable] = None,
                 vae_encode: Optional[Callable] = None, vae_decode: Optional[Callable] = None, clip_embeddings_dim: int = 1024,
                 refiner_unet: Optional[HipUNet2DConditionModel] = None, refiner_text_encoder: Optional[Callable] = None, prior=None,
                 refiner_handoff: str = "image", vae=None, llm=None, llm_tokenizer: Optional[Callable] = None,
                 modality_encoder: Optional[Callable] = None, imagebind=None, segmenter=None, detector: Optional[Callable] = None, controlnet=None):
        # llm: a HipInstructAny2PixLM (reference :117 `self.any2pix_lm`; built with `load_in_4bit=True` it computes from 4-bit weights as the
        # reference's `from_pretrained(..., load_in_4bit=True)` model does, nothing changes here) with its tokenizer (:126 `self.any2pix_tokenizer`, injected: the
        # sentencepiece model is checkpoint data); modality_encoder(entry) -> [1024] embedding of an mm_data entry (reference :155-166:
        # ImageBind; an entry may carry its vector directly as entry["embed"]); imagebind: a HipImageBindModel (reference :118-121 `self.model_imb`) that
        # encodes the entries' files itself when neither of the two is given
        self.any2pix_lm, self.any2pix_tokenizer, self.modality_encoder = llm, llm_tokenizer, modality_encoder
        # the checkpoint's own generation_config.json (reference :28 `from_pretrained(f"{ckpt}/{llm_folder}")` reads it; `generate` then starts from its top_k /
        # top_p): loaded into the LLM's `generation_defaults` when the folder holds one. forward_llm passes neither keyword, so they come from there.
        gen_cfg = os.path.join(str(ckpt), str(llm_folder), "generation_config.json")
        if llm is not None and hasattr(llm, "load_generation_config") and os.path.isfile(gen_cfg):
            llm.load_generation_config(gen_cfg)
        self.model_imb = imagebind
        # segmenter: a sam.HipSamPredictor (reference :147 `self.sam`); detector(image uint8 [H, W, 3], text_prompt) -> (boxes cxcywh in [0, 1] [n, 4], phrases): stands in
        # for GroundingDINO (:148 `self.gdino`, not built here). Both serve subjects the conditioner names by phrase: subject_data = [(phrase, embedding)]
        self.sam, self.gdino = segmenter, detector
        self._text_encoder, self._refiner_text_encoder = text_encoder, refiner_text_encoder
        # vae: a HipAutoencoderKL shared by every pipeline (in place of the vae_encode / vae_decode hooks): base images in, images out
        # how the base result reaches the refiner: "image" = the reference's route (decode, 8-bit image, VAE re-encode with a posterior
        # sample; needs vae_encode and vae_decode), "latent" = the sampled latents go in directly (no VAE round trip; the only route
        # when no VAE is attached)
        if refiner_handoff not in ("image", "latent"):
            raise ValueError("refiner_handoff must be 'image' or 'latent'")
        self.refiner_handoff = refiner_handoff
        self._warned_handoff = False
        # the embedding prior (reference :97-98,:120-122 `self.model`): prior.py::InstructAny2PixPrior on the HIP kernels, or None when
        # the conditioner supplies `y` itself
        self.model = prior
        if unet is None:
            unet = HipUNet2DConditionModel(unet_config or sdxl_base(), device)
            if unet_state_dict is not None:
                unet.load_state_dict(unet_state_dict)
        self.unet = unet
        new_sch = DDIMScheduler()
        # one shared UNet object for sampling and inversion (reference :106-116)
        self.vae = vae
        # controlnet: a HipControlNetModel (new: the reference attaches none). The guided sampling stage then takes `control_image=`; without one, or with the
        # control off, the stage is the plain pipeline's call
        self.controlnet = controlnet
        if controlnet is not None:
            self.pipe = StableDiffusionXLControlNetPipeline(unet, controlnet, DDIMScheduler(), encode_prompt=text_encoder, vae_decode=vae_decode, vae=vae)
        else:
            self.pipe = StableDiffusionXLPipeline(unet, DDIMScheduler(), encode_prompt=text_encoder, vae_decode=vae_decode, vae=vae)
        self.pipe_inversion = SDXLDDIMPipeline(unet, new_sch, encode_prompt=text_encoder, vae_encode=vae_encode, vae=vae)
        # the refiner pipeline object (:128-131): second UNet config of the same engine, Euler img2img loop (img2img.py)
        self.piperf = StableDiffusionXLImg2ImgPipeline(refiner_unet, encode_prompt=refiner_text_encoder, vae_encode=vae_encode,
                                                       vae_decode=vae_decode, vae=vae) if refiner_unet is not None else None
        # inpainting pipeline assembled from the base pipeline's own modules: same UNet object, same scheduler object (:132-139)
        self.pipe_inpainting = StableDiffusionXLInpaintPipeline(unet, self.pipe.scheduler, encode_prompt=text_encoder, vae_encode=vae_encode,
                                                                vae_decode=vae_decode, vae=vae)
        self.conditioner = conditioner           # stands in for forward_llm + prior (:309-317)
        self.cache = None
        self.mode = "ipa_v2"
        self.ip_adapter_xl = IPAdapterXL(self.pipe, "", ip_ckpt=ip_ckpt, device=device, clip_embeddings_dim=clip_embeddings_dim) if ip_ckpt is not None else None
        # second adapter object over the same UNet (:143-146): it re-installs the same processors and weights
        self.ip_adapter_xl_inpaint = IPAdapterXL(self.pipe_inpainting, "", ip_ckpt=ip_ckpt, device=device,
                                                 clip_embeddings_dim=clip_embeddings_dim) if ip_ckpt is not None else None

    # ---- LoRA adapters on the UNets (lora.py) ----------------------------------------------------------
    def _lora_unets(self, target=None):
        both = {"unet": self.unet, "refiner": self.piperf.unet if self.piperf is not None else None}
        if target is None:
            return [u for u in both.values() if u is not None]
        if target not in both:
            raise ValueError("target must be 'unet' or 'refiner'")
        if both[target] is None:
            raise ValueError("this pipeline has no refiner UNet")
        return [both[target]]

    def load_lora_weights(self, path_or_dict, adapter_name: str = "default", target: str = "unet", text_encoder_keys: str = "error"):
        """Load a LoRA adapter (`.safetensors` path or state dict; spellings: `lora.parse_lora_state_dict`) into the base UNet (`target="unet"`) or the
        refiner's and activate it at weight 1 beside the adapters already active there, as diffusers' `load_lora_weights` does. Text-encoder keys are
        refused (`"error"`) or dropped (`"skip"`): adapters are applied to the UNets only. In a multi-rank run every rank loads the adapter itself."""
        (u,) = self._lora_unets(target)
        u.load_lora_adapter(path_or_dict, adapter_name, text_encoder_keys=text_encoder_keys)
        act = u.lora.active
        u.set_adapters(list(act) + [adapter_name], list(act.values()) + [1.0])

    def set_adapters(self, names, weights=1.0, target: str = "unet"):
        self._lora_unets(target)[0].set_adapters(names, weights)

    def disable_lora(self):
        for u in self._lora_unets():
            u.disable_lora()

    def enable_lora(self):
        for u in self._lora_unets():
            u.enable_lora()

    def delete_adapters(self, names, target: str = "unet"):
        self._lora_unets(target)[0].delete_adapters(names)

    def unload_lora_weights(self):
        for u in self._lora_unets():
            u.unload_lora()

    def get_active_adapters(self, target: str = "unet"):
        return [n for n, _ in self._lora_unets(target)[0].active_adapters()]

    @contextlib.contextmanager
    def lora_scaled(self, lora_scale):
        """Inside the block the active adapter weights of both UNets are multiplied by `lora_scale`; the state before comes back afterwards, also when the
        block raises. None: no launch, no bit."""
        if lora_scale is None:
            yield
            return
        with contextlib.ExitStack() as st:
            for u in self._lora_unets():
                if u._lora is not None:
                    st.enter_context(u._lora.scaled(lora_scale))
            yield

    # ---- the hot segment on explicit conditioning ------------------------------------------------------------------
    @torch.no_grad()
    def denoise(self, base_latents, latent_la, *, prompt_embeds, pooled_prompt_embeds, negative_prompt_embeds, negative_pooled_prompt_embeds,
                inv_prompt_embeds=None, inv_pooled_prompt_embeds=None, alpha=0.7, num_inference_steps=25, cfg=10, scale=1.0, noise=None, seed=None,
                edit_mask=None, auto_mask=None, sampler=None, sample_steps=None, step_noise=None, sample_adapters=None,
                control_image=None, control_scale=1.0, control_start=0.0, control_end=1.0, control_from=None, control_base=None):
        """inversion -> polar mixing -> IP-Adapter guided sampling; returns (sampled latents, inverted latents).
        `control_from` (None: nothing changes, no launch, no allocation and no bit): "canny", "blur", "grey", a dict such as {"kind": "canny", "low": 50, "high": 150,
        "blur_sigma": 1.4} or a `condition.Condition` -- the condition map is made on the device (condition.py) from `control_base`, the base image's
        8-bit pixels at 8 x the latent grid (a uint8 tensor / array [H, W, 3], a PIL image or a path), and passed on exactly as a `control_image` would be. This
        call gets latents: without `control_base` the base image is not available as 8-bit pixels and the call raises. Together with `control_image`: ValueError.
        `control_image` (None: nothing changes, no launch and no bit; needs the pipeline built with controlnet=): the structure that must survive the edit -- a
        condition map the caller brings (edges, depth, pose, a sketch), a PIL image, a uint8 / float array or a path, resized and cropped like the base image to
        8 x the latent grid, values in [0, 1]. It guides the guided sampling stage only, at `control_scale` over the fraction [`control_start`, `control_end`] of
        its steps (diffusers' `controlnet_conditioning_scale`, `control_guidance_start` / `_end`); a scale of 0 or a window that holds no step is the plain call.
        The inversion, the automatic mask's evaluations, the refiner and the subject passes run without control.
        `sampler` ("ddim", "lcm"; None: what `self.pipe.scheduler` is -- DDIM, or LCM once an `LCMScheduler` is assigned there; with None nothing changes, no
        launch and no draw) and `sample_steps` (the length of the LCM schedule, default 4, 1 .. 50; refused under DDIM): the guided sampling stage runs the
        few-step consistency sampler for the length of the `generate` call -- the scheduler is swapped and put back, also when the call raises.
        `num_inference_steps` keeps governing the inversion; inversion and mixing are untouched. The noise re-injected after every step but the last:
        `step_noise` (fp16 [sample_steps - 1, 4, h, w]), else draw DRAW_LCM of `seed` made inside the update launch, else fp16 draws from the global CPU
        generator right after the polar-mixing draw, in step order. `cfg <= 1` evaluates the conditional rows only. Under an edit mask the base latents,
        re-noised with the step's own noise, replace every step's result outside the mask; the inversion records no trajectory.
        `sample_adapters` (a name, a list or (names, weights); None: nothing happens): LoRA adapters active around the guided sampling loop only
        (`LoraManager.using`), so that the inversion and the mask estimate run on the weights the caller left active.
        `auto_mask` (None: nothing changes, no launch and no draw): True, a dict or an `auto_mask.AutoMask` -- the edit mask is estimated from the request itself
        before the inversion (`estimate_edit_mask`) and, where `edit_mask` is given too, multiplied by its latent mask; the rest is the `edit_mask` path.
        `edit_mask` (None: nothing changes): edit inside the mask only (`resolve_edit_mask`: a pixel mask at vae_scale_factor x the latent grid, or a latent
        mask tensor [1, 1, h, w]). The inversion records its trajectory, the sampling start and every sampling step are replaced outside the mask by the
        inverted latents of the same noise level, and the sampled latents equal `base_latents` (as the loop holds them in fp16) wherever the latent mask is 0.
        `seed` (None: the draw below, as ever): the mixing noise is draw DRAW_POLAR of the request's own Philox stream (noise.py), made and mixed on the device
        (`noise.randn_seeded`, `noise.polar_mix`): the inverted latents never leave it -- no `.cpu()`, no host `randn`, no CPU mix, no upload. Row b of a
        batch of base latents draws from seed + b. A supplied `noise` wins over the seed. The device mix is fp32 arithmetic rounded once; it is not bit-equal
        to the CPU fp16 mix of the unseeded path."""
        from .batch import resolve_sample_adapters
        smp, n_lcm = resolve_sampler(self.pipe.scheduler, sampler, sample_steps)
        if step_noise is not None:
            if smp != "lcm":
                raise ValueError("`step_noise` is the noise of the LCM sampler; this call samples with DDIM")
            check_step_noise(step_noise, n_lcm, base_latents.shape)
        sample_adapters = resolve_sample_adapters(self.pipe.unet, sample_adapters)
        self.pipe_inversion.unet = self.pipe.unet                                              # :306
        self.pipe_inversion.scheduler = DDIMScheduler.from_config(self.pipe.scheduler.config)  # :307
        if inv_prompt_embeds is None:        # reference inverts with prompt='' (:330); callers pass its embedding
            inv_prompt_embeds, inv_pooled_prompt_embeds = negative_prompt_embeds, negative_pooled_prompt_embeds
        masked, control = {}, {}
        if control_from is not None:
            control_image = self.control_map(check_control_from(self, control_from, control_image), control_base, base_latents)
        if control_image is not None:
            if self.controlnet is None:
                raise ValueError("control_image needs the pipeline built with controlnet=<HipControlNetModel>")
            control.update(image=self.control_tensor(control_image, base_latents), controlnet_conditioning_scale=float(control_scale),
                          control_guidance_start=float(control_start), control_guidance_end=float(control_end))
        if edit_mask is not None:
            masked["edit_mask"] = resolve_edit_mask(self, edit_mask, base_latents, pixels=False)[1]
        if auto_mask is not None:
            from .auto_mask import intersect
            est = self.estimate_edit_mask(base_latents, latent_la, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                                          inv_prompt_embeds=inv_prompt_embeds, inv_pooled_prompt_embeds=inv_pooled_prompt_embeds,
                                          num_inference_steps=num_inference_steps, scale=scale, seed=seed, auto_mask=auto_mask)[0]
            masked["edit_mask"] = intersect(est, masked.get("edit_mask"))
        inverted =self.pipe_inversion.inverse(num_inference_steps=num_inference_steps, latents=base_latents, prompt_embeds=inv_prompt_embeds,
                                               pooled_prompt_embeds=inv_pooled_prompt_embeds, **({"return_trajectory": True} if masked and smp == "ddim" else {}))
        latent_inv = inverted.images
        if masked and smp == "ddim":
            masked["known_trajectory"] = inverted.trajectory
        elif masked:
            masked["known_latents"] = base_latents
        if noise is None and seed is not None:
            z = _noise.randn_seeded(_noise.batch_seeds(seed, latent_inv.shape[0]), _noise.DRAW_POLAR, latent_inv.shape[1:], torch.float16, latent_inv.device)
            mixed = _noise.polar_mix(latent_inv, z, float(alpha))
        else:
            latent_inv_cpu = latent_inv.cpu()                                                  # :331
            if noise is None:
                noise = torch.randn_like(latent_inv_cpu)                                       # :335 global RNG, CPU, fp16
            mixed = polar_intrtpolate(latent_inv_cpu, noise, alpha)                            # :333-337
        saved = self.pipe.scheduler
        if smp == "lcm":
            masked.update({} if step_noise is None else {"step_noise": step_noise}, **({} if seed is None or step_noise is not None else {"noise_seed": seed}))
            num_inference_steps = n_lcm
        try:
            if (smp == "lcm") != isinstance(saved, LCMScheduler):                              # the sampler asked for, for the length of this call
                self.pipe.scheduler = (LCMScheduler if smp == "lcm" else DDIMScheduler).from_config(saved.config)
            with (contextlib.nullcontext() if sample_adapters is None else self.pipe.unet.lora.using(*sample_adapters)):
                images = self.ip_adapter_xl.generate(pil_image=None, num_samples=1, clip_image_embeds=latent_la, num_inference_steps=num_inference_steps,
                                                     scale=scale, mode="global", guidance_scale=cfg, latents=mixed,
                                                     prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                                                     pooled_prompt_embeds=pooled_prompt_embeds, negative_pooled_prompt_embeds=negative_pooled_prompt_embeds,
                                                     output_type="latent", **masked, **control)
        finally:
            self.pipe.scheduler = saved
        return images, latent_inv

    def control_tensor(self, control_image, base_latents):
        """a condition map -> fp16 [1, 3, 8 h, 8 w] in [0, 1] on the device: a path or PIL image goes through the base image's resize-and-crop and the 8-bit upload
        (`ia2p_image_from_u8` without normalisation); a uint8 array [H, W, 3] likewise without the resize; float arrays / tensors ([3, H, W] or [1, 3, H, W], in [0, 1])
        are taken as they are. The size must be 8 x the latent grid."""
        from .image_processor import image_from_u8
        H, W = 8 * base_latents.shape[-2], 8 * base_latents.shape[-1]
        dev = self.pipe.unet.device
        if isinstance(control_image, (str, os.PathLike)):
            control_image = PIL.Image.open(control_image)
        if isinstance(control_image, PIL.Image.Image):
            control_image = np.asarray(resize_and_crop(control_image.convert("RGB"), (W, H), crop_type="middle").resize((W, H)))
        if isinstance(control_image, np.ndarray) and control_image.dtype == np.uint8:
            if control_image.ndim != 3 or control_image.shape[2] != 3:
                raise ValueError(f"a uint8 control image is [H, W, 3]; got {control_image.shape}")
            t = image_from_u8(torch.from_numpy(np.ascontiguousarray(control_image))[None].to(dev), normalize=False)
        elif torch.is_tensor(control_image) and control_image.dtype == torch.uint8:      # a map made on the device (`control_map`): one or three channels
            from .condition import to_condition
            t = to_condition(control_image.to(dev))
        else:
            t = torch.as_tensor(control_image)
            if not t.is_floating_point():
                raise ValueError("control_image: a path, a PIL image, a uint8 array [H, W, 3] or a float map in [0, 1]")
            t = (t[None] if t.ndim == 3 else t).to(device=dev, dtype=torch.float16)
        if t.ndim != 4 or tuple(t.shape[1:]) != (3, H, W):
            raise ValueError(f"the control image must be 3 x {H} x {W} (8 x the latent grid {base_latents.shape[-2]} x {base_latents.shape[-1]}); got {tuple(t.shape)}")
        return t.contiguous()

    def base_pixels(self, base_image):
        """a base image (a path: through `loas_base_img`; a PIL image; a uint8 array [H, W, 3]) -> uint8 [1, H, W, 3] on the device, as the pipeline holds it: the
        host half of the inversion pipeline's `preprocess` (its resize to multiples of the VAE's scale factor) -- the bytes the VAE encode is fed. A uint8 tensor
        ([H, W, 3] or [1, H, W, 3]) is taken as it is."""
        from .condition import as_u8
        if torch.is_tensor(base_image):
            return as_u8(base_image, self.pipe.unet.device)[0]
        if isinstance(base_image, (str, os.PathLike)):
            base_image = self.loas_base_img(base_image)
        if isinstance(base_image, np.ndarray) and base_image.dtype == np.uint8 and base_image.ndim == 3:
            base_image = PIL.Image.fromarray(base_image)
        if not isinstance(base_image, PIL.Image.Image):
            raise ValueError("the base image of a condition map is a path, a PIL image, a uint8 array [H, W, 3] or a uint8 tensor")
        proc = self.pipe_inversion.image_processor
        if proc is None:
            from .image_processor import VaeImageProcessor
            proc = VaeImageProcessor(vae_scale_factor=8, device=self.pipe.unet.device)
        return as_u8(proc.pil_to_u8([base_image])[0], self.pipe.unet.device)[0]

    def control_map(self, cond, control_base, base_latents=None):
        """the condition map `cond` asks for (condition.py) of the base image's 8-bit pixels -> uint8 [1, H, W] or [1, H, W, 3] on the device. `control_base` None:
        the base image is not available as 8-bit pixels (the caller brought latents), which is refused; a size other than 8 x the latent grid is refused too."""
        from . import condition
        if control_base is None:
            raise ValueError("control_from makes the condition map from the base image's 8-bit pixels, and this request brings base latents only: give the base "
                             "image (base_image / base_img_path from the conditioner; `control_base=` on denoise), or bring the map as control_image=")
        px = self.base_pixels(control_base)
        if px.shape[0] != 1 or px.shape[-1] != 3:
            raise ValueError(f"control_from: the base image must be one RGB image, got {tuple(px.shape)}")
        if base_latents is not None and tuple(px.shape[1:3]) != (8 * base_latents.shape[-2], 8 * base_latents.shape[-1]):
            raise ValueError(f"control_from: the base image is {px.shape[1]} x {px.shape[2]}, not 8 x the latent grid {base_latents.shape[-2]} x {base_latents.shape[-1]}")
        return condition.make(cond, px)

    def make_control_image(self, kind, base_image=None):
        """The condition map `control_from=kind` would make, as a PIL image ("L" for canny and grey, "RGB" for blur), for a caller who wants to look at it or edit
        it and pass it back as `control_image=`. `base_image`: a path (loaded by `loas_base_img`), a PIL image or a uint8 array; None: the base image of the last
        request a `conditioner=` served (`self.cache`)."""
        from . import condition
        cond = condition.resolve(kind)
        if base_image is None:
            c = self.cache if isinstance(self.cache, dict) else {}
            base_image = c.get("base_image") if c.get("base_image") is not None else c.get("base_img_path")
            if base_image is None:
                raise ValueError("make_control_image: no base image is held (the last request brought none): pass base_image=")
        m = self.control_map(cond, base_image)[0].cpu().numpy()
        return PIL.Image.fromarray(m)

    def estimate_edit_mask(self, base_latents, latent_la, **kw):
        """The automatic edit mask of one request on explicit conditioning, for a caller who wants to look at it (or change it) before `denoise(edit_mask=)`:
        -> (latent mask fp16 [1, 1, h, w] in {0, 1}, contrast map fp32 [1, h, w], stats fp32 [2] = (mean, tau)), on the device. Keywords: the embeddings `denoise`
        takes, `num_inference_steps`, `scale`, `seed`, `auto_mask` (`auto_mask.estimate_edit_mask`)."""
        from .auto_mask import estimate_edit_mask
        self.pipe_inversion.unet = self.pipe.unet
        return estimate_edit_mask(self, base_latents, latent_la, **kw)

    # ---- N independent requests as one batch per evaluation, sharded over the ranks (batch.py) ---------------------------------------------------
    def denoise_batch(self, requests, group: int = 4, shard: bool = True, sample_adapters=None):
        """`denoise` for a list of `batch.EditRequest`s with their own `num_inference_steps` / `cfg` / `scale` / `alpha`: grouped `group` at a time
        (B_eff = 2 x group in the guided loop), contiguous shards per rank when a process group is up, results all-gathered in request order.
        -> (sampled latents [N,4,h,w], inverted latents [N,4,h,w])."""
        from .batch import denoise_batch
        self.pipe_inversion.unet = self.pipe.unet
        return denoise_batch(self, requests, group=group, shard=shard, **({} if sample_adapters is None else {"sample_adapters": sample_adapters}))

    # ---- base image -> latents (reference :289-293, :328-330) -------------------------------------------------------------
    base_image_size = 1024          # the square `loas_base_img` loads a base_img_path to

    def loas_base_img(self, base_img_path):
        return loas_base_img(base_img_path, self.base_image_size)

    def _base_latents(self, c, seed=None, keep=None):
        """the conditioner's `base_latents`, else its `base_image` (PIL) or `base_img_path` (loaded by `loas_base_img`) through the inversion
        pipeline's image processor and the VAE (a posterior sample, as in the reference's `inverse(image=...)`; with `seed`, draw DRAW_BASE_POSTERIOR of it).
        `keep` (a dict; an edit inside a mask composites with the base image): receives the preprocessed image as keep["image"] (`_image_latents(keep=)`)."""
        if c.get("base_latents") is not None:
            return c["base_latents"]
        img = base_image(self, c)
        kw = {} if keep is None else {"keep": keep}
        if seed is not None:
            kw.update(seeds=[_noise.check_seed(seed)], draw=_noise.DRAW_BASE_POSTERIOR)
        return self.pipe_inversion._image_latents(img, **kw)

    # ---- the instruction LLM (reference :151-279) ---------------------------------------------------------------------------
    def _modality_embeds(self, mm_data):
        """:154-168: one 1024-d vector per mm_data entry, normalised to norm 20 (host fp32, as the reference's CPU ImageBind run leaves them)"""
        all_tensors, files = [None] * len(mm_data), {}
        for i, r in enumerate(mm_data):
            if r.get("embed") is not None:
                all_tensors[i] = torch.as_tensor(r["embed"])
            elif self.modality_encoder is not None:
                all_tensors[i] = self.modality_encoder(r)
            elif self.model_imb is not None:
                files.setdefault(r["type"], []).append(i)      # the entries of one type go through their tower as one batch
            else:
                raise ValueError("an mm_data entry needs entry['embed'] or the pipeline built with modality_encoder=")
        for kind, idx in files.items():
            from .imagebind import encode_mm_entries
            for i, row in zip(idx, encode_mm_entries(self.model_imb, kind, [mm_data[i]["fname"] for i in idx])):
                all_tensors[i] = row
        all_tensors = [t.detach().float().cpu().reshape(1, -1) for t in all_tensors]
        if not all_tensors:
            raise ValueError("forward_llm needs at least one mm_data entry (the reference's torch.cat of none fails the same way)")
        aux_info = torch.cat(all_tensors)
        return aux_info / (aux_info.norm(dim=-1, keepdim=True) + 1e-9) * 20

    def _llm_special_ids(self):
        tok = self.any2pix_tokenizer
        return {k: tok(k, add_special_tokens=False).input_ids[0] for k in ("<video>", "<base>", "<base_null>", "<im_gen>")}

    def _llm_request(self, inst, aux_info):
        """:171-200: -> (input_ids, extra_replacement, stopping criterion) of one request"""
        from .llm import KeywordsStoppingCriteria, REPLACEMENT_TYPE, VICUNA_V1_SEP2, vicuna_v1_prompt
        extra_replacement = {"data": aux_info, "mask": torch.tensor([REPLACEMENT_TYPE.INPUT] * aux_info.shape[0], dtype=torch.long)}
        prompt = vicuna_v1_prompt(inst)
        input_ids = self.any2pix_tokenizer(prompt, return_tensors="pt").input_ids
        stopping_criteria = KeywordsStoppingCriteria([VICUNA_V1_SEP2], self.any2pix_tokenizer, input_ids)
        lm = self.any2pix_lm
        if lm.DEFAULT_VIDEO_TOKEN_IDX is None:
            lm.DEFAULT_VIDEO_TOKEN_IDX = self._llm_special_ids()["<video>"]
        lm.eval()
        return input_ids, extra_replacement, stopping_criteria

    def _llm_seed_kw(self, key, value):
        """{key: value} where the LLM draws its tokens on the device (its Philox stream is keyed by the request's seed); {} under the host sampler, which
        keeps torch's global generator whatever the request's seed"""
        return {key: value} if value is not None and getattr(self.any2pix_lm, "sampler", "host") == "device" else {}

    def _llm_generate(self, inst, aux_info, seed=None):
        """:171-211: prompt, stopping criterion and the one `generate` call -> (input_ids, generate output). Where the token is drawn (host or
        device) is the LLM's own setting, `HipInstructAny2PixLM(sampler=...)`; `_llm_generate_batch` likewise. `seed`: the request's seed, which keys
        the token stream under the device sampler (and is ignored under the host sampler)."""
        input_ids, extra_replacement, stopping_criteria = self._llm_request(inst, aux_info)
        lm = self.any2pix_lm
        out = lm.generate(input_ids, images=None, do_sample=True, temperature=0.3, max_new_tokens=100, output_hidden_states=True, use_cache=False,
                          return_dict_in_generate=True, extra_replacement=extra_replacement, stopping_criteria=[stopping_criteria],
                          **self._llm_seed_kw("seed", seed))
        return input_ids, out

    def forward_llm(self, inst, mm_data=[], use_cache=False, seed=None):
        """-> (image_embeds, base_embed, output_caption, base_img_path, extra_data); (None, None, text, None, None) without an `<im_gen>`"""
        if use_cache:
            return self.cache
        if self.any2pix_lm is None or self.any2pix_tokenizer is None:
            raise NotImplementedError("forward_llm needs the pipeline built with llm=<HipInstructAny2PixLM> and llm_tokenizer=")
        from .llm import parse_generation
        aux_info = self._modality_embeds(mm_data)
        input_ids, out = self._llm_generate(inst, aux_info) if seed is None else self._llm_generate(inst, aux_info, seed=seed)
        ids = self._llm_special_ids()
        tp = self.any2pix_tokenizer.batch_decode(out.sequences)
        return parse_generation(out.sequences, input_ids.shape[1], out.hidden_states, tp[0], aux_info, mm_data,
                                self.any2pix_lm.get_model().vae_predictor_image, ids["<video>"], ids["<base>"], ids["<im_gen>"])

    def _llm_generate_batch(self, requests, seeds=None):
        """the one `generate_batch` call for [(input_ids, extra_replacement, stopping criterion), ...] -> list of generate outputs. `seeds` (one per request,
        all given): the requests' token streams under the device sampler."""
        return self.any2pix_lm.generate_batch([r[0] for r in requests], extra_replacements=[r[1] for r in requests], do_sample=True, temperature=0.3,
                                              max_new_tokens=100, stopping_criteria=[[r[2]] for r in requests], **self._llm_seed_kw("seeds", seeds))

    def forward_llm_batch(self, insts, mm_datas, seeds=None):
        """`forward_llm` for several requests, their decode steps sharing every read of the LLM's weights (`HipInstructAny2PixLM.generate_batch`):
        -> a list of the five-tuples `forward_llm` returns, in request order. More requests than the LLM's `max_batch` run in consecutive groups.
        The sampled tokens are reproducible for a seed but are not those of serial `forward_llm` calls (the draws of a step interleave across the
        requests). `self.cache` is not touched. `seeds` (one per request; an entry None gets a fresh one from the global generator): under the LLM's device sampler
        request i draws its tokens from its own stream, the same alone and in any batch; the host sampler ignores them."""
        insts, mm_datas = list(insts), list(mm_datas)
        if len(insts) != len(mm_datas):
            raise ValueError(f"{len(insts)} instructions for {len(mm_datas)} mm_data lists")
        if self.any2pix_lm is None or self.any2pix_tokenizer is None:
            raise NotImplementedError("forward_llm_batch needs the pipeline built with llm=<HipInstructAny2PixLM> and llm_tokenizer=")
        if len(insts) > 1 and getattr(self.any2pix_lm, "max_batch", 1) == 1:
            raise ValueError(f"{len(insts)} requests for an LLM built with max_batch=1: build it with max_batch > 1, or call forward_llm per request")
        if not insts:
            return []
        from .llm import parse_generation
        aux = [self._modality_embeds(mm) for mm in mm_datas]
        requests = [self._llm_request(inst, a) for inst, a in zip(insts, aux)]
        if seeds is not None and any(s is not None for s in seeds):
            fresh = iter(_noise.seeds_from_global(sum(s is None for s in seeds)))
            outs = self._llm_generate_batch(requests, seeds=[next(fresh) if s is None else s for s in seeds])
        else:
            outs = self._llm_generate_batch(requests)
        ids = self._llm_special_ids()
        results = []
        for (input_ids, _, _), out, a, mm in zip(requests, outs, aux, mm_datas):
            tp = self.any2pix_tokenizer.batch_decode(out.sequences)
            results.append(parse_generation(out.sequences, input_ids.shape[1], out.hidden_states, tp[0], a, mm,
                                            self.any2pix_lm.get_model().vae_predictor_image, ids["<video>"], ids["<base>"], ids["<im_gen>"]))
        return results

    def _condition_from_llm(self, inst, mm_data, use_cache, llm_only, seed=None):
        """the conditioning dict a `conditioner=` would return, from forward_llm + the attached text encoders (:309-310, :330, :342-345, :358-361)"""
        self.cache = self.forward_llm(inst, mm_data, use_cache=use_cache, **({} if seed is None else {"seed": seed}))
        c = condition_from_llm_output(self.cache, mm_data)
        if llm_only:
            return c
        if c["image_embeds"] is None:
            raise RuntimeError(f"the LLM produced no <im_gen>: {c['caption']!r}")
        if self._text_encoder is None:
            raise ValueError("a pipeline built with llm= needs text_encoder=<encode_prompt callable> for the denoise stages")
        pe, ne, pp, npl = self._text_encoder(prompt=CAPTION_PREFIX + c["caption"], negative_prompt=NEGATIVE_PROMPT, do_classifier_free_guidance=True)
        ipe, _, ipp, _ = self._text_encoder(prompt=INVERSION_PROMPT, do_classifier_free_guidance=False)
        c.update(prompt_embeds=pe, pooled_prompt_embeds=pp, negative_prompt_embeds=ne, negative_pooled_prompt_embeds=npl,
                 inv_prompt_embeds=ipe, inv_pooled_prompt_embeds=ipp)
        if "subject_data" in c:
            spe, sne, spp, snp = self._text_encoder(prompt=SUBJECT_PROMPT, negative_prompt=SUBJECT_NEGATIVE_PROMPT, do_classifier_free_guidance=True)
            c.update(subject_prompt_embeds=spe, subject_pooled_prompt_embeds=spp, subject_negative_prompt_embeds=sne, subject_negative_pooled_prompt_embeds=snp)
        if self._refiner_text_encoder is not None:
            rpe, rne, rpp, rnp = self._refiner_text_encoder(prompt=c["caption"] + REFINER_CAPTION_SUFFIX, negative_prompt=NEGATIVE_PROMPT,
                                                            do_classifier_free_guidance=True)
            c.update(refiner_prompt_embeds=rpe, refiner_pooled_prompt_embeds=rpp, refiner_negative_prompt_embeds=rne,
                     refiner_negative_pooled_prompt_embeds=rnp)
        return c

    def _subjects_from_phrases(self, c, subject_data, latents, subject_strength, kw):
        """the subject-consistency pass for subjects named by phrase: boxes from c["subject_boxes"] = (boxes, phrases) or from the detector on the decoded
        result (prompt: the phrases joined by '. ', gdino/lib.py:70), masks from the segmenter"""
        boxes, phrases = self._subject_boxes(c, subject_data, latents)
        out, self.subject_masks = subject_consistency_from_boxes(subject_data, latents, self.ip_adapter_xl_inpaint, self.sam, boxes, phrases, self.vae,
                                                                 subject_strength, **kw)
        return out

    def _subject_boxes(self, c, subject_data, latents):
        """(boxes, phrases) for subjects named by phrase: the conditioner's, else the detector's on the decoded `latents`"""
        if self.sam is None:
            raise ValueError("subject_data names subjects by phrase: build the pipeline with segmenter=<HipSamPredictor> (or pass subject_strength=0)")
        if self.vae is None:
            raise ValueError("subject_data names subjects by phrase: build the pipeline with vae=<HipAutoencoderKL> (the segmenter sees the decoded image)")
        if c.get("subject_boxes") is not None:
            return c["subject_boxes"]
        if self.gdino is not None:
            x = self.vae.decode_from_latents(latents)[:1]
            img = ((x.float() / 2 + 0.5).clamp(0, 1) * 255.0).round().to(torch.uint8)[0].permute(1, 2, 0).cpu().numpy()
            return self.gdino(img, ". ".join(k for k, _ in subject_data))
        raise KeyError("subject_data names subjects by phrase: the conditioner returned no 'subject_boxes' and the pipeline has no detector= "
                       "(pass subject_strength=0 to skip the subject-consistency pass)")

    def _subject_mask_pairs(self, c, subject_data, latents):
        """[(mask, subject embedding)] of one request, all masks taken before any pass repaints `latents`: the conditioner's own masks, or the
        phrase -> box -> SAM path of `_subjects_from_phrases` (the PIL masks are kept in `self.subject_masks`, as there)"""
        from .inpaint import subject_masks_from_boxes
        by_phrase = [isinstance(k, str) for k, _ in subject_data]
        if any(by_phrase) and not all(by_phrase):
            raise ValueError("subject_data mixes (mask, embedding) and (phrase, embedding) entries: give one kind")
        if not all(by_phrase):
            return list(subject_data)
        boxes, phrases = self._subject_boxes(c, subject_data, latents)
        pairs, self.subject_masks = subject_masks_from_boxes(subject_data, latents, self.sam, boxes, phrases, self.vae)
        return pairs

    # ---- N whole requests: conditioning for all, then every stage batched (batch.py) -------------------------------------------------------------
    def _conditions_for_batch(self, insts, mm_datas, seeds=None):
        """one conditioning dict per request, as `__call__` gets it from the conditioner or from `_condition_from_llm`. With an LLM: ONE
        `forward_llm_batch` call, the inversion prompt '' encoded once, the other prompts in one `encode_prompt` call per text-encoder role. A request
        whose LLM output has no `<im_gen>` comes back as dict(image_embeds=None, caption=...)."""
        if self.conditioner is not None:
            cs = [self.conditioner(inst, mm, use_cache=False) for inst, mm in zip(insts, mm_datas)]
            self.cache = cs[-1]
            return cs
        if self.any2pix_lm is None:
            raise NotImplementedError("edit_batch needs the pipeline built with conditioner=<callable> or with llm= / llm_tokenizer= / text_encoder=")
        if self._text_encoder is None:
            raise ValueError("a pipeline built with llm= needs text_encoder=<encode_prompt callable> for the denoise stages")
        outs = self.forward_llm_batch(insts, mm_datas, **({} if seeds is None else {"seeds": seeds}))
        cs = [condition_from_llm_output(out, mm) for out, mm in zip(outs, mm_datas)]
        live = [c for c in cs if c["image_embeds"] is not None]
        if not live:
            return cs
        te, row = self._text_encoder, lambda t, j: t[j:j + 1]
        ipe, _, ipp, _ = te(prompt=INVERSION_PROMPT, do_classifier_free_guidance=False)
        pe, ne, pp, npl = te(prompt=[CAPTION_PREFIX + c["caption"] for c in live], negative_prompt=[NEGATIVE_PROMPT] * len(live), do_classifier_free_guidance=True)
        for j, c in enumerate(live):
            c.update(prompt_embeds=row(pe, j), pooled_prompt_embeds=row(pp, j), negative_prompt_embeds=row(ne, j), negative_pooled_prompt_embeds=row(npl, j),
                     inv_prompt_embeds=ipe, inv_pooled_prompt_embeds=ipp)
        if any("subject_data" in c for c in live):          # the same for every request
            spe, sne, spp, snp = te(prompt=SUBJECT_PROMPT, negative_prompt=SUBJECT_NEGATIVE_PROMPT, do_classifier_free_guidance=True)
            for c in live:
                if "subject_data" in c:
                    c.update(subject_prompt_embeds=spe, subject_pooled_prompt_embeds=spp, subject_negative_prompt_embeds=sne, subject_negative_pooled_prompt_embeds=snp)
        if self._refiner_text_encoder is not None:
            rpe, rne, rpp, rnp = self._refiner_text_encoder(prompt=[c["caption"] + REFINER_CAPTION_SUFFIX for c in live],
                                                            negative_prompt=[NEGATIVE_PROMPT] * len(live), do_classifier_free_guidance=True)
            for j, c in enumerate(live):
                c.update(refiner_prompt_embeds=row(rpe, j), refiner_pooled_prompt_embeds=row(rpp, j), refiner_negative_prompt_embeds=row(rne, j),
                         refiner_negative_pooled_prompt_embeds=row(rnp, j))
        return cs

    def edit_batch(self, insts, mm_datas, *, alpha=0.7, h=(0.0, 0.4, 1.0), norm=20.0, refinement=0.5, num_inference_steps=25, subject_strength=0.0, cfg=10,
                   scale=1.0, output_type="latent", debug=False, group: int = 4, shard: bool = True, seeds=None, edit_masks=None, edit_feather=8, auto_masks=None,
                   lora_scale=None, samplers=None, sample_steps=None, sample_adapters=None, subject_modes=None):
        """`__call__` for N instructions on N images -> the list of its `(non_refined, oo, msg)` tuples, in request order. Every knob of `__call__` is a
        scalar (for all requests) or a list of N (`h`: one triple or N triples). `group` requests share one launch sequence in every loop.

        Conditioning: the `conditioner` per request, or ONE `forward_llm_batch` call and the text encoders over the list of prompts; a request whose
        LLM output has no `<im_gen>` gets `(None, None, "FAILED: ...")` and the others go on. The prior runs per request. A conditioner may add
        `polar_noise` (the mixing noise of `denoise`) next to `refiner_noise` / `subject_noise`.
        Stages: base images encoded in batches -> `denoise_batch` -> for the requests with `refinement > 0` the refiner hand-off as configured
        (`refiner_handoff="image"`: batched decode, `requantize`, batched encode) and `batch.refine_batch` -> for `subject_strength > 0` every request's
        masks first (its own masks, or phrase -> box -> SAM), then inpaint pass k batches the requests with more than k subjects (`batch.inpaint_batch`;
        the subjects of one request stay sequential, as in the reference) -> one decode per latent for `output_type != "latent"`.
        Refused: `cfg <= 1` (no guidance in the reference: use `__call__`), mixed latent sizes, `group` outside 1..8, a strength that leaves no step,
        `refinement > 0` on a pipeline without a refiner (where `__call__` skips the pass silently).

        RNG rule: every stage draws from the global CPU generator in REQUEST order -- the VAE posterior samples of the base images, the polar-mixing
        noise, the posterior samples of the refiner hand-off, the refiner noise, the inpaint noise of every pass -- where N serial calls interleave the
        stages per request. A seeded `edit_batch` is therefore reproducible, and equals N serial calls only when the noises are supplied.
        Sharding: as `denoise_batch` -- with a process group up (and `shard`), each of the three loops runs a contiguous shard of its requests per rank
        and all-gathers the result in request order; the stages around them (conditioning, VAE, masks) run on every rank, which must be seeded alike
        for the draws that come from the global generator.

        Seeded RNG rule (`seeds`: a list of N 64-bit seeds, entries None allowed, or ONE int s meaning s + i for request i; None: the rule above, bit for bit
        as ever). Every normal draw of a seeded request comes from the request's own Philox stream on the device (include/ia2p.h, "Seeded noise"), draw ids of
        noise.py: 0 the base image's posterior sample, 1 the polar-mixing noise, 2 the posterior sample of the refiner hand-off, 3 the refiner noise, 4 + k the
        inpaint noise of subject pass k. A value depends on (seed, draw id, element) only, so request i with seed s gets the same noise -- and, rows of a group
        being independent, the same bits in a group of the same size -- whatever shares the call, in whatever order; `__call__(seed=s)` serves it from the
        same noise alone (equal within the batch-against-serial tolerance: bit identity across GROUP SIZES is not promised). The inverted latents stay on the
        device: noise, mix (`ia2p_polar_mix_v`: fp32, not the bits of the unseeded path's CPU fp16 mix), posterior samples and `add_noise` inputs are all made
        there. Where the LLM samples on the device the request's seed is also its entry of `generate_batch(seeds=)`; under the host sampler the LLM keeps the
        global generator. Precedence: a noise tensor the conditioner supplies (`polar_noise`, `refiner_noise`, `subject_noise`) wins over the seed, the seed
        over the global generator. Seeded and unseeded requests may share a call and a group; the unseeded ones draw from the global generator in request
        order among themselves. Seeded draws need no rank to be seeded alike. With `debug=True` a seeded request's message also carries `seed`.

        Edit masks (`edit_masks`: ONE mask for all requests, or a list of N with None entries; None: today's launches, bit for bit; `edit_feather` as in
        `__call__`). Request i may change inside its mask only, as `__call__(edit_mask=)` serves it: in a group where at least one request has a mask the
        inversion records its trajectory and every sampling step is followed by one selection launch (`ia2p_known_blend_v`), request r at its own level
        max(N_r - 1 - i, 0); the requests without a mask carry all ones there, which returns their bits. The refiner loop blends the base latents at its own
        noise level with its own noise (no new draw), the subject masks are multiplied by the edit mask, and "pil" results are composited with the base
        image in 8 bits; "np" / "pt" are refused. A group where nobody has a mask runs exactly the unmasked launch sequence.

        Automatic masks (`auto_masks`: ONE value for all requests -- True, a dict or an `auto_mask.AutoMask` -- or a list of N with None entries; None: nothing
        changes, no launch and no draw). Request i's edit mask is estimated from the request itself before the inversion, the requests that ask
        for one `group` at a time, 2 x group rows per UNet evaluation, on every rank; where `edit_masks[i]` is given too the two latent masks are multiplied. From
        there on the request is served as under `edit_masks`. An unseeded request's n estimate noises come from the global generator in request order, after the
        posterior samples of the base images and before the polar-mixing noise; a seeded one's are draw 65536 of its own stream. With `debug=True` the message
        also carries `edit_mask`, `auto_mask_map` and `auto_mask_stats`.

        LoRA (`lora_scale`: ONE number for the call; None: no launch, no bit): the active adapter weights of both UNets are multiplied by it for this call and
        the state before is put back afterwards, also when the call raises. A batch shares its weights: per-request adapters inside one `edit_batch` are not
        offered (requests that want different adapters go into different calls).

        Few-step sampling (`samplers`, `sample_steps`: a scalar or a list of N; None: nothing changes, no launch, no draw, no bit). Request i with
        sampler "lcm" (or None once an `LCMScheduler` is assigned to `pipe.scheduler`) is sampled by the consistency sampler over `sample_steps` steps (default 4)
        after the same inversion and mixing. A group holds one sampler; a call that mixes them runs the DDIM requests' groups, then the LCM requests'. The step
        noise: the conditioner's `step_noise`, else draw 65537 of the request's seed inside the update launch, else host draws right after the request's own
        polar-mixing draw. LCM requests with cfg <= 1 run without guidance (all LCM requests of a call must agree on that). `sample_adapters` (ONE value per
        call: a name, a list or (names, weights)): LoRA adapters active around the guided sampling loops only.

        Subject passes (`subject_modes`: "serial", "joint" or a list of N; None: serial, as ever). A "joint" request repaints ALL its subjects in one inpaint
        stage -- every subject's image tokens in one context, each acting under its own mask (regional image prompts, `ia2p_attention_regions`), the blend
        under the union of the masks, one noise (draw DRAW_INPAINT + 0) -- so S subjects cost one loop instead of S. It is NOT the serial result: serially,
        pass k + 1 starts from the repaint of pass k and draws its own noise; jointly, all subjects are repainted from the same start under one noise. The
        joint requests of a call share groups (padded to the group's largest subject count, which changes no bit of a row); the serial ones keep their bits."""
        from .batch import edit_batch
        return edit_batch(self, insts, mm_datas, **({} if lora_scale is None else dict(lora_scale=lora_scale)), alpha=alpha, h=h, norm=norm, refinement=refinement, num_inference_steps=num_inference_steps,
                          subject_strength=subject_strength, cfg=cfg, scale=scale, output_type=output_type, debug=debug, group=group, shard=shard, seeds=seeds,
                          **({} if edit_masks is None else dict(edit_masks=edit_masks)), **({} if auto_masks is None else dict(auto_masks=auto_masks)),
                          **({} if edit_masks is None and auto_masks is None else dict(edit_feather=edit_feather)),
                          **({} if samplers is None else dict(samplers=samplers)), **({} if sample_steps is None else dict(sample_steps=sample_steps)),
                          **({} if sample_adapters is None else dict(sample_adapters=sample_adapters)), **({} if subject_modes is None else dict(subject_modes=subject_modes)))

    # ---- reference keyword surface ----------------------------------------------------------------------------------
    def __call__(self, inst, mm_data, alpha=0.7, h=[0.0, 0.4, 1.0], norm=20.0, refinement=0.5, llm_only=False, num_inference_steps=25,
                 use_cache=False, debug=False, diffusion_mode="default", subject_strength=0.0, cfg=10, scale=1.0, output_type="latent", seed=None,
                 edit_mask=None, edit_feather=8, *, auto_mask=None, lora_scale=None, sampler=None, sample_steps=None, sample_adapters=None,
                 subject_mode="serial", control_image=None, control_scale=1.0, control_start=0.0, control_end=1.0, control_from=None) -> Any:
        """-> (non_refined, oo, msg). output_type "latent" (default): latents; "pil" / "np" / "pt" (needs vae=): decoded images as diffusers'
        `postprocess` gives them, each latent decoded once (reference :356-386 returns PIL images).
        `seed` (a 64-bit unsigned integer; None: every draw from the global CPU generator, as ever): every normal draw of the request comes from its own
        Philox stream on the device, by the draw ids of noise.py -- the base image's posterior sample, the polar-mixing noise, the posterior sample of the
        refiner hand-off, the refiner noise, the inpaint noise of subject pass k -- and, where the LLM samples on the device, so do its tokens (under the
        host sampler the LLM keeps the global generator). The image then depends on the request and its seed alone: `edit_batch(seeds=[seed])` serves the
        same request from the same noise (equal within the batch-against-serial tolerance; bit identity across group sizes is not promised, as the UNet's
        batch-dependent plans sum in other orders). A noise the conditioner supplies (`polar_noise`, `refiner_noise`, `subject_noise`) wins over the seed.
        With `debug=True` the message also carries `seed`.
        `edit_mask` (None: nothing changes, no launch and no bit): the edit may change the image inside the mask only (forms and sizes:
        `image_processor.load_edit_mask`). Inversion records its trajectory; outside the mask every sampling step is replaced by the inverted latents of the
        same noise level (the last step lands on the base latents), the refiner pass keeps `base_latents` re-noised with its own noise there, and every
        subject mask is multiplied by the edit mask. "latent": both results equal `base_latents` wherever the latent mask (a cell is 1 if any of its
        pixels is in the mask) is 0. "pil": both images are composited in 8 bits with the base image (the loaded one, or the 8-bit decode of `base_latents`)
        through the mask feathered inwards over `edit_feather` pixels (0 .. 64; 8 is a design choice): every pixel outside the mask carries the base image's
        byte. "np" / "pt" are refused with a mask. With `debug=True` the message also carries `edit_mask_latent`.
        `auto_mask` (keyword only; None: nothing changes, no launch, no draw, no bit): True (the defaults), a dict or an `auto_mask.AutoMask(num_maps=8,
        strength=0.5, ratio=3.0, dilate=1, noise=None, max_rows=None)`. The edit mask is estimated from the request itself, before the inversion:
        the base latents noised `num_maps` times at the schedule's `strength` level, the UNet's noise prediction under the inversion's condition and under the
        edit's (prompt embeddings + IP tokens, this call's `scale`), a cell on where their mean absolute difference exceeds `ratio / 2` times its mean over the
        grid, grown by `dilate` cells. With `edit_mask` too the two latent masks are multiplied. From there on everything is the `edit_mask` path, its output
        types and `edit_feather` included; the pixel mask of the composite is the latent mask's cells (inside the user's pixel mask where there is one). The
        noises: the knob's `noise`, else draw 65536 of the request's `seed`, else ONE `torch.randn(n, C, h, w)` from the global CPU generator, drawn before the
        polar-mixing noise. An empty mask returns the base image, a full one the unmasked edit. With `debug=True` the message also carries `edit_mask` (the
        latent mask used), `auto_mask_map` (fp32 [1, h, w]) and `auto_mask_stats` (fp32 [2]: mean, threshold).
        `lora_scale` (keyword only; None: nothing changes, no launch, no bit): ONE number that multiplies the active LoRA adapter weights of both UNets for this
        call (`set_adapters` / `load_lora_weights`); the state before is put back afterwards, also when the call raises.
        `sampler`, `sample_steps`, `sample_adapters` (keyword only; None: nothing changes, no launch, no draw, no bit): the few-step consistency sampler for the
        guided sampling stage, and LoRA adapters active around that stage only (`denoise`). The conditioner may supply `step_noise`, which wins
        over the seed (draw 65537 of it), which wins over the global generator. The refiner and the subject passes are untouched.
        `control_image`, `control_scale`, `control_start`, `control_end` (keyword only; None: nothing changes, no launch, no bit; needs controlnet=): a ControlNet
        guides the guided sampling stage by the condition map the caller brings (`denoise`). The other stages run without control.
        `control_from` (keyword only; None: nothing changes, no launch, no allocation, no bit; needs controlnet=): "canny", "blur", "grey", a dict such as
        {"kind": "canny", "low": 50, "high": 150, "blur_sigma": 1.4} or a `condition.Condition` -- the condition map is made on the device from the base image as
        the pipeline holds it (the 8-bit image after `loas_base_img`'s resize and crop, at 8 x the latent grid) and passed on exactly as a
        `control_image` would be, under the same `control_scale` / `control_start` / `control_end`. Together with `control_image`: ValueError. A conditioner that
        brings `base_latents` leaves no 8-bit pixels to make the map from: ValueError. With `debug=True` the message also carries `control_map` (uint8, on the
        device). `make_control_image` returns the same map as a PIL image.
        `subject_mode` (keyword only; "serial": as ever, one inpainting loop per subject as the reference runs them): "joint" repaints all subjects in ONE
        loop -- every subject's image tokens in one context, each under its own mask, the blend under the union of the masks, one noise (draw
        DRAW_INPAINT + 0 of a seeded request). "joint" is NOT the serial result: in the serial form later passes see earlier repaints and draw their own
        noise; in the joint form all subjects are repainted from the same start under one noise."""
        if subject_mode not in ("serial", "joint"):
            raise ValueError(f"subject_mode: 'serial' or 'joint', got {subject_mode!r}")
        if lora_scale is not None:
            with self.lora_scaled(lora_scale):
                return self(inst, mm_data, alpha=alpha, h=h, norm=norm, refinement=refinement, llm_only=llm_only, num_inference_steps=num_inference_steps,
                            use_cache=use_cache, debug=debug, diffusion_mode=diffusion_mode, subject_strength=subject_strength, cfg=cfg, scale=scale,
                            output_type=output_type, seed=seed, edit_mask=edit_mask, edit_feather=edit_feather, auto_mask=auto_mask, sampler=sampler,
                            sample_steps=sample_steps, sample_adapters=sample_adapters, subject_mode=subject_mode, control_image=control_image,
                            control_scale=control_scale, control_start=control_start, control_end=control_end, control_from=control_from)
        if control_from is not None:
            control_from = check_control_from(self, control_from, control_image)
        if control_image is not None and self.controlnet is None:
            raise ValueError("control_image needs the pipeline built with controlnet=<HipControlNetModel>")
        control = {} if control_image is None else dict(control_image=control_image, control_scale=control_scale, control_start=control_start, control_end=control_end)
        if seed is not None:
            seed = _noise.check_seed(seed)
        few, smp = {}, "ddim"
        if sampler is not None or sample_steps is not None or sample_adapters is not None or isinstance(getattr(getattr(self, "pipe", None), "scheduler", None), LCMScheduler):
            from .batch import resolve_sample_adapters
            smp, _ = resolve_sampler(self.pipe.scheduler, sampler, sample_steps)                # every refusal before the conditioner is asked
            resolve_sample_adapters(self.pipe.unet, sample_adapters)
            few = {k: v for k, v in dict(sampler=sampler, sample_steps=sample_steps, sample_adapters=sample_adapters).items() if v is not None}
        check_output_type(self, output_type)
        if auto_mask is not None:
            from .auto_mask import auto_mask_t_start, intersect, resolve_auto_mask
            auto_mask = resolve_auto_mask(auto_mask)
        if auto_mask is not None:                                                              # (False resolves to None: off)
            auto_mask_t_start(num_inference_steps, auto_mask.strength)
        if edit_mask is not None or auto_mask is not None:
            from .image_processor import check_edit_feather
            check_edit_output_type(output_type)
            edit_feather = check_edit_feather(edit_feather)
        if self.conditioner is None and self.any2pix_lm is not None:
            c = self._condition_from_llm(inst, mm_data, use_cache, llm_only, **({} if seed is None else {"seed": seed}))
            if llm_only:
                return None, None, c["caption"]
        elif self.conditioner is None:
            raise NotImplementedError("the LLM / ImageBind / prior stages are outside the denoise hot path (SURVEY.md §8): construct with "
                                      "conditioner=<callable returning dict(image_embeds, base_embed, y, caption, base_latents, "
                                      "prompt_embeds, pooled_prompt_embeds, negative_prompt_embeds, negative_pooled_prompt_embeds)> "
                                      "or call .denoise() with explicit conditioning")
        else:
            c = self.conditioner(inst, mm_data, use_cache=use_cache)
            self.cache = c
            if llm_only:
                return None, None, c["caption"]
        latent_la = fuse_instruction_embedding(c["base_embed"], c["image_embeds"], prior_y0(self, c), h, norm)
        masked, kept, edit_px, edit_m = {}, {}, None, None
        base_latents = self._base_latents(c, seed) if edit_mask is None and auto_mask is None and control_from is None else self._base_latents(c, seed, kept)
        control_map = None
        if control_from is not None:                                                           # the map of the image the VAE encode was fed, made on the device
            from .image_processor import image_to_u8
            control_map = self.control_map(control_from, image_to_u8(kept["image"]) if "image" in kept else None, base_latents)
            control = dict(control_image=control_map, control_scale=control_scale, control_start=control_start, control_end=control_end)
        if edit_mask is not None:
            edit_px, edit_m = resolve_edit_mask(self, edit_mask, base_latents, edit_mask_file_size(c))
            masked = dict(edit_mask=edit_m)
        auto = None
        if auto_mask is not None:                                                              # the estimate, before the inversion; times the user's latent mask
            auto = self.estimate_edit_mask(base_latents, latent_la.reshape(1, -1)[0], **embeds(c), inv_prompt_embeds=c.get("inv_prompt_embeds"),
                                           inv_pooled_prompt_embeds=c.get("inv_pooled_prompt_embeds"), num_inference_steps=num_inference_steps, scale=scale,
                                           seed=seed, auto_mask=auto_mask)
            px, edit_m = resolve_edit_mask(self, intersect(auto[0], edit_m), base_latents)
            edit_px = px if edit_px is None else torch.minimum(px, edit_px)
            masked = dict(edit_mask=edit_m)
        images, latent_inv = self.denoise(base_latents, latent_la.reshape(1, -1)[0], **embeds(c),
                                          inv_prompt_embeds=c.get("inv_prompt_embeds"), inv_pooled_prompt_embeds=c.get("inv_pooled_prompt_embeds"),
                                          alpha=alpha, num_inference_steps=num_inference_steps, cfg=cfg, scale=scale, seed=seed,
                                          noise=c.get("polar_noise") if seed is not None else None, **masked,      # (unseeded: this call has always drawn its own)
                                          **few, **({"step_noise": c["step_noise"]} if smp == "lcm" and c.get("step_noise") is not None else {}), **control)
        non_refined = images
        oo = images
        decoded = None          # the decode of `images`, when the refiner hand-over made it
        if refinement > 0 and self.piperf is not None:                                         # :358-361
            _need(c, REFINER_KEYS, "refiner pass")
            # Conditioning = text encoder 2 on caption + ',high quality,well-formed,award-winning' (the conditioner supplies its embeddings).
            kw = dict(strength=refinement, **embeds(c, "refiner_"), noise=c.get("refiner_noise"), output_type="latent", **({} if seed is None else {"noise_seed": seed}))
            if edit_m is not None:                                                             # outside the mask: the base latents at the loop's noise level
                kw.update(known_latents=base_latents, edit_mask=edit_m)
            if refiner_handoff_by_image(self):
                # the reference hands a decoded 8-bit image over and the refiner pipeline re-encodes it with the shared VAE
                # (`retrieve_latents(vae.encode(image)) * scaling_factor`: a posterior SAMPLE, global RNG)
                decoded = self.pipe._vae_decode(images)
                if self.vae is not None:    # the same steps with the 8-bit round trip in one HIP launch (bit-identical to to_8bit_image)
                    enc = {} if seed is None else dict(seeds=[seed], draw=_noise.DRAW_HANDOFF_POSTERIOR)
                    oo = self.piperf(latents=self.piperf._vae_encode(requantize(decoded), **enc), **kw).images
                else:
                    oo = self.piperf(image=to_8bit_image(decoded), **kw).images
            else:
                oo = self.piperf(latents=images, **kw).images
        subject_data = c.get("subject_data") or []
        if subject_strength > 0 and len(subject_data) > 0:                                     # :363-368
            _need(c, SUBJECT_KEYS, "subject-consistency pass")
            kw = dict(output_type="latent", **embeds(c, "subject_"), noise=c.get("subject_noise"), **({"joint": True} if subject_mode == "joint" else {}))
            if seed is not None:
                kw["noise_seed"] = seed                                                        # pass k draws from DRAW_INPAINT + k (inpaint.subject_consistency)
            by_phrase = [isinstance(k, str) for k, _ in subject_data]
            if any(by_phrase) and not all(by_phrase):
                raise ValueError("subject_data mixes (mask, embedding) and (phrase, embedding) entries: give one kind")
            if edit_px is not None:                                                            # every subject mask times the edit mask, then the same passes
                pairs = [(intersect_subject_mask(mk, edit_px), emb) for mk, emb in self._subject_mask_pairs(c, subject_data, oo)]
                oo = subject_consistency(pairs, oo, self.ip_adapter_xl_inpaint, subject_strength, **kw)
            elif all(by_phrase):                                                               # gdino/lib.py:69-103: masks from SAM on the detector's boxes
                oo = self._subjects_from_phrases(c, subject_data, oo, subject_strength, kw)
            else:                                                                              # masks given by the conditioner
                oo = subject_consistency(subject_data, oo, self.ip_adapter_xl_inpaint, subject_strength, **kw)
        msg = "SUCCESS!" if not debug else dict(output_caption=c["caption"], latent_inv=latent_inv, latent_la=latent_la, **({} if seed is None else {"seed": seed}),
                                                **({} if edit_m is None else {"edit_mask_latent": edit_m}), **({} if control_map is None else {"control_map": control_map}),
                                                **({} if auto is None else {"edit_mask": edit_m, "auto_mask_map": auto[1], "auto_mask_stats": auto[2]}))
        if output_type != "latent" and edit_px is not None:                                    # "pil": composited with the base image in 8 bits
            from .image_processor import image_to_u8, mask_feather
            base_u8 = image_to_u8(kept["image"] if "image" in kept else self.pipe._vae_decode(base_latents.to(self.pipe.unet.device, torch.float16)))
            alpha_u8 = mask_feather(edit_px, edit_feather)
            refined_is_base = oo is non_refined
            non_refined = composite_edit(self, decoded if decoded is not None else self.pipe._vae_decode(non_refined), base_u8, alpha_u8)
            oo = non_refined if refined_is_base else composite_edit(self, self.pipe._vae_decode(oo), base_u8, alpha_u8)
        elif output_type != "latent":
            post = self.pipe.image_processor.postprocess
            refined_is_base = oo is non_refined
            non_refined = post(decoded if decoded is not None else self.pipe._vae_decode(non_refined), output_type=output_type)
            oo = non_refined if refined_is_base else post(self.pipe._vae_decode(oo), output_type=output_type)
        return non_refined, oo, msg
