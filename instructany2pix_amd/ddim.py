"""DDIM inversion and sampling loops of the denoise hot path, behind the reference's pipeline surfaces.

  SDXLDDIMPipeline.inverse(...)            <- instructany2pix/ddim/pnp_pipeline.py:92-278 (hot loop :251-275)
  StableDiffusionXLPipeline.__call__(...)  <- the diffusers SDXL loop the reference drives through
                                              IPAdapterXL.generate (ip_adapter.py:346-354); loop text vendored at
                                              instructany2pix/ddim/sdxl_pipeline.py:764-857
Every tensor update runs on the GPU through the C ABI (UNet: ia2p_unet_forward; CFG + DDIM: ia2p_ddim_step).

The stages either side are injectable callables: CLIP text encoders (`encode_prompt`, out of scope) and the VAE
(`vae_encode` / `vae_decode`; `instructany2pix_amd.vae.HipAutoencoderKL` provides HIP implementations). Without them
the loops take `prompt_embeds` / `pooled_prompt_embeds` / `latents` directly, which is also how bench.py and the
parity tests drive them.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Callable, Optional, Tuple

import torch

from . import noise as _noise
from .scheduler import DDIMScheduler, LCMScheduler, fused_update, known_blend_v, level_table

OUTPUT_TYPES = ("latent", "pt", "np", "pil")            # (image_processor.OUTPUT_TYPES; repeated so that importing this module loads no PIL)


class StableDiffusionXLPipelineOutput(SimpleNamespace):
    """`.images` like diffusers' output class (reference pnp_pipeline.py:278)."""


def get_add_time_ids(unet, original_size, crops_coords_top_left, target_size, projection_dim, dtype=torch.float16):
    """`_get_add_time_ids` (reference pnp_pipeline.py:23-71, requires_aesthetics_score=False branch;
    same check as sdxl_pipeline.py:506-520)."""
    add_time_ids = list(original_size + crops_coords_top_left + target_size)
    passed = unet.config.addition_time_embed_dim * len(add_time_ids) + projection_dim
    expected = unet.add_embedding.linear_1.in_features
    if expected != passed:
        raise ValueError(f"Model expects an added time embedding vector of length {expected}, but a vector of {passed} was created. "
                         f"The model has an incorrect config. Please check `unet.config.time_embedding_type` and "
                         f"`text_encoder_2.config.projection_dim`.")
    return torch.tensor([add_time_ids], dtype=dtype)


def expand_rows(t, batch: int):
    """the embeddings of one prompt for every row of a serial call's batch"""
    return t if t.shape[0] == batch else t.expand(batch, *([-1] * (t.ndim - 1)))


def conditioning(device, prompt_embeds, pooled_prompt_embeds, time_ids, negative_prompt_embeds=None, negative_pooled_prompt_embeds=None, negative_time_ids=None):
    """What every loop, serial or batched, hands the UNet next to the latents: -> (context, added_cond_kwargs), contiguous fp16 on `device`.
    The embeddings come batched, [B, ...] (a serial pipeline's expanded to its batch, a group's concatenated over its requests); `time_ids` is ONE row.
    With the negative embeddings the rows are [uncond x B | cond x B] (the reference's cat([negative, positive]), sdxl_pipeline.py:800-803) and the
    uncond half carries `negative_time_ids` where the refiner gives some; without them the evaluation is unguided: the B cond rows alone."""
    f16 = lambda t: t.to(device=device, dtype=torch.float16)
    B = prompt_embeds.shape[0]
    ctx, pooled, tid = f16(prompt_embeds), f16(pooled_prompt_embeds), time_ids.repeat(B, 1)
    if negative_prompt_embeds is not None:
        ctx = torch.cat([f16(negative_prompt_embeds), ctx], dim=0)
        pooled = torch.cat([f16(negative_pooled_prompt_embeds), pooled], dim=0)
        tid = torch.cat([(time_ids if negative_time_ids is None else negative_time_ids).repeat(B, 1), tid], dim=0)
    return ctx.contiguous(), {"text_embeds": pooled.contiguous(), "time_ids": tid.to(device)}


class _PipelineBase:
    vae_scale_factor = 8
    vae = None
    image_processor = None          # VaeImageProcessor when a VAE is attached (vae=): images in and out as in diffusers
    mask_processor = None

    def __init__(self, unet, scheduler: Optional[DDIMScheduler] = None, encode_prompt: Optional[Callable] = None,
                 vae_encode: Optional[Callable] = None, vae_decode: Optional[Callable] = None, vae=None):
        self.unet = unet
        self.scheduler = scheduler or DDIMScheduler()
        self._encode_prompt = encode_prompt
        self._vae_encode = vae_encode
        self._vae_decode = vae_decode
        if vae is not None:
            # a HipAutoencoderKL: its encode / decode become the hooks, and `image=` / `output_type` mean what they mean in diffusers
            if vae_encode is not None or vae_decode is not None:
                raise ValueError("pass either vae= or the vae_encode= / vae_decode= hooks, not both")
            from .image_processor import VaeImageProcessor
            self.vae = vae
            self.vae_scale_factor = 2 ** (len(vae.config.block_out_channels) - 1)
            self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor, device=vae.device)
            self.mask_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor, do_normalize=False, do_binarize=True,
                                                    do_convert_grayscale=True, device=vae.device)
            self._vae_encode = vae.encode_to_latents
            self._vae_decode = vae.decode_from_latents

    @property
    def device(self):
        return self.unet.device

    def to(self, *a, **kw):
        return self

    def encode_prompt(self, prompt=None, num_images_per_prompt=1, do_classifier_free_guidance=True, negative_prompt=None, **kw):
        if self._encode_prompt is None:
            raise NotImplementedError("text encoders are outside the denoise hot path: pass prompt_embeds / pooled_prompt_embeds, "
                                      "or construct the pipeline with encode_prompt=<callable>")
        return self._encode_prompt(prompt=prompt, num_images_per_prompt=num_images_per_prompt,
                                   do_classifier_free_guidance=do_classifier_free_guidance, negative_prompt=negative_prompt, **kw)

    def _check_output_type(self, output_type):
        if self.vae is not None and output_type not in OUTPUT_TYPES:
            raise ValueError(f"output_type must be one of {OUTPUT_TYPES}, got {output_type!r}")

    def _image_latents(self, image, height=None, width=None, seeds=None, draw=0, keep=None):
        """`image=` -> scaled latents: with a VAE attached, `image_processor.preprocess` (PIL, uint8 arrays, [0, 1] floats, [-1, 1] tensors;
        4-channel tensors are latents already) then the posterior sample; with hooks only, the hook gets `image` as it is.
        `seeds` (one per image) / `draw`: the posterior sample from the images' own streams (`HipAutoencoderKL.encode_to_latents`); an attached VAE only --
        a `vae_encode=` hook draws its own sample and never sees a seed. `keep` (a dict, an attached VAE only): receives the preprocessed image the
        encoder sees as keep["image"] (an edit inside a mask composites its result with it)."""
        if self._vae_encode is None:
            raise NotImplementedError("VAE encode is not attached: pass latents=, or construct with vae= or vae_encode=<callable>")
        if self.vae is None:
            return self._vae_encode(image)
        image = self.image_processor.preprocess(image, height=height, width=width)
        if image.shape[1] == 4:
            return image
        if keep is not None:
            keep["image"] = image
        return self._vae_encode(image) if seeds is None else self._vae_encode(image, seeds=seeds, draw=draw)

    def _output(self, latents, output_type):
        """final latents -> what `output_type` asks for; with hooks only every type but "latent" returns the decode hook's raw tensor"""
        if output_type == "latent":
            return latents
        if self._vae_decode is None:
            raise NotImplementedError("VAE decode is not attached: use output_type='latent' or pass vae= or vae_decode=")
        image = self._vae_decode(latents)
        return image if self.vae is None else self.image_processor.postprocess(image, output_type=output_type)

    def _check_embeds(self, prompt, prompt_embeds, pooled):
        # same conditions as check_inputs (reference sdxl_pipeline.py:429-486) for the arguments that remain
        if prompt is not None and prompt_embeds is not None:
            raise ValueError("Cannot forward both `prompt` and `prompt_embeds`. Please make sure to only forward one of the two.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        if prompt_embeds is not None and pooled is None:
            raise ValueError("If `prompt_embeds` are provided, `pooled_prompt_embeds` also have to be passed.")


class SDXLDDIMPipeline(_PipelineBase):
    """DDIM inversion x0 -> xT. No classifier-free guidance (reference :161)."""

    @torch.no_grad()
    def inverse(self, prompt=None, prompt_2=None, image=None, strength: float = 0.3, num_inference_steps: int = 50,
                guidance_scale: float = 5.0, negative_prompt=None, num_images_per_prompt: int = 1, eta: float = 0.0,
                generator=None, latents: Optional[torch.Tensor] = None, prompt_embeds=None, negative_prompt_embeds=None,
                pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, output_type="pil", return_dict=True,
                cross_attention_kwargs=None, original_size: Tuple[int, int] = None, crops_coords_top_left=(0, 0),
                target_size: Tuple[int, int] = None, image_embeds=None, callback=None, return_trajectory: bool = False, **unused):
        """`return_trajectory` (new; False: nothing changes): the output also carries `.trajectory`, fp16 [N + 1, B, 4, h, w]: level 0 the latents the loop
        starts from, level j + 1 the result of iteration j (what `callback` sees there), written through `out2` of the update launch the loop makes anyway.
        An edit inside a mask replaces the outside of every sampling step with the level of the same noise (`StableDiffusionXLPipeline(known_trajectory=)`)."""
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)                       # :133
        if strength < 0 or strength > 1:
            raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        if num_inference_steps is None or not isinstance(num_inference_steps, int) or num_inference_steps <= 0:
            raise ValueError(f"`num_inference_steps` has to be a positive integer but is {num_inference_steps}")
        self._check_embeds(prompt, prompt_embeds, pooled_prompt_embeds)
        self._check_output_type(output_type)
        if prompt_embeds is None:
            prompt_embeds, _, pooled_prompt_embeds, _ = self.encode_prompt(
                prompt=prompt, num_images_per_prompt=num_images_per_prompt, do_classifier_free_guidance=False, negative_prompt=negative_prompt)
        dev = self.device
        if latents is None:                                                                     # :190-204 (VAE: "next" row)
            if image is None:
                raise ValueError("inverse() needs `image` (with vae= or a vae_encode callable) or `latents`")
            if self._vae_encode is None:
                raise NotImplementedError("VAE encode is outside the denoise hot path: pass latents=, or construct with vae= or vae_encode=<callable>")
            latents = self._image_latents(image)
        latents = latents.to(device=dev, dtype=torch.float16).contiguous().clone()    # the loop ping-pongs buffers: never the caller's tensor
        batch = latents.shape[0]
        self.scheduler.set_timesteps(num_inference_steps, device=dev)                           # :192
        height, width = latents.shape[-2] * self.vae_scale_factor, latents.shape[-1] * self.vae_scale_factor
        original_size = original_size or (height, width)
        target_size = target_size or (height, width)
        add_time_ids = get_add_time_ids(self.unet, original_size, crops_coords_top_left, target_size, int(pooled_prompt_embeds.shape[-1]))      # :228-240
        # unguided; `image_embeds` zeros (:246-248) are ignored by a text_time UNet
        prompt_embeds, added = conditioning(dev, expand_rows(prompt_embeds, batch), expand_rows(pooled_prompt_embeds, batch), add_time_ids)

        eps = torch.empty_like(latents)
        nxt = torch.empty_like(latents)
        traj = None
        if return_trajectory:
            traj = torch.empty((num_inference_steps + 1,) + tuple(latents.shape), dtype=torch.float16, device=dev)
            traj[0].copy_(latents)
        prev_t = None
        acp = self.scheduler.alphas_cumprod
        for i, t in enumerate(reversed(self.scheduler.timesteps)):                              # :251 ascending t
            t = int(t)
            self.unet(latents, t, encoder_hidden_states=prompt_embeds, cross_attention_kwargs=cross_attention_kwargs,
                      added_cond_kwargs=added, return_dict=False, out=eps)
            a_t = acp[t]
            a_prev = acp[prev_t] if prev_t is not None else self.scheduler.final_alpha_cumprod  # :262-267
            prev_t = t
            c_x, c_e = DDIMScheduler.inversion_coeffs(float(a_t), float(a_prev))
            fused_update(latents, eps, None, 1.0, c_x, c_e, nxt, None if traj is None else traj[i + 1])      # :270-275 _backward_ddim
            latents, nxt = nxt, latents
            if callback is not None:
                callback(i, t, latents)
        if traj is not None:
            return StableDiffusionXLPipelineOutput(images=latents, trajectory=traj)
        return StableDiffusionXLPipelineOutput(images=latents)                                  # :278 raw latents


class StableDiffusionXLPipeline(_PipelineBase):
    """DDIM sampling xT -> x0 with classifier-free guidance (2x batch UNet evaluation); under an `LCMScheduler` the few-step consistency sampler."""

    @torch.no_grad()
    def __call__(self, prompt=None, height=None, width=None, num_inference_steps: int = 50, guidance_scale: float = 5.0,
                 negative_prompt=None, num_images_per_prompt: int = 1, eta: float = 0.0, generator=None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None,
                 output_type="latent", return_dict=True, callback=None, callback_steps=1, cross_attention_kwargs=None,
                 guidance_rescale: float = 0.0, original_size=None, crops_coords_top_left=(0, 0), target_size=None, known_trajectory=None, edit_mask=None,
                 step_noise=None, noise_seed=None, known_latents=None, **unused):
        """`known_trajectory` + `edit_mask` (new; both None: nothing changes): mask-guided decoding. `known_trajectory` is `inverse(return_trajectory=True)`'s
        store over the SAME `num_inference_steps`, fp16 [N + 1, B, 4, h, w]; `edit_mask` a {0, 1} latent mask [B or 1, 1, h, w]. Where the mask is 0 the start
        is level N and the result of sampling step i is replaced by level N - 1 - i (`ia2p_known_blend_v`: a selection, one launch per step), so the last
        step leaves level 0 there, bit for bit.
        With `self.scheduler` an `LCMScheduler` (as diffusers users switch samplers) the loop is the consistency sampler over `num_inference_steps` LCM steps
        (`batch.lcm_sample`). The noise injected after step s: `step_noise` (fp16 [steps - 1, 4, h, w], or [steps - 1, B, 4, h, w] for a
        batch), else draw DRAW_LCM of `noise_seed` (row b: seed + b) made inside the update launch, else one fp16 CPU draw of the latents' shape per step
        from `generator` or the global RNG. An edit inside a mask takes `known_latents` (the base latents) + `edit_mask` there: the LCM timesteps are not the
        inversion's levels. Under DDIM these three keywords are refused."""
        lcm = isinstance(self.scheduler, LCMScheduler)
        if not lcm and (step_noise is not None or noise_seed is not None or known_latents is not None):
            raise ValueError("`step_noise`, `noise_seed` and `known_latents` belong to the LCM sampler: assign an LCMScheduler to `.scheduler` first")
        if lcm and known_trajectory is not None:
            raise ValueError("the LCM timesteps are not the inversion's levels: pass `known_latents`, not `known_trajectory`")
        if lcm and (known_latents is None) != (edit_mask is None):
            raise ValueError("`known_latents` and `edit_mask` go together: pass both or neither")
        if lcm:
            known_trajectory = known_latents           # (for the pairing check below)
        if guidance_rescale != 0.0 or eta != 0.0:
            raise NotImplementedError("guidance_rescale / eta are inactive on the reference's path (sdxl_pipeline.py:846, eta=0)")
        if (known_trajectory is None) != (edit_mask is None):
            raise ValueError("`known_trajectory` and `edit_mask` go together: pass both or neither")
        self._check_embeds(prompt, prompt_embeds, pooled_prompt_embeds)
        self._check_output_type(output_type)
        do_cfg = guidance_scale > 1.0                                                           # sdxl_pipeline.py:735
        if prompt_embeds is None:
            prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds = self.encode_prompt(
                prompt=prompt, num_images_per_prompt=num_images_per_prompt, do_classifier_free_guidance=do_cfg, negative_prompt=negative_prompt)
        if do_cfg and (negative_prompt_embeds is None or negative_pooled_prompt_embeds is None):
            raise ValueError("classifier-free guidance needs negative_prompt_embeds and negative_pooled_prompt_embeds")
        dev = self.device
        batch = prompt_embeds.shape[0]
        sample_size = getattr(self.unet.config, "sample_size", 128)
        height = height or sample_size * self.vae_scale_factor
        width = width or sample_size * self.vae_scale_factor
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        self.scheduler.set_timesteps(num_inference_steps, device=dev)                           # :765
        shape = (batch, self.unet.config.in_channels, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if latents is None:                                                                     # prepare_latents :489-504
            g = generator if not isinstance(generator, list) else generator[0]
            gen_dev = g.device if g is not None else torch.device("cpu")
            latents = torch.randn(shape, generator=g, device=gen_dev, dtype=torch.float16)
        else:
            if tuple(latents.shape[-2:]) != shape[-2:]:
                height, width = latents.shape[-2] * self.vae_scale_factor, latents.shape[-1] * self.vae_scale_factor
        latents = (latents.to(dev) * self.scheduler.init_noise_sigma).to(torch.float16).contiguous()
        if latents.shape[0] != batch:
            latents = latents.expand(batch, -1, -1, -1).contiguous()
        original_size = original_size or (height, width)
        target_size = target_size or (height, width)
        add_time_ids = get_add_time_ids(self.unet, original_size, crops_coords_top_left, target_size,
                                        int(pooled_prompt_embeds.shape[-1]))
        neg = (negative_prompt_embeds, negative_pooled_prompt_embeds) if do_cfg else ()          # :800-807
        prompt_embeds, added = conditioning(dev, prompt_embeds, pooled_prompt_embeds, add_time_ids, *neg)

        B = latents.shape[0]
        if lcm:
            latents = self._lcm_sample(latents, prompt_embeds, added, num_inference_steps, guidance_scale, do_cfg, step_noise, noise_seed, generator, known_latents,
                                       edit_mask, cross_attention_kwargs, callback, callback_steps)
            image = self._output(latents, output_type)
            return StableDiffusionXLPipelineOutput(images=image) if return_dict else (image,)
        lv = None
        if known_trajectory is not None:
            known = known_trajectory.to(device=dev, dtype=torch.float16).contiguous()
            if tuple(known.shape) != (num_inference_steps + 1,) + tuple(latents.shape):
                raise ValueError(f"`known_trajectory` must be [num_inference_steps + 1 = {num_inference_steps + 1}, {', '.join(map(str, latents.shape))}], "
                                 f"got {tuple(known.shape)}")
            edit_mask = edit_mask.to(device=dev, dtype=torch.float16)
            if tuple(edit_mask.shape) not in ((1, 1) + tuple(latents.shape[-2:]), (B, 1) + tuple(latents.shape[-2:])):
                raise ValueError(f"`edit_mask` must be a latent mask [{B} or 1, 1, {latents.shape[-2]}, {latents.shape[-1]}], got {tuple(edit_mask.shape)}")
            edit_mask = edit_mask.expand(B, -1, -1, -1).contiguous()
            lv = level_table([[n] * B for n in range(num_inference_steps, -1, -1)], known.shape[0], dev)     # row 0: the start; row i + 1: after step i
            latents = known_blend_v(latents, known, lv[0], edit_mask, torch.empty_like(latents))
        if do_cfg:
            model_in = torch.cat([latents, latents], dim=0)                                     # :826 cat([latents]*2)
            eps = torch.empty_like(model_in)
            nxt_in = torch.empty_like(model_in)
        else:
            model_in, eps, nxt_in = latents, torch.empty_like(latents), torch.empty_like(latents)
        for i, t in enumerate(self.scheduler.timesteps):                                        # :824 descending t
            t = int(t)
            self.unet(model_in, t, encoder_hidden_states=prompt_embeds, cross_attention_kwargs=cross_attention_kwargs,
                      added_cond_kwargs=added, return_dict=False, out=eps)
            c_x, c_e = self.scheduler.step_coeffs(t)
            if do_cfg:                                                                          # :842-844 + :851 fused
                fused_update(model_in[:B], eps[:B], eps[B:], guidance_scale, c_x, c_e, nxt_in[:B], nxt_in[B:])
            else:
                fused_update(model_in, eps, None, 1.0, c_x, c_e, nxt_in)
            if lv is not None:                                                                  # outside the mask: the inverted latents of this noise level
                known_blend_v(nxt_in[:B], known, lv[i + 1], edit_mask, nxt_in[:B], nxt_in[B:] if do_cfg else None)
            model_in, nxt_in = nxt_in, model_in
            if callback is not None and i % callback_steps == 0:
                callback(i, t, model_in[:B])
        latents = model_in[:B]
        image = self._output(latents, output_type)                                              # :859-880
        return StableDiffusionXLPipelineOutput(images=image) if return_dict else (image,)

    def _lcm_sample(self, latents, ctx, added, steps, guidance_scale, do_cfg, step_noise, noise_seed, generator, known_latents, edit_mask, cross_attention_kwargs,
                    callback, callback_steps):
        """the serial call's rows as B requests of one schedule through `batch.lcm_sample`"""
        from .batch import lcm_sample                                                           # (batch.py imports this module)
        dev, B, steps = self.device, latents.shape[0], int(steps)
        rows = seeds = None
        if step_noise is not None:
            z = step_noise.reshape((steps - 1, -1) + tuple(latents.shape[1:])) if torch.is_tensor(step_noise) and step_noise.numel() == (steps - 1) * latents.numel() else None
            if z is None or step_noise.dtype != torch.float16:
                raise ValueError(f"`step_noise` must be an fp16 tensor [steps - 1 = {steps - 1}, {', '.join(map(str, latents.shape))}] (the batch axis may be left out for "
                                 f"one row), got {tuple(step_noise.shape) if torch.is_tensor(step_noise) else type(step_noise)}")
            rows = [z[:, b].contiguous() for b in range(B)]
        elif noise_seed is not None:
            seeds = _noise.batch_seeds(noise_seed, B)
        elif steps > 1:
            g = generator if not isinstance(generator, list) else generator[0]
            gen_dev = g.device if g is not None else torch.device("cpu")
            z = torch.stack([torch.randn(tuple(latents.shape), generator=g, device=gen_dev, dtype=torch.float16) for _ in range(steps - 1)])
            rows = [z[:, b].contiguous() for b in range(B)]
        if edit_mask is not None:
            known_latents = known_latents.to(device=dev, dtype=torch.float16).contiguous()
            edit_mask = edit_mask.to(device=dev, dtype=torch.float16)
            if tuple(known_latents.shape) != tuple(latents.shape) or tuple(edit_mask.shape) not in ((1, 1) + tuple(latents.shape[-2:]), (B, 1) + tuple(latents.shape[-2:])):
                raise ValueError(f"`known_latents` must have the latents' shape {tuple(latents.shape)} and `edit_mask` be a latent mask [{B} or 1, 1, {latents.shape[-2]}, "
                                 f"{latents.shape[-1]}], got {tuple(known_latents.shape)} and {tuple(edit_mask.shape)}")
            edit_mask = edit_mask.expand(B, -1, -1, -1).contiguous()
        cb = None if callback is None else (lambda i, t, x: callback(i, int(t), x) if i % callback_steps == 0 else None)
        return lcm_sample(self.unet, self.scheduler.config, latents, ctx, added, [steps] * B, [float(guidance_scale)] * B, do_cfg, rows, seeds, None, known_latents,
                          edit_mask, dict(cross_attention_kwargs=cross_attention_kwargs, return_dict=False), cb)


# ---- ControlNet: structure-guided sampling (diffusers 0.26.3 StableDiffusionXLControlNetPipeline) ---------------------------------------------------
def control_active(i: int, n: int, start: float, end: float) -> bool:
    """does step i of n run the ControlNet? diffusers' `control_guidance_start` / `control_guidance_end`: `controlnet_keep[i] = 1 - (i / n < start or (i + 1) / n > end)`"""
    return not (i / n < start or (i + 1) / n > end)


class ControlledUNet:
    """The (ControlNet, UNet) pair behind the UNet's call signature: evaluation i of a sampling loop of `steps` steps runs the ControlNet on the same inputs and the
    UNet with its residuals while the step lies in the control window, the plain UNet entry otherwise. The DDIM loop and `batch.lcm_sample` run it unchanged; every
    other attribute is the UNet's."""

    def __init__(self, unet, controlnet, image, scale, start, end, steps):
        self.unet, self.controlnet, self.image, self.scale, self.window, self.steps, self.calls = unet, controlnet, image, scale, (float(start), float(end)), int(steps), 0

    def __getattr__(self, name):            # (only what this object does not carry itself: config, device, add_embedding, lora, ...)
        return getattr(self.__dict__["unet"], name)

    def __call__(self, sample, timestep, encoder_hidden_states=None, cross_attention_kwargs=None, added_cond_kwargs=None, **kw):
        i, self.calls = self.calls, self.calls + 1
        if not control_active(i, self.steps, *self.window):
            return self.unet(sample, timestep, encoder_hidden_states=encoder_hidden_states, cross_attention_kwargs=cross_attention_kwargs,
                             added_cond_kwargs=added_cond_kwargs, **kw)
        down, mid = self.controlnet(sample, timestep, encoder_hidden_states=encoder_hidden_states, controlnet_cond=self.image, conditioning_scale=self.scale,
                                    added_cond_kwargs=added_cond_kwargs, return_dict=False)
        return self.unet(sample, timestep, encoder_hidden_states=encoder_hidden_states, cross_attention_kwargs=cross_attention_kwargs,
                         added_cond_kwargs=added_cond_kwargs, down_block_additional_residuals=down, mid_block_additional_residual=mid, **kw)


class StableDiffusionXLControlNetPipeline(StableDiffusionXLPipeline):
    """`StableDiffusionXLPipeline` with a `.controlnet` (a `HipControlNetModel` whose block_out_channels, layers_per_block and cross_attention_dim match the UNet's:
    refused here otherwise). `image=` is the condition map the caller brings (edges, depth, pose, a sketch; no detector runs here): a float tensor or array in [0, 1],
    [B or 1, 3, H, W] with H x W the sampled image's size, 8 x the latent grid. With classifier-free guidance it is repeated for both halves. `image=None`,
    `controlnet_conditioning_scale=0` or a control window that holds no step run today's `StableDiffusionXLPipeline` call: no ControlNet launch, the plain UNet
    entry, the same bits. Multi-ControlNet, `guess_mode=True` and T2I-Adapters are not built."""

    def __init__(self, unet, controlnet, *a, **kw):
        super().__init__(unet, *a, **kw)
        controlnet.check_unet(unet)
        self.controlnet = controlnet

    @torch.no_grad()
    def __call__(self, *a, image=None, controlnet_conditioning_scale=1.0, control_guidance_start: float = 0.0, control_guidance_end: float = 1.0,
                 guess_mode: bool = False, **kw):
        if guess_mode:
            raise ValueError("guess_mode=True is not supported")
        if isinstance(controlnet_conditioning_scale, (list, tuple)) or isinstance(control_guidance_start, (list, tuple)) or isinstance(control_guidance_end, (list, tuple)):
            raise ValueError("one ControlNet: controlnet_conditioning_scale, control_guidance_start and control_guidance_end are single numbers")
        start, end = float(control_guidance_start), float(control_guidance_end)
        if not (0.0 <= start <= 1.0 and 0.0 <= end <= 1.0) or start > end:
            raise ValueError(f"control guidance window [{start}, {end}] must lie in [0, 1] with start <= end")
        steps = int(kw.get("num_inference_steps", a[3] if len(a) > 3 else 50))
        scale = controlnet_conditioning_scale
        off = image is None or (not torch.is_tensor(scale) and float(scale) == 0.0) or not any(control_active(i, steps, start, end) for i in range(steps))
        if off:
            return super().__call__(*a, **kw)
        if kw.get("cross_attention_kwargs") and kw["cross_attention_kwargs"].get("ip_adapter_masks") is not None:
            raise ValueError("ControlNet residuals together with ip_adapter_masks: the regional pass is not combined with a ControlNet")
        cond = torch.as_tensor(image)
        if cond.ndim == 3:
            cond = cond[None]
        if cond.ndim != 4 or cond.shape[1] != self.controlnet.config.conditioning_channels or not cond.is_floating_point():
            raise ValueError(f"`image` must be a float condition map [B or 1, {self.controlnet.config.conditioning_channels}, H, W] in [0, 1]; got {tuple(cond.shape)} {cond.dtype}")
        lat = kw.get("latents")
        if lat is not None:
            hw = (lat.shape[-2] * self.vae_scale_factor, lat.shape[-1] * self.vae_scale_factor)
        else:
            ss = getattr(self.unet.config, "sample_size", 128) * self.vae_scale_factor
            hw = (kw.get("height") or (a[1] if len(a) > 1 else None) or ss, kw.get("width") or (a[2] if len(a) > 2 else None) or ss)
        if tuple(cond.shape[-2:]) != tuple(hw) or self.vae_scale_factor != 8:
            raise ValueError(f"the condition image is {cond.shape[-2]} x {cond.shape[-1]}; the sampled image is {hw[0]} x {hw[1]} (8 x the latent grid)")
        cond = cond.to(device=self.device, dtype=torch.float16).contiguous()
        plain = self.unet
        self.unet = ControlledUNet(plain, self.controlnet, cond, scale, start, end, steps)
        try:
            return super().__call__(*a, **kw)
        finally:
            self.unet = plain
