"""ControlNet on the MI355X: the HIP ControlNet against tests/controlnet_ref.ControlNetRef, the UNet with residuals against UNetWithResidualsRef under every GroupNorm mode,
the control-off paths on the bits, the controlled DDIM loop against oracle.sample_loop, the LCM sampler, the top-level pipeline and the refusals.
Tolerances are test_unet_gpu.py's for forwards and loops (rel-L2 <= 3e-2, cos >= 0.999); zero-valued residuals within 2e-3 rel-L2 of the plain output (the bound
test_region_unet_gpu.py uses between two routes whose statistics are summed differently)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import controlnet_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL, COS = 3e-2, 0.999


def metrics(a, b):
    a, b = a.float().cpu().reshape(-1), b.float().cpu().reshape(-1)
    return float((a - b).norm() / b.norm()), float(torch.dot(a, b) / (a.norm() * b.norm()))


def close(a, b, what=""):
    r, c = metrics(a, b)
    print(f"[controlnet] {what}: rel-L2 {r:.3g}, cos {c:.6f}")
    assert bool(torch.isfinite(a.float()).all()) and r <= REL and c >= COS, (what, r, c)


class Models:
    def __init__(self):
        from instructany2pix_amd.config import tiny, tiny_controlnet
        from instructany2pix_amd.controlnet import HipControlNetModel
        from instructany2pix_amd.unet import HipUNet2DConditionModel
        from instructany2pix_amd.weights import controlnet_param_specs, ip_adapter_specs, synthetic_state_dict, unet_param_specs
        self.ucfg, self.ccfg = tiny(), tiny_controlnet()
        self.usd = synthetic_state_dict(unet_param_specs(self.ucfg), seed=7)
        self.csd = synthetic_state_dict(controlnet_param_specs(self.ccfg), seed=9)
        specs = ip_adapter_specs(self.ucfg, 64)
        self.ck = {"image_proj": synthetic_state_dict(specs["image_proj"], seed=7), "ip_adapter": synthetic_state_dict(specs["ip_adapter"], seed=7)}
        self.unet = HipUNet2DConditionModel(self.ucfg, DEV)
        self.unet.load_state_dict(self.usd)
        self.cn = HipControlNetModel(self.ccfg, DEV)
        self.cn.load_state_dict(self.csd)
        self._refs = {}

    def plain_unet(self):
        from instructany2pix_amd.attention_processor import AttnProcessor2_0
        self.unet.set_attn_processor(AttnProcessor2_0())
        return self.unet

    def ref_cn(self, num_tokens):
        return CR.build_controlnet(self.ccfg, self.csd, num_tokens)

    def ref_unet(self, ip_scale=None):
        if ip_scale not in self._refs:
            self._refs[ip_scale] = CR.build_unet_with_residuals(self.ucfg, self.usd, *(() if ip_scale is None else (self.ck["ip_adapter"], ip_scale)))
        return self._refs[ip_scale]


@pytest.fixture(scope="module")
def m():
    mm = Models()
    yield mm
    from instructany2pix_amd import _ffi
    _ffi.lib().ia2p_debug_set_gn_plan(-1)


def _inputs(cfg, B, h, w, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, h, w, generator=g).half()
    ctx = torch.randn(B, L, cfg.cross_attention_dim, generator=g).half()
    te = torch.randn(B, cfg.pooled_dim, generator=g).half()
    tid = torch.tensor([[h * 8.0, w * 8.0, 0, 0, h * 8.0, w * 8.0]] * B).half()
    cond = torch.rand(B, 3, 8 * h, 8 * w, generator=g).half()
    return x, ctx, te, tid, cond


def _added(te, tid, f=lambda t: t.to(DEV)):
    return dict(text_embeds=f(te), time_ids=f(tid))


# ---- 1. the ControlNet forward ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(16, 16), (16, 24)])
def test_controlnet_forward_vs_reference(m, h, w):
    """B = 2, per-row scales (0.6, 1.3), an 81-row context of which the ControlNet sees 77 (the four image-token rows are loud: a ControlNet that read them would
    not match); every one of the ten residuals on its own; both routes to the context K/V"""
    B, L = 2, 81
    x, ctx, te, tid, cond = _inputs(m.ucfg, B, h, w, L, seed=h * w)
    ctx[:, 77:] *= 6.0
    scales = torch.tensor([0.6, 1.3])
    m.cn.set_image_tokens(4)
    try:
        with torch.no_grad():
            ref_d, ref_m = m.ref_cn(4)(x.float(), 501, ctx.float(), cond.float(), scales, added_cond_kwargs=_added(te, tid, lambda t: t.float()))
            all_d, all_m = m.ref_cn(0)(x.float(), 501, ctx.float(), cond.float(), scales, added_cond_kwargs=_added(te, tid, lambda t: t.float()))
        emb_ref = None
        outs = {}
        for cache in (True, False):
            m.cn.cache_context_kv = cache
            down, mid = m.cn(x.to(DEV), 501, encoder_hidden_states=ctx.to(DEV), controlnet_cond=cond.to(DEV), conditioning_scale=scales, added_cond_kwargs=_added(te, tid))
            torch.cuda.synchronize()
            assert len(down) == 9
            for k, (got, ref) in enumerate(zip(list(down) + [mid], ref_d + [ref_m])):
                assert tuple(got.shape) == tuple(ref.shape) and got.permute(0, 2, 3, 1).is_contiguous()          # logical NCHW, channels-last strides: a view of the buffer
                close(got, ref, f"{h}x{w} kv cache {cache} residual {k}")
            outs[cache] = [t.clone() for t in list(down) + [mid]]
        for a, b in zip(outs[True], outs[False]):
            assert torch.equal(a, b), "the two K/V routes give other bits"
        r, c = metrics(outs[True][-1], all_m)
        print(f"[controlnet] {h}x{w} against a reference that sees all 81 rows: rel-L2 {r:.3g}, cos {c:.6f}")
        assert r > REL, "the match survives a reference that sees the image-token rows: the ControlNet read them"
        # the embedded condition on its own, and handed in embedded
        e = m.cn.embed_condition(cond.to(DEV))
        with torch.no_grad():
            emb_ref = m.ref_cn(4).controlnet_cond_embedding(cond.float())
        close(e.permute(0, 3, 1, 2), emb_ref, f"{h}x{w} condition embedding")
        d2, m2 = m.cn(x.to(DEV), 501, encoder_hidden_states=ctx.to(DEV), controlnet_cond=e, conditioning_scale=scales, added_cond_kwargs=_added(te, tid))
        assert torch.equal(m2, outs[True][-1]) and all(torch.equal(a, b) for a, b in zip(d2, outs[True][:-1]))
    finally:
        m.cn.cache_context_kv = True
        m.cn.set_image_tokens(0)


# ---- 2. the UNet with residuals -----------------------------------------------------------------------------------------------------------------------------------
def _random_residuals(m, x, ctx, te, tid, seed, zero=False):
    """residuals scaled to the skips' magnitude (the reference's own skips), as logical-NCHW tensors: even ones contiguous NCHW (converted by the call), odd ones with
    channels-last strides (passed by pointer)"""
    ref = m.ref_unet()
    with torch.no_grad():
        emb = CR._embeddings(ref, m.ucfg, x.float(), 301, _added(te, tid, lambda t: t.float()))
        skips, mid = CR._down_and_mid(ref, ref.conv_in(x.float()), emb, ctx.float())
    g = torch.Generator().manual_seed(seed)
    res = [(torch.zeros_like(s) if zero else torch.randn(s.shape, generator=g) * float(s.std())).half() for s in skips + [mid]]
    dev = [r.to(DEV) if k % 2 == 0 else r.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for k, r in enumerate(res)]
    return res, dev


@pytest.mark.parametrize("plan,h", [(-1, 16), (1, 32)])
def test_unet_with_residuals_under_every_groupnorm_mode(m, plan, h):
    """plan 1: every eligible 3x3 site fuses its GroupNorm, so the up path reads the injected skips' statistics from the injection launch"""
    from instructany2pix_amd import _ffi
    unet = m.plain_unet()
    B, L = 2, 77
    x, ctx, te, tid, _ = _inputs(m.ucfg, B, h, h, L, seed=5 + h)
    res, dev = _random_residuals(m, x, ctx, te, tid, seed=11)
    kw = dict(encoder_hidden_states=ctx.to(DEV), added_cond_kwargs=_added(te, tid))
    with torch.no_grad():
        ref = m.ref_unet()(x.float(), 301, ctx.float(), added_cond_kwargs=_added(te, tid, lambda t: t.float()),
                           down_block_additional_residuals=[r.float() for r in res[:-1]], mid_block_additional_residual=res[-1].float())[0]
    _ffi.lib().ia2p_debug_set_gn_plan(plan)
    out = {}
    try:
        for mode in (0, 1, 2):
            unet.set_gn_fuse(mode)
            plain = unet(x.to(DEV), 301, **kw)[0].clone()
            out[mode] = unet(x.to(DEV), 301, down_block_additional_residuals=dev[:-1], mid_block_additional_residual=dev[-1], **kw)[0].clone()
            close(out[mode], ref, f"UNet with residuals, plan {plan}, GroupNorm mode {mode}")
            assert metrics(out[mode], plain)[0] > REL, "the residuals do not move the output"
            again = unet(x.to(DEV), 301, **kw)[0]
            assert torch.equal(again, plain), "a plain call after a controlled one returns other bits"
        assert torch.equal(out[1], out[2]), "GroupNorm modes 1 and 2 give other bits"
    finally:
        unet.set_gn_fuse(1)
        _ffi.lib().ia2p_debug_set_gn_plan(-1)


@pytest.mark.parametrize("plan,h", [(-1, 16), (1, 32)])
def test_zero_valued_residuals_are_the_plain_output(m, plan, h):
    from instructany2pix_amd import _ffi
    unet = m.plain_unet()
    x, ctx, te, tid, _ = _inputs(m.ucfg, 2, h, h, 77, seed=8)
    _, dev = _random_residuals(m, x, ctx, te, tid, seed=1, zero=True)
    kw = dict(encoder_hidden_states=ctx.to(DEV), added_cond_kwargs=_added(te, tid))
    _ffi.lib().ia2p_debug_set_gn_plan(plan)
    try:
        for mode in (0, 1, 2):
            unet.set_gn_fuse(mode)
            plain = unet(x.to(DEV), 301, **kw)[0].clone()
            zero = unet(x.to(DEV), 301, down_block_additional_residuals=dev[:-1], mid_block_additional_residual=dev[-1], **kw)[0]
            r = metrics(zero, plain)[0]
            print(f"[controlnet] zero residuals, plan {plan}, mode {mode}: rel-L2 {r:.3g}")
            assert r <= 2e-3, (plan, mode, r)
            none = unet(x.to(DEV), 301, down_block_additional_residuals=None, mid_block_additional_residual=None, **kw)[0]
            assert torch.equal(none, plain)
    finally:
        unet.set_gn_fuse(1)
        _ffi.lib().ia2p_debug_set_gn_plan(-1)


# ---- 3. the loops -------------------------------------------------------------------------------------------------------------------------------------------------
def _loop_setup(m, seed=21, h=16, w=16):
    from instructany2pix_amd.ddim import StableDiffusionXLControlNetPipeline, StableDiffusionXLPipeline
    from instructany2pix_amd.ip_adapter import IPAdapterXL
    cfg = m.ucfg
    pipe = StableDiffusionXLControlNetPipeline(m.unet, m.cn)
    ipa = IPAdapterXL(pipe, "", ip_ckpt=m.ck, device=DEV, clip_embeddings_dim=64)
    assert m.cn.num_tokens == 4                                   # set_ip_adapter told the ControlNet
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(64, generator=g)
    ctx, nctx = torch.randn(1, 77, cfg.cross_attention_dim, generator=g).half(), torch.randn(1, 77, cfg.cross_attention_dim, generator=g).half()
    pooled, npooled = torch.randn(1, cfg.pooled_dim, generator=g).half(), torch.randn(1, cfg.pooled_dim, generator=g).half()
    xT = torch.randn(1, 4, h, w, generator=g).half()
    cond = torch.rand(1, 3, 8 * h, 8 * w, generator=g).half()
    kw = dict(clip_image_embeds=emb, prompt_embeds=ctx, negative_prompt_embeds=nctx, pooled_prompt_embeds=pooled, negative_pooled_prompt_embeds=npooled, latents=xT,
              height=h * 8, width=w * 8, output_type="latent")
    plain_pipe = StableDiffusionXLPipeline(m.unet)
    return pipe, ipa, plain_pipe, kw, (emb, ctx, nctx, pooled, npooled, xT, cond)


def test_controlled_ddim_loop_vs_oracle_and_control_off_on_the_bits(m):
    import oracle
    pipe, ipa, plain_pipe, kw, (emb, ctx, nctx, pooled, npooled, xT, cond) = _loop_setup(m)
    N, scale, window = 10, 0.8, (0.2, 0.8)
    try:
        lat = ipa.generate(num_inference_steps=N, scale=0.7, guidance_scale=7.5, image=cond, controlnet_conditioning_scale=scale, control_guidance_start=window[0],
                           control_guidance_end=window[1], **kw)
        proj = oracle.ImageProjModelRef(m.ucfg.cross_attention_dim, 64, 4)
        proj.load_state_dict({k: v.float() for k, v in m.ck["image_proj"].items()})
        e = torch.stack([emb.half().float()[None], torch.zeros(1, 64)], dim=1)
        tid = torch.tensor([[128.0, 128.0, 0, 0, 128.0, 128.0]])
        with torch.no_grad():
            p, n = proj(e, "global"), proj(torch.zeros_like(e), "global")
            pair = CR.ControlledRef(m.ref_unet(0.7), m.ref_cn(4), cond.float(), scale, window[0], window[1], N)
            ref = oracle.sample_loop(pair, oracle.DDIMSchedulerRef(), xT.float(), torch.cat([ctx.float(), p], 1), dict(text_embeds=pooled.float(), time_ids=tid), N, 7.5,
                                     torch.cat([nctx.float(), n], 1), dict(text_embeds=npooled.float(), time_ids=tid))
            assert pair.calls == N
            free = oracle.sample_loop(m.ref_unet(0.7), oracle.DDIMSchedulerRef(), xT.float(), torch.cat([ctx.float(), p], 1), dict(text_embeds=pooled.float(), time_ids=tid), N,
                                      7.5, torch.cat([nctx.float(), n], 1), dict(text_embeds=npooled.float(), time_ids=tid))
        close(lat, ref, "controlled DDIM loop, steps 2..7 of 10 active")
        assert metrics(lat, free)[0] > REL, "the control does not move the loop"
        # control off, three ways: today's call of StableDiffusionXLPipeline on the same inputs, bit for bit
        ipa_plain = ipa
        ipa_plain.pipe = plain_pipe
        today = ipa_plain.generate(num_inference_steps=N, scale=0.7, guidance_scale=7.5, **kw).clone()
        ipa.pipe = pipe
        for what, off in (("image=None", dict()), ("scale 0", dict(image=cond, controlnet_conditioning_scale=0.0)),
                          ("empty window", dict(image=cond, control_guidance_start=0.5, control_guidance_end=0.5))):
            got = ipa.generate(num_inference_steps=N, scale=0.7, guidance_scale=7.5, **off, **kw)
            assert torch.equal(got, today), f"control off ({what}) is not today's call on the bits"
        close(today, free, "the uncontrolled loop")
        # refusals of the pipeline, before any launch
        with pytest.raises(ValueError, match="guess_mode"):
            ipa.generate(num_inference_steps=N, image=cond, guess_mode=True, **kw)
        with pytest.raises(ValueError, match="8 x the latent grid"):
            ipa.generate(num_inference_steps=N, image=cond[..., :120], **kw)
    finally:
        ipa.disable()
        assert m.cn.num_tokens == 0


def test_lcm_sampler_composes(m):
    from instructany2pix_amd.scheduler import LCMScheduler
    pipe, ipa, plain_pipe, kw, (emb, ctx, nctx, pooled, npooled, xT, cond) = _loop_setup(m, seed=23)
    try:
        pipe.scheduler = LCMScheduler.from_config(pipe.scheduler.config)
        a = ipa.generate(num_inference_steps=4, scale=0.7, guidance_scale=7.5, noise_seed=5, image=cond, controlnet_conditioning_scale=0.8, **kw).clone()
        b = ipa.generate(num_inference_steps=4, scale=0.7, guidance_scale=7.5, noise_seed=5, **kw)
        assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all())
        assert not torch.equal(a, b) and metrics(a, b)[0] > 1e-2
    finally:
        ipa.disable()


# ---- 4. the top level ---------------------------------------------------------------------------------------------------------------------------------------------
def test_top_level_pipeline(m):
    from instructany2pix_amd.config import tiny_refiner
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    g = torch.Generator().manual_seed(31)
    rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    b = m.ucfg
    c = dict(image_embeds=rn(1, 64), base_embed=rn(1, 64), y=rn(1, 64), caption="a photo", base_latents=rn(1, 4, 16, 16).half(),
             prompt_embeds=rn(1, 77, b.cross_attention_dim).half(), pooled_prompt_embeds=rn(1, b.pooled_dim).half(),
             negative_prompt_embeds=rn(1, 77, b.cross_attention_dim).half(), negative_pooled_prompt_embeds=rn(1, b.pooled_dim).half(), polar_noise=rn(1, 4, 16, 16).half())
    pipe = InstructAny2PixPipeline(unet=m.unet, ip_ckpt=m.ck, device=DEV, clip_embeddings_dim=64, conditioner=lambda inst, mm, use_cache=False: c, controlnet=m.cn)
    pipe.ip_adapter_xl.set_scale(1.0)
    cond = (torch.rand(128, 128, 3, generator=g) * 255).to(torch.uint8).numpy()
    try:
        kw = dict(num_inference_steps=3, refinement=0, seed=11)
        plain = pipe("edit", [], **kw)[0].clone()
        ctl = pipe("edit", [], control_image=cond, control_scale=0.9, **kw)[0].clone()
        assert bool(torch.isfinite(ctl.float()).all()) and metrics(ctl, plain)[0] > 1e-2, "control_image does not change the result"
        assert torch.equal(pipe("edit", [], control_image=cond, control_scale=0.0, **kw)[0], plain)
        assert torch.equal(pipe("edit", [], control_image=None, **kw)[0], plain)
        mask = torch.zeros(1, 1, 16, 16)
        mask[..., 4:12, 4:12] = 1.0
        masked = pipe("edit", [], control_image=cond, edit_mask=mask, **kw)[0]
        base = c["base_latents"].to(masked.device)
        keep = (mask == 0).expand_as(base).to(masked.device)
        assert torch.equal(masked[keep], base[keep]), "outside the edit mask the base latents' bits are gone"
        assert not torch.equal(masked[~keep], base[~keep])
        with pytest.raises(ValueError, match="8 x the latent grid"):
            pipe("edit", [], control_image=cond[:120], **kw)
        bare = InstructAny2PixPipeline(unet=m.unet, ip_ckpt=m.ck, device=DEV, clip_embeddings_dim=64, conditioner=lambda inst, mm, use_cache=False: c)
        with pytest.raises(ValueError, match="controlnet="):
            bare("edit", [], control_image=cond, **kw)
        bare.ip_adapter_xl.disable()
    finally:
        pipe.ip_adapter_xl.disable()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(m):
    from instructany2pix_amd import _ffi
    from instructany2pix_amd.config import tiny
    from instructany2pix_amd.ddim import StableDiffusionXLControlNetPipeline
    from instructany2pix_amd.unet import HipUNet2DConditionModel
    unet = m.plain_unet()
    x, ctx, te, tid, cond = _inputs(m.ucfg, 2, 16, 16, 77, seed=2)
    kw = dict(encoder_hidden_states=ctx.to(DEV), added_cond_kwargs=_added(te, tid))
    unet(x.to(DEV), 300, **kw)
    L_ = unet._lib
    t, ts, p = torch.zeros(1 << 16, dtype=torch.half, device=DEV), torch.zeros(2, device=DEV), _ffi.ptr
    n = L_.ia2p_unet_num_skips(unet._ctx)
    assert n == 9
    ptrs = lambda k, hole=None: (C.c_void_p * k)(*[None if i == hole else t.data_ptr() for i in range(k)])      # noqa: E731
    call = lambda down, k, mid, masks=None, G=0: L_.ia2p_unet_forward_c(unet._ctx, _ffi.current_stream(), p(t), p(ts), None, p(t), None, 77, p(t), p(t), p(t), 2, 16, 16,      # noqa: E731
                                                                         p(t), 2 * t.numel(), down, k, mid, masks, G)
    assert call(None, n, p(t)) == 1 and call(ptrs(n), n, None) == 1 and call(ptrs(n, hole=4), n, p(t)) == 1          # a null pointer
    assert call(ptrs(n - 1), n - 1, p(t)) == 2 and b"skips" in L_.ia2p_last_error(unet._ctx)                       # a wrong residual count
    assert call(ptrs(n + 1), n + 1, p(t)) == 2
    assert call(ptrs(n), n, p(t), p(t), 1) == 1 and b"region_masks" in L_.ia2p_last_error(unet._ctx)               # residuals together with region masks
    assert L_.ia2p_workspace_bytes_c(unet._ctx, 2, 16, 16, 77) == L_.ia2p_workspace_bytes(unet._ctx, 2, 16, 16, 77) > 0
    assert L_.ia2p_workspace_bytes_c(unet._ctx, 2, 15, 16, 77) == 0
    # a ControlNet handle at the UNet's entry, and the other way round
    assert L_.ia2p_unet_forward_v(m.cn._h, _ffi.current_stream(), p(t), p(ts), None, p(t), None, 77, p(t), p(t), p(t), 2, 16, 16, p(t), 2 * t.numel()) == 4
    assert L_.ia2p_controlnet_forward(unet._ctx, _ffi.current_stream(), p(t), p(ts), p(t), None, 77, p(t), p(t), p(t), p(ts), p(t), 2 * t.numel(), 2, 16, 16, p(t), 2 * t.numel()) == 4
    # a ControlNet context that still holds the image-token rows: nothing is left of a 4-row context under 4 image tokens
    m.cn.set_image_tokens(4)
    try:
        assert L_.ia2p_controlnet_forward(m.cn._h, _ffi.current_stream(), p(t), p(ts), p(t), None, 4, p(t), p(t), p(t), p(ts), p(t), 2 * t.numel(), 2, 16, 16, p(t), 2 * t.numel()) == 2
    finally:
        m.cn.set_image_tokens(0)
    torch.cuda.synchronize()
    assert bool((t == 0).all()), "a refused call wrote"
    # the Python surface: ValueError before any launch
    down, mid = m.cn(x.to(DEV), 300, controlnet_cond=cond.to(DEV), **kw)
    with pytest.raises(ValueError, match="skips"):
        unet(x.to(DEV), 300, down_block_additional_residuals=list(down)[:-1], mid_block_additional_residual=mid, **kw)
    with pytest.raises(ValueError, match="ip_adapter_masks"):
        unet(x.to(DEV), 300, down_block_additional_residuals=down, mid_block_additional_residual=mid, cross_attention_kwargs=dict(ip_adapter_masks=torch.ones(2, 1, 16, 16)), **kw)
    with pytest.raises(ValueError, match="guess_mode"):
        m.cn(x.to(DEV), 300, controlnet_cond=cond.to(DEV), guess_mode=True, **kw)
    with pytest.raises(ValueError, match="controlnet_cond must be"):
        m.cn(x.to(DEV), 300, controlnet_cond=cond[..., :120].to(DEV), **kw)                                         # an image that is not 8h x 8w
    other = tiny()
    other.block_out_channels, other.attention_head_dim = (64, 128, 320), (1, 2, 5)
    with pytest.raises(ValueError, match="must match the UNet"):
        StableDiffusionXLControlNetPipeline(HipUNet2DConditionModel(other, DEV), m.cn)
