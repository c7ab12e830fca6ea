"""Regional image prompts through the executor and the Python layers: `ia2p_unet_forward_r` (cross_attention_kwargs={"ip_adapter_masks": ...}), the joint subject pass
of `IPAdapterXL.generate(joint=True)` / `subject_consistency(joint=True)`, `inpaint_batch` on requests that carry several subjects and `edit_batch(subject_modes=)`.

The oracle is `oracle.build_unet` with the regional processor of tests/region_unet_ref.py installed through `set_attn_processor`. config.tiny() and synthetic weights, as
tests/test_inpaint_gpu.py builds them; tolerances as in test_unet_gpu.py's loops: rel-L2 <= 3e-2, cos >= 0.999."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import region_unet_ref as RU  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 0.8


def _metrics(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return float((a - b).norm() / b.norm()), float(torch.dot(a, b) / (a.norm() * b.norm()))


@pytest.fixture(scope="module")
def models():
    import oracle
    from instructany2pix_amd.config import tiny
    from instructany2pix_amd.inpaint import StableDiffusionXLInpaintPipeline
    from instructany2pix_amd.ip_adapter import IPAdapterXL
    from instructany2pix_amd.unet import HipUNet2DConditionModel
    from instructany2pix_amd.weights import ip_adapter_specs, synthetic_state_dict, unet_param_specs
    cfg = tiny()
    sd = synthetic_state_dict(unet_param_specs(cfg), seed=7)
    specs = ip_adapter_specs(cfg, 64)
    ck = {"image_proj": synthetic_state_dict(specs["image_proj"], seed=7), "ip_adapter": synthetic_state_dict(specs["ip_adapter"], seed=7)}
    hip = HipUNet2DConditionModel(cfg, DEV)
    hip.load_state_dict(sd)
    pipe = StableDiffusionXLInpaintPipeline(hip)
    ipa = IPAdapterXL(pipe, "", ip_ckpt=ck, device=DEV, clip_embeddings_dim=64)
    ipa.set_scale(SCALE)
    proj = oracle.ImageProjModelRef(cfg.cross_attention_dim, 64, 4)
    proj.load_state_dict({k: v.float() for k, v in ck["image_proj"].items()})
    net, holder = RU.build_regional_unet(oracle, cfg, sd, ck["ip_adapter"], SCALE)
    return cfg, hip, pipe, ipa, proj, net, holder, oracle


def _region_masks(G, h, w, B, seed, soft=False):
    """[B, G, h, w]: overlapping rectangles on the latent grid, the rows different; soft: values in [0, 1]"""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(B, G, h, w)
    for b in range(B):
        for k in range(G):
            y0, x0 = int(torch.randint(0, h // 2, (1,), generator=g)), int(torch.randint(0, w // 2, (1,), generator=g))
            m[b, k, y0:y0 + h // 2 + 1, x0:x0 + w // 2 + 1] = 1.0
    if soft:
        m = m * torch.rand(B, G, h, w, generator=g)
    return m.half()


def _inputs(cfg, B, hw, G, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    return (rn(B, 4, hw, hw).half(), rn(B, 77 + 4 * G, cfg.cross_attention_dim).half(), rn(B, cfg.pooled_dim).half(),
            torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]] * B).half())


@pytest.mark.parametrize("hw,G,soft", [(16, 3, False), (16, 16, True), (32, 3, True), (32, 16, False)])
def test_one_forward_vs_oracle_both_kv_routes(models, hw, G, soft):
    """B = 2; 16 x 16 latents attend on 8 x 8 and 4 x 4, 32 x 32 on 16 x 16 (256 tokens) and 8 x 8. Through `context=` and through cached `kv=`"""
    cfg, hip, pipe, ipa, proj, net, holder, oracle = models
    x, ctx, te, tid = _inputs(cfg, 2, hw, G, 100 * hw + G)
    m = _region_masks(G, hw, hw, 2, 7 * hw + G, soft)
    kw = dict(encoder_hidden_states=ctx.to(DEV), added_cond_kwargs=dict(text_embeds=te.to(DEV), time_ids=tid.to(DEV)))
    outs, plain = {}, {}
    try:
        for cache in (True, False):
            hip.cache_context_kv = cache
            hip.invalidate_context_kv()
            outs[cache] = hip(x.to(DEV), 500, cross_attention_kwargs={"ip_adapter_masks": m.to(DEV)}, **kw)[0].clone()
            hip.invalidate_context_kv()
            plain[cache] = hip(x.to(DEV), torch.full((2,), 500.0), **kw)[0].clone()      # today's per-row path, num_tokens 4: the last 4 rows are image tokens
    finally:
        hip.cache_context_kv = True
        hip.invalidate_context_kv()
    holder.masks = m.float()
    with torch.no_grad():
        ref = net(x.float(), 500, ctx.float(), added_cond_kwargs=dict(text_embeds=te.float(), time_ids=tid.float()))[0]
    for cache, out in outs.items():
        rel, cos = _metrics(out, ref)
        print(f"[region-unet] forward hw={hw} G={G} cached kv={cache}: rel-L2 {rel:.3e} cos {cos:.6f}")
        assert rel <= 3e-2 and cos >= 0.999, (cache, rel, cos)
    assert not torch.equal(outs[True], plain[True])
    if torch.equal(plain[True], plain[False]):      # the two routes agree to the bit where today's plain path does
        assert torch.equal(outs[True], outs[False])
    else:
        assert _metrics(outs[True], outs[False])[0] < 2e-3


def test_state_is_restored(models):
    cfg, hip, pipe, ipa, proj, net, holder, oracle = models
    x, ctx, te, tid = _inputs(cfg, 2, 16, 3, 5)
    kw = dict(encoder_hidden_states=ctx.to(DEV), added_cond_kwargs=dict(text_embeds=te.to(DEV), time_ids=tid.to(DEV)))
    a = hip(x.to(DEV), 300, **kw)[0].clone()
    sig = hip._ip_sig
    r = hip(x.to(DEV), 300, cross_attention_kwargs={"ip_adapter_masks": _region_masks(3, 16, 16, 2, 1).to(DEV)}, **kw)[0].clone()
    assert hip._ip_sig == sig and sig[2] == 4 and all(p.num_tokens == 4 for n, p in hip.attn_processors.items() if n.endswith("attn2.processor"))
    b = hip(x.to(DEV), 300, **kw)[0].clone()
    assert torch.equal(a, b) and not torch.equal(a, r)
    with pytest.raises(ValueError):
        hip(x.to(DEV), 300, cross_attention_kwargs={"ip_adapter_masks": torch.zeros(2, 3, 8, 8)}, **kw)      # not the latent grid of `sample`
    with pytest.raises(ValueError):
        hip(x.to(DEV), 300, cross_attention_kwargs={"ip_adapter_masks": torch.zeros(2, 17, 16, 16)}, **kw)
    assert torch.equal(hip(x.to(DEV), 300, **kw)[0], a)


def _subjects(S, seed, hw=16):
    """S pixel-space masks (8 x the latent grid), overlapping rectangles, and S embeddings"""
    g = torch.Generator().manual_seed(seed)
    masks = []
    for k in range(S):
        mk = torch.zeros(hw * 8, hw * 8)
        mk[16 * k + 8:16 * k + 72, 24 + 8 * k:104 - 8 * k] = 1.0
        masks.append(mk)
    return masks, torch.randn(S, 64, generator=g)


def _cond(cfg, seed, hw=16):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    return dict(prompt_embeds=rn(1, 77, cfg.cross_attention_dim).half(), negative_prompt_embeds=rn(1, 77, cfg.cross_attention_dim).half(),
                pooled_prompt_embeds=rn(1, cfg.pooled_dim).half(), negative_pooled_prompt_embeds=rn(1, cfg.pooled_dim).half()), rn(1, 4, hw, hw).half(), rn(1, 4, hw, hw).half()


def test_joint_loop_vs_oracle(models):
    """S = 3 subjects, strength 0.7, 10 steps, guidance 7.5, one loop, against oracle.inpaint_loop under the regional processor"""
    cfg, hip, pipe, ipa, proj, net, holder, oracle = models
    emb, lat, noise = _cond(cfg, 21)
    masks, e = _subjects(3, 22)
    out = ipa.generate(latents=lat, mask_image=masks, pil_image=None, strength=0.7, clip_image_embeds_local=e, mode="local", joint=True, num_inference_steps=10,
                       scale=SCALE, guidance_scale=7.5, noise=noise, output_type="latent", **emb)
    torch.cuda.synchronize()
    ee = torch.stack([torch.zeros(3, 64), e.half().float()], dim=1)
    tid = torch.tensor([[128.0, 128.0, 0, 0, 128.0, 128.0]])
    regions = torch.stack([torch.nn.functional.interpolate((mk >= 0.5).float()[None, None], size=(16, 16))[0, 0] for mk in masks])
    holder.masks = regions
    union = torch.stack(masks).amax(0)[None, None]
    with torch.no_grad():
        p, n_ = proj(ee, "local", [1.0, 0.5]).reshape(1, 12, -1), proj(torch.zeros_like(ee), "local").reshape(1, 12, -1)
        ref = oracle.inpaint_loop(net, oracle.DDIMSchedulerRef(), lat.float(), noise.float(), union, torch.cat([emb["prompt_embeds"].float(), p], 1),
                                  dict(text_embeds=emb["pooled_prompt_embeds"].float(), time_ids=tid), 10, 0.7, 7.5, torch.cat([emb["negative_prompt_embeds"].float(), n_], 1),
                                  dict(text_embeds=emb["negative_pooled_prompt_embeds"].float(), time_ids=tid))
    rel, cos = _metrics(out, ref)
    print(f"[region-unet] joint loop: rel-L2 {rel:.3e} cos {cos:.6f}")
    assert rel <= 3e-2 and cos >= 0.999, (rel, cos)
    keep = (regions.amax(0) < 0.5)[None, None].expand_as(out)      # outside the union the input latents come back bit for bit
    assert bool(keep.any()) and torch.equal(out.cpu()[keep], lat[keep]) and not torch.equal(out.cpu()[~keep], lat[~keep])


def test_one_subject_joint_is_the_serial_call(models):
    """S = 1 and a region weight that covers everything: the regional formula is the plain one"""
    cfg, hip, pipe, ipa, proj, net, holder, oracle = models
    emb, lat, noise = _cond(cfg, 31)
    full, e = torch.ones(128, 128), torch.randn(1, 64, generator=torch.Generator().manual_seed(32))
    kw = dict(latents=lat, pil_image=None, strength=0.7, clip_image_embeds_local=e, mode="local", num_inference_steps=10, scale=SCALE, guidance_scale=7.5, noise=noise,
              output_type="latent", **emb)
    serial = ipa.generate(mask_image=full, **kw)
    joint = ipa.generate(mask_image=[full], joint=True, **kw)
    rel, cos = _metrics(joint, serial)
    print(f"[region-unet] S = 1 joint against serial: rel-L2 {rel:.3e} cos {cos:.6f}")
    assert rel <= 3e-2 and cos >= 0.999, (rel, cos)


def _request(cfg, seed, S, joint=True):
    from instructany2pix_amd.batch import InpaintRequest
    emb, lat, noise = _cond(cfg, seed)
    masks, e = _subjects(S, seed + 1)
    return InpaintRequest(latents=lat, mask=None, subject_embed=None, masks=masks, subject_embeds=list(e), strength=0.7, noise=noise, **emb)


def test_inpaint_batch_padding_is_neutral(models):
    """two requests with 1 and 3 subjects in one group: each row has the bits of the same request in a group of its own -- a group of the same size that holds only this
    request, so that nothing but the padding differs (bit identity across group sizes is not promised anywhere in batch.py)"""
    from instructany2pix_amd.batch import inpaint_batch
    cfg, hip, pipe, ipa, proj, net, holder, oracle = models
    one, three = _request(cfg, 41, 1), _request(cfg, 51, 3)
    both = inpaint_batch(ipa, [one, three], group=2, num_inference_steps=8, scale=SCALE).clone()
    own1 = inpaint_batch(ipa, [one, one], group=2, num_inference_steps=8, scale=SCALE).clone()        # G = 1: no padding
    own3 = inpaint_batch(ipa, [three, three], group=2, num_inference_steps=8, scale=SCALE).clone()
    assert torch.isfinite(both.float()).all() and torch.equal(own1[0], own1[1]) and torch.equal(own3[0], own3[1])
    assert torch.equal(both[0], own1[0]), "padding a one-subject row to three subjects moved a bit"
    assert torch.equal(both[1], own3[1])
    assert not torch.equal(both[0].cpu(), one.latents[0]) and not torch.equal(both[0], both[1])


def test_edit_batch_joint_and_serial_rows(models):
    """edit_batch(subject_modes=["joint", "serial"]) with an injected conditioner: the serial row has the bits it has today (the same call with the joint request's
    subject stage switched off, so that the groups of every stage the serial row runs in are the same)"""
    from test_edit_batch_gpu import Models, _cond as _econd
    m = Models()
    conds = {f"edit {i}": _econd(m, 120 + i, n_subjects=2) for i in range(2)}
    pipe = m.pipeline(conds, refiner_handoff="latent")
    insts = list(conds)
    kw = dict(num_inference_steps=3, cfg=4.0, refinement=0.0, group=2)
    got = pipe.edit_batch(insts, [[]] * 2, subject_strength=[0.1, 0.1], subject_modes=["joint", "serial"], **kw)
    today = pipe.edit_batch(insts, [[]] * 2, subject_strength=[0.0, 0.1], **kw)
    assert [g[2] for g in got] == ["SUCCESS!"] * 2
    assert torch.equal(got[1][0], today[1][0]) and torch.equal(got[1][1], today[1][1]), "the serial row of a mixed call lost its bits"
    assert torch.equal(got[0][0], today[0][0]) and not torch.equal(got[0][1], got[0][0])
    serial0 = pipe.edit_batch(insts, [[]] * 2, subject_strength=[0.1, 0.0], **kw)
    assert not torch.equal(got[0][1], serial0[0][1])      # joint is not the serial result
    with pytest.raises(ValueError):
        pipe.edit_batch(insts, [[]] * 2, subject_strength=0.1, subject_modes="both", **kw)


def test_forward_r_refusals(models):
    """`ia2p_unet_forward_r` refuses before any launch: a NULL mask pointer, G outside 1 .. 16, and an adapter whose token count is not 4 G (IA2P_ERR_STATE)"""
    from instructany2pix_amd import _ffi
    cfg, hip, pipe, ipa, proj, net, holder, oracle = models
    x, ctx, te, tid = _inputs(cfg, 2, 16, 1, 9)
    hip(x.to(DEV), 300, encoder_hidden_states=ctx.to(DEV), added_cond_kwargs=dict(text_embeds=te.to(DEV), time_ids=tid.to(DEV)))      # the adapter is on, num_tokens = 4
    t, ts, p = torch.zeros(1 << 16, dtype=torch.half, device=DEV), torch.zeros(2, device=DEV), _ffi.ptr
    call = lambda masks, G: hip._lib.ia2p_unet_forward_r(hip._ctx, _ffi.current_stream(), p(t), p(ts), None, p(t), None, 85, p(t), p(t), p(t), 2, 16, 16, p(t), 2 * t.numel(), masks, G)      # noqa: E731
    assert call(None, 1) == 1 and call(p(t), 0) == 2 and call(p(t), 17) == 2
    assert call(p(t), 2) == 4 and b"num_tokens" in hip._lib.ia2p_last_error(hip._ctx)
    size = hip._lib.ia2p_workspace_bytes_r      # (no comparison with ia2p_workspace_bytes: that one also covers the autotune pass, which runs no regions)
    assert size(hip._ctx, 2, 16, 16, 85, 0) == 0 and size(hip._ctx, 2, 16, 16, 85, 17) == 0 and size(hip._ctx, 2, 15, 16, 85, 1) == 0
    # the pyramid sits in front of the plain pass's tensors: fp16 [B, G, 64] and [B, G, 16] at B = 2 (the 8 x 8 and 4 x 4 grids), each rounded up to the
    # allocator's 256 bytes (which is why G = 1 already takes 512: the difference to G = 16 is counted between the ALIGNED sizes)
    pyramid = lambda G: sum(-(-2 * G * hw * 2 // 256) * 256 for hw in (64, 16))      # noqa: E731
    one, sixteen = size(hip._ctx, 2, 16, 16, 81, 1), size(hip._ctx, 2, 16, 16, 81, 16)
    print(f"[region-unet] workspace_bytes_r: G = 1 {one}, G = 16 {sixteen}; pyramid {pyramid(1)}, {pyramid(16)}")
    assert one >= pyramid(1) and sixteen - one >= pyramid(16) - pyramid(1)
    torch.cuda.synchronize()
    assert bool((t == 0).all())
