"""Whole edit requests in batches (instructany2pix_amd/batch.py: `refine_batch`, `inpaint_batch`, `edit_batch`; C ABI: ia2p_mask_blend_v) on the MI355X.

What must hold, as for the hot segment in tests/test_batch_gpu.py:
  * the per-request blend agrees with its scalar form bit for bit, and a (1, 0) row over a {0, 1} mask returns its inputs' bits (the loops HOLD a finished
    request that way);
  * row i of a HETEROGENEOUS batch gets exactly the bits it gets in a UNIFORM batch of the same size carrying request i in every slot;
  * against the serial pipelines (batch 1) and the CPU oracle only batch-dependent summation orders differ: the trajectory bar of test_batch_gpu.py and
    test_refiner_gpu.py, rel-L2 < 3e-2 and cosine > 0.999;
  * `edit_batch` is `denoise_batch` -> `refine_batch` -> `inpaint_batch` by hand, bit for bit.
Tiny configs, 16 x 16 latents, synthetic weights; the loops run 8-step schedules (strengths 0.3 / 0.5 / 0.7 / 1.0 -> 2 / 4 / 5 / 8 steps)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_STEPS = 8


def _traj(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return float((a - b).norm() / b.norm()), float(torch.dot(a, b) / (a.norm() * b.norm()))


# ---- 1. the per-request blend ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,h,w", [(4, 4, 16, 16), (3, 4, 12, 20), (2, 3, 5, 7), (16, 4, 8, 8)])
def test_mask_blend_v_equals_the_scalar_form(B, C, h, w):
    from instructany2pix_amd.scheduler import mask_blend, mask_blend_v
    g = torch.Generator().manual_seed(B * 100 + h)
    x, init, noise = (torch.randn(B, C, h, w, generator=g).half().to(DEV) for _ in range(3))
    mask = (torch.rand(B, 1, h, w, generator=g) > 0.5).half().to(DEV)
    n, pad, sentinel = x.numel(), 96, -77.0

    def fresh():            # two outputs with sentinel elements behind them
        bufs = [torch.full((n + pad,), sentinel, dtype=torch.float16, device=DEV) for _ in range(2)]
        return bufs, [b[:n].view(B, C, h, w) for b in bufs]

    ref = torch.empty_like(x)
    mask_blend(x, init, noise, mask, 0.8, 0.6, ref)
    bufs, (out, out2) = fresh()
    mask_blend_v(x, init, noise, mask, torch.tensor([[0.8, 0.6]] * B).to(DEV), out, out2)
    assert torch.equal(out, ref) and torch.equal(out2, out)                       # equal rows: the scalar call, bit for bit
    assert all(bool((b[n:] == sentinel).all()) for b in bufs)                     # nothing past B * C * HW is written
    rows = [(0.8, 0.6), (1.0, 0.0), (0.25, 0.97), (0.0, 1.0)]
    coef = torch.tensor([rows[b % 4] for b in range(B)])
    bufs, (out, out2) = fresh()
    mask_blend_v(x, init, noise, mask, coef.to(DEV), out, out2)
    for b in range(B):                                                            # mixed rows: every row is the scalar call on its own slice
        mask_blend(x[b:b + 1].contiguous(), init[b:b + 1].contiguous(), noise[b:b + 1].contiguous(), mask[b:b + 1].contiguous(), float(coef[b, 0]), float(coef[b, 1]),
                   ref[b:b + 1])
    assert torch.equal(out, ref) and torch.equal(out2, out)
    assert all(bool((b[n:] == sentinel).all()) for b in bufs)
    m = mask[1].bool().expand(C, h, w)                                            # row 1 carries (1, 0): x where m = 1, init where m = 0, bit for bit
    assert torch.equal(out[1][m], x[1][m]) and torch.equal(out[1][~m], init[1][~m])
    out3 = torch.empty_like(x)
    mask_blend_v(x, init, noise, mask, coef.to(DEV), out3)                        # out2 is optional
    assert torch.equal(out3, out)
    with pytest.raises(AssertionError):
        mask_blend_v(x, init, noise, mask, coef[:, :1].contiguous().to(DEV), out)
    with pytest.raises(AssertionError):
        mask_blend_v(x, init, noise, mask, coef, out)                             # coefficients on the host


def test_mask_blend_v_refusals_come_from_the_host():
    from instructany2pix_amd import _ffi
    L, s = _ffi.lib(), _ffi.current_stream()
    x = torch.zeros(2, 4, 8, 8, dtype=torch.float16, device=DEV)
    mask, coef, out = torch.zeros(2, 1, 8, 8, dtype=torch.float16, device=DEV), torch.zeros(2, 2, device=DEV), torch.full_like(x, 5.0)
    p = _ffi.ptr
    good = [p(x), p(x), p(x), p(mask), p(coef), p(out)]
    for i in range(6):                                                            # x, init, noise, mask, coef, out: none may be null
        a = list(good)
        a[i] = None
        assert L.ia2p_mask_blend_v(s, *a, None, 2, 4, 64) == 1, i                 # IA2P_ERR_INVALID
    for B, C, HW in ((0, 4, 64), (2, 0, 64), (2, 4, 0), (-1, 4, 64)):
        assert L.ia2p_mask_blend_v(s, *good, None, B, C, HW) == 2, (B, C, HW)     # IA2P_ERR_SHAPE
    with pytest.raises(ValueError, match="SHAPE"):
        _ffi.check(L.ia2p_mask_blend_v(s, *good, None, 2, 4, 0))
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())                                               # no refused call launched anything
    assert L.ia2p_mask_blend_v(s, *good, None, 2, 4, 64) == 0


# ---- models shared by the loop tests --------------------------------------------------------------------------------------------------------
class Models:
    def __init__(self):
        from instructany2pix_amd.config import tiny, tiny_refiner
        from instructany2pix_amd.unet import HipUNet2DConditionModel
        from instructany2pix_amd.weights import ip_adapter_specs, synthetic_state_dict, unet_param_specs
        self.bcfg, self.rcfg = tiny(), tiny_refiner()
        self.bsd, self.rsd = synthetic_state_dict(unet_param_specs(self.bcfg), seed=7), synthetic_state_dict(unet_param_specs(self.rcfg), seed=11)
        specs = ip_adapter_specs(self.bcfg, 64)
        self.ck = {"image_proj": synthetic_state_dict(specs["image_proj"], seed=7), "ip_adapter": synthetic_state_dict(specs["ip_adapter"], seed=7)}
        self.base, self.ref = HipUNet2DConditionModel(self.bcfg, DEV), HipUNet2DConditionModel(self.rcfg, DEV)
        self.base.load_state_dict(self.bsd)
        self.ref.load_state_dict(self.rsd)
        self._vae = None

    @property
    def vae(self):
        if self._vae is None:
            from instructany2pix_amd.config import tiny_vae
            from instructany2pix_amd.vae import HipAutoencoderKL
            from instructany2pix_amd.weights import synthetic_state_dict, vae_param_specs
            self._vae = HipAutoencoderKL(tiny_vae(), DEV)
            self._vae.load_state_dict(synthetic_state_dict(vae_param_specs(tiny_vae()), seed=7))
        return self._vae

    def pipeline(self, conds=None, **kw):
        """`conds`: instruction -> conditioning dict (the conditioner looks the instruction up)"""
        from instructany2pix_amd.pipeline import InstructAny2PixPipeline
        conditioner = (lambda inst, mm, use_cache=False: conds[inst]) if conds is not None else None
        pipe = InstructAny2PixPipeline(unet=self.base, ip_ckpt=self.ck, device=DEV, clip_embeddings_dim=64, conditioner=conditioner, refiner_unet=self.ref, **kw)
        pipe.ip_adapter_xl.set_scale(1.0)
        return pipe


@pytest.fixture(scope="module")
def models():
    return Models()


def _cond(m, seed, n_subjects=0, hw=16):
    """everything a conditioner returns for one request, every noise included"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    b, r = m.bcfg, m.rcfg
    emb = lambda cfg: dict(prompt_embeds=rn(1, 77, cfg.cross_attention_dim).half(), pooled_prompt_embeds=rn(1, cfg.pooled_dim).half(),
                           negative_prompt_embeds=rn(1, 77, cfg.cross_attention_dim).half(), negative_pooled_prompt_embeds=rn(1, cfg.pooled_dim).half())
    c = dict(image_embeds=rn(1, 64), base_embed=rn(1, 64), y=rn(1, 64), caption=f"a photo {seed}", base_latents=rn(1, 4, hw, hw).half(), **emb(b),
             polar_noise=rn(1, 4, hw, hw).half(), refiner_noise=rn(1, 4, hw, hw).half(), subject_noise=rn(1, 4, hw, hw).half())
    c.update({"refiner_" + k: v for k, v in emb(r).items()})
    c.update({"subject_" + k: v for k, v in emb(b).items()})
    masks = []
    for k in range(n_subjects):          # pixel-space rectangles, 8 x the latent grid
        mk = torch.zeros(hw * 8, hw * 8)
        mk[16 * k + 8 * (seed % 3):16 * k + 72, 24:104 - 16 * k] = 1.0
        masks.append((mk, rn(64)))
    c["subject_data"] = masks
    return c


# ---- 2 + 3. the refiner loop ------------------------------------------------------------------------------------------------------------------
REFINE_STRENGTHS = (0.3, 0.5, 0.5, 1.0)          # 2 / 4 / 4 / 8 of 8 steps


def _refine_requests(conds, strengths):
    from instructany2pix_amd.batch import RefineRequest
    return [RefineRequest(latents=c["base_latents"], prompt_embeds=c["refiner_prompt_embeds"], pooled_prompt_embeds=c["refiner_pooled_prompt_embeds"],
                          negative_prompt_embeds=c["refiner_negative_prompt_embeds"], negative_pooled_prompt_embeds=c["refiner_negative_pooled_prompt_embeds"],
                          strength=s, noise=c["refiner_noise"]) for c, s in zip(conds, strengths)]


@pytest.fixture(scope="module")
def refined(models):
    from instructany2pix_amd.batch import refine_batch
    pipe = models.pipeline()
    reqs = _refine_requests([_cond(models, 40 + i) for i in range(4)], REFINE_STRENGTHS)
    out = refine_batch(pipe.piperf, reqs, group=4, num_inference_steps=N_STEPS).clone()
    return pipe, reqs, out


def test_refine_batch_rows_equal_the_uniform_batches_bit_for_bit(refined, models):
    from instructany2pix_amd.batch import refine_batch
    pipe, reqs, out = refined
    assert out.shape == (4, 4, 16, 16) and out.dtype == torch.float16 and torch.isfinite(out.float()).all()
    for i, r in enumerate(reqs):
        uni = refine_batch(pipe.piperf, [r, r, r, r], group=4, num_inference_steps=N_STEPS)
        assert torch.equal(uni[0], uni[3])
        assert torch.equal(out[i], uni[i]), i                    # 2-, 4- and 8-step rows: the held iterations changed nothing
    # two rows that differ only in strength differ
    a, b = _refine_requests([_cond(models, 40)] * 2, (0.3, 0.5))
    two = refine_batch(pipe.piperf, [a, b], group=2, num_inference_steps=N_STEPS)
    assert not torch.equal(two[0], two[1])
    assert reqs[0].latents.abs().max() > 0 and torch.equal(reqs[0].latents, _cond(models, 40)["base_latents"])      # the caller's latents are not written


def test_refine_batch_vs_serial_pipeline_and_oracle(refined, models):
    import oracle
    pipe, reqs, out = refined
    ref_net, rcfg = oracle.build_unet(models.rcfg, models.rsd), models.rcfg
    H = 16 * 8
    ids, neg_ids = oracle.get_add_time_ids_aesthetic((H, H), (0, 0), (H, H), 6.0, 2.5, (H, H), (0, 0), (H, H), rcfg.addition_time_embed_dim, rcfg.pooled_dim,
                                                     rcfg.projection_class_embeddings_input_dim)
    for i, r in enumerate(reqs):
        serial = pipe.piperf(latents=r.latents, noise=r.noise, strength=r.strength, num_inference_steps=N_STEPS, prompt_embeds=r.prompt_embeds,
                             pooled_prompt_embeds=r.pooled_prompt_embeds, negative_prompt_embeds=r.negative_prompt_embeds,
                             negative_pooled_prompt_embeds=r.negative_pooled_prompt_embeds, output_type="latent").images
        with torch.no_grad():
            orc = oracle.img2img_loop(ref_net, oracle.EulerDiscreteSchedulerRef(), r.latents.float(), r.noise.float(), r.prompt_embeds.float(),
                                      dict(text_embeds=r.pooled_prompt_embeds.float(), time_ids=ids), N_STEPS, r.strength, 5.0, r.negative_prompt_embeds.float(),
                                      dict(text_embeds=r.negative_pooled_prompt_embeds.float(), time_ids=neg_ids))
        for what, ref in (("serial", serial[0]), ("oracle", orc[0])):
            rel, cos = _traj(out[i], ref)
            print(f"refine row {i} ({r.strength}) vs {what}: rel-L2 {rel:.3e} cos {cos:.6f}")
            assert rel < 3e-2 and cos > 0.999, (i, what, rel, cos)


# ---- 4. the inpaint loop ----------------------------------------------------------------------------------------------------------------------
INPAINT_STRENGTHS = (0.3, 0.7, 1.0, 0.5)         # 2 / 5 / 8 / 4 of 8 steps; row 2 starts from pure noise


def _inpaint_requests(conds, strengths):
    from instructany2pix_amd.batch import InpaintRequest
    return [InpaintRequest(latents=c["base_latents"], mask=c["subject_data"][0][0], subject_embed=c["subject_data"][0][1], prompt_embeds=c["subject_prompt_embeds"],
                           pooled_prompt_embeds=c["subject_pooled_prompt_embeds"], negative_prompt_embeds=c["subject_negative_prompt_embeds"],
                           negative_pooled_prompt_embeds=c["subject_negative_pooled_prompt_embeds"], strength=s, noise=c["subject_noise"])
            for c, s in zip(conds, strengths)]


@pytest.fixture(scope="module")
def inpainted(models):
    from instructany2pix_amd.batch import inpaint_batch
    pipe = models.pipeline()
    reqs = _inpaint_requests([_cond(models, 60 + i, n_subjects=1) for i in range(4)], INPAINT_STRENGTHS)
    out = inpaint_batch(pipe.ip_adapter_xl_inpaint, reqs, group=4, num_inference_steps=N_STEPS).clone()
    return pipe, reqs, out


def test_inpaint_batch_rows_equal_the_uniform_batches_bit_for_bit(inpainted, models):
    from instructany2pix_amd.batch import inpaint_batch
    pipe, reqs, out = inpainted
    assert out.shape == (4, 4, 16, 16) and torch.isfinite(out.float()).all()
    for i, r in enumerate(reqs):
        uni = inpaint_batch(pipe.ip_adapter_xl_inpaint, [r, r, r, r], group=4, num_inference_steps=N_STEPS)
        assert torch.equal(uni[0], uni[3])
        assert torch.equal(out[i], uni[i]), i
        # where the mask is 0 the request's own latents come back bit for bit (no re-noising after its last step, none while it is held)
        keep = (torch.nn.functional.interpolate(r.mask[None, None], size=(16, 16)) < 0.5).expand(1, 4, 16, 16)
        assert keep.any() and (~keep).any()
        assert torch.equal(out[i:i + 1].cpu()[keep], r.latents[keep]), i
        assert not torch.equal(out[i:i + 1].cpu()[~keep], r.latents[~keep])
    a, b = _inpaint_requests([_cond(models, 60, n_subjects=1)] * 2, (0.3, 0.7))
    two = inpaint_batch(pipe.ip_adapter_xl_inpaint, [a, b], group=2, num_inference_steps=N_STEPS)
    assert not torch.equal(two[0], two[1])


def test_inpaint_batch_vs_serial_generate(inpainted):
    pipe, reqs, out = inpainted
    for i, r in enumerate(reqs):
        serial = pipe.ip_adapter_xl_inpaint.generate(latents=r.latents, mask_image=r.mask, pil_image=None, strength=r.strength,
                                                     clip_image_embeds_local=r.subject_embed[None], mode="local", num_inference_steps=N_STEPS, scale=0.8,
                                                     guidance_scale=7.5, noise=r.noise, prompt_embeds=r.prompt_embeds, negative_prompt_embeds=r.negative_prompt_embeds,
                                                     pooled_prompt_embeds=r.pooled_prompt_embeds, negative_pooled_prompt_embeds=r.negative_pooled_prompt_embeds,
                                                     output_type="latent")
        rel, cos = _traj(out[i], serial[0])
        print(f"inpaint row {i} ({r.strength}) vs serial: rel-L2 {rel:.3e} cos {cos:.6f}")
        assert rel < 3e-2 and cos > 0.999, (i, rel, cos)
    pipe.ip_adapter_xl.set_scale(1.0)            # `generate` leaves 0.8 on the shared processors


# ---- 5 + 6. whole requests -------------------------------------------------------------------------------------------------------------------
def _by_hand(pipe, conds, knobs, group):
    """`denoise_batch` -> `refine_batch` -> `inpaint_batch` on the conditioners' values, stage by stage (latent hand-off)"""
    from instructany2pix_amd.batch import EditRequest, InpaintRequest, RefineRequest, inpaint_batch, refine_batch
    from instructany2pix_amd.pipeline import fuse_instruction_embedding
    P = ("prompt_embeds", "pooled_prompt_embeds", "negative_prompt_embeds", "negative_pooled_prompt_embeds")
    reqs = [EditRequest(base_latents=c["base_latents"], latent_la=fuse_instruction_embedding(c["base_embed"], c["image_embeds"], c["y"], k["h"], k["norm"]).reshape(1, -1)[0],
                        **{p: c[p] for p in P}, alpha=k["alpha"], num_inference_steps=k["num_inference_steps"], cfg=k["cfg"], scale=k["scale"], noise=c["polar_noise"])
            for c, k in zip(conds, knobs)]
    base, _ = pipe.denoise_batch(reqs, group=group)
    cur = [base[i:i + 1] for i in range(len(conds))]
    ref = [i for i, k in enumerate(knobs) if k["refinement"] > 0]
    out = refine_batch(pipe.piperf, [RefineRequest(latents=cur[i], **{p: conds[i]["refiner_" + p] for p in P}, strength=knobs[i]["refinement"],
                                                   noise=conds[i]["refiner_noise"]) for i in ref], group=group)
    for j, i in enumerate(ref):
        cur[i] = out[j:j + 1]
    for k in range(2):
        now = [i for i, kn in enumerate(knobs) if kn["subject_strength"] > 0 and len(conds[i]["subject_data"]) > k]
        if now:
            out = inpaint_batch(pipe.ip_adapter_xl_inpaint, [InpaintRequest(latents=cur[i], mask=conds[i]["subject_data"][k][0], subject_embed=conds[i]["subject_data"][k][1],
                                                                            **{p: conds[i]["subject_" + p] for p in P}, strength=knobs[i]["subject_strength"],
                                                                            noise=conds[i]["subject_noise"]) for i in now], group=group)
            for j, i in enumerate(now):
                cur[i] = out[j:j + 1]
    return base, cur


KNOBS = [dict(alpha=0.7, h=[0.0, 0.4, 1.0], norm=20.0, refinement=0.1, num_inference_steps=4, subject_strength=0.1, cfg=4.0, scale=1.0),
         dict(alpha=0.6, h=[0.2, 0.4, 0.8], norm=18.0, refinement=0.0, num_inference_steps=3, subject_strength=0.16, cfg=7.5, scale=0.5),
         dict(alpha=0.8, h=[0.0, 0.5, 1.0], norm=20.0, refinement=0.16, num_inference_steps=5, subject_strength=0.1, cfg=10.0, scale=0.0),
         dict(alpha=0.5, h=[0.1, 0.4, 1.0], norm=22.0, refinement=0.1, num_inference_steps=4, subject_strength=0.0, cfg=2.0, scale=1.3)]
SUBJECTS = [2, 1, 0, 1]                          # (request 3 has a subject but subject_strength 0: no pass)


def _lists(knobs):
    return {k: [kn[k] for kn in knobs] for k in knobs[0]}


def test_edit_batch_is_its_three_stages_by_hand_bit_for_bit(models):
    conds = {f"edit {i}": _cond(models, 80 + i, n_subjects=SUBJECTS[i]) for i in range(4)}
    pipe = models.pipeline(conds, refiner_handoff="latent")
    insts = list(conds)
    got = pipe.edit_batch(insts, [[]] * 4, **_lists(KNOBS), group=4)
    assert len(got) == 4 and all(msg == "SUCCESS!" for _, _, msg in got)
    base, final = _by_hand(pipe, [conds[i] for i in insts], KNOBS, 4)
    for i, (non_refined, oo, _) in enumerate(got):
        assert non_refined.shape == (1, 4, 16, 16) and torch.equal(non_refined, base[i:i + 1]), i
        assert torch.equal(oo, final[i]), i
    assert not torch.equal(got[0][1], got[0][0]) and not torch.equal(got[1][1], got[1][0])      # refined + two subjects; not refined, one subject
    assert not torch.equal(got[2][1], got[2][0])                                                # refined, no subject
    # the debug message carries what `__call__`'s does
    dbg = pipe.edit_batch(insts[:2], [[]] * 2, **_lists(KNOBS[:2]), group=4, debug=True)
    assert dbg[1][2]["output_caption"] == conds[insts[1]]["caption"] and dbg[1][2]["latent_inv"].shape == (1, 4, 16, 16) and dbg[1][2]["latent_la"].shape == (1, 64)


def test_edit_batch_skipped_stages_scalars_groups_and_order(models):
    conds = {f"edit {i}": _cond(models, 90 + i, n_subjects=[0, 1, 2, 0, 1][i]) for i in range(5)}
    pipe = models.pipeline(conds, refiner_handoff="latent")
    insts = list(conds)
    kw = dict(num_inference_steps=3, cfg=4.0, refinement=[0.0, 0.1, 0.0, 0.1, 0.0], subject_strength=[0.1, 0.1, 0.1, 0.0, 0.0])
    got = pipe.edit_batch(insts, [[]] * 5, group=2, **kw)
    assert [msg for _, _, msg in got] == ["SUCCESS!"] * 5
    assert got[0][1] is got[0][0] and got[4][1] is got[4][0]                    # no refinement, no subject pass (none given / strength 0): oo IS non_refined
    assert all(got[i][1] is not got[i][0] and not torch.equal(got[i][1], got[i][0]) for i in (1, 2, 3))
    # 5 requests in groups of 2 (2 + 2 + 1) come back in request order: the same groups alone give the same bits
    sub = lambda lo, hi: {k: (v[lo:hi] if isinstance(v, list) else v) for k, v in kw.items()}
    first, last = pipe.edit_batch(insts[0:2], [[]] * 2, group=2, **sub(0, 2)), pipe.edit_batch(insts[4:5], [[]], group=2, **sub(4, 5))
    assert torch.equal(got[0][0], first[0][0]) and torch.equal(got[1][0], first[1][0]) and torch.equal(got[4][1], last[0][1])
    assert torch.equal(got[0][1], first[0][1])                                 # (request 0's subject pass shares its group of 2 with request 1 both times)


def test_edit_batch_images_out_and_seeded_image_handoff(models):
    """tiny VAE (factor 4: 64 x 64 images, 16 x 16 latents), the reference's hand-off (decode, 8-bit image, re-encode with a posterior sample), PIL out"""
    import PIL.Image
    conds = {f"edit {i}": _cond(models, 100 + i, n_subjects=[1, 0, 0][i]) for i in range(3)}
    for c in conds.values():                     # nothing supplied: every noise comes from the global generator
        for k in ("polar_noise", "refiner_noise", "subject_noise"):
            del c[k]
        c["subject_data"] = [(torch.nn.functional.interpolate(mk[None, None], size=(64, 64))[0, 0], e) for mk, e in c["subject_data"]]
    pipe = models.pipeline(conds, vae=models.vae)
    assert pipe.refiner_handoff == "image"
    insts = list(conds)
    kw = dict(num_inference_steps=3, cfg=4.0, refinement=[0.1, 0.1, 0.0], subject_strength=0.1, group=4)
    torch.manual_seed(11)
    a = pipe.edit_batch(insts, [[]] * 3, **kw)
    torch.manual_seed(11)
    b = pipe.edit_batch(insts, [[]] * 3, **kw)
    torch.manual_seed(12)
    c = pipe.edit_batch(insts, [[]] * 3, **kw)
    for (nr_a, oo_a, _), (nr_b, oo_b, _) in zip(a, b):
        assert torch.equal(nr_a, nr_b) and torch.equal(oo_a, oo_b)               # reproducible for a seed ...
    assert not torch.equal(a[0][1], c[0][1])                                     # ... and the seed matters
    torch.manual_seed(11)
    pil = pipe.edit_batch(insts, [[]] * 3, output_type="pil", **kw)
    for i, (nr, oo, msg) in enumerate(pil):
        assert msg == "SUCCESS!" and isinstance(nr, list) and len(nr) == 1 and isinstance(nr[0], PIL.Image.Image) and nr[0].size == (64, 64)
        assert isinstance(oo[0], PIL.Image.Image) and oo[0].size == (64, 64)
    assert pil[2][1] is pil[2][0]                                                # request 2: nothing after the base sample, one decode
    # the images are the decodes of the latents the seeded latent run returned
    want = pipe.pipe.image_processor.postprocess(models.vae.decode_from_latents(a[0][1]), output_type="pil")[0]
    assert want.tobytes() == pil[0][1][0].tobytes()


def test_edit_batch_subjects_by_phrase_take_their_masks_from_sam_first(models):
    """(phrase, embedding) subjects: every request's masks come from the segmenter on the ONE decode of its result, before any pass; the outcome equals the
    batch that is handed those masks (the SAM of test_sam_gpu.py::test_pipeline_subjects_by_phrase, whose masks survive the erosion)"""
    import numpy as np
    from tests import sam_ref as R
    from instructany2pix_amd.sam import HipSamModel, HipSamPredictor, get_mask, sam_tiny_config
    sd = {k: v.clone() for k, v in R.oracle_model().state_dict().items()}
    sd["mask_decoder.upscale_conv2.bias"] += 2.0
    sd["mask_decoder.output_hypernetworks_mlps.0.proj_out.bias"] += 1.0
    pred = HipSamPredictor(HipSamModel(sam_tiny_config(), DEV).load_state_dict(sd))
    boxes, phrases = torch.tensor([[0.35, 0.40, 0.40, 0.50], [0.70, 0.60, 0.45, 0.55]]), ["dog", "a cat"]
    conds = {f"edit {i}": _cond(models, 110 + i, n_subjects=2) for i in range(2)}
    embs = {k: [e for _, e in c["subject_data"]] for k, c in conds.items()}
    conds["edit 0"].update(subject_data=[("the dog.", embs["edit 0"][0]), ("cat's", embs["edit 0"][1])], subject_boxes=(boxes, phrases))
    conds["edit 1"].update(subject_data=[("a cat", embs["edit 1"][0])], subject_boxes=(boxes, phrases))
    pipe = models.pipeline(conds, vae=models.vae, segmenter=pred)
    kw = dict(num_inference_steps=3, cfg=4.0, refinement=0.0, subject_strength=0.1, group=2)
    got = pipe.edit_batch(list(conds), [[]] * 2, **kw)
    assert all(msg == "SUCCESS!" and not torch.equal(nr, oo) for nr, oo, msg in got)
    # by hand: masks on the decoded base results, then the same batch on (mask, embedding) subjects
    for i, (key, words) in enumerate((("edit 0", ("the dog", "cat")), ("edit 1", ("a cat",)))):
        x = models.vae.decode_from_latents(got[i][0])[:1]
        pred.set_image(np.ascontiguousarray(((x.float() / 2 + 0.5).clamp(0, 1) * 255.0).round().to(torch.uint8)[0].permute(1, 2, 0).cpu().numpy()))
        masks = [get_mask(w, boxes, phrases, pred, i=0, d=40, b=20, size=64) for w in words]
        assert all(np.array(m).max() == 255 for m in masks)
        conds[key]["subject_data"] = [(torch.from_numpy(np.array(m)), e) for m, e in zip(masks, embs[key])]
    assert all(np.array_equal(np.array(a), np.array(b)) for a, b in zip(masks, pipe.subject_masks))      # the last request's, as `__call__` leaves them
    want = pipe.edit_batch(list(conds), [[]] * 2, **kw)
    for (nr, oo, _), (wnr, woo, _) in zip(got, want):
        assert torch.equal(nr, wnr) and torch.equal(oo, woo)


# ---- 7. the LLM in front ---------------------------------------------------------------------------------------------------------------------
def test_edit_batch_calls_forward_llm_batch_once_and_answers_a_request_without_im_gen(models):
    """The tiny LLM of test_llm_batch_gpu.py (random weights, two cache slots) decodes all three requests in ONE `forward_llm_batch` call. What such a model
    says is noise, so the five-tuples it returns are then replaced by fixed ones -- request 1 without an `<im_gen>` -- and the text encoders and the prior
    are stand-ins that return seeded tensors: the test is about the wiring behind the call."""
    from stub_llm_tokenizer import StubLlamaTokenizer
    from test_llm_batch_gpu import _make
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
    lcfg = tiny_llm()
    lm = _make(lcfg, synthetic_state_dict(llm_param_specs(lcfg, lcfg.embed_dim, "linear"), seed=21), "fp16", 256, 2)
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g)
    encoded = []

    def encoder(cfg):
        def encode_prompt(prompt=None, negative_prompt=None, do_classifier_free_guidance=True, **kw):
            n = len(prompt) if isinstance(prompt, list) else 1
            encoded.append((cfg is models.rcfg, prompt))
            return rn(n, 77, cfg.cross_attention_dim).half(), rn(n, 77, cfg.cross_attention_dim).half(), rn(n, cfg.pooled_dim).half(), rn(n, cfg.pooled_dim).half()
        return encode_prompt

    from types import SimpleNamespace
    prior = SimpleNamespace(generate_diffusion=lambda *a, **kw: [rn(64)])
    pipe = models.pipeline(None, llm=lm, llm_tokenizer=StubLlamaTokenizer(503), text_encoder=encoder(models.bcfg), refiner_text_encoder=encoder(models.rcfg),
                           prior=prior, refiner_handoff="latent")
    real, calls = pipe.forward_llm_batch, []
    fixed = [(rn(64), rn(64), " a blue fox", "fox.png", None), (None, None, "I cannot do that", None, None), (rn(64), rn(64), " an owl at night", "owl.png", None)]

    def counted(insts, mm_datas):
        out = real(insts, mm_datas)
        assert len(out) == 3 and all(isinstance(t, tuple) and len(t) == 5 for t in out)
        calls.append(len(insts))
        return fixed
    pipe.forward_llm_batch = counted
    # the requests test_llm_batch_gpu.py decodes (greedy, so that what the random model says does not depend on a draw)
    gen_batch = lm.generate_batch
    lm.generate_batch = lambda *a, **kw: gen_batch(*a, **{**kw, "do_sample": False})
    fox = [{"type": "image", "fname": "fox.png", "embed": rn(1024)}]
    owl = [{"type": "image", "fname": "owl.png", "embed": rn(1024)}, {"type": "audio", "fname": "rain.wav", "embed": rn(1024)}]
    base = {name: rn(1, 4, 16, 16).half() for name in ("fox.png", "owl.png")}
    got = _edit_with_latent_images(pipe, ["turn the fox in <video> blue", "add <video> to <video> and make it night", "turn the fox in <video> blue"], [fox, owl, fox], base)
    assert calls == [3]
    assert got[1][0] is None and got[1][1] is None and got[1][2].startswith("FAILED") and "I cannot do that" in got[1][2]
    for i in (0, 2):
        assert got[i][2] == "SUCCESS!" and got[i][0].shape == (1, 4, 16, 16) and torch.isfinite(got[i][1].float()).all() and not torch.equal(got[i][0], got[i][1])
    # '' once (the inversion prompt), then ONE call per role over the two live captions
    assert encoded == [(False, ""), (False, ["best quality, high quality a blue fox", "best quality, high quality an owl at night"]),
                       (True, [" a blue fox,high quality,well-formed,award-winning", " an owl at night,high quality,well-formed,award-winning"])]


def _edit_with_latent_images(pipe, insts, mm_datas, base):
    """no VAE in this pipeline: hand the base latents in where `_conditions_for_batch` leaves the image path"""
    inner = pipe._conditions_for_batch

    def with_latents(i, m):
        cs = inner(i, m)
        for c in cs:
            if c.get("base_img_path") in base:
                c["base_latents"] = base[c["base_img_path"]]
        return cs
    pipe._conditions_for_batch = with_latents
    return pipe.edit_batch(insts, mm_datas, num_inference_steps=3, cfg=4.0, refinement=0.1, group=4)


# ---- 8. two ranks ------------------------------------------------------------------------------------------------------------------------------
def test_edit_batch_sharded_over_two_ranks():
    """world_size 2 on one GPU (gloo): every loop shards its requests contiguously, groups of 2, all-gather in request order == the single-process result"""
    import socket
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "dist_edit_batch_two_ranks.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "EDIT_BATCH_DIST_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
