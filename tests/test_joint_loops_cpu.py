"""Host code the serial and the batched serving paths share (instructany2pix_amd/batch.py: `invert_tables`, `sample_tables`, the four joint loops' launch
sequences; scheduler.py: `kept_steps`; the serial pipelines' refusals). Needs no GPU: the tables are host arithmetic, the launch sequences are recorded by
stand-ins for the UNet and the two per-request update entry points on CPU tensors, and every refusal comes before the first use of a model.

Beside tests/test_edit_batch_cpu.py, whose two table tests these follow: row r of a group's `[iterations][requests]` tables carries exactly what the scheduler
gives request r alone on the serial pipelines' path, and a request that is through is HELD at its last timestep with coefficients that keep its latents."""
from types import SimpleNamespace

import pytest
import torch

STEPS = (6, 4, 5)


def _alone(n):
    from instructany2pix_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler.from_config(DDIMScheduler().config)
    sch.set_timesteps(n)
    return sch


def test_invert_tables_equal_the_ddim_scheduler_per_request():
    from instructany2pix_amd.batch import invert_tables
    from instructany2pix_amd.scheduler import DDIMScheduler
    cfg = DDIMScheduler().config
    ts, coef = invert_tables(cfg, STEPS)
    assert len(ts) == len(coef) == 6 and all(len(row) == 3 for row in ts + coef)
    for r, n in enumerate(STEPS):
        sch = _alone(n)                                          # the request alone: `SDXLDDIMPipeline.inverse`'s walk in ascending t
        asc, acp = [int(t) for t in reversed(sch.timesteps)], sch.alphas_cumprod
        assert len(asc) == n and asc == sorted(asc)
        for k in range(6):
            if k < n:
                a_prev = float(acp[asc[k - 1]]) if k > 0 else float(sch.final_alpha_cumprod)      # the first step starts from final_alpha_cumprod
                assert ts[k][r] == float(asc[k])
                assert coef[k][r] == (0.0,) + DDIMScheduler.inversion_coeffs(float(acp[asc[k]]), a_prev)
            else:                                                # held: its last (largest) timestep, latents kept
                assert ts[k][r] == float(asc[-1]) == float(max(asc))
                assert coef[k][r] == (0.0, 1.0, 0.0)
        assert coef[0][r] != (0.0,) + DDIMScheduler.inversion_coeffs(float(acp[asc[0]]), float(acp[asc[0]]))      # (the first row is not the identity)
    # a group of one short request has as many iterations as that request has steps
    one_ts, one_coef = invert_tables(cfg, [4])
    assert len(one_ts) == len(one_coef) == 4 and [row[0] for row in one_ts] == [row[1] for row in ts[:4]] and [row[0] for row in one_coef] == [row[1] for row in coef[:4]]


def test_sample_tables_equal_the_ddim_scheduler_per_request():
    from instructany2pix_amd.batch import sample_tables
    from instructany2pix_amd.scheduler import DDIMScheduler
    cfg, g = DDIMScheduler().config, (4.0, 7.5, 10.0)
    ts, coef = sample_tables(cfg, STEPS, g)
    assert len(ts) == len(coef) == 6 and all(len(row) == 6 for row in ts) and all(len(row) == 3 for row in coef)
    for r, n in enumerate(STEPS):
        sch = _alone(n)
        desc = [int(t) for t in sch.timesteps]
        assert len(desc) == n and desc == sorted(desc, reverse=True)
        for k in range(6):
            if k < n:
                assert ts[k][r] == ts[k][3 + r] == float(desc[k])            # duplicated over [uncond x n | cond x n]
                assert coef[k][r] == (g[r],) + sch.step_coeffs(desc[k])
            else:                                                # held: its last timestep; g = 0 here (the refiner and inpaint loops hold with their g)
                assert ts[k][r] == ts[k][3 + r] == float(desc[-1])
                assert coef[k][r] == (0.0, 1.0, 0.0)
    one_ts, one_coef = sample_tables(cfg, [4], [7.5])
    assert len(one_ts) == len(one_coef) == 4 and [row[0] for row in one_coef] == [row[1] for row in coef[:4]] and all(row == [row[0]] * 2 for row in one_ts)


def test_kept_steps_is_the_get_timesteps_of_both_serial_pipelines():
    from instructany2pix_amd.img2img import StableDiffusionXLImg2ImgPipeline
    from instructany2pix_amd.inpaint import StableDiffusionXLInpaintPipeline
    from instructany2pix_amd.scheduler import check_kept_steps, kept_steps
    assert [kept_steps(50, s) for s in (0.0, 0.01, 0.3, 0.5, 0.9999, 1.0)] == [(50, 0), (50, 0), (35, 15), (25, 25), (1, 49), (0, 50)]
    assert kept_steps(8, 0.3) == (6, 2) and kept_steps(8, 1.0) == (0, 8)
    rf, ip = StableDiffusionXLImg2ImgPipeline(None), StableDiffusionXLInpaintPipeline(None)
    for p in (rf, ip):
        p.scheduler.set_timesteps(50)
    for s in (0.0, 0.3, 1.0):
        t_start, n = kept_steps(50, s)
        ts, got_n, got_start = rf.get_timesteps(50, s)
        assert (got_n, got_start, len(ts)) == (n, t_start, n)
        ts, got_n = ip.get_timesteps(50, s)
        assert (got_n, len(ts)) == (n, n)
    check_kept_steps(1, 0.02)
    with pytest.raises(ValueError, match=r"strength parameter: 0.01, the number of pipeline steps is 0 which is < 1 and not appropriate for this pipeline\.$"):
        check_kept_steps(0, 0.01)
    with pytest.raises(ValueError, match=r"for this pipeline\. \(request 3\)$"):
        check_kept_steps(0, 0.01, " (request 3)")


# ---- launch sequences -------------------------------------------------------------------------------------------------------------------------------------
CTX, POOLED, TED, HW = 16, 8, 2, 8


class RecordingUNet:
    """stands where a HipUNet2DConditionModel stands: records one event per evaluation and checks what it is handed"""
    device = torch.device("cpu")

    def __init__(self, log, time_ids_len):
        self.log = log
        self.config = SimpleNamespace(addition_time_embed_dim=TED)
        self.add_embedding = SimpleNamespace(linear_1=SimpleNamespace(in_features=TED * time_ids_len + POOLED))

    def __call__(self, x, timesteps, encoder_hidden_states=None, added_cond_kwargs=None, out=None, ip_scales=None):
        B = x.shape[0]
        assert tuple(timesteps.shape) == (B,) and timesteps.dtype == torch.float32
        assert encoder_hidden_states.shape[0] == B and encoder_hidden_states.dtype == torch.float16 and encoder_hidden_states.is_contiguous()
        assert tuple(added_cond_kwargs["text_embeds"].shape) == (B, POOLED) and added_cond_kwargs["time_ids"].shape[0] == B
        assert out.shape == x.shape and (ip_scales is None or tuple(ip_scales.shape) == (B,))
        self.log.append(("unet", B))
        out.zero_()


def _image_tokens(n):
    return torch.zeros(n, 4, CTX, dtype=torch.float16), torch.zeros(n, 4, CTX, dtype=torch.float16)


@pytest.fixture()
def log(monkeypatch):
    from instructany2pix_amd import batch
    events = []

    def fused_update_v(x, eps_u, eps_c, coef, out, out2=None):
        assert tuple(coef.shape) == (x.shape[0], 3) and coef.dtype == torch.float32
        events.append(("update", x.shape[0]))
        out.zero_()
        return out

    def mask_blend_v(x, init, noise, mask, coef, out, out2=None):
        assert tuple(coef.shape) == (x.shape[0], 2) and tuple(mask.shape) == (x.shape[0], 1, HW, HW)
        events.append(("blend", x.shape[0]))
        return out
    monkeypatch.setattr(batch, "fused_update_v", fused_update_v)
    monkeypatch.setattr(batch, "mask_blend_v", mask_blend_v)
    return events


def _embeds():
    z = torch.zeros
    return dict(prompt_embeds=z(1, 77, CTX), pooled_prompt_embeds=z(1, POOLED), negative_prompt_embeds=z(1, 77, CTX), negative_pooled_prompt_embeds=z(1, POOLED))


def test_inversion_and_sampling_launch_a_unet_and_an_update_per_iteration(log):
    """a mixed group of three (6 / 4 / 5 steps): the joint loops run 6 iterations each, nothing before them"""
    from instructany2pix_amd.batch import EditRequest, denoise_batch
    from instructany2pix_amd.scheduler import DDIMScheduler
    unet = RecordingUNet(log, 6)
    ipa = SimpleNamespace(get_image_embeds=lambda clip_image_embeds=None, mode=None: _image_tokens(clip_image_embeds.shape[0]))
    pipe = SimpleNamespace(ip_adapter_xl=ipa, pipe=SimpleNamespace(unet=unet, scheduler=DDIMScheduler()))
    reqs = [EditRequest(base_latents=torch.zeros(1, 4, HW, HW), latent_la=torch.zeros(32), num_inference_steps=n, cfg=4.0, noise=torch.ones(1, 4, HW, HW).half(), **_embeds())
            for n in STEPS]
    out, inv = denoise_batch(pipe, reqs, group=4)
    assert out.shape == inv.shape == (3, 4, HW, HW)
    assert log == [("unet", 3), ("update", 3)] * 6 + [("unet", 6), ("update", 3)] * 6        # inversion on 3 rows; sampling on [uncond x 3 | cond x 3]


def test_the_refiner_loop_launches_scale_unet_update_after_one_add_noise(log):
    """strengths 0.3 / 0.5 / 1.0 of 8 steps: 8 iterations"""
    from instructany2pix_amd.batch import RefineRequest, refine_batch
    from instructany2pix_amd.scheduler import EulerDiscreteScheduler
    piperf = SimpleNamespace(unet=RecordingUNet(log, 5), scheduler=EulerDiscreteScheduler(), vae_scale_factor=8, config=SimpleNamespace(requires_aesthetics_score=True))
    reqs = [RefineRequest(latents=torch.zeros(1, 4, HW, HW), strength=s, noise=torch.ones(1, 4, HW, HW).half(), **_embeds()) for s in (0.3, 0.5, 1.0)]
    assert refine_batch(piperf, reqs, group=4, num_inference_steps=8).shape == (3, 4, HW, HW)
    assert log == [("update", 3)] + [("update", 3), ("unet", 6), ("update", 3)] * 8


def test_the_inpaint_loop_launches_unet_update_blend_after_one_start_launch(log):
    from instructany2pix_amd.batch import InpaintRequest, inpaint_batch
    from instructany2pix_amd.scheduler import DDIMScheduler
    ipa = SimpleNamespace(pipe=SimpleNamespace(unet=RecordingUNet(log, 6), scheduler=DDIMScheduler(), vae_scale_factor=8),
                          get_image_embeds=lambda clip_image_embeds_local=None, mode=None, scale_g=None, scale_l=None: _image_tokens(clip_image_embeds_local.shape[0]))
    reqs = [InpaintRequest(latents=torch.zeros(1, 4, HW, HW), mask=torch.ones(HW * 8, HW * 8), subject_embed=torch.zeros(32), strength=s,
                           noise=torch.ones(1, 4, HW, HW).half(), **_embeds()) for s in (0.3, 0.5, 1.0)]
    assert inpaint_batch(ipa, reqs, group=4, num_inference_steps=8).shape == (3, 4, HW, HW)
    assert log == [("update", 3)] + [("unet", 6), ("update", 3), ("blend", 3)] * 8


# ---- refusals of the serial pipelines -----------------------------------------------------------------------------------------------------------------------
class UntouchedUNet:
    """a model no refusal may reach: it has a device and nothing else"""
    device = torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError(f"a refusal came after the first use of the model (.{name})")

    def __call__(self, *a, **kw):
        raise AssertionError("a refusal came after the first use of the model")


def test_the_serial_pipelines_refuse_bad_arguments_before_touching_a_model():
    from instructany2pix_amd.ddim import SDXLDDIMPipeline, StableDiffusionXLPipeline
    from instructany2pix_amd.img2img import StableDiffusionXLImg2ImgPipeline
    from instructany2pix_amd.inpaint import StableDiffusionXLInpaintPipeline
    z, net = torch.zeros, UntouchedUNet()
    e = dict(prompt_embeds=z(1, 77, CTX), pooled_prompt_embeds=z(1, POOLED))
    neg = dict(negative_prompt_embeds=z(1, 77, CTX), negative_pooled_prompt_embeds=z(1, POOLED))
    lat = z(1, 4, HW, HW)
    inv, smp, rf, ip = SDXLDDIMPipeline(net), StableDiffusionXLPipeline(net), StableDiffusionXLImg2ImgPipeline(net), StableDiffusionXLInpaintPipeline(net)
    both = [(rf, dict(latents=lat)), (ip, dict(latents=lat, mask_image=z(HW, HW)))]
    for p, kw in both + [(inv.inverse, dict(latents=lat))]:
        with pytest.raises(ValueError, match=r"The value of strength should in \[0.0, 1.0\] but is 1.5$"):
            p(strength=1.5, **e, **neg, **kw)
    for p, kw in both:
        with pytest.raises(ValueError, match=r"strength parameter: 0.01, the number of pipeline steps is 0 which is < 1 and not appropriate for this pipeline\.$"):
            p(strength=0.01, **e, **neg, **kw)
        with pytest.raises(ValueError, match="classifier-free guidance needs negative_prompt_embeds"):
            p(**e, **kw)
        with pytest.raises(ValueError, match="Cannot forward both `prompt` and `prompt_embeds`"):
            p(prompt="a", **e, **neg, **kw)
        with pytest.raises(ValueError, match="Provide either `prompt` or `prompt_embeds`"):
            p(**kw)
        with pytest.raises(ValueError, match="`pooled_prompt_embeds` also have to be passed"):
            p(prompt_embeds=e["prompt_embeds"], **kw)
    for p, kw in ((rf, dict(latents=lat)), (inv.inverse, dict(latents=lat))):
        with pytest.raises(ValueError, match="`num_inference_steps` has to be a positive integer but is 0"):
            p(num_inference_steps=0, **e, **neg, **kw)
    with pytest.raises(ValueError, match=r"img2img needs `image` \(with vae= or a vae_encode callable\) or `latents`"):
        rf(**e, **neg)
    with pytest.raises(ValueError, match=r"inpainting needs `image` \(with vae= or a vae_encode callable\) or `latents`"):
        ip(mask_image=z(HW, HW), **e, **neg)
    with pytest.raises(ValueError, match="`mask_image` input cannot be undefined"):
        ip(latents=lat, **e, **neg)
    with pytest.raises(NotImplementedError, match="guidance_rescale / eta are inactive"):
        ip(latents=lat, mask_image=z(HW, HW), eta=0.5, **e, **neg)
    with pytest.raises(NotImplementedError, match="guidance_rescale / eta are inactive"):
        smp(guidance_rescale=0.7, **e, **neg)
    with pytest.raises(ValueError, match="classifier-free guidance needs negative_prompt_embeds"):
        smp(**e)
    with pytest.raises(ValueError, match=r"inverse\(\) needs `image`"):
        inv.inverse(**e)


def test_call_refuses_what_edit_batch_refuses_with_the_same_words():
    """the request-level refusals `__call__` and `edit_batch` share, on a pipeline object without a model"""
    from instructany2pix_amd.batch import edit_batch
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    c = dict(image_embeds=torch.ones(1, 8), base_embed=torch.ones(1, 8), caption="a")
    stub = SimpleNamespace(vae=None, ip_adapter_xl=object(), piperf=None, model=None, any2pix_lm=None, conditioner=lambda inst, mm, use_cache=False: dict(c),
                           loas_base_img=lambda path: object(), denoise=lambda *a, **kw: pytest.fail("a refusal came after the hot segment began"))
    stub._conditions_for_batch = lambda insts, mms: [stub.conditioner(i, m) for i, m in zip(insts, mms)]
    call = lambda **kw: InstructAny2PixPipeline.__call__(stub, "a", [], refinement=0.0, **kw)
    batch = lambda **kw: edit_batch(stub, ["a"], [[]], refinement=0.0, **kw)
    for fn in (call, batch):
        with pytest.raises(ValueError, match="output_type must be one of"):
            fn(output_type="jpeg")
        with pytest.raises(ValueError, match=r"output_type='pil' needs the pipeline built with vae=<HipAutoencoderKL>"):
            fn(output_type="pil")
        with pytest.raises(NotImplementedError, match="the conditioner returned no `y` and no prior= was attached"):
            fn()
    c["y"] = torch.ones(1, 8)
    stub._base_latents = lambda cond, seed=None: InstructAny2PixPipeline._base_latents(stub, cond, seed)
    with pytest.raises(KeyError, match=r"none of base_latents / base_image / base_img_path'$"):
        call()
    with pytest.raises(KeyError, match=r"none of base_latents / base_image / base_img_path \(request 0\)'$"):
        batch()
    c["base_img_path"] = "fox.png"
    for fn in (call, batch):
        with pytest.raises(ValueError, match="a base_image / base_img_path needs the pipeline built with vae=<HipAutoencoderKL>"):
            fn()
