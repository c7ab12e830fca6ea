"""End-to-end latency of ONE edit request at the reference's own defaults, every model at full size with seeded synthetic weights:
1024x1024 image, num_inference_steps=25, cfg=10, refinement=0.5 (reference pipeline.py:303-386). A seeded synthetic PIL image goes in and PIL
images come out (`output_type="pil"`); everything downstream of ImageBind runs on the HIP path: instruction LLM -> image in (8-bit codec) -> VAE
encode -> embedding prior (CLIP ViT-H text + GPT-2 medium) -> encode_prompt (CLIP-L + bigG) -> 25-step DDIM inversion (B=1) -> polar mixing
-> 25-step IP-Adapter guided CFG sampling (B_eff=2) -> VAE decode + 8-bit hand-over -> SDXL-refiner img2img (strength 0.5 of 50 steps, CFG)
-> VAE decode -> image out (8-bit codec, uint8 back to the host). The request's conditioning comes from `forward_llm`: the instruction LLM at full
size (Vicuna-7B shape) prefills the prompt and generates 100 tokens on the HIP engine, `vae_predictor_image` reads the hidden rows. Two stand-ins
remain: the ImageBind vectors of the mm_data entries are seeded 1024-d noise unless --imagebind is given (then the entries name PNG files that
`imagebind_huge`-sized towers with seeded weights encode on the HIP path, timed as their own stage), and, because synthetic weights cannot
speak, the TOKEN CHOSEN at each step follows a script ("[ caption ] <base> <video> <im_gen> <video> </s>", 100 tokens) instead of the sampled one; every step's
engine work, its logits and its sampling arithmetic still run.
Prints per-stage wall times (stream-synchronised) after one warm-up request.

--sampler device (the switch of tools/llm_decode_bench.py; also spelled --llm-sampler) draws the token on the device (`HipInstructAny2PixLM(sampler="device")`): the sampler kernel runs on every step's logits row and the
script then overwrites the id in device memory (one fill launch per step, which the product does not have), so the next decode step still reads it there.

    python tools/e2e_edit_bench.py [--llm-bits 4] [--llm-quant-type fp4|nf4] [--sampler host|device] [--top-p P] [--imagebind]      (4: the LLM loaded as the reference loads it, `load_in_4bit`)

--batch 1,4,8 measures `InstructAny2PixPipeline.edit_batch` against the serial loop instead: for each N, in this one process, N serial `__call__`s and one
`edit_batch` of the same N requests (groups of min(N, 8)) alternate --reps times after both have run once untimed (every shape warm); times are a host clock
around a device synchronise. Printed per N: per-stage ms of both (median over the repeats), total ms per image with its min..max over the repeats, images/s.
What a request carries into the timed region is what the LLM and the text encoders leave behind (`forward_llm_batch` and `encode_prompt` are measured by
tools/llm_decode_bench.py and the single-request mode): a conditioner hands every request its seeded embeddings, its prompt embeddings (encoded once, before
the clock, by the full-size text encoders) and its own 1024 x 1024 PIL image; the LLM is not built. Timed: image in, VAE encode, embedding prior, inversion,
polar mixing, guided sampling, the refiner hand-over (decode, 8-bit, encode), the refiner pass, VAE decode, image out.

    python tools/e2e_edit_bench.py --batch 1,4,8 [--reps 3] [--steps 25] [--refinement 0.5]

--seeded (with --batch) runs the same requests WITH per-request seeds (`__call__(seed=)`, `edit_batch(seeds=)`: every normal draw on the device from the request's
own Philox stream, the inverted latents never leave it) next to the unseeded run, interleaved repeat by repeat in the one process: serial, serial seeded,
edit_batch, edit_batch seeded. Its stage table gains the three seeded-noise launches ALONE (`ia2p_randn_seeded`, `ia2p_posterior_sample_seeded`, `ia2p_polar_mix_v`
at B = 1 and B = 8 on 4 x PX/8 x PX/8 latents): microseconds per launch between two device events around 200 back-to-back launches, median of 5 such trains.

    python tools/e2e_edit_bench.py --seeded --batch 1,8

--edit-mask (with --batch) runs the same requests WITH a centred square mask of half the image's area (`__call__(edit_mask=)`, `edit_batch(edit_masks=)`, the
default feather) next to the unmasked run, interleaved repeat by repeat in the one process: serial, serial masked, edit_batch, edit_batch masked. The masked path
adds one selection launch per sampling step, one blend launch per refiner step and the image launches per request; its stage table gains `edit mask` (load, upload,
`ia2p_mask_to_latent`) and `mask feather`, and its `image_out` is the 8-bit composite.

    python tools/e2e_edit_bench.py --edit-mask --batch 1,8

--auto-mask [N_MAPS] (with --batch; default 8 maps) runs the same requests WITH an automatic edit mask (`__call__(auto_mask=)`, `edit_batch(auto_masks=)`: the other knobs at
their defaults) next to the run without one, interleaved repeat by repeat in the one process: serial, serial auto-masked, edit_batch, edit_batch auto-masked. The estimate --
add_noise, two UNet evaluations of N_MAPS rows per request, the two mask launches -- is timed as a stage of its own, `mask estimate`.

    python tools/e2e_edit_bench.py --auto-mask 8 --batch 1,8

--lcm N (with --batch) runs the same requests with the guided sampling stage under the consistency sampler over N steps (`__call__(sampler="lcm", sample_steps=N)`,
`edit_batch(samplers="lcm", sample_steps=N)`; per-request seeds, so the step noise is drawn inside the update launch) next to the DDIM run, interleaved repeat by
repeat in the one process: serial, serial lcm, edit_batch, edit_batch lcm. --steps keeps governing the inversion. The stage to read is `guided sampling loop`:
N evaluations against --steps. Its table gains the two update launches ALONE (`ia2p_ddim_step_v`, `ia2p_lcm_step_v` with every row seeded, guided, B = 1 and B = 8
on 4 x PX/8 x PX/8 latents), measured like the seeded-noise launches of --seeded. Synthetic weights: the figures are times, the images mean nothing.

    python tools/e2e_edit_bench.py --lcm 4 --batch 1,4

--subjects 1,2,4 [--subject-mode serial,joint] times the SUBJECT-CONSISTENCY STAGE of one full-size request alone (`inpaint.subject_consistency` on PX/8 x PX/8
latents: 50 steps at strength 0.7 = 35 UNet evaluations of 2 rows per loop, IP scale 0.8, guidance 7.5): for each S, the serial form (S loops) and the joint form
(one loop under regional image prompts, `ia2p_unet_forward_r`) alternate --reps times after both have run once untimed; a host clock around a device synchronise.
Only the base UNet and the IP-Adapter are built. Printed per S: ms per stage of both (median, min..max), serial / joint, and ms per UNet step of the regional route
against the plain one (stage time over the loop's steps; the image-token projection and the start launch are in it).

    python tools/e2e_edit_bench.py --subjects 1,2,4 --subject-mode serial,joint

--control times the GUIDED SAMPLING STAGE of one full-size request alone (`IPAdapterXL.generate` over `StableDiffusionXLControlNetPipeline`: --steps steps, guidance 10,
B_eff = 2) with and without a full-size ControlNet of seeded synthetic weights (scale 1, the whole window): the two sides alternate --reps times after both have run once
untimed; a host clock around a device synchronise. Only the base UNet, the IP-Adapter and the ControlNet are built. Printed: ms per stage of both (median, min..max), ms
per step of both and their ratio (a controlled step is one ControlNet evaluation -- the UNet's down path and mid block, ten small GEMMs -- plus the UNet with ten
injections: dearer than two plain steps would mean something is wrong), and the one-off cost of `embed_condition` (median of --reps, the condition image on the device).
The uncontrolled side is the plain pipeline's call: it is the number to hold against another build's.

    python tools/e2e_edit_bench.py --control [--steps 25] [--reps 5]"""
import argparse
import os
import sys
import time
import numpy as np
import PIL.Image
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from stub_tokenizer import StubTokenizer
from instructany2pix_amd.clip import HipCLIPTextModel, SDXLTextEncoders
from instructany2pix_amd.config import sdxl_base, sdxl_refiner, sdxl_vae, sdxl_text_encoder, sdxl_text_encoder_2
from instructany2pix_amd.pipeline import InstructAny2PixPipeline
from instructany2pix_amd.prior import InstructAny2PixPrior, prior_config
from instructany2pix_amd.unet import HipUNet2DConditionModel
from instructany2pix_amd.vae import HipAutoencoderKL
from instructany2pix_amd.weights import (unet_param_specs, ip_adapter_specs, vae_param_specs, clip_param_specs, prior_param_specs,
                                         iter_synthetic, synthetic_state_dict)
from instructany2pix_amd.config import gpt2_medium, laion_clip_h_text, vicuna_7b
import instructany2pix_amd.llm as llm_mod
from instructany2pix_amd.weights import llm_param_specs
from stub_llm_tokenizer import ADDED_TOKENS, StubLlamaTokenizer

_ap = argparse.ArgumentParser()
_ap.add_argument("--llm-bits", type=int, default=16, choices=(16, 4))
_ap.add_argument("--llm-quant-type", default="fp4", choices=("fp4", "nf4"))
_ap.add_argument("--sampler", "--llm-sampler", dest="llm_sampler", default="host", choices=("host", "device"))
_ap.add_argument("--top-p", type=float, default=None, help="nucleus of the LLM's sampler, as a checkpoint's generation_config.json would set it (default: none, top_p = 1)")
_ap.add_argument("--imagebind", action="store_true", help="encode the mm_data entries' files with the HIP ImageBind towers instead of seeded vectors")
_ap.add_argument("--batch", default=None, help="comma-separated request counts: compare edit_batch with the serial loop (see the module docstring)")
_ap.add_argument("--reps", type=int, default=3)
_ap.add_argument("--seeded", action="store_true", help="with --batch: the same requests with per-request seeds next to the unseeded run, and the three noise launches alone")
_ap.add_argument("--edit-mask", action="store_true", help="with --batch: the same requests with a centred half-area edit mask next to the unmasked run")
_ap.add_argument("--auto-mask", type=int, nargs="?", const=8, default=None, metavar="N_MAPS", help="with --batch: the same requests with an automatic edit mask of N_MAPS maps next to the run without")
_ap.add_argument("--lcm", type=int, default=None, metavar="N", help="with --batch: the same requests sampled by the N-step consistency sampler next to the DDIM run, and the two update launches alone")
_ap.add_argument("--subjects", default=None, help="comma-separated subject counts: time the subject-consistency stage of one request alone (see the module docstring)")
_ap.add_argument("--subject-mode", default="serial,joint", help="with --subjects: the forms to time, interleaved")
_ap.add_argument("--control", action="store_true", help="time the guided sampling stage of one request with and without a ControlNet (see the module docstring)")
_ap.add_argument("--steps", type=int, default=25)
_ap.add_argument("--refinement", type=float, default=0.5)
ARGS = _ap.parse_args()
if ARGS.seeded and not ARGS.batch:
    _ap.error("--seeded compares against the unseeded run of --batch: give --batch too")
if ARGS.edit_mask and not ARGS.batch:
    _ap.error("--edit-mask compares against the unmasked run of --batch: give --batch too")
if ARGS.auto_mask is not None and not ARGS.batch:
    _ap.error("--auto-mask compares against the run without a mask of --batch: give --batch too")
if ARGS.lcm is not None and not ARGS.batch:
    _ap.error("--lcm compares against the DDIM run of --batch: give --batch too")
BATCHES = [int(n) for n in ARGS.batch.split(",")] if ARGS.batch else []
DEV = "cuda:0"
PX = int(os.environ.get("PX", 1024))
t_all = time.perf_counter()
bcfg, rcfg, vcfg = sdxl_base(), sdxl_refiner(), sdxl_vae()
base = HipUNet2DConditionModel(bcfg, DEV); base.load_state_dict(iter_synthetic(unet_param_specs(bcfg), 7, DEV, torch.float16))
if ARGS.control:
    import statistics
    from instructany2pix_amd.config import controlnet_sdxl
    from instructany2pix_amd.controlnet import HipControlNetModel
    from instructany2pix_amd.ddim import StableDiffusionXLControlNetPipeline
    from instructany2pix_amd.ip_adapter import IPAdapterXL
    from instructany2pix_amd.weights import controlnet_param_specs
    ccfg = controlnet_sdxl()
    cn = HipControlNetModel(ccfg, DEV); cn.load_state_dict(iter_synthetic(controlnet_param_specs(ccfg), 13, DEV, torch.float16))
    specs = ip_adapter_specs(bcfg, 1024)
    ipa = IPAdapterXL(StableDiffusionXLControlNetPipeline(base, cn), "", ip_ckpt={"image_proj": synthetic_state_dict(specs["image_proj"], seed=7),
                                                                                "ip_adapter": synthetic_state_dict(specs["ip_adapter"], seed=7)}, device=DEV, clip_embeddings_dim=1024)
    print(f"models ready in {time.perf_counter() - t_all:.1f} s (base UNet + IP-Adapter, ControlNet: arena {cn.arena.numel() / 1e9:.2f} GB)", flush=True)
    gg = torch.Generator().manual_seed(3)
    rn = lambda *sh: torch.randn(*sh, generator=gg)      # noqa: E731
    hl = PX // 8
    kw = dict(clip_image_embeds=rn(1024), prompt_embeds=rn(1, 77, bcfg.cross_attention_dim).half(), pooled_prompt_embeds=rn(1, bcfg.pooled_dim).half(),
              negative_prompt_embeds=rn(1, 77, bcfg.cross_attention_dim).half(), negative_pooled_prompt_embeds=rn(1, bcfg.pooled_dim).half(),
              latents=rn(1, 4, hl, hl).half(), num_inference_steps=ARGS.steps, guidance_scale=10, scale=1.0, output_type="latent")
    cond = torch.rand(1, 3, PX, PX, generator=gg).half().to(DEV)

    def stage(controlled):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = ipa.generate(**kw, **(dict(image=cond, controlnet_conditioning_scale=1.0) if controlled else {}))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.float()).all())
        return (time.perf_counter() - t0) * 1e3

    def embed():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        cn.embed_condition(cond)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    print(f"# {PX} x {PX}, guided sampling stage alone: {ARGS.steps} steps, guidance 10, B_eff = 2; {ARGS.reps} alternating repeats after one untimed run of each; cost-model plans", flush=True)
    for c_ in (False, True):
        stage(c_)
    embed()
    ms = {False: [], True: []}
    for _ in range(ARGS.reps):
        for c_ in (False, True):
            ms[c_].append(stage(c_))
    em = [embed() for _ in range(ARGS.reps)]
    med = {c_: statistics.median(v) for c_, v in ms.items()}
    print("; ".join(f"{'controlled' if c_ else 'plain'} {med[c_]:.1f} ms (min {min(v):.1f}, max {max(v):.1f})" for c_, v in ms.items()), flush=True)
    print(f"ms per step: plain {med[False] / ARGS.steps:.2f}, controlled {med[True] / ARGS.steps:.2f}, "
          f"controlled / plain {med[True] / med[False]:.3f}; embed_condition alone {statistics.median(em):.2f} ms (min {min(em):.2f}, max {max(em):.2f})", flush=True)
    sys.exit(0)
ref = HipUNet2DConditionModel(rcfg, DEV); ref.load_state_dict(iter_synthetic(unet_param_specs(rcfg), 11, DEV, torch.float16))
if ARGS.subjects:
    import statistics
    from instructany2pix_amd.inpaint import StableDiffusionXLInpaintPipeline, subject_consistency
    from instructany2pix_amd.ip_adapter import IPAdapterXL
    specs = ip_adapter_specs(bcfg, 1024)
    ipa = IPAdapterXL(StableDiffusionXLInpaintPipeline(base), "", ip_ckpt={"image_proj": synthetic_state_dict(specs["image_proj"], seed=7),
                                                                          "ip_adapter": synthetic_state_dict(specs["ip_adapter"], seed=7)}, device=DEV, clip_embeddings_dim=1024)
    print(f"models ready in {time.perf_counter() - t_all:.1f} s (base UNet + IP-Adapter)", flush=True)
    gg = torch.Generator().manual_seed(3)
    rn = lambda *sh: torch.randn(*sh, generator=gg)      # noqa: E731
    hl = PX // 8
    emb = dict(prompt_embeds=rn(1, 77, bcfg.cross_attention_dim).half(), pooled_prompt_embeds=rn(1, bcfg.pooled_dim).half(),
               negative_prompt_embeds=rn(1, 77, bcfg.cross_attention_dim).half(), negative_pooled_prompt_embeds=rn(1, bcfg.pooled_dim).half())
    lat, noise = rn(1, 4, hl, hl).half().to(DEV), rn(1, 4, hl, hl).half().to(DEV)
    modes = ARGS.subject_mode.split(",")
    assert all(m in ("serial", "joint") for m in modes)
    STEPS = 35      # 50 steps at strength 0.7
    print(f"# {PX} x {PX}, subject stage alone: 50 steps at strength 0.7 = {STEPS} UNet evaluations of 2 rows per loop; {ARGS.reps} alternating repeats after one untimed run of each", flush=True)
    for S in (int(n) for n in ARGS.subjects.split(",")):
        data = []
        for k in range(S):      # S overlapping pixel-space rectangles, each about a quarter of the image
            mk = torch.zeros(PX, PX)
            y0, x0 = (PX // 8) * (k % 4), (PX // 8) * ((k // 2) % 4)
            mk[y0:y0 + PX // 2, x0:x0 + PX // 2] = 1.0
            data.append((mk, rn(1024)))

        def stage(mode):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = subject_consistency(data, lat, ipa, 0.7, joint=mode == "joint", output_type="latent", noise=noise, **emb)
            torch.cuda.synchronize()
            assert out.shape == lat.shape and bool(torch.isfinite(out.float()).all())
            return (time.perf_counter() - t0) * 1e3

        for m in modes:
            stage(m)
        ms = {m: [] for m in modes}
        for _ in range(ARGS.reps):
            for m in modes:
                ms[m].append(stage(m))
        med = {m: statistics.median(v) for m, v in ms.items()}
        line = f"S = {S}: " + ", ".join(f"{m} {med[m]:.1f} ms (min {min(v):.1f}, max {max(v):.1f})" for m, v in ms.items())
        if len(med) == 2:
            line += f"; serial / joint {med['serial'] / med['joint']:.3f}; ms per UNet step: plain route {med['serial'] / (S * STEPS):.2f}, regional route {med['joint'] / STEPS:.2f}"
        print(line, flush=True)
    sys.exit(0)
vae = HipAutoencoderKL(vcfg, DEV); vae.load_state_dict(iter_synthetic(vae_param_specs(vcfg), 5, DEV, torch.float16))
c1, c2 = sdxl_text_encoder(), sdxl_text_encoder_2()
te1 = HipCLIPTextModel(c1, DEV); te1.load_state_dict(iter_synthetic(clip_param_specs(c1), 7, DEV, torch.float16))
te2 = HipCLIPTextModel(c2, DEV); te2.load_state_dict(iter_synthetic(clip_param_specs(c2), 8, DEV, torch.float16))
enc = SDXLTextEncoders(StubTokenizer(1, c1.vocab_size), StubTokenizer(2, c2.vocab_size), te1, te2)
enc_ref = SDXLTextEncoders(None, StubTokenizer(2, c2.vocab_size), None, te2)           # the refiner checkpoint has text encoder 2 only
prior = InstructAny2PixPrior(**prior_config, device=DEV, tokenizer=StubTokenizer(5, laion_clip_h_text().vocab_size))
prior.load_state_dict(synthetic_state_dict(prior_param_specs(gpt2_medium(), laion_clip_h_text()), seed=47))
specs = ip_adapter_specs(bcfg, 1024)
ck = {"image_proj": synthetic_state_dict(specs["image_proj"], seed=7), "ip_adapter": synthetic_state_dict(specs["ip_adapter"], seed=7)}
lcfg = vicuna_7b(32000 + len(ADDED_TOKENS))
ltok = StubLlamaTokenizer(32000)
lm = None
if not BATCHES:
    lm = llm_mod.HipInstructAny2PixLM(lcfg, DEV, max_positions=512, load_in_4bit=ARGS.llm_bits == 4, bnb_4bit_quant_type=ARGS.llm_quant_type,
                                      sampler=ARGS.llm_sampler)
    lm.load_state_dict(iter_synthetic(llm_param_specs(lcfg), 9, DEV, torch.float16))
    if ARGS.top_p is not None:      # forward_llm passes no top_p: it reaches `generate` the way a loaded generation config does
        lm.load_generation_config({"top_p": ARGS.top_p})
    print(f"models ready in {time.perf_counter() - t_all:.1f} s (base UNet + IP-Adapter, refiner UNet, VAE, CLIP-L, bigG, prior, LLM with {lm.weight_bits}-bit "
          f"projections: arena {lm.arena.numel() / 1e9:.2f} GB)", flush=True)
else:
    print(f"models ready in {time.perf_counter() - t_all:.1f} s (base UNet + IP-Adapter, refiner UNet, VAE, CLIP-L, bigG, prior; no LLM in --batch mode)", flush=True)

stages = {}


def timed(name, fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(); stages[name] = stages.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
    return out


g = torch.Generator().manual_seed(1)
image = PIL.Image.fromarray(np.random.default_rng(1).integers(0, 256, size=(PX, PX, 3), dtype=np.uint8))      # the base image (reference: loas_base_img)
# the scripted reply: 100 tokens, "[ <93 caption words> ] <base> <video> <im_gen> <video> </s>" (two mm_data entries: the base image is chosen by the `<base>` rule)
SCRIPT = ltok("[ " + " ".join(f"word{i}" for i in range(93)) + " ] <base> <video> <im_gen> <video> </s>", add_special_tokens=False).input_ids
assert len(SCRIPT) == 100
_sample_next, _script = llm_mod.sample_next, iter(())


def scripted_sample_next(logits, *a, **k):
    _sample_next(logits, *a, **k)                       # the sampling arithmetic of the step still runs (and draws from the RNG)
    return torch.tensor([next(_script)])


llm_mod.sample_next = scripted_sample_next
_sample_tokens = lm.sample_tokens if lm is not None else None


def scripted_sample_tokens(logits, *a, **k):
    out = _sample_tokens(logits, *a, **k)               # the sampler kernel of the step still runs
    return out.fill_(next(_script))                     # (stream-ordered behind it: the look-ahead decode reads the scripted id)


if lm is not None:
    lm.sample_tokens = scripted_sample_tokens
mm_data = [{"type": "image", "fname": "base.png", "image": image, "embed": torch.randn(1024, generator=g)},
           {"type": "image", "fname": "style.png", "image": image, "embed": torch.randn(1024, generator=g)}]      # (either may be chosen as the base)
imb = None
if ARGS.imagebind:              # the entries carry files instead of vectors: `_modality_embeds` runs them through the vision tower as one batch
    import tempfile
    from instructany2pix_amd.imagebind import HipImageBindModel, imagebind_huge_config, imagebind_param_specs
    imb = HipImageBindModel(imagebind_huge_config(), DEV, modalities=("vision",))
    imb.load_state_dict(iter_synthetic(imagebind_param_specs(imb.config, ("vision",)), 13, DEV, torch.float16))
    _dir = tempfile.mkdtemp(prefix="ia2p_e2e_")
    for r in mm_data:
        r["fname"] = os.path.join(_dir, r["fname"])
        image.save(r["fname"])
        del r["embed"]
pipe = InstructAny2PixPipeline(unet=base, ip_ckpt=ck, device=DEV, clip_embeddings_dim=1024, refiner_unet=ref, prior=prior, vae=vae,
                               llm=lm, llm_tokenizer=ltok, imagebind=imb,
                               text_encoder=lambda **k: timed("encode_prompt(base, inversion '')", lambda: enc.encode_prompt(**k)),
                               refiner_text_encoder=lambda **k: timed("encode_prompt(refiner)", lambda: enc_ref.encode_prompt(**k)))
if os.environ.get("TUNE", "0" if BATCHES else "1") == "1":      # measure kernel plans for the three UNet shapes of a request (what bench.py does for its shape)
    t0 = time.perf_counter()
    h = PX // 8
    for net, B, L, cd, pd, nid in ((base, 1, 77, bcfg.cross_attention_dim, bcfg.pooled_dim, 6), (base, 2, 81, bcfg.cross_attention_dim, bcfg.pooled_dim, 6),
                                   (ref, 2, 77, rcfg.cross_attention_dim, rcfg.pooled_dim, 5)):
        x = torch.randn(B, 4, h, h, generator=g).half().to(DEV)
        ehs = torch.randn(B, L, cd, generator=g).half().to(DEV)
        added = dict(text_embeds=torch.randn(B, pd, generator=g).half().to(DEV), time_ids=torch.tensor([[float(PX)] * 2 + [0.0] * 2 + [float(PX)] * (nid - 4)] * B).half().to(DEV))
        net.autotune(x, 500, ehs, added, reps=3)
    print(f"kernel plans measured in {time.perf_counter() - t0:.1f} s", flush=True)
# stage timers around the four loops of a request (synchronising wrappers: they add a few host round trips, nothing else)
def _wrap(obj, name, label):
    fn = getattr(obj, name)
    setattr(obj, name, lambda *a, **k: timed(label, lambda: fn(*a, **k)))


LABEL = (lambda long, short: short) if BATCHES else (lambda long, short: long)      # --batch: one label per stage for the serial and the batched side
_wrap(pipe.pipe_inversion, "inverse", LABEL("inversion loop (25 x B=1)", "inversion loop"))
_wrap(pipe.pipe_inversion.image_processor, "preprocess", "image_in")
_wrap(pipe.pipe_inversion, "_vae_encode", "vae_encode")
_wrap(pipe.pipe, "_vae_decode", LABEL("vae_decode (hand-over + 2 outputs)", "vae_decode"))
_wrap(pipe.pipe.image_processor, "postprocess", "image_out")
_wrap(pipe.ip_adapter_xl, "generate", LABEL("guided sampling loop (25 x B_eff=2, incl. image-token projection)", "guided sampling loop"))
if imb is not None:
    _wrap(pipe, "_modality_embeds", "ImageBind (2 PNG files: load, transform, vision tower; inside forward_llm)")
if lm is not None:
    _wrap(pipe, "forward_llm", f"LLM (forward_llm: prefill + 100 tokens + predictor heads, {ARGS.llm_sampler} sampler)")
if getattr(pipe, "model", None) is not None:
    _wrap(pipe.model, "generate_diffusion", "embedding prior")
_piperf_call = pipe.piperf.__call__
pipe.piperf = type("TimedRefiner", (), {"__call__": lambda self, *a, **k: timed("refiner pass", lambda: _piperf_call(*a, **k)),
                                        "__getattr__": lambda self, n: getattr(_piperf_call.__self__, n)})()
_wrap(pipe.piperf, "_vae_encode", "vae_encode (refiner hand-over)")
for rnd in range(0 if BATCHES else 2):            # request 0 warms up (workspaces, kernel plans from the cost model), request 1 is reported
    stages.clear()
    torch.manual_seed(3)
    _script = iter(SCRIPT)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    non_refined, refined, msg = pipe("add <video> to <video> and turn the fox blue", mm_data, num_inference_steps=25, cfg=10, refinement=0.5, output_type="pil")
    torch.cuda.synchronize(); total = (time.perf_counter() - t0) * 1e3
    assert msg == "SUCCESS!" and all(isinstance(o, list) and o[0].size == (PX, PX) and o[0].mode == "RGB" for o in (non_refined, refined))
    outer = sum(v for k, v in stages.items() if not k.startswith("ImageBind"))      # (the ImageBind stage is part of forward_llm's)
    print(f"request {rnd}: {total:.0f} ms total; stages (ms): " + ", ".join(f"{k} {v:.1f}" for k, v in stages.items())
          + f", host glue / the rest {total - outer:.0f}", flush=True)


# ---- --batch: N serial calls against one edit_batch of the same requests ---------------------------------------------------------------------------------
if BATCHES:
    import statistics
    import instructany2pix_amd.auto_mask as auto_mod
    import instructany2pix_amd.batch as batch_mod
    import instructany2pix_amd.image_processor as ip_mod
    import instructany2pix_amd.pipeline as pipeline_mod
    _wrap(pipeline_mod, "composite_edit", "image_out")              # the masked path's image out: 8-bit codec + composite
    _wrap(pipeline_mod, "resolve_edit_mask", "edit mask")
    _wrap(ip_mod, "mask_feather", "mask feather")
    _wrap(auto_mod, "estimate_group", "mask estimate")
    for _name, _label in (("invert_batch", "inversion loop"), ("sample_batch", "guided sampling loop"), ("refine_batch", "refiner pass")):
        _wrap(batch_mod, _name, _label)
    NMAX = max(BATCHES)
    rng = np.random.default_rng(2)
    images = [PIL.Image.fromarray(rng.integers(0, 256, size=(PX, PX, 3), dtype=np.uint8)) for _ in range(NMAX)]
    insts = [f"request {i}: turn the fox blue" for i in range(NMAX)]
    conds = {}
    ipe, _, ipp, _ = enc.encode_prompt(prompt="", do_classifier_free_guidance=False)
    for i, inst in enumerate(insts):            # what forward_llm + encode_prompt leave behind, made once, before the clock
        cap = f" a blue fox, variation {i}"
        pe, ne, pp, npl = enc.encode_prompt(prompt="best quality, high quality" + cap, negative_prompt="", do_classifier_free_guidance=True)
        rpe, rne, rpp, rnp = enc_ref.encode_prompt(prompt=cap + ",high quality,well-formed,award-winning", negative_prompt="", do_classifier_free_guidance=True)
        conds[inst] = dict(image_embeds=torch.randn(1, 1024, generator=g), base_embed=torch.randn(1, 1024, generator=g), caption=cap, base_image=images[i],
                           prompt_embeds=pe, pooled_prompt_embeds=pp, negative_prompt_embeds=ne, negative_pooled_prompt_embeds=npl, inv_prompt_embeds=ipe,
                           inv_pooled_prompt_embeds=ipp, refiner_prompt_embeds=rpe, refiner_pooled_prompt_embeds=rpp, refiner_negative_prompt_embeds=rne,
                           refiner_negative_pooled_prompt_embeds=rnp)
    pipe.conditioner = lambda inst, mm, use_cache=False: conds[inst]
    knobs = dict(num_inference_steps=ARGS.steps, cfg=10, refinement=ARGS.refinement, output_type="pil")

    def serial(n):
        return [pipe(inst, [], **knobs) for inst in insts[:n]]

    def batched(n):
        return pipe.edit_batch(insts[:n], [[]] * n, group=min(n, 8), **knobs)

    SEEDS = [0x5EED0000 + 977 * i for i in range(NMAX)]

    def serial_seeded(n):
        return [pipe(inst, [], seed=SEEDS[i], **knobs) for i, inst in enumerate(insts[:n])]

    def batched_seeded(n):
        return pipe.edit_batch(insts[:n], [[]] * n, group=min(n, 8), seeds=SEEDS[:n], **knobs)

    side_px = int(round(PX / 2 ** 0.5))            # a centred square of half the area
    MASK = np.zeros((PX, PX), np.uint8)
    MASK[(PX - side_px) // 2:(PX + side_px) // 2, (PX - side_px) // 2:(PX + side_px) // 2] = 255

    def serial_masked(n):
        return [pipe(inst, [], edit_mask=MASK, **knobs) for inst in insts[:n]]

    def batched_masked(n):
        return pipe.edit_batch(insts[:n], [[]] * n, group=min(n, 8), edit_masks=MASK, **knobs)

    AUTO = None if ARGS.auto_mask is None else dict(num_maps=ARGS.auto_mask)

    def serial_auto(n):
        return [pipe(inst, [], auto_mask=AUTO, **knobs) for inst in insts[:n]]

    def batched_auto(n):
        return pipe.edit_batch(insts[:n], [[]] * n, group=min(n, 8), auto_masks=AUTO, **knobs)

    def serial_lcm(n):
        return [pipe(inst, [], seed=SEEDS[i], sampler="lcm", sample_steps=ARGS.lcm, **knobs) for i, inst in enumerate(insts[:n])]

    def batched_lcm(n):
        return pipe.edit_batch(insts[:n], [[]] * n, group=min(n, 8), seeds=SEEDS[:n], samplers="lcm", sample_steps=ARGS.lcm, **knobs)

    def updates_alone():
        """the DDIM and the LCM update launch on their own, guided: us per launch, median of 5 trains of 200 launches between two device events"""
        import statistics as st_
        from instructany2pix_amd import noise, scheduler
        h = PX // 8
        rows = []
        for B in (1, 8):
            x, eu, ec = (noise.randn_seeded([k + 1] * B, 9, (4, h, h), torch.float16, DEV) for k in range(3))
            out, out2 = torch.empty_like(x), torch.empty_like(x)
            c3 = torch.tensor([[10.0, 1.02, -0.05]] * B).to(DEV)
            c4 = torch.tensor([[10.0, 2.31, -2.25, 0.85]] * B).to(DEV)
            seeds, draws, firsts = [SEEDS[0] + b for b in range(B)], [noise.DRAW_LCM] * B, [noise.lcm_first(1, 4 * h * h)] * B
            work = {"ia2p_ddim_step_v": lambda: scheduler.fused_update_v(x, eu, ec, c3, out, out2),
                    "ia2p_lcm_step_v": lambda: scheduler.lcm_update_v(x, eu, ec, c4, out, out2, seeds=seeds, draws=draws, firsts=firsts)}
            for name, fn in work.items():
                for _ in range(20):
                    fn()
                us = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(200):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    us.append(e0.elapsed_time(e1) * 1e3 / 200)
                rows.append(f"{name} B={B} {st_.median(us):.1f} (min {min(us):.1f}, max {max(us):.1f})")
        print(f"# sampler update launches alone, guided, 4 x {h} x {h} latents, us per launch incl. the Python call: " + "; ".join(rows), flush=True)

    def launches_alone():
        """the three seeded-noise launches on their own: us per launch, median of 5 trains of 200 launches between two device events"""
        import statistics as st_
        from instructany2pix_amd import noise
        h = PX // 8
        rows = []
        for B in (1, 8):
            seeds = SEEDS[:1] * B if NMAX < B else SEEDS[:B]
            z = torch.empty(B, 4, h, h, dtype=torch.float16, device=DEV)
            x = noise.randn_seeded(seeds, 9, (4, h, h), torch.float16, DEV)
            mom = noise.randn_seeded(seeds, 8, (8, h, h), torch.float16, DEV)
            work = {"ia2p_randn_seeded": lambda: noise.randn_seeded(seeds, noise.DRAW_POLAR, (4, h, h), torch.float16, DEV, out=z),
                    "ia2p_posterior_sample_seeded": lambda: noise.posterior_sample(mom, seeds, noise.DRAW_BASE_POSTERIOR, 0.13025),
                    "ia2p_polar_mix_v": lambda: noise.polar_mix(x, z, 0.7)}
            for name, fn in work.items():
                for _ in range(20):
                    fn()
                us = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(200):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    us.append(e0.elapsed_time(e1) * 1e3 / 200)
                rows.append(f"{name} B={B} {st_.median(us):.1f} (min {min(us):.1f}, max {max(us):.1f})")
        print(f"# seeded-noise launches alone, 4 x {h} x {h} latents, us per launch incl. the Python call (posterior_sample and polar_mix allocate their output): "
              + "; ".join(rows), flush=True)

    def run(fn, n):
        stages.clear()
        torch.manual_seed(3)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn(n)
        torch.cuda.synchronize(); total = (time.perf_counter() - t0) * 1e3
        assert len(out) == n and all(msg == "SUCCESS!" and oo[0].size == (PX, PX) for _, oo, msg in out)
        return total, dict(stages)

    print(f"# {PX} x {PX}, {ARGS.steps} steps, cfg 10, refinement {ARGS.refinement}, output_type pil; {ARGS.reps} alternating repeats after one untimed run of each; "
          f"kernel plans: {'measured for the single-request shapes' if os.environ.get('TUNE', '0') == '1' else 'cost model'}", flush=True)
    for n in BATCHES:
        run(serial, n), run(batched, n)             # every shape warm: workspaces, plans
        runs = {"serial": [], "edit_batch": []}
        sides = [("serial", serial), ("edit_batch", batched)]
        if ARGS.seeded:
            run(serial_seeded, n), run(batched_seeded, n)
            runs = {"serial": [], "serial seeded": [], "edit_batch": [], "edit_batch seeded": []}
            sides = [("serial", serial), ("serial seeded", serial_seeded), ("edit_batch", batched), ("edit_batch seeded", batched_seeded)]
        if ARGS.edit_mask:
            run(serial_masked, n), run(batched_masked, n)
            runs.update({"serial masked": [], "edit_batch masked": []})
            sides += [("serial masked", serial_masked), ("edit_batch masked", batched_masked)]
        if AUTO is not None:
            run(serial_auto, n), run(batched_auto, n)
            runs.update({"serial auto-masked": [], "edit_batch auto-masked": []})
            sides += [("serial auto-masked", serial_auto), ("edit_batch auto-masked", batched_auto)]
        if ARGS.lcm is not None:
            run(serial_lcm, n), run(batched_lcm, n)
            runs.update({"serial lcm": [], "edit_batch lcm": []})
            sides += [("serial lcm", serial_lcm), ("edit_batch lcm", batched_lcm)]
        for _ in range(ARGS.reps):
            for side, fn in sides:
                runs[side].append(run(fn, n))
        print(f"N = {n} (group {min(n, 8)}, B_eff = {2 * min(n, 8)} in the guided loops)", flush=True)
        per_image = {}
        for side, rr in runs.items():
            tot = [t / n for t, _ in rr]
            per_image[side] = statistics.median(tot)
            names = list(rr[0][1])
            st = {k: statistics.median(s_.get(k, 0.0) for _, s_ in rr) for k in names}
            glue = per_image[side] * n - sum(st.values())
            print(f"  {side:17s}: {per_image[side]:8.1f} ms / image (min {min(tot):.1f}, max {max(tot):.1f} over {ARGS.reps}), {1e3 / per_image[side]:.3f} images/s; "
                  f"stages, ms per call of {n}: " + ", ".join(f"{k} {v:.1f}" for k, v in st.items()) + f", host glue / the rest {glue:.0f}", flush=True)
        print(f"  per image, edit_batch / serial: {per_image['edit_batch'] / per_image['serial']:.3f}", flush=True)
        if ARGS.seeded:
            print(f"  per image, seeded / unseeded: serial {per_image['serial seeded'] / per_image['serial']:.4f}, "
                  f"edit_batch {per_image['edit_batch seeded'] / per_image['edit_batch']:.4f}", flush=True)
        if ARGS.edit_mask:
            print(f"  per image, masked / unmasked: serial {per_image['serial masked'] / per_image['serial']:.4f}, "
                  f"edit_batch {per_image['edit_batch masked'] / per_image['edit_batch']:.4f}", flush=True)
        if AUTO is not None:
            print(f"  per image, auto-masked / without: serial {per_image['serial auto-masked'] / per_image['serial']:.4f}, "
                  f"edit_batch {per_image['edit_batch auto-masked'] / per_image['edit_batch']:.4f}", flush=True)
        if ARGS.lcm is not None:
            print(f"  per image, lcm ({ARGS.lcm} steps) / ddim ({ARGS.steps} steps): serial {per_image['serial lcm'] / per_image['serial']:.4f}, "
                  f"edit_batch {per_image['edit_batch lcm'] / per_image['edit_batch']:.4f}", flush=True)
    if ARGS.seeded:
        launches_alone()
    if ARGS.lcm is not None:
        updates_alone()
