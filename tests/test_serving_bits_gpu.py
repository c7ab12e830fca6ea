"""Host-side refactors of the serving paths leave every output bit alone: sha256 of the output bytes of the batched loops (`denoise_batch`, `refine_batch`,
`inpaint_batch`, `edit_batch`) and of the serial entry points they mirror (`inverse`, the three pipelines' `__call__`, `InstructAny2PixPipeline.__call__`), one
digest per case. Recorded on an MI355X from the parent of the commit that folded the serial and the batched host code into shared helpers (schedule tables,
conditioning, noise precedence, group driver, request-level stages), in the manner of tests/test_parent_bits_gpu.py. A digest that differs is a finding to
explain from the code, not a number to record again.

Cost-model plans only; the tiny configs, synthetic weights (seeds 7 / 11 / 7) and conditioners of tests/test_edit_batch_gpu.py; 16 x 16 latents; every case sets
`torch.manual_seed` and the shared processors' scale first, so that it gives the same bits alone and in any order."""
import hashlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_batch_gpu import _requests  # noqa: E402
from test_edit_batch_gpu import INPAINT_STRENGTHS, N_STEPS, REFINE_STRENGTHS, Models, _cond, _inpaint_requests, _refine_requests  # noqa: E402

pytestmark = pytest.mark.gpu

PARENT = {
    "denoise_group4": "0f5170aa39c4c32ae53ba2d89525ab060bde03b9243d3750d54bd14c51adf26c",
    "denoise_five_in_groups_of_two": "ef6b2e1e2e813c3ce5e6f1177d3635ecb7be2ff53e33da71bb5234eb7bc3fa9d",
    "denoise_mixed_noise_sources": "71593de65e955344aee3803455cfe777216b686243b11a098e7d74e5f4d2e2bb",
    "refine": "0bf6d8d7fd8393d58e4663c5d13eeb5092c0710a0bfc1d2b1877aac38800d7d5",
    "inpaint": "8971d0776f74828364701949cb5432d85d09caa4e47a8964eab91eddb43d9b87",
    "edit_seeded": "f771a99a56555e18d51ababf93fc8f3e0883ca4f0ffbbfc0221e397364f93a61",
    "edit_unseeded": "92d67dbd949b1b13ebc87f5c8a509f30e37499e4041d9e854e29f2c3949d53ef",
    "serial_inverse": "41cb8d9a237235c6fa760573722860724fa266e8248aa449f38e71b83cdc60dc",
    "serial_sample_guided": "410e48d954980b0a8035e83a9a681bb4ddf4e9b4e540b5face1736b20eaf9b51",
    "serial_sample_unguided": "9cad8e0dd427c1cea75037081f59ec2e9946c126111b68b18e5842ddcceed176",
    "serial_img2img_guided": "8131f56e8561e59537ab901b534b2d717ae48ad7a5361e89388f7dd09eae8148",
    "serial_img2img_unguided": "e0b65e51fe930d7e98a53d6c107ce9884c8f8dca18811b27a378ff391cb184e4",
    "serial_inpaint_strength_07": "b5409e6cf3df39a55f100d5a5dc7e9931a93efd923d30caace162b14bb225811",
    "serial_inpaint_strength_10": "4e2beaf3f3848ea8f5791c687fbdb793caec33694ed7231fd6f0a24c84fc0f24",
    "serial_call_seeded": "cdf4d5c3cf316ae7407b236e066d11f02b6e83fbe55373625c553e5210ad3fb1",
    "serial_call_unseeded": "2c74fbafd7e9707c576bc567cc29fcfb7d00c9539e434c10321432fada701b45",
}

P = ("prompt_embeds", "pooled_prompt_embeds", "negative_prompt_embeds", "negative_pooled_prompt_embeds")
EDIT_KW = dict(num_inference_steps=3, cfg=4.0, refinement=0.1, subject_strength=0.1)      # 3 DDIM steps each way, 5 refiner steps, 5 steps per subject pass


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def models():
    return Models()


def _start(pipe, seed):
    torch.manual_seed(seed)
    pipe.ip_adapter_xl.set_scale(1.0)            # the serial `generate` calls leave their own scale on the shared processors
    return pipe


# ---- the batched loops ------------------------------------------------------------------------------------------------------------------------------------
def denoise_group4(m):
    pipe = _start(m.pipeline(), 1)
    return sha(*pipe.denoise_batch(_requests(m.bcfg, 4), group=4))                # 6 / 4 / 5 / 6 steps, noise supplied


def denoise_five_in_groups_of_two(m):
    pipe = _start(m.pipeline(), 1)
    return sha(*pipe.denoise_batch(_requests(m.bcfg, 5, seed=9), group=2))


def denoise_mixed_noise_sources(m):
    """two seeded requests, one that draws from the global generator, one with its noise supplied, in one group"""
    pipe = _start(m.pipeline(), 2)
    reqs = _requests(m.bcfg, 4, seed=13)
    reqs[0].noise, reqs[0].seed = None, 41
    reqs[1].noise = None
    reqs[2].noise, reqs[2].seed = None, 43
    reqs[3].seed = 44                            # (its supplied noise wins)
    return sha(*pipe.denoise_batch(reqs, group=4))


def refine(m):
    from instructany2pix_amd.batch import refine_batch
    pipe = _start(m.pipeline(), 3)
    reqs = _refine_requests([_cond(m, 40 + i) for i in range(4)], REFINE_STRENGTHS)
    return sha(refine_batch(pipe.piperf, reqs, group=4, num_inference_steps=N_STEPS))


def inpaint(m):
    from instructany2pix_amd.batch import inpaint_batch
    pipe = _start(m.pipeline(), 4)
    reqs = _inpaint_requests([_cond(m, 60 + i, n_subjects=1) for i in range(4)], INPAINT_STRENGTHS)
    return sha(inpaint_batch(pipe.ip_adapter_xl_inpaint, reqs, group=4, num_inference_steps=N_STEPS))


def _vae_conds(m, first, n, noises):
    """two subjects per request, their masks at the tiny VAE's 64 x 64 pixels"""
    conds = {f"edit {first + i}": _cond(m, first + i, n_subjects=2) for i in range(n)}
    for c in conds.values():
        if not noises:
            for k in ("polar_noise", "refiner_noise", "subject_noise"):
                del c[k]
        c["subject_data"] = [(torch.nn.functional.interpolate(mk[None, None], size=(64, 64))[0, 0], e) for mk, e in c["subject_data"]]
    return conds


def _edit_sha(results):
    out = []
    for nr, oo, msg in results:
        out += [nr, oo, msg["latent_inv"], msg["latent_la"]]
    return sha(*out)


def edit_seeded(m):
    """image hand-off through the tiny VAE, base images as PIL: every draw id of a seeded request is exercised"""
    import PIL.Image
    conds = _vae_conds(m, 300, 3, noises=False)
    g = torch.Generator().manual_seed(9)
    for c in conds.values():
        del c["base_latents"]
        c["base_image"] = PIL.Image.fromarray(torch.randint(0, 256, (64, 64, 3), generator=g, dtype=torch.uint8).numpy())
    pipe = _start(m.pipeline(conds, vae=m.vae), 5)
    assert pipe.refiner_handoff == "image"
    return _edit_sha(pipe.edit_batch(list(conds), [[]] * 3, seeds=[5, 6, 7], output_type="pt", debug=True, group=4, **EDIT_KW))


def edit_unseeded(m):
    """every noise from the conditioner; the posterior samples of the hand-off from the global generator"""
    conds = _vae_conds(m, 320, 3, noises=True)
    pipe = _start(m.pipeline(conds, vae=m.vae), 6)
    return _edit_sha(pipe.edit_batch(list(conds), [[]] * 3, output_type="pt", debug=True, group=4, **EDIT_KW))


# ---- the serial entry points ------------------------------------------------------------------------------------------------------------------------------
def _emb(c, prefix=""):
    return {p: c[prefix + p] for p in P}


def serial_inverse(m):
    pipe, c = _start(m.pipeline(), 7), _cond(m, 500)
    return sha(pipe.pipe_inversion.inverse(num_inference_steps=5, latents=c["base_latents"], prompt_embeds=c["negative_prompt_embeds"],
                                           pooled_prompt_embeds=c["negative_pooled_prompt_embeds"]).images)


def _serial_sample(m, g):
    pipe, c = _start(m.pipeline(), 8), _cond(m, 501)
    return sha(pipe.ip_adapter_xl.generate(pil_image=None, clip_image_embeds=c["image_embeds"][0], latents=c["base_latents"], num_inference_steps=5, scale=0.7,
                                           mode="global", guidance_scale=g, output_type="latent", **_emb(c)))        # `StableDiffusionXLPipeline.__call__` as `denoise` reaches it


def serial_sample_guided(m):
    return _serial_sample(m, 5.0)


def serial_sample_unguided(m):
    return _serial_sample(m, 1.0)


def _serial_img2img(m, g):
    pipe, c = _start(m.pipeline(), 9), _cond(m, 502)
    return sha(pipe.piperf(latents=c["base_latents"], noise=c["refiner_noise"], strength=0.5, num_inference_steps=N_STEPS, guidance_scale=g,
                           output_type="latent", **_emb(c, "refiner_")).images)


def serial_img2img_guided(m):
    return _serial_img2img(m, 5.0)


def serial_img2img_unguided(m):
    return _serial_img2img(m, 1.0)


def _serial_inpaint(m, strength):
    pipe, c = _start(m.pipeline(), 10), _cond(m, 503, n_subjects=1)
    mask, emb = c["subject_data"][0]
    return sha(pipe.ip_adapter_xl_inpaint.generate(latents=c["base_latents"], mask_image=mask, pil_image=None, strength=strength, clip_image_embeds_local=emb[None],
                                                   mode="local", num_inference_steps=N_STEPS, scale=0.8, guidance_scale=7.5, noise=c["subject_noise"],
                                                   output_type="latent", **_emb(c, "subject_")))


def serial_inpaint_strength_07(m):
    return _serial_inpaint(m, 0.7)


def serial_inpaint_strength_10(m):
    return _serial_inpaint(m, 1.0)


def _serial_call(m, seed):
    conds = _vae_conds(m, 340, 1, noises=False)
    pipe = _start(m.pipeline(conds, vae=m.vae), 11)
    nr, oo, msg = pipe(list(conds)[0], [], seed=seed, output_type="pt", debug=True, **EDIT_KW)
    return sha(nr, oo, msg["latent_inv"], msg["latent_la"])


def serial_call_seeded(m):
    return _serial_call(m, 77)


def serial_call_unseeded(m):
    return _serial_call(m, None)


CASES = [denoise_group4, denoise_five_in_groups_of_two, denoise_mixed_noise_sources, refine, inpaint, edit_seeded, edit_unseeded, serial_inverse,
         serial_sample_guided, serial_sample_unguided, serial_img2img_guided, serial_img2img_unguided, serial_inpaint_strength_07, serial_inpaint_strength_10,
         serial_call_seeded, serial_call_unseeded]


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__)
def test_output_bits_are_the_parent_commits(models, case):
    got = case(models)
    print(f'    "{case.__name__}": "{got}",')
    assert got == PARENT[case.__name__]
