"""The handle lifecycle the six executors share (`_ffi.Executor`), twice in one process: build, load, run, drop the object (destroy, arena and workspace freed), then
build a second instance, load the same weights, run the same input, and require the first instance's output bytes. Covers destroy-then-create and a fresh workspace
after an earlier one was freed. Tiny configs, seeded synthetic weights; every call is a legal one."""
import gc

import pytest
import torch

from tests.test_parent_bits_gpu import rnd, sha

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _unet():
    from instructany2pix_amd.config import tiny
    from instructany2pix_amd.unet import HipUNet2DConditionModel
    from instructany2pix_amd.weights import synthetic_state_dict, unet_param_specs
    cfg = tiny()
    net = HipUNet2DConditionModel(cfg, DEV)
    net.load_state_dict(synthetic_state_dict(unet_param_specs(cfg), seed=7))
    cond = dict(text_embeds=rnd(2, cfg.pooled_dim, seed=3), time_ids=torch.tensor([[128.0, 128.0, 0, 0, 128.0, 128.0]] * 2).half())
    return net, [net(rnd(2, 4, 16, 16, seed=1), 981.0, encoder_hidden_states=rnd(2, 77, cfg.cross_attention_dim, seed=2), added_cond_kwargs=cond)[0]]


def _vae():
    from instructany2pix_amd.config import tiny_vae
    from instructany2pix_amd.vae import HipAutoencoderKL
    from instructany2pix_amd.weights import synthetic_state_dict, vae_param_specs
    cfg = tiny_vae()
    hip = HipAutoencoderKL(cfg, DEV)
    hip.load_state_dict(synthetic_state_dict(vae_param_specs(cfg), seed=7))
    return hip, [hip.decode(rnd(2, 4, 8, 8, seed=11), return_dict=False)[0], hip.encode(rnd(2, 3, 32, 32, seed=12)).latent_dist.parameters]


def _clip():
    from instructany2pix_amd.clip import HipCLIPTextModel
    from instructany2pix_amd.config import tiny_clip
    from instructany2pix_amd.weights import clip_param_specs, synthetic_state_dict
    cfg = tiny_clip(64, "gelu")
    hip = HipCLIPTextModel(cfg, DEV)
    hip.load_state_dict(synthetic_state_dict(clip_param_specs(cfg), seed=21))
    ids = torch.randint(3, cfg.vocab_size - 1, (3, 77), generator=torch.Generator().manual_seed(5))
    ids[:, 0], ids[:, 40:] = 0, cfg.vocab_size - 1
    out = hip(ids, output_hidden_states=True, want_last_hidden=True)
    return hip, [out.hidden_states[-2], out.last_hidden_state, out.text_embeds]


def _vit():
    from instructany2pix_amd.imagebind import HipImageBindModel, imagebind_param_specs, imagebind_tiny_config
    from instructany2pix_amd.weights import synthetic_state_dict
    cfg = imagebind_tiny_config()
    model = HipImageBindModel(cfg, DEV)
    model.load_state_dict(synthetic_state_dict(imagebind_param_specs(cfg), seed=51))
    outs = []
    for m, t in (("vision", cfg.vision), ("audio", cfg.audio)):
        outs += list(model.towers[m](rnd(2, t.in_channels, t.image_h, t.image_w, seed=52), return_hidden=True))
    return model, outs


def _sam():
    from instructany2pix_amd.sam import HipSamModel, sam_tiny_config
    from tests import sam_ref as R
    model = HipSamModel(sam_tiny_config(), DEV).load_state_dict(R.oracle_model().state_dict())
    emb = model.encode_image(R.pixels_of(R.sample_image()))
    return model, [emb, *model.predict_boxes(emb, R.BOXES)]


def _llm():
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
    cfg = tiny_llm()
    lm = HipInstructAny2PixLM(cfg, DEV, max_positions=16, video_token_id=cfg.vocab_size - 3)
    lm.load_state_dict(synthetic_state_dict(llm_param_specs(cfg, cfg.embed_dim, "linear"), seed=21))
    ids = torch.randint(3, cfg.vocab_size - 9, (8,), generator=torch.Generator().manual_seed(5))
    hid, logits = lm.prefill(lm.embed_tokens(ids))
    hid2, logits2 = lm.decode(int(logits.argmax()))
    return lm, [hid, logits, hid2, logits2]


@pytest.mark.parametrize("family", ["unet", "vae", "clip", "vit", "sam", "llm"])
def test_a_second_instance_after_the_first_was_dropped_gives_the_same_bytes(family):
    build = globals()["_" + family]
    digests = []
    for _ in range(2):
        model, outs = build()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(o.float()).all()) for o in outs)
        digests.append(sha(*outs))
        del model, outs           # destroy: the handle, then its arena and workspace go back to the allocator
        gc.collect()
    assert digests[0] == digests[1]
