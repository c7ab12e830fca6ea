"""ImageBind's vision and audio towers on the MI355X (csrc/vit.hip, csrc/vit_engine.hip, instructany2pix_amd/imagebind.py) against the torch restatement in
tests/imagebind_ref.py, fp32 on the CPU with the same fp16-rounded weights and inputs.

Tolerances: the attention launch alone rel-L2 < 2e-3 (what test_ops_gpu.py::test_self_attention holds `ia2p_attention` to), a dominant late key max abs < 6e-3
(test_self_attention_online_softmax_rescale); tower outputs rel-L2 <= 5e-3 (tests/test_clip_gpu.py: the same GEMMs, fp16 activations vs an fp32 oracle);
end to end after L2 normalisation <= 1e-2 (normalising a vector at most doubles a relative error of 5e-3).
The per-launch fp64 bound of `ia2p_attention_full`, at every sub-tile edge up to its 272 keys, lives in tests/attn_ops_ref.py / tests/test_attn_ops_gpu.py."""
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

from tests.imagebind_ref import RefTower, postprocess, rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    from instructany2pix_amd import _ffi
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib = _ffi.lib()
    assert lib.ia2p_device_is_gfx950() == 1
    return lib


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


# ---- the attention launch alone --------------------------------------------------------------------------------------------------------------------------
def _attention(L, qkv, B, T, heads, D, bk=None, bv=None):
    from instructany2pix_amd import _ffi
    dq = qkv.to(DEV)
    dk, dv = (bk.to(DEV), bv.to(DEV)) if bk is not None else (None, None)
    out = torch.empty(B * T, heads * D, dtype=torch.half, device=DEV)
    _ffi.check(L.ia2p_attention_full(_ffi.current_stream(), _ffi.ptr(dq), _ffi.ptr(out), _ffi.ptr(dk), _ffi.ptr(dv), B, T, heads, D))
    torch.cuda.synchronize()
    return out.cpu()


def _attention_ref(qkv, B, T, heads, D, bk=None, bv=None):
    q, k, v = [t.float().reshape(B, T, heads, D).transpose(1, 2) for t in qkv.chunk(3, dim=-1)]
    if bk is not None:      # add_bias_kv: one more key / value row after the T token rows
        k = torch.cat([k, bk.float().reshape(1, heads, 1, D).expand(B, -1, -1, -1)], dim=2)
        v = torch.cat([v, bv.float().reshape(1, heads, 1, D).expand(B, -1, -1, -1)], dim=2)
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v)
    return o.transpose(1, 2).reshape(B * T, heads * D)


@pytest.mark.parametrize("T,D,bias", [(17, 80, False), (64, 80, False), (65, 80, False), (257, 80, False), (230, 64, True), (33, 64, True)])
def test_attention_full(L, T, D, bias):
    """one partial query tile, an exact tile, one row over, the vision tower's ragged length; with a bias row: T token rows + bias_k / bias_v read as key T
    by the launch itself, the route the audio tower takes (229 tokens + 1)"""
    B, heads = 2, 3
    qkv = rnd(B * T, 3 * heads * D, seed=T + D)
    bk, bv = (rnd(heads * D, seed=1), rnd(heads * D, seed=2)) if bias else (None, None)
    out = _attention(L, qkv, B, T, heads, D, bk, bv)
    err = rel_l2(out, _attention_ref(qkv, B, T, heads, D, bk, bv))
    print(f"attention_full T={T} D={D} bias={bias}: rel_l2 {err:.2e}")
    assert err < 2e-3
    assert torch.equal(out, _attention(L, qkv, B, T, heads, D, bk, bv))          # fixed reduction order: the same bits again


def test_attention_full_dominant_late_key(L):
    """one late key dominates one query: the row maximum comes from the 13th key tile"""
    T, D = 257, 80
    qkv = rnd(T, 3 * D, seed=17)
    qkv[5, 0:D] = 3.0
    qkv[200, D:2 * D] = 3.0
    out = _attention(L, qkv, 1, T, 1, D)
    ref = _attention_ref(qkv, 1, T, 1, D)
    err = float((out.float() - ref).abs().max())
    print(f"dominant late key: max abs error {err:.2e}")
    assert err < 6e-3
    assert float((out[5].float() - qkv[200, 2 * D:].float()).abs().max()) < 6e-3      # query 5 returns value row 200


def test_attention_full_refuses_what_it_cannot_hold(L):
    q = torch.zeros(273 * 192, dtype=torch.half, device=DEV)
    o = torch.zeros(273 * 64, dtype=torch.half, device=DEV)
    b = torch.zeros(64, dtype=torch.half, device=DEV)
    from instructany2pix_amd import _ffi
    assert L.ia2p_attention_full(None, _ffi.ptr(q), _ffi.ptr(o), None, None, 1, 273, 1, 64) == 2          # more than 272 keys
    assert L.ia2p_attention_full(None, _ffi.ptr(q), _ffi.ptr(o), _ffi.ptr(b), _ffi.ptr(b), 1, 272, 1, 64) == 2
    assert L.ia2p_attention_full(None, _ffi.ptr(q), _ffi.ptr(o), None, None, 1, 64, 1, 96) == 2           # head dim
    assert L.ia2p_attention_full(None, _ffi.ptr(q), _ffi.ptr(o), _ffi.ptr(b), None, 1, 64, 1, 64) == 1    # bias_k without bias_v


# ---- towers ------------------------------------------------------------------------------------------------------------------------------------------
def _build(cfg, m, seed):
    from instructany2pix_amd.imagebind import HipImageBindModel, imagebind_param_specs
    from instructany2pix_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(imagebind_param_specs(cfg, (m,)), seed=seed)
    model = HipImageBindModel(cfg, DEV, modalities=(m,))
    model.load_state_dict(sd)
    return model, RefTower(getattr(cfg, m), m, sd)


def _check_tower(cfg, m, B, seed, sub=(None,)):
    """head output and last hidden state against the oracle, at B and at every leading sub-batch in `sub` (the oracle is computed once)"""
    t = getattr(cfg, m)
    model, ref = _build(cfg, m, seed)
    x = rnd(B, t.in_channels, t.image_h, t.image_w, seed=seed + 1)
    want_head, want_hid = ref(x)
    for n in sub:
        n = n or B
        head, hid = model.towers[m](x[:n], return_hidden=True)
        torch.cuda.synchronize()
        assert head.dtype == torch.float32 and head.shape == (n, t.out_dim) and hid.shape == (n, t.tokens, t.hidden_size)
        e1, e2 = rel_l2(head, want_head[:n]), rel_l2(hid, want_hid[:n])
        print(f"{m} tower hidden {t.hidden_size} x {t.num_layers} layers, B={n}: head rel_l2 {e1:.2e}, last hidden rel_l2 {e2:.2e}")
        assert e1 <= 5e-3 and e2 <= 5e-3


def test_small_vision_tower():
    from instructany2pix_amd.imagebind import imagebind_tiny_config
    _check_tower(imagebind_tiny_config(), "vision", 2, seed=51)            # hidden 320 = 4 x 80, 257 tokens


def test_small_audio_tower():
    from instructany2pix_amd.imagebind import imagebind_tiny_config
    _check_tower(imagebind_tiny_config(), "audio", 2, seed=52)             # hidden 128 = 2 x 64, 229 tokens + bias row, stem LayerNorm


def test_small_vision_tower_17_tokens():
    from instructany2pix_amd.imagebind import imagebind_tiny_config
    cfg = imagebind_tiny_config()
    cfg.vision = replace(cfg.vision, image_h=56, image_w=56)
    assert cfg.vision.tokens == 17
    _check_tower(cfg, "vision", 3, seed=53)


def test_full_width_vision_tower():
    from instructany2pix_amd.imagebind import imagebind_huge_config
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    cfg = imagebind_huge_config()
    cfg.vision = replace(cfg.vision, num_layers=4)
    _check_tower(cfg, "vision", 3, seed=54, sub=(1, 3))


def test_full_width_audio_tower():
    from instructany2pix_amd.imagebind import imagebind_huge_config
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    cfg = imagebind_huge_config()
    cfg.audio = replace(cfg.audio, num_layers=2)
    _check_tower(cfg, "audio", 3, seed=55, sub=(1, 3))


# ---- files -> embeddings ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_model():
    from instructany2pix_amd.imagebind import HipImageBindModel, imagebind_param_specs, imagebind_tiny_config
    from instructany2pix_amd.weights import synthetic_state_dict
    cfg = imagebind_tiny_config()
    sd = synthetic_state_dict(imagebind_param_specs(cfg), seed=61)
    sd["modality_postprocessors.audio.1.log_logit_scale"] = torch.tensor(2.9957)        # in the checkpoint, not read
    sd["modality_trunks.text.blocks.0.attn.in_proj_weight"] = torch.zeros(3, 1)         # another modality: skipped
    model = HipImageBindModel(cfg, DEV).eval()
    model.load_state_dict(sd, strict=True)
    return model, {m: RefTower(getattr(cfg, m), m, sd) for m in ("vision", "audio")}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image
    from scipy.io import wavfile
    d = tmp_path_factory.mktemp("mm")
    g = np.random.default_rng(7)
    yy, xx = np.mgrid[0:240, 0:320]
    for i, name in enumerate(("a.png", "b.png")):
        img = np.stack([127 + 100 * np.sin(xx / (9.0 + i) + c) * np.cos(yy / (13.0 - i)) for c in range(3)], axis=-1) + g.normal(0, 12, (240, 320, 3))
        Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(d / name)
    t = np.arange(5 * 16000) / 16000.0
    wav = 0.3 * np.sin(2 * np.pi * (300 + 200 * t) * t) + 0.05 * g.standard_normal(t.size)
    wavfile.write(d / "c.wav", 16000, wav.astype(np.float32))
    return str(d / "a.png"), str(d / "b.png"), str(d / "c.wav")


def test_model_end_to_end(tiny_model, files):
    from instructany2pix_amd import imagebind as ib
    model, refs = tiny_model
    a, b, c = files
    px = ib.load_and_transform_vision_data([a, b], DEV)
    two = model({ib.ModalityType.VISION: px})[ib.ModalityType.VISION]
    assert two.shape == (2, 1024) and two.dtype == torch.float32
    want = postprocess("vision", refs["vision"](px.cpu())[0])
    e = rel_l2(two, want)
    print(f"vision end to end: rel_l2 {e:.2e}")
    assert e <= 1e-2 and torch.allclose(two.norm(dim=-1).cpu(), torch.ones(2), atol=1e-4)
    for i in range(2):      # a batch of two equals the two single calls (tile plans depend on M: not bit for bit)
        one = model({"vision": px[i:i + 1]})["vision"]
        assert rel_l2(two[i:i + 1], one) <= 1e-2 and rel_l2(one, want[i:i + 1]) <= 1e-2
    au = ib.load_and_transform_audio_data([c], DEV)
    assert au.shape == (1, 3, 1, 128, 204)
    emb = model({"audio": au})["audio"]
    assert emb.shape == (1, 1024) and emb.dtype == torch.float32
    want = postprocess("audio", refs["audio"](au[0].cpu())[0], clips=3)
    e = rel_l2(emb, want)
    print(f"audio end to end: rel_l2 {e:.2e}")
    assert e <= 1e-2
    clips = torch.cat([model({"audio": au[:, i:i + 1]})["audio"] for i in range(3)])      # each clip alone: norm 20; the file is their mean
    assert torch.allclose(clips.norm(dim=-1).cpu(), torch.full((3,), 20.0), atol=1e-3)
    assert rel_l2(emb, clips.mean(dim=0, keepdim=True)) <= 1e-2
    with pytest.raises(ValueError):
        model({"depth": px})


def test_pipeline_modality_embeds(tiny_model, files):
    from instructany2pix_amd import imagebind as ib
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    model, _ = tiny_model
    a, _, c = files
    pipe = InstructAny2PixPipeline(unet=object(), imagebind=model)
    assert pipe.model_imb is model
    out = pipe._modality_embeds([{"type": "image", "fname": a}, {"type": "audio", "fname": c}])
    assert out.shape == (2, 1024) and out.dtype == torch.float32 and out.device.type == "cpu"
    assert torch.allclose(out.norm(dim=-1), torch.full((2,), 20.0), atol=1e-3)
    own = torch.cat([model({"vision": ib.load_and_transform_vision_data([a], DEV)})["vision"], model({"audio": ib.load_and_transform_audio_data([c], DEV)})["audio"]]).cpu()
    own = own / own.norm(dim=-1, keepdim=True) * 20
    assert torch.allclose(out, own, atol=1e-5)
