"""Host-runtime refactors leave every executor's output bits alone: sha256 of the output bytes on seeded inputs, one digest per entry point, recorded from a run of
the parent commit's library on an MI355X (the commit that introduced pass_enter / GemmOpt / ConvOpt; the CLIP digest is older: it moved here from
test_imagebind_gpu.py unchanged). A digest that differs is a finding to explain from the code, not a number to record again.

Also here, because it compares bits before and after: a workspace that does not even cover the loss of aligning its pointer to 256 bytes is refused with
IA2P_ERR_NOMEM before anything is launched (the UNet, context-projection, VAE and CLIP entry points used to subtract unchecked and hand the allocator 2^64 bytes)."""
import ctypes as C
import hashlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

PARENT = {
    "unet_gn0": "5f5b034f68cfc3f1cf98bf8b6754b23cf5864aa8305c68a9b320f952a674e12d",
    "unet_gn12": "5f5b034f68cfc3f1cf98bf8b6754b23cf5864aa8305c68a9b320f952a674e12d",      # ia2p_set_gn_fuse(1) and its unfused twin (2): one digest
    # (the cost model gives no 3x3 site of this network a halo-staged tile, so the three modes above launch the same kernels; with tile 24 forced every eligible site fuses)
    "unet_halo_gn0": "a60ad8af8277f23c530ccc722c4748630dc7604aa793bbf0753c374b7eb9793a",
    "unet_halo_gn12": "7bee3b3a39c04856df149a559e32f656ce75fb0ebe74e6fbbf4c3f358a0010f6",
    "unet_kv": "5f5b034f68cfc3f1cf98bf8b6754b23cf5864aa8305c68a9b320f952a674e12d",
    "unet_v": "50a8c4eba196253cdd11c0fb6d925326b49b9fdee23dd0eabbfb5ea6ea39244b",
    "unet_r": "a447c40ac2e920d8fdcb15870c439bbcf5100c9301375bc17be3846ef2642dcd",
    "unet_c": "8c691c270425bf697d0e4802a7963247ca7517b13ec198cb631de7c10c4a1eef",
    "controlnet": "ec5e129c67447fa8e5b66e17c33bb4c59c8250d1587dbd2c84f51a81e40930dd",
    "vae_decode": "bd8dbd6d5816b11c407b3c74e8338e9956c56b33b2686af0163f3c2ef34263e6",
    "vae_encode": "9475492b2bd7c96785f720bce78130c91585102a21939cdd2e1aadc97568b7b4",
    "vit": "4b5e5cd8cc3a31327579324404146a8b34afc6a523e8e47895684ed845d34d6a",
    "llm_fp16": "35df8186de5d5d7314e22453d2391d067703e4c770f9edd3e3581725107033f4",
    "llm_q4": "bf7cbc1937248ccdab76c4fde4c775d3f116aafb8426c0cdc003a42ba9116585",
    "clip": "03f2a83fb3b60b0a0fc165e30c4546de8708939a0225ccbdd205ecd7ef4d472f",
}


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).half()


# ---- conditional UNet: tiny config + synthetic IP-Adapter, B = 2, 16 x 16, L = 81, t = 981, every eligible 3x3 site on its GroupNorm-fused plan --------------------
class UNetCase:
    B, h, L, t = 2, 16, 81, 981.0

    def __init__(self):
        from instructany2pix_amd import _ffi
        from instructany2pix_amd.config import tiny
        from instructany2pix_amd.unet import HipUNet2DConditionModel
        from instructany2pix_amd.weights import ip_adapter_specs, synthetic_state_dict, unet_param_specs
        self.lib = _ffi.lib()
        self.lib.ia2p_debug_set_gn_plan(1)
        cfg = tiny()
        self.net = HipUNet2DConditionModel(cfg, DEV)
        self.net.load_state_dict(synthetic_state_dict(unet_param_specs(cfg), seed=7))
        self.net.load_ip_adapter_weights(synthetic_state_dict(ip_adapter_specs(cfg, 64)["ip_adapter"], seed=7), scale=1.0, num_tokens=4)
        self.sample = rnd(self.B, 4, self.h, self.h, seed=1).to(DEV)
        self.ctx = rnd(self.B, self.L, cfg.cross_attention_dim, seed=2).to(DEV)
        self.cond = dict(text_embeds=rnd(self.B, cfg.pooled_dim, seed=3).to(DEV), time_ids=torch.tensor([[128.0, 128.0, 0, 0, 128.0, 128.0]] * self.B).half().to(DEV))

    def run(self, gn, kv=False, timestep=None, ip_scales=None, tile=-1, ctx=None, **options):
        self.net.set_gn_fuse(gn)
        self.net.cache_context_kv = kv
        self.net.invalidate_context_kv()
        self.lib.ia2p_debug_set_gemm_tile(tile)
        self.net._ws_key = None      # (the forced tile changes the K splits: the workspace is sized again)
        try:
            out = self.net(self.sample, self.t if timestep is None else timestep, encoder_hidden_states=self.ctx if ctx is None else ctx, added_cond_kwargs=self.cond,
                           ip_scales=ip_scales, **options)[0]
            torch.cuda.synchronize()
        finally:
            self.lib.ia2p_debug_set_gemm_tile(-1)
            self.net._ws_key = None
        return out


@pytest.fixture(scope="module")
def unet():
    u = UNetCase()
    yield u
    u.lib.ia2p_debug_set_gn_plan(-1)


def test_unet_forward_groupnorm_launches(unet):
    assert sha(unet.run(0)) == PARENT["unet_gn0"]


@pytest.mark.parametrize("gn", [1, 2])
def test_unet_forward_groupnorm_fused_and_its_twin(unet, gn):
    assert sha(unet.run(gn)) == PARENT["unet_gn12"]


def test_unet_forward_on_halo_staged_tiles_groupnorm_launches(unet):
    assert sha(unet.run(0, tile=24)) == PARENT["unet_halo_gn0"]


@pytest.mark.parametrize("gn", [1, 2])
def test_unet_forward_on_halo_staged_tiles_groupnorm_fused_and_its_twin(unet, gn):
    assert sha(unet.run(gn, tile=24)) == PARENT["unet_halo_gn12"]
    assert PARENT["unet_halo_gn12"] != PARENT["unet_halo_gn0"]      # (other summation order of the statistics: the fused path did run)


def test_unet_project_context_then_forward_kv(unet):
    assert sha(unet.run(1, kv=True)) == PARENT["unet_kv"]


def test_unet_forward_v_two_timesteps_two_ip_scales(unet):
    assert sha(unet.run(1, timestep=torch.tensor([981.0, 441.0]), ip_scales=torch.tensor([1.0, 0.4]))) == PARENT["unet_v"]


# ---- the option paths of the UNet callable and the ControlNet, through the public `__call__` only: recorded from the parent of the commit that made one call record
# (ia2p_unet_call) of the five argument lists. Both routes to the context K/V in one digest.
TS2 = torch.tensor([981.0, 441.0])


def test_unet_regional_image_prompts(unet):
    """ip_adapter_masks [2, 2, 16, 16]: two token groups, an 85-row context (77 text rows + 2 x 4 image tokens), per-row timesteps"""
    masks = torch.rand(2, 2, 16, 16, generator=torch.Generator().manual_seed(5)).half().to(DEV)
    ctx = rnd(unet.B, 85, unet.ctx.shape[2], seed=4).to(DEV)
    outs = [unet.run(1, kv=kv, timestep=TS2, ctx=ctx, cross_attention_kwargs={"ip_adapter_masks": masks}) for kv in (False, True)]
    assert sha(*outs) == PARENT["unet_r"]


def test_unet_controlnet_residuals(unet):
    """a residual per skip of the 16 x 16 latent and one for the mid block's output, logical NCHW"""
    shapes = unet.net.skip_shapes(unet.h, unet.h)
    res = [0.25 * rnd(unet.B, c, hh, ww, seed=40 + k).to(DEV) for k, (c, hh, ww) in enumerate(shapes + [shapes[-1]])]
    outs = [unet.run(1, kv=kv, timestep=TS2, down_block_additional_residuals=res[:-1], mid_block_additional_residual=res[-1]) for kv in (False, True)]
    assert sha(*outs) == PARENT["unet_c"]


def test_controlnet_residual_buffer(unet):
    """the tiny ControlNet on the UNet case's inputs, a seeded condition [2, 3, 128, 128], conditioning scales (0.6, 1.3): the whole residual buffer"""
    from instructany2pix_amd.config import tiny_controlnet
    from instructany2pix_amd.controlnet import HipControlNetModel
    from instructany2pix_amd.weights import controlnet_param_specs, synthetic_state_dict
    cfg = tiny_controlnet()
    cn = HipControlNetModel(cfg, DEV)
    cn.load_state_dict(synthetic_state_dict(controlnet_param_specs(cfg), seed=9))
    cn.set_gn_fuse(1)
    cond = torch.rand(unet.B, 3, 128, 128, generator=torch.Generator().manual_seed(6)).half().to(DEV)
    bufs = []
    for kv in (False, True):
        cn.cache_context_kv = kv
        cn(unet.sample, TS2, encoder_hidden_states=unet.ctx, controlnet_cond=cond, conditioning_scale=torch.tensor([0.6, 1.3]), added_cond_kwargs=unet.cond)
        torch.cuda.synchronize()
        bufs.append(cn._res.clone())
    assert sha(*bufs) == PARENT["controlnet"]


# ---- VAE, ViT towers, LLM prefill, CLIP ----------------------------------------------------------------------------------------------------------------------------
def _vae():
    from instructany2pix_amd.config import tiny_vae
    from instructany2pix_amd.vae import HipAutoencoderKL
    from instructany2pix_amd.weights import synthetic_state_dict, vae_param_specs
    cfg = tiny_vae()
    hip = HipAutoencoderKL(cfg, DEV)
    hip.load_state_dict(synthetic_state_dict(vae_param_specs(cfg), seed=7))
    return hip, 2 ** (len(cfg.block_out_channels) - 1)


@pytest.fixture(scope="module")
def vae():
    return _vae()


def test_vae_decode(vae):
    hip, _ = vae
    img = hip.decode(rnd(2, 4, 8, 8, seed=11).to(DEV), return_dict=False)[0]
    torch.cuda.synchronize()
    assert sha(img) == PARENT["vae_decode"]


def test_vae_encode(vae):
    hip, f = vae
    mom = hip.encode(rnd(2, 3, 8 * f, 8 * f, seed=12).to(DEV)).latent_dist.parameters
    torch.cuda.synchronize()
    assert sha(mom) == PARENT["vae_encode"]


def test_vit_towers():
    from instructany2pix_amd.imagebind import HipImageBindModel, imagebind_param_specs, imagebind_tiny_config
    from instructany2pix_amd.weights import synthetic_state_dict
    cfg = imagebind_tiny_config()
    outs = []
    for m, seed in (("vision", 51), ("audio", 52)):
        t = getattr(cfg, m)
        model = HipImageBindModel(cfg, DEV, modalities=(m,))
        model.load_state_dict(synthetic_state_dict(imagebind_param_specs(cfg, (m,)), seed=seed))
        outs += list(model.towers[m](rnd(2, t.in_channels, t.image_h, t.image_w, seed=seed + 1), return_hidden=True))
    torch.cuda.synchronize()
    assert sha(*outs) == PARENT["vit"]


@pytest.mark.parametrize("fmt", ["fp16", "q4"])
def test_llm_prefill_logits(fmt):
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
    cfg = tiny_llm()
    kw = dict(load_in_4bit=True, bnb_4bit_quant_type="fp4") if fmt == "q4" else {}
    lm = HipInstructAny2PixLM(cfg, DEV, max_positions=16, video_token_id=cfg.vocab_size - 3, **kw)
    lm.load_state_dict(synthetic_state_dict(llm_param_specs(cfg, cfg.embed_dim, "linear"), seed=21))
    ids = torch.randint(3, cfg.vocab_size - 9, (8,), generator=torch.Generator().manual_seed(5))
    _, logits = lm.prefill(lm.embed_tokens(ids))
    torch.cuda.synchronize()
    assert sha(logits) == PARENT["llm_" + fmt]


def _clip():
    from instructany2pix_amd.clip import HipCLIPTextModel
    from instructany2pix_amd.config import tiny_clip
    from instructany2pix_amd.weights import clip_param_specs, synthetic_state_dict
    cfg = tiny_clip(64, "gelu")
    hip = HipCLIPTextModel(cfg, DEV)
    hip.load_state_dict(synthetic_state_dict(clip_param_specs(cfg), seed=21))
    ids = torch.randint(3, cfg.vocab_size - 1, (3, 77), generator=torch.Generator().manual_seed(5))
    ids[:, 0] = 0
    ids[:, 40:] = cfg.vocab_size - 1
    return hip, ids


def _clip_sha(hip, ids):
    out = hip(ids, output_hidden_states=True, want_last_hidden=True)
    torch.cuda.synchronize()
    return sha(out.hidden_states[-2], out.last_hidden_state, out.text_embeds)


def test_clip_outputs_bit_identical_to_the_parent():
    assert _clip_sha(*_clip()) == PARENT["clip"]


# ---- the alignment refusal -----------------------------------------------------------------------------------------------------------------------------------------
NOMEM = 5


def _refused(lib, call, query_bytes, out, last_error):
    """call(ws, ws_bytes) with ws = buffer + 16 and 100 bytes: IA2P_ERR_NOMEM, `out` untouched. The buffer behind the pointer is the full workspace + 512 bytes, so a
    wrong check still writes only memory this test owns."""
    buf = torch.empty(query_bytes + 512, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    out.fill_(float("nan")) if out.is_floating_point() else out.fill_(-7)
    before = sha(out)
    torch.cuda.synchronize()
    assert call(C.c_void_p(buf.data_ptr() + 16), 100) == NOMEM
    torch.cuda.synchronize()
    assert b"workspace too small" in last_error()
    assert sha(out) == before, "something was launched"


def test_unet_workspace_below_its_alignment_loss_is_refused(unet):
    from instructany2pix_amd import _ffi
    lib, net, B, h, L = unet.lib, unet.net, unet.B, unet.h, unet.L
    first = sha(unet.run(1))
    n = lib.ia2p_workspace_bytes(net._ctx, B, h, h, L)
    out = torch.empty(B, 4, h, h, dtype=torch.half, device=DEV)
    te, tid = unet.cond["text_embeds"], unet.cond["time_ids"]
    _refused(lib, lambda ws, nb: lib.ia2p_unet_forward(net._ctx, _ffi.current_stream(), _ffi.ptr(unet.sample), unet.t, _ffi.ptr(unet.ctx), L, _ffi.ptr(te), _ffi.ptr(tid),
                                                      _ffi.ptr(out), B, h, h, ws, nb), n, out, lambda: lib.ia2p_last_error(net._ctx))
    assert sha(unet.run(1)) == first


def test_project_context_workspace_below_its_alignment_loss_is_refused(unet):
    from instructany2pix_amd import _ffi
    lib, net, B, h, L = unet.lib, unet.net, unet.B, unet.h, unet.L
    unet.run(1)      # (the IP-Adapter topology is pushed into the context by a call)
    n = lib.ia2p_workspace_bytes(net._ctx, B, h, h, L)
    nkv = lib.ia2p_context_kv_bytes(net._ctx, B, L)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    kv = torch.empty(nkv // 2, dtype=torch.half, device=DEV)
    project = lambda w, nb: lib.ia2p_project_context(net._ctx, _ffi.current_stream(), _ffi.ptr(unet.ctx), L, B, _ffi.ptr(kv), nkv, w, nb)
    assert project(_ffi.ptr(ws), n) == 0
    torch.cuda.synchronize()
    first = sha(kv)
    _refused(lib, project, n, kv, lambda: lib.ia2p_last_error(net._ctx))
    assert project(_ffi.ptr(ws), n) == 0
    torch.cuda.synchronize()
    assert sha(kv) == first


def test_vae_decode_workspace_below_its_alignment_loss_is_refused(vae):
    from instructany2pix_amd import _ffi
    hip, f = vae
    lib = hip._lib
    z = rnd(2, 4, 8, 8, seed=11).to(DEV)
    first = sha(hip.decode(z, return_dict=False)[0])
    img = torch.empty(2, 3, 8 * f, 8 * f, dtype=torch.half, device=DEV)
    _refused(lib, lambda ws, nb: lib.ia2p_vae_decode(hip._h, _ffi.current_stream(), _ffi.ptr(z), _ffi.ptr(img), 2, 8, 8, ws, nb), lib.ia2p_vae_workspace_bytes(hip._h, 2, 8, 8, 1), img,
             lambda: lib.ia2p_vae_last_error(hip._h))
    assert sha(hip.decode(z, return_dict=False)[0]) == first


def test_clip_encode_workspace_below_its_alignment_loss_is_refused():
    from instructany2pix_amd import _ffi
    hip, ids = _clip()
    lib = hip._lib
    first = _clip_sha(hip, ids)
    dids = ids.to(device=DEV, dtype=torch.int32).contiguous()
    last = torch.empty(3, 77, hip.config.hidden_size, dtype=torch.half, device=DEV)
    _refused(lib, lambda ws, nb: lib.ia2p_clip_encode(hip._h, _ffi.current_stream(), _ffi.ptr(dids), 3, 77, None, _ffi.ptr(last), None, ws, nb), lib.ia2p_clip_workspace_bytes(hip._h, 3, 77), last,
             lambda: lib.ia2p_clip_last_error(hip._h))
    assert _clip_sha(hip, ids) == first
