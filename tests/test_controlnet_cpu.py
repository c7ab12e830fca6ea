"""ControlNet, host side: the parameter inventory against the restated reference (tests/controlnet_ref.py), the reference's own invariants, the step-window rule, and
what `ia2p_controlnet_*` answers without a device (create, arena, size queries)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import controlnet_ref as CR  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import _ffi
    return _ffi.lib()


def _cfgs():
    from instructany2pix_amd.config import controlnet_sdxl, tiny_controlnet
    return controlnet_sdxl(), tiny_controlnet()


def test_param_specs_are_the_reference_keys_and_shapes():
    from instructany2pix_amd.weights import controlnet_param_specs
    for cfg in _cfgs():
        with torch.device("meta"):
            want = {k: tuple(v.shape) for k, v in CR.ControlNetRef(cfg).state_dict().items()}
        specs = controlnet_param_specs(cfg)
        got = {k: tuple(s) for k, s, _ in specs}
        assert len(got) == len(specs), "duplicate keys"
        assert got == want, (sorted(set(got) ^ set(want))[:6], [k for k in got if k in want and got[k] != want[k]][:6])
        zero = [k for k in got if k.startswith(("controlnet_down_blocks.", "controlnet_mid_block.")) and k.endswith(".weight")]
        emb = [k for k in got if k.startswith("controlnet_cond_embedding.") and k.endswith(".weight")]
        assert len(zero) == 9 + 1 and len(emb) == 8
        assert not [k for k in got if k.startswith(("up_blocks.", "conv_norm_out.", "conv_out."))]


def test_synthetic_zero_convolutions_are_not_zero():
    from instructany2pix_amd.config import tiny_controlnet
    from instructany2pix_amd.weights import controlnet_param_specs, synthetic_state_dict
    sd = synthetic_state_dict(controlnet_param_specs(tiny_controlnet()), seed=7)
    for k, v in sd.items():
        if k.startswith(("controlnet_down_blocks.", "controlnet_mid_block.")) and k.endswith(".weight"):
            assert float(v.float().abs().mean()) > 1e-2, k


def _tiny_pair(zero=False):
    from instructany2pix_amd.config import tiny, tiny_controlnet
    from instructany2pix_amd.weights import controlnet_param_specs, synthetic_state_dict, unet_param_specs
    ucfg, ccfg = tiny(), tiny_controlnet()
    usd = synthetic_state_dict(unet_param_specs(ucfg), seed=7)
    csd = synthetic_state_dict(controlnet_param_specs(ccfg), seed=9)
    if zero:
        csd = {k: (torch.zeros_like(v) if k.startswith(("controlnet_down_blocks.", "controlnet_mid_block.")) else v) for k, v in csd.items()}
    return ucfg, ccfg, CR.build_unet_with_residuals(ucfg, usd), CR.build_controlnet(ccfg, csd), usd


def _inputs(cfg, B=1, h=8, w=8, L=9, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, h, w, generator=g)
    ctx = torch.randn(B, L, cfg.cross_attention_dim, generator=g)
    added = dict(text_embeds=torch.randn(B, cfg.pooled_dim, generator=g), time_ids=torch.tensor([[h * 8.0, w * 8.0, 0, 0, h * 8.0, w * 8.0]] * B))
    cond = torch.rand(B, 3, 8 * h, 8 * w, generator=g)
    return x, ctx, added, cond


def test_zero_valued_zero_convolutions_leave_the_reference_unet_alone():
    import oracle
    ucfg, ccfg, unet, cn, usd = _tiny_pair(zero=True)
    x, ctx, added, cond = _inputs(ucfg)
    with torch.no_grad():
        down, mid = cn(x, 500, ctx, cond, 1.3, added_cond_kwargs=added)
        assert all(float(d.abs().max()) == 0.0 for d in down) and float(mid.abs().max()) == 0.0
        plain = oracle.build_unet(ucfg, usd)(x, 500, ctx, added_cond_kwargs=added)[0]
        assert torch.equal(unet(x, 500, ctx, added_cond_kwargs=added)[0], plain)                                  # the restated forward IS the oracle's
        assert torch.equal(unet(x, 500, ctx, added_cond_kwargs=added, down_block_additional_residuals=down, mid_block_additional_residual=mid)[0], plain)


def test_reference_residuals_act_and_scale_linearly():
    ucfg, ccfg, unet, cn, _ = _tiny_pair()
    x, ctx, added, cond = _inputs(ucfg, B=2)
    with torch.no_grad():
        d1, m1 = cn(x, 500, ctx, cond, 1.0, added_cond_kwargs=added)
        d2, m2 = cn(x, 500, ctx, cond, torch.tensor([0.5, 2.0]), added_cond_kwargs=added)
        assert len(d1) == 9 and [tuple(d.shape[1:]) for d in d1] == [(64, 8, 8)] * 3 + [(64, 4, 4), (128, 4, 4), (128, 4, 4), (128, 2, 2), (256, 2, 2), (256, 2, 2)]
        assert tuple(m1.shape[1:]) == (256, 2, 2)
        for a, b in zip(d1 + [m1], d2 + [m2]):
            assert torch.allclose(b[0], 0.5 * a[0]) and torch.allclose(b[1], 2.0 * a[1])
        plain = unet(x, 500, ctx, added_cond_kwargs=added)[0]
        ctl = unet(x, 500, ctx, added_cond_kwargs=added, down_block_additional_residuals=d1, mid_block_additional_residual=m1)[0]
        assert not torch.allclose(plain, ctl, atol=1e-3)
        cn.num_tokens = 4                                                                                       # the last four context rows are not seen
        d3, _ = cn(x, 500, ctx, cond, 1.0, added_cond_kwargs=added)
        d4, _ = cn(x, 500, torch.cat([ctx[:, :5], torch.zeros(2, 4, ctx.shape[2])], 1), cond, 1.0, added_cond_kwargs=added)
        assert all(torch.equal(a, b) for a, b in zip(d3, d4)) and not torch.allclose(d3[-1], d1[-1], atol=1e-4)


@pytest.mark.parametrize("n", [4, 10, 25])
def test_step_window_rule(n):
    from instructany2pix_amd.ddim import control_active
    for start, end in ((0.0, 1.0), (0.2, 0.8), (0.5, 0.5), (0.0, 0.5), (0.3, 1.0), (1.0, 1.0), (0.0, 0.0)):
        want = [not (i / n < start or (i + 1) / n > end) for i in range(n)]
        assert [control_active(i, n, start, end) for i in range(n)] == want == [CR.control_active(i, n, start, end) for i in range(n)]
        if (start, end) == (0.0, 1.0):
            assert all(want)
        if (start, end) == (0.5, 0.5):
            assert not any(want)                                                                                # a window that holds no step
        if (start, end) == (0.2, 0.8) and n == 10:
            assert [i for i, a in enumerate(want) if a] == [2, 3, 4, 5, 6, 7]
        on = [i for i, a in enumerate(want) if a]
        assert on == list(range(on[0], on[-1] + 1)) if on else True                                             # one run of steps


def _create(lib, cfg):
    from instructany2pix_amd import _ffi
    h = C.c_void_p()
    st = lib.ia2p_controlnet_create(C.byref(_ffi.make_controlnet_config(cfg)), C.byref(h))
    return st, h


def test_create_arena_and_queries(lib):
    from instructany2pix_amd import _ffi
    from instructany2pix_amd.config import tiny
    from instructany2pix_amd.weights import controlnet_param_specs, param_count
    for cfg in _cfgs():
        st, h = _create(lib, cfg)
        _ffi.check(st, None, "controlnet")
        n = param_count(controlnet_param_specs(cfg))
        arena = lib.ia2p_controlnet_arena_bytes(h)
        # the specs, + the LayerNorm-folded copies (12 C^2 per transformer block against the >= 20 C^2 it loads: below 0.6 of the whole) and the 128-element padding
        assert n * 2 <= arena < n * 2 * 1.6 + (1 << 20), (n * 2, arena)
        assert lib.ia2p_controlnet_num_residuals(h) == 10
        B, hh, ww = 2, 16, 24
        offs, ch, hs, ws = (C.c_int64 * 10)(), (C.c_int * 10)(), (C.c_int * 10)(), (C.c_int * 10)()
        total = lib.ia2p_controlnet_residual_layout(h, B, hh, ww, offs, ch, hs, ws)
        c = list(cfg.block_out_channels)
        want = [(c[0], 16, 24)] * 3 + [(c[0], 8, 12), (c[1], 8, 12), (c[1], 8, 12), (c[1], 4, 6), (c[2], 4, 6), (c[2], 4, 6), (c[2], 4, 6)]
        assert [(ch[k], hs[k], ws[k]) for k in range(10)] == want
        assert offs[0] == 0 and all(offs[k + 1] - offs[k] == B * want[k][0] * want[k][1] * want[k][2] for k in range(9))
        assert total == 2 * (offs[9] + B * want[9][0] * want[9][1] * want[9][2])
        assert lib.ia2p_controlnet_embed_bytes(h, B, hh, ww) == B * hh * ww * c[0] * 2
        assert lib.ia2p_controlnet_embed_workspace_bytes(h, B, hh, ww) >= 2 * B * 64 * hh * ww * 16 * 2      # two full-resolution 16-channel maps are live at once
        assert lib.ia2p_controlnet_workspace_bytes(h, B, hh, ww, 77) > 0
        assert lib.ia2p_controlnet_context_kv_bytes(h, B, 77) > 0
        # bad shapes: 0
        assert lib.ia2p_controlnet_workspace_bytes(h, B, 15, 24, 77) == 0 and b"divisible" in lib.ia2p_controlnet_last_error(h)
        assert lib.ia2p_controlnet_residual_layout(h, B, 15, 24, None, None, None, None) == 0
        assert lib.ia2p_controlnet_embed_bytes(h, 0, hh, ww) == 0 and lib.ia2p_controlnet_embed_workspace_bytes(h, B, 0, ww) == 0
        _ffi.check(lib.ia2p_controlnet_set_image_tokens(h, 4), h, "controlnet")
        assert lib.ia2p_controlnet_workspace_bytes(h, B, hh, ww, 4) == 0 and lib.ia2p_controlnet_context_kv_bytes(h, B, 4) == 0      # no text row left
        assert lib.ia2p_controlnet_workspace_bytes(h, B, hh, ww, 81) > 0
        # the UNet's entry points refuse the handle, before anything else
        assert lib.ia2p_workspace_bytes(h, 1, 16, 16, 77) == 0
        with pytest.raises(_ffi.IA2PError):
            _ffi.check(lib.ia2p_controlnet_finalize_weights(h), h, "controlnet")                                   # no arena bound
        # attaching: the UNet of the same widths fits, another does not
        u = C.c_void_p()
        ucfg = tiny() if c[0] == 64 else None
        if ucfg is not None:
            _ffi.check(lib.ia2p_create(C.byref(_ffi.make_config(ucfg)), C.byref(u)))
            assert lib.ia2p_controlnet_check_unet(h, u) == 0
            assert lib.ia2p_unet_num_skips(u) == 9
            lib.ia2p_destroy(u)
            ucfg.block_out_channels = (64, 128, 320)
            ucfg.attention_head_dim = (1, 2, 5)
            _ffi.check(lib.ia2p_create(C.byref(_ffi.make_config(ucfg)), C.byref(u)))
            with pytest.raises(ValueError, match="must match the UNet"):
                _ffi.check(lib.ia2p_controlnet_check_unet(h, u), h, "controlnet")
            lib.ia2p_destroy(u)
        lib.ia2p_controlnet_destroy(h)


def test_create_refuses_a_bad_config_with_the_family_message(lib):
    from instructany2pix_amd import _ffi
    from instructany2pix_amd.config import tiny_controlnet
    for field, bad, words in (("conditioning_embedding_out_channels", (16, 32, 100, 256), "conditioning_embedding_out_channels[2]=100"),
                              ("conditioning_channels", 9, "conditioning_channels 9"), ("cross_attention_dim", 100, "divisibility")):
        cfg = tiny_controlnet()
        setattr(cfg, field, bad)
        cc = _ffi.make_controlnet_config(cfg)
        h = C.c_void_p()
        st = lib.ia2p_controlnet_create(C.byref(cc), C.byref(h))
        assert st == 2 and not h.value
        with pytest.raises(ValueError) as e:
            _ffi.check(st, None, "controlnet")
        assert words in str(e.value) and str(e.value) == f"ia2p SHAPE: {lib.ia2p_controlnet_last_error(None).decode()}"
    assert lib.ia2p_controlnet_create(None, None) == 1


def test_finalize_checks_exactly_the_key_set(lib):
    """every key of the specs is known to the handle with the specs' element count, an up-path key is not (load_tensor refuses before it touches a pointer's data)"""
    from instructany2pix_amd import _ffi
    from instructany2pix_amd.config import tiny_controlnet
    from instructany2pix_amd.weights import controlnet_param_specs
    cfg = tiny_controlnet()
    st, h = _create(lib, cfg)
    _ffi.check(st, None, "controlnet")
    one = (C.c_int64 * 1)(1)
    for k in ("up_blocks.0.resnets.0.conv1.weight", "conv_out.weight", "conv_norm_out.weight", "controlnet_down_blocks.9.weight", "ip_adapter.1.to_k_ip.weight"):
        assert lib.ia2p_controlnet_load_tensor(h, k.encode(), C.c_void_p(16), one, 1, None) == 4                   # (STATE: no arena yet -- the order of the checks)
    arena = (C.c_char * 256)()
    assert lib.ia2p_controlnet_bind_arena(h, C.cast(arena, C.c_void_p), 256) == 5                                # too small: NOMEM, nothing bound
    lib.ia2p_controlnet_destroy(h)
    keys = [k for k, _, _ in controlnet_param_specs(cfg)]
    assert len(keys) == len(set(keys))
