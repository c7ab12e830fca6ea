"""LoRA adapters, the part that needs no GPU: the adapter-file reader (`instructany2pix_amd/lora.py::parse_lora_state_dict`: every accepted spelling, the SGM name
rule against pairs written out by hand, every refusal), the fp64 reference of the merge (tests/lora_ref.py: lattice exactness, mutants of a numpy model of the kernel),
and the two new symbols of the C ABI."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lora_ref as R  # noqa: E402
from instructany2pix_amd import lora as L  # noqa: E402
from instructany2pix_amd.config import sdxl_base, sdxl_refiner, tiny, tiny_refiner  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = tiny()
MODS = L.unet_lora_modules(CFG)
ATTN = "down_blocks.1.attentions.0.transformer_blocks.0.attn1"
PICK = [f"{ATTN}.to_q", f"{ATTN}.to_out.0", "mid_block.attentions.0.transformer_blocks.1.attn2.to_k", "up_blocks.0.attentions.2.transformer_blocks.0.ff.net.0.proj",
        "down_blocks.1.resnets.0.conv1", "down_blocks.1.resnets.0.conv_shortcut", "up_blocks.2.resnets.1.time_emb_proj", "down_blocks.0.downsamplers.0.conv",
        "up_blocks.0.upsamplers.0.conv", "conv_in", "conv_out", "time_embedding.linear_2", "add_embedding.linear_1", "mid_block.attentions.0.proj_in"]


def factors(module, r, seed=0, conv4d=True, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed + len(module))
    shape = MODS[module]
    down = torch.randn((r,) + tuple(shape[1:]), generator=g) * 0.1
    up = torch.randn((shape[0], r) + ((1, 1) if len(shape) == 4 else ()), generator=g) * 0.1
    if not conv4d:
        down, up = down.reshape(r, -1), up.reshape(shape[0], r)
    return down.to(dtype), up.to(dtype)


def adapter(spelling, modules=PICK, r=4, alpha=2.0, names=None, **kw):
    """the same adapter in one of the accepted spellings"""
    sd = {}
    sgm = {v: k for k, v in L.sgm_module_names(CFG).items()}
    for m in modules:
        down, up = factors(m, r, **kw)
        if spelling == "peft":
            sd[f"unet.{m}.lora_A.weight"], sd[f"unet.{m}.lora_B.weight"] = down, up
        elif spelling == "peft_named":
            sd[f"{m}.lora_A.default_0.weight"], sd[f"{m}.lora_B.default_0.weight"] = down, up
        elif spelling == "lora_dot":
            sd[f"unet.{m}.lora.down.weight"], sd[f"unet.{m}.lora.up.weight"] = down, up
        elif spelling == "lora_underscore":
            sd[f"{m}.lora_down.weight"], sd[f"{m}.lora_up.weight"] = down, up
        elif spelling in ("kohya_diffusers", "kohya_sgm"):
            flat = "lora_unet_" + (m if spelling == "kohya_diffusers" else sgm[m]).replace(".", "_")
            sd[flat + ".lora_down.weight"], sd[flat + ".lora_up.weight"] = down, up
            if alpha is not None:
                sd[flat + ".alpha"] = torch.tensor(alpha)
            continue
        else:
            raise AssertionError(spelling)
        if alpha is not None:
            sd[("unet." if spelling in ("peft", "lora_dot") else "") + m + ".alpha"] = torch.tensor(alpha)
    return sd


def same(a, b):
    assert list(a) == list(b)
    for m in a:
        assert torch.equal(a[m][0], b[m][0]) and torch.equal(a[m][1], b[m][1]) and a[m][2] == b[m][2], m


# ---- the reader: what it accepts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spelling", ["peft_named", "lora_dot", "lora_underscore", "kohya_diffusers", "kohya_sgm"])
def test_every_spelling_parses_to_the_same_adapter(spelling):
    want = L.parse_lora_state_dict(adapter("peft"), CFG)
    assert list(want) == [m for m in MODS if m in PICK] and len(want) == len(PICK)      # the UNet's registration order
    for m, (down, up, alpha) in want.items():
        shape = MODS[m]
        assert down.dtype == up.dtype == torch.float16 and alpha == 2.0
        assert tuple(down.shape) == (4, int(np.prod(shape[1:]))) and tuple(up.shape) == (shape[0], 4), m      # convolutions flattened
    same(L.parse_lora_state_dict(adapter(spelling), CFG), want)


def test_old_attention_processor_spelling():
    want = L.parse_lora_state_dict(adapter("peft", [f"{ATTN}.to_q", f"{ATTN}.to_k", f"{ATTN}.to_v", f"{ATTN}.to_out.0"], alpha=None), CFG)
    sd = {}
    for short, m in (("to_q", "to_q"), ("to_k", "to_k"), ("to_v", "to_v"), ("to_out", "to_out.0")):
        down, up = factors(f"{ATTN}.{m}", 4)
        sd[f"unet.{ATTN}.processor.{short}_lora.down.weight"], sd[f"unet.{ATTN}.processor.{short}_lora.up.weight"] = down, up
    same(L.parse_lora_state_dict(sd, CFG), want)
    assert all(v[2] == 4.0 for v in want.values())                       # no alpha key: alpha = rank


def test_linear_factors_of_a_convolution_and_other_dtypes():
    m = ["down_blocks.1.resnets.0.conv_shortcut", f"{ATTN}.to_q"]
    want = L.parse_lora_state_dict(adapter("peft", m), CFG)
    same(L.parse_lora_state_dict(adapter("peft", m, conv4d=False), CFG), want)                     # a 1 x 1 convolution's factors given as matrices
    for dt in (torch.float32, torch.bfloat16):
        got = L.parse_lora_state_dict(adapter("peft", m, dtype=dt), CFG)
        for k in m:
            down, up = factors(k, 4, dtype=dt)
            assert got[k][0].dtype == torch.float16 and torch.equal(got[k][0], down.reshape(4, -1).to(torch.float16))      # one rounding to nearest, at load
            assert torch.equal(got[k][1], up.reshape(up.shape[0], 4).to(torch.float16))


def test_safetensors_round_trip(tmp_path):
    from safetensors.torch import save_file
    sd = adapter("kohya_sgm")
    p = str(tmp_path / "adapter.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, p)
    same(L.parse_lora_state_dict(p, CFG), L.parse_lora_state_dict(sd, CFG))
    with pytest.raises(ValueError, match="safetensors"):
        L.parse_lora_state_dict(str(tmp_path / "adapter.bin"), CFG)


# SGM <-> diffusers for SDXL-base, written out by hand (not produced by the rule under test)
SGM_PAIRS = (
    ("input_blocks_0_0", "conv_in"),
    ("input_blocks_1_0_in_layers_2", "down_blocks.0.resnets.0.conv1"),
    ("input_blocks_2_0_emb_layers_1", "down_blocks.0.resnets.1.time_emb_proj"),
    ("input_blocks_3_0_op", "down_blocks.0.downsamplers.0.conv"),
    ("input_blocks_4_0_skip_connection", "down_blocks.1.resnets.0.conv_shortcut"),
    ("input_blocks_4_1_transformer_blocks_0_attn1_to_q", "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q"),
    ("input_blocks_5_1_transformer_blocks_1_attn2_to_out_0", "down_blocks.1.attentions.1.transformer_blocks.1.attn2.to_out.0"),
    ("input_blocks_6_0_op", "down_blocks.1.downsamplers.0.conv"),
    ("input_blocks_7_1_proj_in", "down_blocks.2.attentions.0.proj_in"),
    ("input_blocks_8_1_transformer_blocks_9_ff_net_0_proj", "down_blocks.2.attentions.1.transformer_blocks.9.ff.net.0.proj"),
    ("input_blocks_8_0_out_layers_3", "down_blocks.2.resnets.1.conv2"),
    ("middle_block_0_in_layers_2", "mid_block.resnets.0.conv1"),
    ("middle_block_1_transformer_blocks_3_attn2_to_k", "mid_block.attentions.0.transformer_blocks.3.attn2.to_k"),
    ("middle_block_2_out_layers_3", "mid_block.resnets.1.conv2"),
    ("output_blocks_0_1_transformer_blocks_0_attn1_to_v", "up_blocks.0.attentions.0.transformer_blocks.0.attn1.to_v"),
    ("output_blocks_2_2_conv", "up_blocks.0.upsamplers.0.conv"),
    ("output_blocks_3_1_proj_out", "up_blocks.1.attentions.0.proj_out"),
    ("output_blocks_5_2_conv", "up_blocks.1.upsamplers.0.conv"),
    ("output_blocks_5_0_skip_connection", "up_blocks.1.resnets.2.conv_shortcut"),
    ("output_blocks_6_0_in_layers_2", "up_blocks.2.resnets.0.conv1"),
    ("output_blocks_6_0_skip_connection", "up_blocks.2.resnets.0.conv_shortcut"),
    ("output_blocks_8_0_emb_layers_1", "up_blocks.2.resnets.2.time_emb_proj"),
    ("time_embed_0", "time_embedding.linear_1"), ("time_embed_2", "time_embedding.linear_2"),
    ("label_emb_0_0", "add_embedding.linear_1"), ("label_emb_0_2", "add_embedding.linear_2"),
    ("out_2", "conv_out"),
)


def test_sgm_names_of_sdxl_base_against_pairs_written_by_hand():
    table = L.kohya_names(sdxl_base())
    for flat, module in SGM_PAIRS:
        assert table["lora_unet_" + flat] == module, flat
    assert "lora_unet_output_blocks_8_1_proj_in" not in table            # the last level of SDXL-base carries no transformer
    assert "lora_unet_input_blocks_9_0_op" not in table                  # ... and nothing follows the last level's resnets


@pytest.mark.parametrize("cfg", [sdxl_base(), sdxl_refiner(), tiny(), tiny_refiner()], ids=["base", "refiner", "tiny", "tiny_refiner"])
def test_both_name_trees_cover_every_module_once(cfg):
    mods, sgm = L.unet_lora_modules(cfg), L.sgm_module_names(cfg)
    assert sorted(sgm.values()) == sorted(mods) and len(sgm) == len(mods)
    assert len(L.kohya_names(cfg)) == 2 * len(mods)                      # no flattened name of one tree collides with one of the other
    if cfg.transformer_layers_per_block[-1] == 0 and len(cfg.block_out_channels) == 4:      # the refiner: a plain first up level, its upsampler at position 1
        assert sgm["output_blocks.2.1.conv"] == "up_blocks.0.upsamplers.0.conv" and sgm["output_blocks.5.2.conv"] == "up_blocks.1.upsamplers.0.conv"


# ---- the reader: what it refuses ------------------------------------------------------------------------------------------------------------------------------
def _refused(sd, key_part, cfg=CFG, **kw):
    with pytest.raises(ValueError) as e:
        L.parse_lora_state_dict(sd, cfg, **kw)
    assert key_part in str(e.value), str(e.value)


def test_refusals_name_the_key():
    q = f"{ATTN}.to_q"
    down, up = factors(q, 4)
    ok = {f"unet.{q}.lora_A.weight": down, f"unet.{q}.lora_B.weight": up}
    L.parse_lora_state_dict(ok, CFG)
    _refused({"unet.down_blocks.9.attn.to_q.lora_A.weight": down, "unet.down_blocks.9.attn.to_q.lora_B.weight": up}, "down_blocks.9.attn.to_q")      # no such module
    _refused({"lora_unet_input_blocks_99_1_proj_in.lora_down.weight": down, "lora_unet_input_blocks_99_1_proj_in.lora_up.weight": up}, "input_blocks_99_1_proj_in")
    _refused({f"unet.{q}.norm1.lora_A.weight": down, f"unet.{q}.norm1.lora_B.weight": up}, "norm1")
    _refused({f"unet.{q}.lora_A.weight": down[:, :-1], f"unet.{q}.lora_B.weight": up}, f"{q}.lora_A.weight")                  # K does not fit
    _refused({f"unet.{q}.lora_A.weight": down, f"unet.{q}.lora_B.weight": up[:-1]}, f"{q}.lora_B.weight")                     # N does not fit
    _refused({f"unet.{q}.lora_A.weight": down, f"unet.{q}.lora_B.weight": torch.cat([up, up], 1)}, f"{q}.lora_B.weight")      # the two ranks differ
    big = torch.zeros(257, down.shape[1], dtype=torch.float16)
    _refused({f"unet.{q}.lora_A.weight": big, f"unet.{q}.lora_B.weight": torch.zeros(up.shape[0], 257, dtype=torch.float16)}, f"{q}.lora_A.weight")      # rank 257
    L.parse_lora_state_dict({f"unet.{q}.lora_A.weight": big[:256], f"unet.{q}.lora_B.weight": torch.zeros(up.shape[0], 256, dtype=torch.float16)}, CFG)  # 256 is taken
    c = "down_blocks.1.resnets.0.conv1"
    cd, cu = factors(c, 4)
    _refused({f"{c}.lora_down.weight": cd, f"{c}.lora_up.weight": cu.expand(-1, -1, 3, 3).contiguous()}, f"{c}.lora_up.weight")      # up convolution larger than 1 x 1
    _refused({f"{c}.lora_down.weight": cd[:, :, :1, :1].contiguous(), f"{c}.lora_up.weight": cu}, f"{c}.lora_down.weight")           # a 1 x 1 down for a 3 x 3 weight
    flat = "lora_unet_" + c.replace(".", "_")
    _refused({flat + ".lora_down.weight": cd, flat + ".lora_up.weight": cu, flat + ".lora_mid.weight": torch.zeros(4, 4, 3, 3)}, "lora_mid")
    for extra in ("dora_scale", "lora_magnitude_vector.default.weight", "hada_w1_a", "hada_w2_b", "lokr_w1", "lokr_w2_a"):
        _refused({**ok, f"unet.{q}.{extra}": torch.zeros(4)}, extra)
    for extra in ("lora_B.bias", "lora_B.default.bias", "bias", "diff_b"):
        _refused({**ok, f"unet.{q}.{extra}": torch.zeros(up.shape[0])}, extra)                                                   # bias deltas
    _refused({f"unet.{q}.lora_A.weight": down}, f"{q}.lora_A.weight")                                                            # one half missing
    _refused({f"unet.{q}.lora_B.weight": up}, f"{q}.lora_B.weight")
    _refused({f"unet.{q}.alpha": torch.tensor(1.0)}, f"{q}.alpha")
    _refused({**ok, f"{q}.lora_down.weight": down}, f"{q}.lora_down.weight")                                                     # the same half twice, in two spellings
    _refused({**ok, f"unet.{q}.something_else": down}, "something_else")
    bad = down.float().clone()
    bad[0, 0] = float("inf")
    _refused({f"unet.{q}.lora_A.weight": bad, f"unet.{q}.lora_B.weight": up}, f"{q}.lora_A.weight")                              # finite checks, before ...
    bad[0, 0] = 1e6
    _refused({f"unet.{q}.lora_A.weight": bad, f"unet.{q}.lora_B.weight": up}, f"{q}.lora_A.weight")                              # ... and after the conversion to fp16
    _refused({**ok, f"unet.{q}.alpha": torch.tensor(float("nan"))}, f"{q}.alpha")
    _refused({}, "no LoRA tensors")
    with pytest.raises(ValueError):
        L.parse_lora_state_dict(ok, CFG, text_encoder_keys="ignore")


@pytest.mark.parametrize("te_key", ["lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight", "lora_te1_text_model_encoder_layers_0_mlp_fc1.alpha",
                                    "lora_te2_text_model_encoder_layers_3_self_attn_q_proj.lora_up.weight", "text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_A.weight",
                                    "text_encoder_2.text_model.encoder.layers.0.mlp.fc1.lora_B.weight"])
def test_text_encoder_keys_error_or_skip(te_key):
    sd = adapter("peft", PICK[:2])
    want = L.parse_lora_state_dict(sd, CFG)
    sd[te_key] = torch.zeros(4, 4)
    with pytest.raises(ValueError) as e:
        L.parse_lora_state_dict(sd, CFG)
    assert te_key in str(e.value) and "text_encoder_keys='skip'" in str(e.value)           # says how to skip
    got, dropped = L.parse_lora_state_dict(sd, CFG, text_encoder_keys="skip")
    same(got, want)
    assert dropped == [te_key]
    assert L.parse_lora_state_dict(adapter("peft", PICK[:2]), CFG, text_encoder_keys="skip")[1] == []


def test_coef_is_computed_in_fp32():
    assert L.lora_coef(0.7, 8.0, 64) == float(np.float32(np.float32(0.7) * np.float32(8.0)) / np.float32(64))
    assert L.lora_coef(1.0, 3.5, 7) == 0.5 and L.lora_coef(-0.25, 16.0, 32) == -0.125
    assert L.lora_coef(0.1, 1.0, 3) == float(np.float32(np.float32(0.1) / np.float32(3))) != 0.1 / 3


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,ranks", R.CASES)
def test_lattice_cases_are_exact_in_fp32(N, K, ranks):
    case = R.lora_case(N, K, ranks, lattice=True)
    ok, peak = R.exactness(case)
    assert ok, peak
    for t in [case["base"], *case["ups"], *case["downs"]]:
        assert torch.equal(R.round16(t), t)                              # fp16 values
    ref, bound = R.lora_ref(case)
    assert bound is None
    assert R.worst(R.merge_model(case), ref)[0]                          # the fp32 model gives the reference's bits: nothing but the store rounds
    moved, kept = R.rounding_mix(case)
    if N * K >= 256:
        assert moved > 0 and kept > 0, (moved, kept)                     # some outputs need rounding at the store, some do not


@pytest.mark.parametrize("N,K,ranks", [c for c in R.CASES if c[0] * c[1] <= 129 * 264])
def test_the_model_meets_the_bound_on_real_values(N, K, ranks):
    case = R.lora_case(N, K, ranks, lattice=False)
    ref, bound = R.lora_ref(case)
    ok, n, at = R.worst(R.merge_model(case), ref, bound)
    assert ok, (n, at)
    assert float((bound / R.half_ulp16(ref.abs())).median()) < 1.5       # ... and the bound is the fp16 store plus little: nothing is hidden in it


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_fails_somewhere(mutant):
    failed = []
    for N, K, ranks in [c for c in R.CASES if c[0] * c[1] <= 129 * 264]:
        for lattice in (True, False):
            case = R.lora_case(N, K, ranks, lattice)
            got = R.merge_model(case, mutant)
            if got is None:
                continue
            ref, bound = R.lora_ref(case)
            if not R.worst(got, ref, bound)[0]:
                failed.append((N, K, ranks, lattice))
    assert failed, mutant
    if mutant in ("last_rank_dropped", "alpha_ignored", "roles_transposed"):
        assert any(f[3] for f in failed) and any(not f[3] for f in failed), failed      # caught on the lattice and on real values


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_and_exported():
    from instructany2pix_amd import _ffi, build
    build.build(verbose=False)
    hdr = open(os.path.join(ROOT, "include", "ia2p.h")).read()
    lib = _ffi.lib()
    for name in ("ia2p_lora_merge", "ia2p_read_tensor"):
        assert re.search(r"\bia2p_status\s+" + name + r"\s*\(", hdr), name
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
    assert re.search(r"#define\s+IA2P_LORA_MAX_RANK\s+256\b", hdr) and L.MAX_RANK == 256
    assert re.search(r"#define\s+IA2P_LORA_MAX_ADAPTERS\s+8\b", hdr) and L.MAX_ADAPTERS == 8
