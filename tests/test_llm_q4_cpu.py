"""The 4-bit weight format of the LLM engine without a GPU: the CPU reference quantiser (tests/q4_ref.py) against its own definition, and the
planning / argument checks of ia2p_llm_set_weight_format and the ia2p_llm_*_q4 entry points, none of which reaches a HIP call."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q4_ref  # noqa: E402

KINDS = ["fp4", "nf4"]
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def _weights(shape, seed, scale=0.03):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).half()


def test_package_tables_are_the_reference_tables():
    from instructany2pix_amd.config import BNB_4BIT_CODEBOOKS
    assert set(BNB_4BIT_CODEBOOKS) == set(q4_ref.CODEBOOKS)
    for k in KINDS:
        a, b = torch.tensor(BNB_4BIT_CODEBOOKS[k], dtype=torch.float32), torch.tensor(q4_ref.CODEBOOKS[k], dtype=torch.float32)
        assert torch.equal(a, b) and len(BNB_4BIT_CODEBOOKS[k]) == 16
        assert float(a.abs().max()) == 1.0 and float(a.min()) == -1.0


@pytest.mark.parametrize("kind", KINDS)
def test_reference_round_trip_and_error_bound(kind):
    cb = q4_ref.CODEBOOKS[kind]
    w = _weights((96, 256), 3)
    codes, absmax = q4_ref.quantize_ref(w, cb)
    assert codes.shape == w.shape and codes.dtype == torch.uint8 and absmax.shape == (96 * 256 // 64,) and absmax.dtype == torch.float32
    assert torch.equal(absmax, w.float().reshape(-1, 64).abs().amax(1))
    deq = q4_ref.dequantize_ref(codes, absmax, cb)
    assert deq.dtype == torch.float16
    # quantising the dequantised tensor reproduces the value every weight stood for (fp4 holds 0 twice, as codes 0 and 8: compare values)
    codes2, absmax2 = q4_ref.quantize_ref(deq, cb)
    cbt = torch.tensor(cb, dtype=torch.float32)
    assert torch.equal(cbt[codes2.long()], cbt[codes.long()])
    assert torch.equal(q4_ref.dequantize_ref(codes2, absmax2, cb), deq)
    # nearest entry: no weight is farther from its product than half the largest gap of the codebook, times absmax (+ the fp16 rounding of the product)
    s, _, _ = q4_ref.sorted_codebook(cb)
    gap = float((s[1:] - s[:-1]).max())
    err = (q4_ref.dequantize_unrounded(codes, absmax, cb).double() - w.double()).abs().reshape(-1, 64)
    bound = absmax.double()[:, None] * gap / 2 * (1 + 2.0 ** -20)
    assert bool((err <= bound).all())
    # the threshold rule agrees in value with plain argmin except on midpoint ties
    x = (w.float().reshape(-1, 64) / absmax[:, None]).reshape(-1)
    nearest = (x[:, None] - cbt[None]).abs().argmin(1)
    agree = float((cbt[nearest] == cbt[codes.reshape(-1).long()]).double().mean())
    assert agree > 0.9999


@pytest.mark.parametrize("kind", KINDS)
def test_reference_zero_block_and_negative_extreme(kind):
    cb = q4_ref.CODEBOOKS[kind]
    cbt = torch.tensor(cb, dtype=torch.float32)
    w = _weights((2, 128), 5)
    w[0, 64:] = 0                                   # an all-zero block
    w[1, :64] = w[1, :64].abs()
    w[1, 7] = -0.5                                  # a block whose extreme is negative
    codes, absmax = q4_ref.quantize_ref(w, cb)
    assert float(absmax[1]) == 0.0 and bool((cbt[codes[0, 64:].long()] == 0).all()) and len(set(codes[0, 64:].tolist())) == 1
    assert cb[int(codes[0, 64])] == 0.0 and (kind != "fp4" or int(codes[0, 64]) == 0)
    deq = q4_ref.dequantize_ref(codes, absmax, cb)
    assert bool((deq[0, 64:] == 0).all()) and not bool(deq.isnan().any())
    assert float(absmax[2]) == 0.5 and cb[int(codes[1, 7])] == -1.0 and float(deq[1, 7]) == -0.5


def _expected_q4_arena(lib, cfg):
    """-> (bytes without padding, number of separately aligned pieces)"""
    from instructany2pix_amd.weights import llama_param_specs
    total, pieces = 256, 1                          # the rotary table
    for key, shape, _ in llama_param_specs(cfg):
        n = 1
        for d in shape:
            n *= d
        if any(f".{p}.weight" in key for p in PROJ):
            packed = lib.ia2p_llm_q4_packed_bytes(shape[0], shape[1])
            assert packed == n // 2
            total += packed + 4 * (n // 64)
            pieces += 2
        else:
            total += 2 * n
            pieces += 1
    return total, pieces


def _create(lib, cfg):
    from instructany2pix_amd import _ffi
    h = C.c_void_p()
    _ffi.check(lib.ia2p_llm_create(C.byref(_ffi.make_llm_config(cfg)), C.byref(h)), None, llm=True)
    return h


@pytest.mark.parametrize("kind", KINDS)
def test_set_weight_format_plans_the_smaller_arena(lib, kind):
    from instructany2pix_amd.config import tiny_llm, vicuna_7b
    cb = (C.c_float * 16)(*q4_ref.CODEBOOKS[kind])
    for cfg, is7b in ((tiny_llm(), False), (vicuna_7b(32000), True)):
        h = _create(lib, cfg)
        assert lib.ia2p_llm_weight_bits(h) == 16
        a16 = lib.ia2p_llm_arena_bytes(h)
        assert lib.ia2p_llm_set_weight_format(h, 4, cb) == 0 and lib.ia2p_llm_weight_bits(h) == 4
        a4 = lib.ia2p_llm_arena_bytes(h)
        want, pieces = _expected_q4_arena(lib, cfg)
        print(f"[q4] {kind} {'7B' if is7b else 'tiny'}: arena {a16} -> {a4} bytes ({a4 / a16:.4f}), unpadded {want}")
        assert want <= a4 <= want + 256 * pieces
        if is7b:
            assert a4 < 0.35 * a16
        assert lib.ia2p_llm_set_weight_format(h, 16, None) == 0 and lib.ia2p_llm_weight_bits(h) == 16
        assert lib.ia2p_llm_arena_bytes(h) == a16
        lib.ia2p_llm_destroy(h)


def test_workspace_includes_the_dequantisation_scratch(lib):
    from instructany2pix_amd.config import tiny_llm
    cfg = tiny_llm()
    cb = (C.c_float * 16)(*q4_ref.CODEBOOKS["fp4"])
    h = _create(lib, cfg)
    H, I = cfg.hidden_size, cfg.intermediate_size
    scratch = 2 * max(3 * H * H, 2 * I * H)
    for T in (1, 8, 64):
        w16 = lib.ia2p_llm_workspace_bytes(h, T)
        assert lib.ia2p_llm_set_weight_format(h, 4, cb) == 0
        w4 = lib.ia2p_llm_workspace_bytes(h, T)
        assert lib.ia2p_llm_set_weight_format(h, 16, None) == 0
        assert w16 > 0 and w4 >= w16 + scratch, (T, w16, w4)
    lib.ia2p_llm_destroy(h)


def test_set_weight_format_and_q4_ops_refuse_bad_arguments(lib):
    from instructany2pix_amd.config import tiny_llm
    cb = (C.c_float * 16)(*q4_ref.CODEBOOKS["nf4"])
    one = C.c_void_p(256)           # never dereferenced: every call below is refused before any HIP call
    h = _create(lib, tiny_llm())
    assert lib.ia2p_llm_set_weight_format(None, 4, cb) == 1 and lib.ia2p_llm_weight_bits(None) == 0
    assert lib.ia2p_llm_set_weight_format(h, 8, cb) == 1 and b"8 bits" in lib.ia2p_llm_last_error(h)
    assert lib.ia2p_llm_set_weight_format(h, 4, None) == 1 and b"codebook" in lib.ia2p_llm_last_error(h)
    assert lib.ia2p_llm_weight_bits(h) == 16
    assert lib.ia2p_llm_set_weight_format(h, 4, cb) == 0
    assert lib.ia2p_llm_bind_arena(h, one, 16) == 5              # too small for the 4-bit arena as well
    assert lib.ia2p_llm_bind_arena(h, one, 1 << 40) == 0
    assert lib.ia2p_llm_set_weight_format(h, 16, None) == 4 and b"bind_arena" in lib.ia2p_llm_last_error(h)
    assert lib.ia2p_llm_weight_bits(h) == 4
    lib.ia2p_llm_destroy(h)
    # K must divide into blocks of 64
    assert lib.ia2p_llm_q4_packed_bytes(4, 96) == 0 and lib.ia2p_llm_q4_packed_bytes(0, 64) == 0 and lib.ia2p_llm_q4_packed_bytes(3, 128) == 192
    assert lib.ia2p_llm_quantize_q4(None, one, 4, 96, cb, one, one) == 2
    assert lib.ia2p_llm_dequantize_q4(None, one, one, 4, 100, cb, one) == 2
    assert lib.ia2p_llm_gemv_q4(None, one, one, cb, one, one, 8, 96) == 2
    assert b"multiple of 64" in lib.ia2p_llm_last_error(None)
    assert lib.ia2p_llm_gemv_q4(None, one, one, cb, one, one, 8, 16384) == 2          # past the rows the staged input serves
    # null arguments
    assert lib.ia2p_llm_quantize_q4(None, None, 4, 64, cb, one, one) == 1
    assert lib.ia2p_llm_quantize_q4(None, one, 4, 64, None, one, one) == 1
    assert lib.ia2p_llm_dequantize_q4(None, one, None, 4, 64, cb, one) == 1
    assert lib.ia2p_llm_gemv_q4(None, one, one, None, one, one, 8, 64) == 1
    assert lib.ia2p_llm_gemv_q4(None, one, one, cb, None, one, 8, 64) == 1


def test_constructor_refuses_an_unknown_quant_type():
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    with pytest.raises(ValueError, match="bnb_4bit_quant_type"):
        HipInstructAny2PixLM(tiny_llm(), load_in_4bit=True, bnb_4bit_quant_type="int4")
