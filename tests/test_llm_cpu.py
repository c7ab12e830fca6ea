"""Host side of the LLM stage without a GPU: prompt, stopping criterion, sampling arithmetic, the parsing half of `forward_llm`, and the
argument / state checks of the ia2p_llm_* ABI (none of which reaches a HIP call)."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(HERE, "golden", "llm_host.json")))


@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def test_prompt_matches_reference_conversation(gold):
    from instructany2pix_amd.llm import VICUNA_V1_SEP2, vicuna_v1_prompt
    assert len(gold["prompts"]) == 3
    for rec in gold["prompts"]:
        assert vicuna_v1_prompt(rec["inst"]) == rec["prompt"]
    assert VICUNA_V1_SEP2 == gold["stop_str"]


def test_get_all_objs_matches_reference(gold):
    from instructany2pix_amd.llm import get_all_objs
    assert len(gold["objs"]) == 4
    for rec in gold["objs"]:
        assert get_all_objs(rec["text"]) == rec["objs"]


def test_sampling_step_is_transformers_warpers():
    from transformers import TemperatureLogitsWarper, TopKLogitsWarper
    from instructany2pix_amd.llm import sample_next, sample_probs
    g = torch.Generator().manual_seed(5)
    for vocab, scale in ((512, 3.0), (32003, 6.0), (40, 1.0)):      # (40 < top_k: the warper clamps k to the vocabulary)
        logits = torch.randn(1, vocab, generator=g) * scale
        ids = torch.zeros(1, 4, dtype=torch.long)
        ref = TopKLogitsWarper(50)(ids, TemperatureLogitsWarper(0.3)(ids, logits.clone()))
        ref = torch.nn.functional.softmax(ref, dim=-1)
        got = sample_probs(logits, 0.3, 50)
        assert torch.equal(got, ref)
        assert int((got > 0).sum()) <= 50
        torch.manual_seed(11)
        want = torch.multinomial(ref, num_samples=1).squeeze(1)
        torch.manual_seed(11)
        assert torch.equal(sample_next(logits, True, 0.3, 50), want)
        assert torch.equal(sample_next(logits, False), logits.argmax(-1))
    # top_k=None: temperature only
    assert torch.equal(sample_probs(logits, 0.3, None), torch.nn.functional.softmax(logits / 0.3, dim=-1))


def test_keywords_stopping_criteria():
    from transformers import StoppingCriteria, StoppingCriteriaList
    from stub_llm_tokenizer import StubLlamaTokenizer
    from instructany2pix_amd.llm import KeywordsStoppingCriteria
    tok = StubLlamaTokenizer()
    prompt = tok("USER: hello ASSISTANT:", return_tensors="pt").input_ids
    crit = KeywordsStoppingCriteria(["</s>"], tok, prompt)
    assert isinstance(crit, StoppingCriteria)
    assert crit.start_len == prompt.shape[1] and crit.max_keyword_len == 1 and crit.keyword_ids[0].tolist() == [2]      # BOS stripped
    words = tok("a blue fox", add_special_tokens=False).input_ids
    seq = torch.cat([prompt, torch.tensor([words])], dim=1)
    assert crit(seq, None) is False
    assert not bool(torch.as_tensor(StoppingCriteriaList([crit])(seq, None)).all())
    done = torch.cat([seq, torch.tensor([[2]])], dim=1)
    assert crit(done, None) is True
    assert bool(torch.as_tensor(StoppingCriteriaList([crit])(done, None)).all())
    # a keyword that is ordinary text is found in the decoded tail
    crit2 = KeywordsStoppingCriteria(["fox"], tok, prompt)
    assert crit2(seq, None) is True and crit2(seq[:, :-1], None) is False
    with pytest.raises(AssertionError):
        crit.call_bse(torch.cat([seq, seq]), None)


class _LinearPredictor:
    def __init__(self, W):
        self.W = W

    def __call__(self, x):
        return x.float() @ self.W.t()


def _scripted(tokens, H=16, seed=0):
    """sequences [1, 3 + n] and one hidden-state entry per generated token (entry i: a tuple whose [-1] is [1, 1, H])"""
    g = torch.Generator().manual_seed(seed)
    seq = torch.tensor([[1, 7, 8] + tokens])
    hs = tuple((None, torch.randn(1, 1, H, generator=g)) for _ in tokens)
    return seq, hs


VIDEO, BASE, IM_GEN, EOS = 509, 510, 504, 2


def test_parse_generation_single_entry():
    from instructany2pix_amd.llm import parse_generation
    g = torch.Generator().manual_seed(1)
    W = torch.randn(8, 16, generator=g)
    aux = torch.randn(1, 8, generator=g)
    seq, hs = _scripted([20, 21, IM_GEN, VIDEO, EOS])
    text = "<s> USER: x ASSISTANT: [a blue fox] <im_gen> <video></s>"
    ie, be, cap, path, extra = parse_generation(seq, 3, hs, text, aux, [{"type": "image", "fname": "a.png"}], _LinearPredictor(W), VIDEO, BASE, IM_GEN)
    assert cap == "a blue fox" and path == "a.png"
    assert torch.equal(be, aux[0])                                   # one entry: base = entry 0
    assert ie.shape == (1, 1, 8) and torch.allclose(ie, hs[3][-1] @ W.t())      # the row that PREDICTED the <video> after <im_gen>
    assert extra["all_objs"] == [] and extra["extra_embeds"].shape == (0, 8) and extra["extra_idx"] == []


def test_parse_generation_three_entries_base_rule_and_subjects():
    from instructany2pix_amd.llm import parse_generation
    g = torch.Generator().manual_seed(2)
    W = torch.randn(8, 16, generator=g)
    aux = torch.randn(3, 8, generator=g)
    aux = aux / aux.norm(dim=-1, keepdim=True) * 20
    #          0     1     2    3       4      5    6      7   8      9
    tokens = [BASE, VIDEO, 30, IM_GEN, VIDEO, 31, VIDEO, 32, VIDEO, EOS]
    seq, hs = _scripted(tokens)
    mm = [{"type": "image", "fname": f"{i}.png"} for i in range(3)]
    text = "<s> USER: x ASSISTANT: [a fox and a dog] <base><video> <im_gen><video> additions: fox:<video>, dog:<video></s>"
    ie, be, cap, path, extra = parse_generation(seq, 3, hs, text, aux, mm, _LinearPredictor(W), VIDEO, BASE, IM_GEN)
    assert cap == "a fox and a dog"
    assert torch.allclose(ie, hs[4][-1] @ W.t())
    want_base = (hs[1][-1] @ W.t())[0]                                # the step after <base>
    assert torch.allclose(be, want_base)
    idx = (want_base / want_base.norm() * 20 @ aux.t())[0].argmax().item()
    assert path == f"{idx}.png"
    assert extra["all_objs"] == [" fox", ", dog"]
    ee = torch.cat([(hs[6][-1] @ W.t())[0], (hs[8][-1] @ W.t())[0]])
    want_idx = (ee / ee.norm() * 20 @ aux.t()).argmax(1)
    assert torch.equal(extra["extra_idx"], want_idx) and torch.equal(extra["extra_embeds"], aux[want_idx])
    # subject count mismatch (one name, two <video> rows): all_objs emptied, the raw predicted rows are kept
    text2 = "<s> USER: x ASSISTANT: [a fox and a dog] <base><video> <im_gen><video> additions: fox:<video></s>"
    _, _, _, _, extra2 = parse_generation(seq, 3, hs, text2, aux, mm, _LinearPredictor(W), VIDEO, BASE, IM_GEN)
    assert extra2["all_objs"] == [] and extra2["extra_idx"] == [] and torch.allclose(extra2["extra_embeds"], ee)


def test_parse_generation_without_im_gen():
    from instructany2pix_amd.llm import parse_generation
    seq, hs = _scripted([20, 21, EOS])
    out = parse_generation(seq, 3, hs, "<s> USER: x ASSISTANT: I cannot do that</s>", torch.zeros(1, 8), [{"fname": "a"}], None, VIDEO, BASE, IM_GEN)
    assert out == (None, None, " I cannot do that</s>", None, None)


def _cfg(**kw):
    from instructany2pix_amd import _ffi
    from instructany2pix_amd.config import LLMConfig
    c = LLMConfig(vocab_size=64, hidden_size=256, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128)
    cc = _ffi.make_llm_config(c.validate())
    for k, v in kw.items():
        setattr(cc, k, v)
    return cc


def test_llm_abi_refuses_shapes(lib):
    h = C.c_void_p()
    for kw, word in ((dict(num_heads=4, num_kv_heads=4), b"head dim 128"), (dict(num_kv_heads=1), b"key/value heads"),
                     (dict(hidden_size=288, num_heads=2), b"multiple of 64"), (dict(intermediate_size=100), b"intermediate")):
        assert lib.ia2p_llm_create(C.byref(_cfg(**kw)), C.byref(h)) == 2, kw
        assert not h.value and word in lib.ia2p_llm_last_error(None), lib.ia2p_llm_last_error(None)
    assert lib.ia2p_llm_create(None, C.byref(h)) == 1
    assert lib.ia2p_llm_create(C.byref(_cfg()), None) == 1


def test_llm_abi_sizes_and_state(lib):
    from instructany2pix_amd import _ffi
    from instructany2pix_amd.config import tiny_llm, vicuna_7b
    from instructany2pix_amd.weights import llama_param_specs, param_count
    cfg = vicuna_7b(32000)
    h = C.c_void_p()
    _ffi.check(lib.ia2p_llm_create(C.byref(_ffi.make_llm_config(cfg)), C.byref(h)), None, llm=True)
    n = param_count(llama_param_specs(cfg))
    assert 6.7e9 < n < 6.8e9
    assert 2 * n <= lib.ia2p_llm_arena_bytes(h) <= 2 * n * 1.01
    assert lib.ia2p_llm_kv_bytes(h, 1024) == 2 * 32 * 1024 * 4096 * 2
    assert lib.ia2p_llm_kv_bytes(h, 0) == 0 and lib.ia2p_llm_kv_bytes(h, 8193) == 0 and lib.ia2p_llm_kv_bytes(None, 16) == 0
    lib.ia2p_llm_destroy(h)

    h = C.c_void_p()
    _ffi.check(lib.ia2p_llm_create(C.byref(_ffi.make_llm_config(tiny_llm())), C.byref(h)), None, llm=True)
    assert lib.ia2p_llm_position(h) == 0 and lib.ia2p_llm_position(None) == -1
    ws64, ws8 = lib.ia2p_llm_workspace_bytes(h, 64), lib.ia2p_llm_workspace_bytes(h, 8)      # a host dry run
    assert ws64 > ws8 > 0 and lib.ia2p_llm_workspace_bytes(h, 0) == 0
    one = C.c_void_p(256)           # never dereferenced: every call below is refused before any HIP call
    # null arguments
    assert lib.ia2p_llm_bind_arena(h, None, 1 << 20) == 1
    assert lib.ia2p_llm_bind_kv(h, None, 1 << 20, 16) == 1
    assert lib.ia2p_llm_prefill(h, None, None, 4, one, one, one, 1 << 20) == 1
    assert lib.ia2p_llm_decode(h, None, 3, None, one, one, 1 << 20) == 1
    assert lib.ia2p_llm_embed(h, None, None, 4, one) == 1
    assert lib.ia2p_llm_reset(None) == 1
    assert lib.ia2p_llm_gemv(None, None, one, one, 8, 8) == 1 and lib.ia2p_llm_gemv(None, one, one, one, 8, 12) == 2
    assert lib.ia2p_gelu(None, None, 8) == 1 and lib.ia2p_gelu(None, one, 0) == 2
    # wrong state: nothing bound, nothing loaded
    assert lib.ia2p_llm_load_tensor(h, b"model.norm.weight", one, (C.c_int64 * 1)(512), 1, None) == 4
    assert lib.ia2p_llm_finalize_weights(h) == 4
    assert lib.ia2p_llm_prefill(h, None, one, 4, one, one, one, 1 << 20) == 4
    assert lib.ia2p_llm_decode(h, None, 3, one, one, one, 1 << 20) == 4
    assert b"finalized" in lib.ia2p_llm_last_error(h)
    assert lib.ia2p_llm_embed(h, None, one, 4, one) == 4
    # cache too small / too many positions
    assert lib.ia2p_llm_bind_kv(h, one, 16, 16) == 5
    assert lib.ia2p_llm_bind_kv(h, one, 1 << 40, 8193) == 2
    with pytest.raises(_ffi.IA2PError):
        _ffi.check(lib.ia2p_llm_finalize_weights(h), h, llm=True)
    lib.ia2p_llm_destroy(h)


def test_llm_operation_entry_points_refuse_before_any_launch(lib):
    """every call below is refused on the host (the pointers are never dereferenced and no GPU is needed); a refused call leaves its outputs untouched (the
    host output here; tests/test_llm_ops_gpu.py::test_refused_calls_write_nothing looks at the device outputs)"""
    INVALID, SHAPE = 1, 2
    one, odd = C.c_void_p(256), C.c_void_p(264)          # 16-byte aligned / not
    cb = (C.c_float * 16)(*range(16))
    ptrs, nulls = (C.c_void_p * 8)(*[256] * 8), (C.c_void_p * 8)(256, None)
    pos = lambda *p: (C.c_int32 * 8)(*(list(p) + [0] * (8 - len(p))))      # noqa: E731
    epi, qkv, att, pre = lib.ia2p_llm_gemv_epi, lib.ia2p_llm_gemv_qkv, lib.ia2p_llm_attention_rows, lib.ia2p_llm_attention_prefill
    cases = [
        # the GEMV with an epilogue: W, absmax, codebook, x, gamma, eps, epi, out, hid, N, K, M
        (epi(None, None, None, None, one, None, 0.0, 0, one, None, 64, 64, 1), INVALID),          # W
        (epi(None, one, None, None, None, None, 0.0, 0, one, None, 64, 64, 1), INVALID),          # x
        (epi(None, one, None, None, one, None, 0.0, 0, None, None, 64, 64, 1), INVALID),          # out
        (epi(None, one, one, None, one, None, 0.0, 0, one, None, 64, 64, 1), INVALID),            # absmax without a codebook
        (epi(None, one, None, cb, one, None, 0.0, 0, one, None, 64, 64, 1), INVALID),             # a codebook without absmax
        (epi(None, one, None, None, one, None, 0.0, 3, one, None, 64, 64, 1), INVALID),           # epilogue
        (epi(None, one, None, None, one, None, 0.0, -1, one, None, 64, 64, 1), INVALID),
        (epi(None, one, None, None, one, None, 0.0, 0, one, one, 64, 64, 1), INVALID),            # hid without gamma
        (epi(None, one, None, None, one, one, 1e-5, 1, one, one, 64, 64, 1), INVALID),            # hid with the residual epilogue
        (epi(None, one, None, None, one, one, -1.0, 0, one, None, 64, 64, 1), INVALID),           # eps
        (epi(None, one, None, None, one, None, 0.0, 0, one, None, 64, 64, 0), SHAPE),             # M
        (epi(None, one, None, None, one, None, 0.0, 0, one, None, 64, 64, 9), SHAPE),
        (epi(None, one, None, None, one, None, 0.0, 0, one, None, 64, 12, 1), SHAPE),             # K (fp16: a multiple of 8)
        (epi(None, one, None, None, one, None, 0.0, 0, one, None, 0, 64, 1), SHAPE),              # N
        (epi(None, one, None, None, one, None, 0.0, 2, one, None, 65, 64, 1), SHAPE),             # SwiGLU: an odd N
        (epi(None, one, one, cb, one, None, 0.0, 0, one, None, 64, 96, 2), SHAPE),                # K (4 bits: a multiple of 64, at most 14336)
        (epi(None, one, one, cb, one, None, 0.0, 0, one, None, 64, 14400, 2), SHAPE),
        # QKV: W, absmax, codebook, x, gamma, eps, inv_freq, pos, q, k_cache, v_cache, H, K, M
        (qkv(None, one, None, None, one, None, 0.0, None, pos(1), one, ptrs, ptrs, 128, 64, 1), INVALID),
        (qkv(None, one, None, None, one, None, 0.0, one, None, one, ptrs, ptrs, 128, 64, 1), INVALID),
        (qkv(None, one, None, None, one, None, 0.0, one, pos(1), None, ptrs, ptrs, 128, 64, 1), INVALID),
        (qkv(None, one, None, None, one, None, 0.0, one, pos(1), one, None, ptrs, 128, 64, 1), INVALID),
        (qkv(None, None, None, None, one, None, 0.0, one, pos(1), one, ptrs, ptrs, 128, 64, 1), INVALID),
        (qkv(None, one, None, None, one, None, 0.0, one, pos(1, 1), one, ptrs, nulls, 128, 64, 2), INVALID),      # the cache of row 1
        (qkv(None, one, None, None, one, None, 0.0, one, pos(1), one, ptrs, ptrs, 192, 64, 1), SHAPE),            # H
        (qkv(None, one, None, None, one, None, 0.0, one, pos(1), one, ptrs, ptrs, 0, 64, 1), SHAPE),
        (qkv(None, one, None, None, one, None, 0.0, one, pos(1), one, ptrs, ptrs, 128, 64, 9), SHAPE),            # M
        (qkv(None, one, None, None, one, None, 0.0, one, pos(1, 8192), one, ptrs, ptrs, 128, 64, 2), SHAPE),      # positions
        (qkv(None, one, None, None, one, None, 0.0, one, pos(-1), one, ptrs, ptrs, 128, 64, 1), SHAPE),
        (qkv(None, one, one, cb, one, None, 0.0, one, pos(1), one, ptrs, ptrs, 128, 32, 1), SHAPE),               # K, 4 bits
        # decode attention: q, k_cache, v_cache, pos, out, heads, H, M
        (att(None, None, ptrs, ptrs, pos(1), one, 1, 128, 1), INVALID),
        (att(None, one, ptrs, ptrs, pos(1), None, 1, 128, 1), INVALID),
        (att(None, one, ptrs, None, pos(1), one, 1, 128, 1), INVALID),
        (att(None, one, nulls, ptrs, pos(1, 1), one, 1, 128, 2), INVALID),
        (att(None, one, (C.c_void_p * 8)(264), ptrs, pos(1), one, 1, 128, 1), INVALID),          # alignment
        (att(None, one, ptrs, ptrs, pos(1), one, 2, 128, 1), SHAPE),                               # H is not heads * 128
        (att(None, one, ptrs, ptrs, pos(1), one, 0, 0, 1), SHAPE),
        (att(None, one, ptrs, ptrs, pos(1), one, 1, 128, 0), SHAPE),
        (att(None, one, ptrs, ptrs, pos(1), one, 1, 128, 9), SHAPE),
        (att(None, one, ptrs, ptrs, pos(1, 8192), one, 1, 128, 2), SHAPE),
        (att(None, one, ptrs, ptrs, pos(-1), one, 1, 128, 1), SHAPE),
        # prefill attention: q, k_cache, v_cache, out, heads, H, p0, T
        (pre(None, None, one, one, one, 1, 128, 0, 1), INVALID),
        (pre(None, one, one, one, None, 1, 128, 0, 1), INVALID),
        (pre(None, one, odd, one, one, 1, 128, 0, 1), INVALID),
        (pre(None, one, one, one, one, 3, 256, 0, 1), SHAPE),
        (pre(None, one, one, one, one, 1, 128, 0, 0), SHAPE),
        (pre(None, one, one, one, one, 1, 128, -1, 1), SHAPE),
        (pre(None, one, one, one, one, 1, 128, 8192, 1), SHAPE),
        (pre(None, one, one, one, one, 1, 128, 8000, 193), SHAPE),
        # the prefill row kernels
        (lib.ia2p_llm_rmsnorm_rows(None, None, one, 1e-5, one, 1, 128), INVALID),
        (lib.ia2p_llm_rmsnorm_rows(None, one, one, 1e-5, None, 1, 128), INVALID),
        (lib.ia2p_llm_rmsnorm_rows(None, one, one, -1.0, one, 1, 128), INVALID),
        (lib.ia2p_llm_rmsnorm_rows(None, one, one, 1e-5, one, 0, 128), SHAPE),
        (lib.ia2p_llm_rmsnorm_rows(None, one, one, 1e-5, one, 1, 0), SHAPE),
        (lib.ia2p_llm_rope_cache_rows(None, one, None, one, one, one, 128, 0, 1), INVALID),
        (lib.ia2p_llm_rope_cache_rows(None, one, one, one, one, None, 128, 0, 1), INVALID),
        (lib.ia2p_llm_rope_cache_rows(None, one, one, one, one, one, 192, 0, 1), SHAPE),
        (lib.ia2p_llm_rope_cache_rows(None, one, one, one, one, one, 128, 8191, 2), SHAPE),
        (lib.ia2p_llm_rope_cache_rows(None, one, one, one, one, one, 128, -1, 1), SHAPE),
        (lib.ia2p_llm_silu_mul_rows(None, None, one, 1, 64), INVALID),
        (lib.ia2p_llm_silu_mul_rows(None, one, one, 0, 64), SHAPE),
        (lib.ia2p_llm_silu_mul_rows(None, one, one, 1, 0), SHAPE),
    ]
    wrong = [(i, got, want) for i, (got, want) in enumerate(cases) if got != want]
    assert not wrong, wrong
    assert b"llm_silu_mul_rows" in lib.ia2p_llm_last_error(None)
    f = (C.c_float * 64)(*[7.0] * 64)
    for theta in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.ia2p_llm_rope_inv_freq(theta, f) == INVALID and list(f) == [7.0] * 64, theta
    assert lib.ia2p_llm_rope_inv_freq(10000.0, None) == INVALID


@pytest.mark.parametrize("theta", [10000.0, 500000.0, 1e6])
def test_rotary_table_against_torch(lib, theta):
    """the table ia2p_llm_finalize_weights uploads (the same host function) against transformers' torch expression: every entry within one fp32 ulp.
    Entries that differ and the largest angle difference they make at position 8191 are printed; docs/LOG.md records them."""
    import numpy as np
    from llm_ops_ref import inv_freq_torch
    f = (C.c_float * 64)()
    assert lib.ia2p_llm_rope_inv_freq(theta, f) == 0
    got, want = np.array(list(f), dtype=np.float32), inv_freq_torch(theta).numpy()
    assert want.dtype == np.float32 and want.shape == (64,) and got[0] == 1.0
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    angle = np.abs(np.float32(8191) * got - np.float32(8191) * want).astype(np.float64)
    print(f"[llm] rotary table theta={theta:g}: {int((ulps != 0).sum())} of 64 entries differ from torch's, largest difference {int(ulps.max())} ulp, "
          f"largest angle difference at position 8191 {float(angle.max()):.3e} rad")
    assert int(ulps.max()) <= 1


@pytest.mark.parametrize("bits", [16, 4])
def test_llm_workspace_bytes_are_the_recorded_ones(lib, bits):
    """`tiny_llm()`: the bytes `ia2p_llm_workspace_bytes(c, T)` and `ia2p_llm_batch_workspace_bytes(c, T, n)` returned before the single-row and the
    batched decode driver became one (host dry runs; a decode step of one row allocates the four buffers it always did)"""
    from instructany2pix_amd import _ffi
    from instructany2pix_amd.config import BNB_4BIT_CODEBOOKS, tiny_llm
    prefill = {16: {1: 18944, 9: 152064, 33: 551424}, 4: {1: 2902528, 9: 3035648, 33: 3435008}}[bits]
    decode = {1: 12032, 2: 23808, 8: 94464}          # n rows, either format (T = 0: no prefill)
    h = C.c_void_p()
    _ffi.check(lib.ia2p_llm_create(C.byref(_ffi.make_llm_config(tiny_llm())), C.byref(h)), None, llm=True)
    if bits == 4:
        _ffi.check(lib.ia2p_llm_set_weight_format(h, 4, (C.c_float * 16)(*BNB_4BIT_CODEBOOKS["fp4"])), h, llm=True)
    for T, want in prefill.items():
        assert lib.ia2p_llm_workspace_bytes(h, T) == want, (bits, T)
        for n in (1, 8):
            assert lib.ia2p_llm_batch_workspace_bytes(h, T, n) == max(want, decode[n]), (bits, T, n)
    for n, want in decode.items():
        assert lib.ia2p_llm_batch_workspace_bytes(h, 0, n) == want, (bits, n)
    lib.ia2p_llm_destroy(h)


def test_llm_param_specs_cover_the_checkpoint_keys():
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
    cfg = tiny_llm()
    sd = synthetic_state_dict(llm_param_specs(cfg, 1024, "linear"))
    assert sd["model.vae_projector_image.weight"].shape == (512, 1024) and sd["model.vae_predictor_image.bias"].shape == (1024,)
    assert sd["model.layers.3.mlp.down_proj.weight"].shape == (512, 1408) and sd["lm_head.weight"].shape == (512, 512)
    keys = [k for k, _, _ in llm_param_specs(cfg, 1024, "mlp2x_gelu")]
    assert "model.vae_projector_image.0.weight" in keys and "model.vae_projector_image.2.bias" in keys and "model.vae_predictor_image.2.weight" in keys
    with pytest.raises(ValueError):
        llm_param_specs(cfg, 1024, "identity")
