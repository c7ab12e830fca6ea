"""The 4-bit weight format of the LLM engine on the GPU (`load_in_4bit`, "fp4" and "nf4"): the quantise / dequantise kernels bit for bit against
the CPU reference of tests/q4_ref.py, the dequantising GEMV against an fp64 dot, and the engine against transformers `LlamaForCausalLM` on the
CPU loaded with the fp16-rounded dequantised projections of that reference.

Tolerances. Kernels: every code, absmax and dequantised value equal. GEMV: `e_q4 <= 2 * e_16 + e_round` against the fp64 dot with the
fp16-rounded dequantised matrix; `e_16` is the error of the existing fp16 `ia2p_llm_gemv` fed that matrix and the same x (factor 2: another
summation order), `e_round` the fp64 rel-L2 between dotting the unrounded and the rounded products (the kernel scales a block's sum by its
absmax once, so it computes from the unrounded ones). Model: the rule of tests/test_llm_gpu.py with the yardstick moved onto the quantised
model -- `e_ref = rel-L2(fp16 oracle, fp32 oracle)` over the checked rows, every HIP row within `2 * e_ref` of the fp32 oracle; greedy:
`delta = 2 * max|fp16 - fp32 oracle logits|`. Every figure is printed before it is asserted (pytest -s); docs/LOG.md §15 records a run."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q4_ref  # noqa: E402
from test_llm_gpu import _ids, _prefill_then_decode, _reference_inputs_embeds, make_oracle, oracle_rows, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["fp4", "nf4"]
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
SMALL = [(520, 512), (2816, 512), (512, 1408)]
LAYER_7B = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)]


def _lib():
    from instructany2pix_amd import _ffi
    return _ffi, _ffi.lib()


def _cb(kind):
    return (C.c_float * 16)(*q4_ref.CODEBOOKS[kind])


def _weights(N, K, seed):
    return (torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) * K ** -0.5).half()


def gpu_quantize(w, kind):
    """fp16 [N, K] on the device -> (packed bytes, absmax fp32 [N K / 64]) from ia2p_llm_quantize_q4"""
    ffi, lib = _lib()
    N, K = w.shape
    packed = torch.empty(lib.ia2p_llm_q4_packed_bytes(N, K), dtype=torch.uint8, device=DEV)
    absmax = torch.empty(N * K // 64, dtype=torch.float32, device=DEV)
    ffi.check(lib.ia2p_llm_quantize_q4(ffi.current_stream(), ffi.ptr(w), N, K, _cb(kind), ffi.ptr(packed), ffi.ptr(absmax)), None, llm=True)
    return packed, absmax


def gpu_dequantize(packed, absmax, N, K, codebook):
    ffi, lib = _lib()
    out = torch.empty(N, K, dtype=torch.float16, device=DEV)
    ffi.check(lib.ia2p_llm_dequantize_q4(ffi.current_stream(), ffi.ptr(packed), ffi.ptr(absmax), N, K, (C.c_float * 16)(*codebook), ffi.ptr(out)), None, llm=True)
    return out


def gpu_codes(packed, N, K):
    """the codes of a packed matrix without knowing its layout: dequantised with the table (0, 1, .., 15) and every absmax 1"""
    ones = torch.ones(N * K // 64, dtype=torch.float32, device=DEV)
    return gpu_dequantize(packed, ones, N, K, list(range(16))).to(torch.uint8).cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SMALL + [(4096, 11008)])
def test_quantize_and_dequantize_kernels_equal_the_reference(kind, shape):
    N, K = shape
    w = _weights(N, K, 50 + N % 97)
    w[3, 64:128] = 0                                 # one all-zero block
    w[5, :64] = w[5, :64].abs()
    w[5, 9] = -float(w[5, :64].max()) * 2            # a block whose extreme is negative
    codes, absmax = q4_ref.quantize_ref(w, q4_ref.CODEBOOKS[kind])
    packed, am = gpu_quantize(w.to(DEV), kind)
    got = gpu_codes(packed, N, K)
    n_codes, n_abs = int((got != codes).sum()), int((am.cpu() != absmax).sum())
    print(f"[q4] quantise {kind} {N} x {K}: {n_codes} of {N * K} codes and {n_abs} of {absmax.numel()} absmax differ from the reference")
    assert n_codes == 0 and n_abs == 0
    assert float(am[(3 * K + 64) // 64]) == 0.0
    deq = gpu_dequantize(packed, am, N, K, q4_ref.CODEBOOKS[kind]).cpu()
    want = q4_ref.dequantize_ref(codes, absmax, q4_ref.CODEBOOKS[kind])
    n_deq = int((deq.view(torch.int16) != want.view(torch.int16)).sum())
    print(f"[q4] dequantise {kind} {N} x {K}: {n_deq} values differ in bits from the reference")
    assert n_deq == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", LAYER_7B + SMALL + [(517, 512)])
def test_gemv_q4_against_fp64(kind, shape):
    ffi, lib = _lib()
    N, K = shape
    cb = q4_ref.CODEBOOKS[kind]
    w = _weights(N, K, 70 + N % 89)
    codes, absmax = q4_ref.quantize_ref(w, cb)
    w_round = q4_ref.dequantize_ref(codes, absmax, cb)
    x = torch.randn(K, generator=torch.Generator().manual_seed(K))
    want = w_round.double() @ x.double()
    e_round = rel_l2(q4_ref.dequantize_unrounded(codes, absmax, cb).double() @ x.double(), want)
    xd = x.to(DEV)
    packed, am = gpu_quantize(w.to(DEV), kind)
    o4 = torch.full((N,), float("nan"), dtype=torch.float32, device=DEV)
    o16 = torch.empty(N, dtype=torch.float32, device=DEV)
    s = ffi.current_stream()
    ffi.check(lib.ia2p_llm_gemv_q4(s, ffi.ptr(packed), ffi.ptr(am), _cb(kind), ffi.ptr(xd), ffi.ptr(o4), N, K), None, llm=True)
    wr = w_round.to(DEV)
    ffi.check(lib.ia2p_llm_gemv(s, ffi.ptr(wr), ffi.ptr(xd), ffi.ptr(o16), N, K), None, llm=True)
    torch.cuda.synchronize()
    e_q4, e_16 = rel_l2(o4, want), rel_l2(o16, want)
    print(f"[q4] gemv {kind} {N} x {K}: e_q4 {e_q4:.3e}, e_16 {e_16:.3e}, e_round {e_round:.3e}, bound {2 * e_16 + e_round:.3e}")
    assert e_q4 <= 2 * e_16 + e_round


# ---- the engine against the oracle on the quantised model -------------------------------------------------------------
def quantised_state_dict(sd, kind, heads=True):
    """the weights bitsandbytes' loader leaves the model computing from: every decoder projection (and the two heads' Linears) quantised and
    dequantised once, in blocks of 64 along the flattened tensor; embeddings, norms, lm_head and biases as they are"""
    out = {}
    for k, v in sd.items():
        q = any(f".{p}.weight" in k for p in PROJ) or (heads and ("vae_pro" in k or "vae_pre" in k) and k.endswith(".weight"))
        out[k] = q4_ref.round_trip(v.reshape(-1, 64), q4_ref.CODEBOOKS[kind]).reshape(v.shape) if q else v
    return out


class Bundle4:
    def __init__(self, cfg, seed, kind, projector_type="linear", max_positions=256):
        from instructany2pix_amd.llm import HipInstructAny2PixLM
        from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
        self.cfg, self.kind = cfg, kind
        self.sd = synthetic_state_dict(llm_param_specs(cfg, cfg.embed_dim, projector_type), seed=seed)
        self.sdq = quantised_state_dict(self.sd, kind)
        self.o32, self.o16 = make_oracle(cfg, self.sdq)
        self.lm = HipInstructAny2PixLM(cfg, DEV, max_positions=max_positions, video_token_id=cfg.vocab_size - 3, load_in_4bit=True, bnb_4bit_quant_type=kind)
        self.lm.load_state_dict(self.sd)             # the unquantised fp16 checkpoint: quantised at load

    def refs(self, ids=None, embeds=None):
        h32, l32 = oracle_rows(self.o32, ids, embeds)
        h16, l16 = oracle_rows(self.o16, ids, embeds)
        return h32, l32, h16, l16


@pytest.fixture(scope="module", params=KINDS)
def tiny4(request):
    from instructany2pix_amd.config import tiny_llm
    return Bundle4(tiny_llm(), seed=21, kind=request.param)


def _check(tag, hip_h, hip_l, h32, l32, eh, el):
    dh, dl = rel_l2(hip_h, h32), rel_l2(hip_l, l32)
    print(f"[q4] {tag}: hidden rel-L2 {dh:.3e} (e_ref {eh:.3e}), logits rel-L2 {dl:.3e} (e_ref {el:.3e})")
    return dh <= 2 * eh and dl <= 2 * el


def test_format_is_reported_and_the_arena_is_smaller(tiny4):
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    lm16 = HipInstructAny2PixLM(tiny4.cfg, DEV, max_positions=8)
    print(f"[q4] {tiny4.kind}: arena {lm16.arena.numel()} -> {tiny4.lm.arena.numel()} bytes")
    assert tiny4.lm.weight_bits == 4 and lm16.weight_bits == 16 and tiny4.lm.quant_type == tiny4.kind and lm16.quant_type is None
    assert tiny4.lm.arena.numel() < 0.35 * lm16.arena.numel()


@pytest.mark.parametrize("T", [1, 7, 40, 129])
def test_prefill_against_quantised_oracle(tiny4, T):
    ids = _ids(T, 512, 100 + T)
    h32, l32, h16, l16 = tiny4.refs(ids)
    tiny4.lm.reset()
    hid, logits = tiny4.lm.prefill(tiny4.lm.embed_tokens(ids))
    assert tiny4.lm.position == T
    assert _check(f"{tiny4.kind} prefill T={T}", hid, logits, h32[-1], l32[-1], rel_l2(h16[-1], h32[-1]), rel_l2(l16[-1], l32[-1]))


def test_decode_steps_teacher_forced(tiny4):
    ids = _ids(41, 512, 7)
    h32, l32, h16, l16 = tiny4.refs(ids)
    hid, logits = _prefill_then_decode(tiny4.lm, ids, 17)
    assert hid.shape[0] == 25 and tiny4.lm.position == 41
    eh, el = rel_l2(h16[16:], h32[16:]), rel_l2(l16[16:], l32[16:])
    oks = [_check(f"{tiny4.kind} decode step {i}", hid[i], logits[i], h32[16 + i], l32[16 + i], eh, el) for i in range(25)]
    assert all(oks)


def test_one_prefill_equals_prefill_plus_decodes_and_runs_are_bit_identical(tiny4):
    ids = _ids(41, 512, 8)
    h32, l32, h16, l16 = tiny4.refs(ids)
    eh, el = rel_l2(h16[-1], h32[-1]), rel_l2(l16[-1], l32[-1])
    tiny4.lm.reset()
    ph, pl = tiny4.lm.prefill(tiny4.lm.embed_tokens(ids))
    a_h, a_l = _prefill_then_decode(tiny4.lm, ids, 17)
    b_h, b_l = _prefill_then_decode(tiny4.lm, ids, 17)
    ok1 = _check(f"{tiny4.kind} 41 rows as one prefill", ph, pl, h32[-1], l32[-1], eh, el)
    ok2 = _check(f"{tiny4.kind} prefill(17) + 24 decodes", a_h[-1], a_l[-1], h32[-1], l32[-1], eh, el)
    assert ok1 and ok2
    assert torch.equal(a_h, b_h) and torch.equal(a_l, b_l)


@pytest.fixture(scope="module", params=KINDS)
def long4(request):
    """two layers and 2048 cached positions: rows past position 255, where the attention's loops over the keys take a second trip and more"""
    from instructany2pix_amd.config import tiny_llm
    cfg = tiny_llm()
    cfg.num_hidden_layers = 2
    return Bundle4(cfg, seed=22, kind=request.param, max_positions=2048)


@pytest.mark.parametrize("T", [257, 1025])
def test_prefill_past_256_positions_against_quantised_oracle(long4, T):
    ids = _ids(T, 512, 200 + T)
    h32, l32, h16, l16 = long4.refs(ids)
    long4.lm.reset()
    hid, logits = long4.lm.prefill(long4.lm.embed_tokens(ids))
    assert long4.lm.position == T
    assert _check(f"{long4.kind} 2 layers, prefill T={T}", hid, logits, h32[-1], l32[-1], rel_l2(h16[-1], h32[-1]), rel_l2(l16[-1], l32[-1]))


@pytest.mark.parametrize("n_prefill,steps", [(250, 10), (1020, 8)])
def test_decode_steps_across_a_256_position_boundary(long4, n_prefill, steps):
    """teacher-forced decode steps whose positions cross 256 (250 .. 259) and 1024 (1020 .. 1027)"""
    ids = _ids(n_prefill + steps, 512, 300 + n_prefill)
    h32, l32, h16, l16 = long4.refs(ids)
    hid, logits = _prefill_then_decode(long4.lm, ids, n_prefill)
    lo = n_prefill - 1
    assert hid.shape[0] == steps + 1 and long4.lm.position == n_prefill + steps
    eh, el = rel_l2(h16[lo:], h32[lo:]), rel_l2(l16[lo:], l32[lo:])
    oks = [_check(f"{long4.kind} 2 layers, position {lo + i}", hid[i], logits[i], h32[lo + i], l32[lo + i], eh, el) for i in range(steps + 1)]
    assert all(oks)


def test_loading_twice_gives_the_same_arena(tiny4):
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    other = HipInstructAny2PixLM(tiny4.cfg, DEV, max_positions=8, load_in_4bit=True, bnb_4bit_quant_type=tiny4.kind)
    other.load_state_dict(tiny4.sd)
    assert other.arena.numel() == tiny4.lm.arena.numel() and torch.equal(other.arena, tiny4.lm.arena)
    assert float(other.arena.float().abs().sum()) > 0


def test_the_flag_changes_the_model(tiny4):
    """the 4-bit engine is far from the UNQUANTISED oracle (it really computes from the 4-bit weights); the fp16 engine on the same checkpoint is not"""
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    ids = _ids(41, 512, 7)
    u32, u16 = make_oracle(tiny4.cfg, tiny4.sd)
    _, l32 = oracle_rows(u32, ids)
    _, l16 = oracle_rows(u16, ids)
    e_ref = rel_l2(l16[-1], l32[-1])
    tiny4.lm.reset()
    _, q_logits = tiny4.lm.prefill(tiny4.lm.embed_tokens(ids))
    lm16 = HipInstructAny2PixLM(tiny4.cfg, DEV, max_positions=64)
    lm16.load_state_dict(tiny4.sd)
    _, f_logits = lm16.prefill(lm16.embed_tokens(ids))
    dq, df = rel_l2(q_logits, l32[-1]), rel_l2(f_logits, l32[-1])
    print(f"[q4] {tiny4.kind} against the unquantised fp32 oracle, last-row logits: 4-bit engine {dq:.3e}, fp16 engine {df:.3e}, e_ref {e_ref:.3e}")
    assert dq > 20 * e_ref
    assert df <= 2 * e_ref


def test_video_replacement_with_quantised_projector(tiny4):
    lm, cfg = tiny4.lm, tiny4.cfg
    vid = lm.DEFAULT_VIDEO_TOKEN_IDX
    ids = _ids(20, 512, 12)
    ids[3], ids[9], ids[15] = vid, vid, vid
    g = torch.Generator().manual_seed(13)
    data = torch.randn(2, cfg.embed_dim, generator=g)
    data = data / data.norm(dim=-1, keepdim=True) * 20
    er = {"data": data, "mask": torch.zeros(2, dtype=torch.long)}
    W, bias = tiny4.sdq["model.vae_projector_image.weight"].float(), tiny4.sdq["model.vae_projector_image.bias"].float()
    assert not torch.equal(W, tiny4.sd["model.vae_projector_image.weight"].float())
    table = tiny4.sd["model.embed_tokens.weight"].float()
    want = _reference_inputs_embeds(table[ids][None], ids[None], vid, er, lambda x: x @ W.t() + bias)[0]
    got = lm.prepare_inputs_embeds(ids[None], er).float().cpu()
    tol = 2 * 2.0 ** -11 * float(want[[3, 9]].abs().max())           # two fp16 roundings: the projection's output, the sum
    err = float((got[[3, 9]] - want[[3, 9]]).abs().max())
    print(f"[q4] {tiny4.kind} <video> rows: max abs error {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    h32, l32, h16, l16 = tiny4.refs(embeds=want)
    lm.reset()
    hid, logits = lm.prefill(lm.prepare_inputs_embeds(ids[None], er))
    assert _check(f"{tiny4.kind} <video> replacement prefill", hid, logits, h32[-1], l32[-1], rel_l2(h16[-1], h32[-1]), rel_l2(l16[-1], l32[-1]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ptype", ["linear", "mlp2x_gelu"])
def test_quantised_heads(kind, ptype):
    """both heads with quantize_heads=True against F.linear with the dequantised weights; bound as tests/test_llm_gpu.py::test_mlp_gelu_heads
    (fp16 storage between the linears: 2^-11 per rounding, three of them)"""
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    from instructany2pix_amd.weights import llm_head_specs, synthetic_state_dict
    cfg = tiny_llm(vocab_size=64, mm_projector_type=ptype)
    cfg.num_hidden_layers = 1
    sd = synthetic_state_dict(llm_head_specs(cfg, cfg.embed_dim, ptype), seed=4)
    f = {k: v.float() for k, v in quantised_state_dict(sd, kind).items()}
    lm = HipInstructAny2PixLM(cfg, DEV, max_positions=8, load_in_4bit=True, bnb_4bit_quant_type=kind)
    lm.load_state_dict(sd, strict=False)
    plain = HipInstructAny2PixLM(cfg, DEV, max_positions=8, load_in_4bit=True, bnb_4bit_quant_type=kind, quantize_heads=False)
    plain.load_state_dict(sd, strict=False)
    F = torch.nn.functional

    def head(name, x):
        if ptype == "linear":
            return F.linear(x, f[name + ".weight"], f[name + ".bias"])
        return F.linear(F.gelu(F.linear(x, f[name + ".0.weight"], f[name + ".0.bias"])), f[name + ".2.weight"], f[name + ".2.bias"])

    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, cfg.embed_dim, generator=g).half()
    y = torch.randn(1, 1, 512, generator=g).half()
    for tag, fn, fn_plain, inp, name in (("projector", lm.vae_projector_image, plain.vae_projector_image, x, "model.vae_projector_image"),
                                         ("predictor", lm.vae_predictor_image, plain.vae_predictor_image, y.float().to(DEV), "model.vae_predictor_image")):
        want = head(name, inp.float().cpu())
        got, got_plain = fn(inp).cpu(), fn_plain(inp).cpu()
        e, e_plain = rel_l2(got, want), rel_l2(got_plain, want)
        print(f"[q4] {kind} {ptype} {tag}: rel-L2 {e:.3e} to the dequantised-weight head; the unquantised head is {e_plain:.3e} away")
        assert got.shape == want.shape and e < 2e-3
        assert e_plain > 2e-2                        # quantize_heads=False really keeps the fp16 weights
    with pytest.raises(ValueError, match="blocks of 64"):
        lm.load_state_dict({"model.vae_projector_image" + (".weight" if ptype == "linear" else ".0.weight"): torch.zeros(3, 10)}, strict=False)


def test_greedy_generate_against_teacher_forced_quantised_oracle(tiny4):
    lm = tiny4.lm
    prompt = _ids(12, 512, 14)[None]
    out = lm.generate(prompt, do_sample=False, max_new_tokens=32)
    assert out.sequences.shape == (1, 44) and len(out.hidden_states) == 32 and torch.equal(out.sequences[:, :12], prompt)
    h32, l32, h16, l16 = tiny4.refs(out.sequences[0, :-1])
    steps32, steps16 = l32[11:], l16[11:]
    delta = 2 * float((steps16 - steps32).abs().max())
    chosen = out.sequences[0, 12:]
    gap = steps32.max(dim=-1).values - steps32.gather(1, chosen[:, None])[:, 0]
    print(f"[q4] {tiny4.kind} greedy: delta {delta:.3e}, largest gap of a chosen token to the oracle's maximum {float(gap.max()):.3e}, "
          f"tokens equal to the oracle's argmax: {int((steps32.argmax(-1) == chosen).sum())}/32")
    assert gap.shape == (32,) and bool((gap <= delta).all())
    eh = rel_l2(h16[11:], h32[11:])
    got = torch.cat([out.hidden_states[i][-1][:, -1:].reshape(1, -1) for i in range(32)])
    assert all(rel_l2(got[i], h32[11 + i]) <= 2 * eh for i in range(32))


@pytest.mark.parametrize("kind", KINDS)
def test_full_width_two_layers(kind):
    """hidden 4096, 32 heads, intermediate 11008, vocabulary 32 003, 2 layers: prefill 33 + 8 decodes"""
    from instructany2pix_amd.config import vicuna_7b
    cfg = vicuna_7b(32003)
    cfg.num_hidden_layers = 2
    b = Bundle4(cfg, seed=33, kind=kind)
    ids = _ids(41, 32003, 15)
    h32, l32, h16, l16 = b.refs(ids)
    hid, logits = _prefill_then_decode(b.lm, ids, 33)
    assert hid.shape == (9, 4096) and logits.shape == (9, 32003)
    eh, el = rel_l2(h16[32:], h32[32:]), rel_l2(l16[32:], l32[32:])
    oks = [_check(f"{kind} full width row {32 + i}", hid[i], logits[i], h32[32 + i], l32[32 + i], eh, el) for i in range(9)]
    assert all(oks)


def test_pipeline_llm_only_end_to_end(tiny4):
    from stub_llm_tokenizer import StubLlamaTokenizer
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    tok = StubLlamaTokenizer(503)
    assert len(tok) == tiny4.cfg.vocab_size
    pipe = InstructAny2PixPipeline(unet=object(), llm=tiny4.lm, llm_tokenizer=tok)
    g = torch.Generator().manual_seed(5)
    mm = [{"type": "image", "fname": "fox.png", "embed": torch.randn(1024, generator=g)},
          {"type": "audio", "fname": "rain.wav", "embed": torch.randn(1024, generator=g)}]
    torch.manual_seed(17)
    a, b, caption = pipe("add <video> to <video> and turn the fox blue", mm, llm_only=True)
    assert a is None and b is None and isinstance(caption, str)
    assert isinstance(pipe.cache, tuple) and len(pipe.cache) == 5 and pipe.cache[2] == caption and tiny4.lm.position >= 1
