"""Several sequences per weight pass: the multi-row GEMVs, `decode_batch` over cache slots, `generate_batch` and `forward_llm_batch`.

The yardstick is the single-sequence path (`ia2p_llm_gemv`, `ia2p_llm_gemv_q4`, `prefill` / `decode`, `generate`, `forward_llm`), whose agreement
with transformers tests/test_llm_gpu.py and tests/test_llm_q4_gpu.py pin. A row of a batched launch does the arithmetic of the single-row kernel on
that row, in the same order, so every comparison here is `torch.equal`: no tolerance."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_llm_gpu import _ids  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMATS = ["fp16", "fp4", "nf4"]
MS = (1, 2, 3, 5, 8)
OK, INVALID, SHAPE, STATE, NOMEM = 0, 1, 2, 4, 5


def _lib():
    from instructany2pix_amd import _ffi
    return _ffi, _ffi.lib()


def _cb(kind):
    from instructany2pix_amd.config import BNB_4BIT_CODEBOOKS
    return (C.c_float * 16)(*BNB_4BIT_CODEBOOKS[kind])


def _rows(K, seed):
    """8 input rows of differing scales (a row taken for another cannot pass)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(8, K, generator=g) * torch.tensor([1.0, 0.25, 3.0, 0.5, 7.0, 0.125, 2.0, 11.0])[:, None]).to(DEV).contiguous()


def _weights(N, K, seed):
    return (torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) * K ** -0.5).half().to(DEV)


# ---- the multi-row GEMVs per operation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(520, 512), (2816, 512), (512, 1408), (517, 512), (8200, 512)])
def test_gemv_rows_equal_single_row_calls(shape):
    ffi, lib = _lib()
    N, K = shape
    w, x, s = _weights(N, K, 11 + N), _rows(K, K + N), ffi.current_stream()
    single = torch.full((8, N), float("nan"), device=DEV)
    for m in range(8):
        ffi.check(lib.ia2p_llm_gemv(s, ffi.ptr(w), ffi.ptr(x[m]), ffi.ptr(single[m]), N, K), None, llm=True)
    for M in MS:
        out = torch.full((M, N), float("nan"), device=DEV)
        ffi.check(lib.ia2p_llm_gemv_rows(s, ffi.ptr(w), ffi.ptr(x), ffi.ptr(out), N, K, M), None, llm=True)
        torch.cuda.synchronize()
        bad = [m for m in range(M) if not torch.equal(out[m], single[m])]
        assert not bad, f"fp16 {N} x {K}, M = {M}: rows {bad} differ from the single-row call"


@pytest.mark.parametrize("kind", ["fp4", "nf4"])
@pytest.mark.parametrize("shape", [(520, 512), (2816, 512), (512, 1408), (517, 512), (520, 11008), (520, 14336)])
def test_gemv_q4_rows_equal_single_row_calls(kind, shape):
    ffi, lib = _lib()
    N, K = shape
    w, x, s, cb = _weights(N, K, 13 + N), _rows(K, K + N + 1), ffi.current_stream(), _cb(kind)
    packed = torch.empty(lib.ia2p_llm_q4_packed_bytes(N, K), dtype=torch.uint8, device=DEV)
    absmax = torch.empty(N * K // 64, dtype=torch.float32, device=DEV)
    ffi.check(lib.ia2p_llm_quantize_q4(s, ffi.ptr(w), N, K, cb, ffi.ptr(packed), ffi.ptr(absmax)), None, llm=True)
    single = torch.full((8, N), float("nan"), device=DEV)
    for m in range(8):
        ffi.check(lib.ia2p_llm_gemv_q4(s, ffi.ptr(packed), ffi.ptr(absmax), cb, ffi.ptr(x[m]), ffi.ptr(single[m]), N, K), None, llm=True)
    for M in MS:
        out = torch.full((M, N), float("nan"), device=DEV)
        ffi.check(lib.ia2p_llm_gemv_q4_rows(s, ffi.ptr(packed), ffi.ptr(absmax), cb, ffi.ptr(x), ffi.ptr(out), N, K, M), None, llm=True)
        torch.cuda.synchronize()
        bad = [m for m in range(M) if not torch.equal(out[m], single[m])]
        assert not bad, f"{kind} {N} x {K}, M = {M}: rows {bad} differ from the single-row call"


def test_gemv_rows_refuse_what_the_single_row_calls_refuse():
    ffi, lib = _lib()
    s, cb = ffi.current_stream(), _cb("fp4")
    w, x, out = _weights(64, 128, 1), _rows(128, 2), torch.zeros(8, 64, device=DEV)
    packed = torch.zeros(lib.ia2p_llm_q4_packed_bytes(64, 128), dtype=torch.uint8, device=DEV)
    absmax = torch.ones(64 * 128 // 64, dtype=torch.float32, device=DEV)
    bad_k = lib.ia2p_llm_gemv(s, ffi.ptr(w), ffi.ptr(x), ffi.ptr(out), 64, 12)
    bad_k4 = lib.ia2p_llm_gemv_q4(s, ffi.ptr(packed), ffi.ptr(absmax), cb, ffi.ptr(x), ffi.ptr(out), 64, 96)
    assert bad_k in (SHAPE, INVALID) and bad_k4 in (SHAPE, INVALID)
    for N, K, M in ((64, 128, 0), (64, 128, 9), (64, 12, 2)):
        assert lib.ia2p_llm_gemv_rows(s, ffi.ptr(w), ffi.ptr(x), ffi.ptr(out), N, K, M) == bad_k, (N, K, M)
    for N, K, M in ((64, 128, 0), (64, 128, 9), (64, 96, 2), (64, 14400, 2)):
        assert lib.ia2p_llm_gemv_q4_rows(s, ffi.ptr(packed), ffi.ptr(absmax), cb, ffi.ptr(x), ffi.ptr(out), N, K, M) == bad_k4, (N, K, M)
    assert lib.ia2p_llm_gemv_rows(s, ffi.ptr(w), ffi.ptr(x), ffi.ptr(out), 64, 128, 8) == OK
    torch.cuda.synchronize()


# ---- decode_batch on the tiny model ---------------------------------------------------------------------------------------------
PROMPTS, SLOTS, N_DECODE = (5, 12, 33), (5, 0, 2), 10


def _make(cfg, sd, fmt, max_positions, max_batch):
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    kw = {} if fmt == "fp16" else dict(load_in_4bit=True, bnb_4bit_quant_type=fmt)
    lm = HipInstructAny2PixLM(cfg, DEV, max_positions=max_positions, video_token_id=cfg.vocab_size - 3, max_batch=max_batch, **kw)
    lm.load_state_dict(sd)
    return lm


def _serial(lm, ids, n_prefill):
    """the stream alone on the single-sequence path -> (hidden rows, logits rows): row 0 the prefill's, row 1 + i decode step i"""
    lm.reset()
    rows = [lm.prefill(lm.embed_tokens(ids[:n_prefill]))]
    rows += [lm.decode(t) for t in ids[n_prefill:].tolist()]
    return torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])


class Tiny:
    def __init__(self, fmt):
        from instructany2pix_amd.config import tiny_llm
        from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
        self.cfg = tiny_llm()
        self.sd = synthetic_state_dict(llm_param_specs(self.cfg, self.cfg.embed_dim, "linear"), seed=21)
        self.one = _make(self.cfg, self.sd, fmt, 64, 1)          # the yardstick: one slot
        self.lm = _make(self.cfg, self.sd, fmt, 64, 6)
        self.ids = [_ids(T + N_DECODE, 512, 40 + T) for T in PROMPTS]
        self.ref = [_serial(self.one, ids, T) for ids, T in zip(self.ids, PROMPTS)]      # computed once, read by every test

    def prefill_all(self):
        for j, (slot, T) in enumerate(zip(SLOTS, PROMPTS)):
            self.lm.reset_slot(slot)
            hid, logits = self.lm.prefill_slot(slot, self.lm.embed_tokens(self.ids[j][:T]))
            assert torch.equal(hid, self.ref[j][0][0]) and torch.equal(logits, self.ref[j][1][0]), f"prefill_slot({slot}) differs from prefill"

    def step(self, streams, step):
        """decode step `step` of the given streams in one call; every row against its yardstick"""
        slots = [SLOTS[j] for j in streams]
        hid, logits = self.lm.decode_batch(slots, [int(self.ids[j][PROMPTS[j] + step]) for j in streams])
        assert hid.shape == (len(streams), 512) and logits.shape == (len(streams), 512)
        for r, j in enumerate(streams):
            assert torch.equal(hid[r], self.ref[j][0][1 + step]), f"step {step}, slot {slots[r]}: hidden row differs"
            assert torch.equal(logits[r], self.ref[j][1][1 + step]), f"step {step}, slot {slots[r]}: logits row differ"


@pytest.fixture(scope="module", params=FORMATS)
def tiny(request):
    return Tiny(request.param)


def test_decode_batch_equals_each_stream_alone(tiny):
    lm = tiny.lm
    assert lm._lib.ia2p_llm_slots(lm._h) == 6
    tiny.prefill_all()
    for step in range(N_DECODE):
        tiny.step([0, 1, 2], step)
        assert [lm.slot_position(s) for s in range(6)] == [12 + step + 1, 0, 33 + step + 1, 0, 0, 5 + step + 1]
    assert lm.position == lm.slot_position(0)


def test_decode_batch_with_a_shrinking_and_a_permuted_row_set(tiny):
    tiny.prefill_all()
    for step in range(4):
        tiny.step([0, 1, 2], step)
    for step in range(4, 8):                 # the middle stream (slot 0) has left: slots [5, 2]
        tiny.step([0, 2], step)
    tiny.step([2, 0], 8)                     # slots [2, 5]
    assert [tiny.lm.slot_position(s) for s in (5, 0, 2)] == [5 + 9, 12 + 4, 33 + 9]


def test_prefill_slot_does_not_disturb_its_neighbours(tiny):
    lm = tiny.lm
    for slot, j in ((0, 0), (1, 1)):
        lm.reset_slot(slot)
        lm.prefill_slot(slot, lm.embed_tokens(tiny.ids[j][:PROMPTS[j]]))
    for step in range(3):
        lm.decode_batch([0, 1], [int(tiny.ids[0][5 + step]), int(tiny.ids[1][12 + step])])
    lm.reset_slot(1)
    lm.prefill_slot(1, lm.embed_tokens(tiny.ids[2][:33]))
    hid, logits = lm.decode_batch([0], [int(tiny.ids[0][5 + 3])])
    assert torch.equal(hid[0], tiny.ref[0][0][4]) and torch.equal(logits[0], tiny.ref[0][1][4])
    assert lm.slot_position(0) == 9 and lm.slot_position(1) == 33


def test_one_row_batches_and_single_decodes_continue_a_batched_stream(tiny):
    """one decode driver serves `decode` and `decode_batch`: a batch of one row on a slot other than 0 is the serial stream, and after a step
    at n = 3 `decode` (slot 0) continues its stream where the batch left it, and the other way round"""
    lm = tiny.lm
    tiny.prefill_all()                       # streams 0, 1, 2 live in slots 5, 0, 2

    def alone(step):
        tiny.step([0], step)                 # n = 1, slot 5
        hid, logits = lm.decode(int(tiny.ids[1][PROMPTS[1] + step]))          # the single-sequence entry point: slot 0
        assert torch.equal(hid, tiny.ref[1][0][1 + step]) and torch.equal(logits, tiny.ref[1][1][1 + step]), f"step {step}: decode after a batch differs"
        tiny.step([2], step)                 # n = 1, slot 2

    alone(0)
    tiny.step([0, 1, 2], 1)
    alone(2)
    tiny.step([0, 1, 2], 3)
    alone(4)
    assert [lm.slot_position(s) for s in (5, 0, 2)] == [5 + 5, 12 + 5, 33 + 5] and lm.position == 12 + 5


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_batched_step_past_256_positions(fmt):
    """two layers, 2048 cached positions, four slots whose streams stand at positions 255, 256, 257 and 1024: one step at n = 4 against each stream alone
    (slot 0 of the same model on the single-sequence path)"""
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
    cfg = tiny_llm()
    cfg.num_hidden_layers = 2
    lm = _make(cfg, synthetic_state_dict(llm_param_specs(cfg, cfg.embed_dim, "linear"), seed=22), fmt, 2048, 4)
    at = (255, 256, 257, 1024)
    ids = [_ids(T + 1, 512, 70 + T) for T in at]
    ref = [_serial(lm, ids[j], T) for j, T in enumerate(at)]
    for j, T in enumerate(at):
        lm.reset_slot(j)
        hid, logits = lm.prefill_slot(j, lm.embed_tokens(ids[j][:T]))
        assert torch.equal(hid, ref[j][0][0]) and torch.equal(logits, ref[j][1][0])
    assert [lm.slot_position(j) for j in range(4)] == list(at)
    hid, logits = lm.decode_batch([0, 1, 2, 3], [int(ids[j][T]) for j, T in enumerate(at)])
    for j, T in enumerate(at):
        assert torch.equal(hid[j], ref[j][0][1]), f"{fmt} position {T}: hidden row differs"
        assert torch.equal(logits[j], ref[j][1][1]), f"{fmt} position {T}: logits row differ"
    assert [lm.slot_position(j) for j in range(4)] == [T + 1 for T in at]


# ---- full width -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16", "fp4"])
def test_full_width_eight_rows(fmt):
    """hidden 4096, 32 heads, intermediate 11008, vocabulary 32 003, 2 layers, 8 slots: prompts of 3..10 rows, 4 steps at n = 8 against 8 serial
    runs (slot 0 of the same model on the single-sequence path)"""
    from instructany2pix_amd.config import vicuna_7b
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    from instructany2pix_amd.weights import iter_synthetic, llm_param_specs
    cfg = vicuna_7b(32003)
    cfg.num_hidden_layers = 2
    kw = {} if fmt == "fp16" else dict(load_in_4bit=True, bnb_4bit_quant_type=fmt)
    lm = HipInstructAny2PixLM(cfg, DEV, max_positions=16, max_batch=8, **kw)
    lm.load_state_dict(iter_synthetic(llm_param_specs(cfg), 7, DEV, torch.float16))
    ids = [_ids(3 + j + 4, 32003, 60 + j) for j in range(8)]
    ref = [_serial(lm, ids[j], 3 + j) for j in range(8)]
    for j in range(8):
        lm.reset_slot(j)
        hid, logits = lm.prefill_slot(j, lm.embed_tokens(ids[j][:3 + j]))
        assert torch.equal(hid, ref[j][0][0]) and torch.equal(logits, ref[j][1][0])
    for step in range(4):
        hid, logits = lm.decode_batch(list(range(8)), [int(ids[j][3 + j + step]) for j in range(8)])
        assert hid.shape == (8, 4096) and logits.shape == (8, 32003)
        for j in range(8):
            assert torch.equal(hid[j], ref[j][0][1 + step]), f"{fmt} step {step} row {j}: hidden row differs"
            assert torch.equal(logits[j], ref[j][1][1 + step]), f"{fmt} step {step} row {j}: logits row differ"
    assert [lm.slot_position(j) for j in range(8)] == [3 + j + 4 for j in range(8)]


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_decode_batch_errors_change_no_position():
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
    ffi, lib = _lib()
    cfg = tiny_llm()
    lm = _make(cfg, synthetic_state_dict(llm_param_specs(cfg, cfg.embed_dim, "linear"), seed=21), "fp16", 64, 6)
    lm.prefill_slot(0, lm.embed_tokens(_ids(4, 512, 1)))
    lm.prefill_slot(1, lm.embed_tokens(_ids(7, 512, 2)))
    lm.prefill_slot(4, lm.embed_tokens(_ids(64, 512, 3)))          # slot 4 is full
    want = [4, 7, 0, 0, 64, 0]
    ws = lm._workspace(64)
    hid, logits = torch.empty(8, 512, device=DEV), torch.empty(8, 512, device=DEV)
    need2 = lib.ia2p_llm_batch_workspace_bytes(lm._h, 0, 2)
    assert 0 < need2 <= ws.numel() and ws.data_ptr() % 256 == 0

    def call(slots, tokens, n=None, ws_bytes=None):
        arr = C.c_int32 * max(len(slots), 1)
        return lib.ia2p_llm_decode_batch(lm._h, ffi.current_stream(), arr(*slots), arr(*tokens), len(slots) if n is None else n, ffi.ptr(hid),
                                         ffi.ptr(logits), ffi.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes)

    cases = [("a duplicate slot", lambda: call([0, 1, 0], [5, 5, 5]), INVALID, b"twice"),
             ("a slot out of range", lambda: call([0, 6], [5, 5]), INVALID, b"slot 6"),
             ("n = 0", lambda: call([0], [5], n=0), INVALID, b"0 rows"),
             ("n = 9", lambda: call(list(range(9)), [5] * 9), INVALID, b"9 rows"),
             ("a slot never prefilled", lambda: call([0, 3], [5, 5]), STATE, b"slot 3 before a prefill"),
             ("a token outside the vocabulary", lambda: call([0, 1], [5, 512]), SHAPE, b"token 512"),
             ("a slot at max_positions", lambda: call([0, 4], [5, 5]), SHAPE, b"past the cache"),
             ("a workspace one byte short", lambda: call([0, 1], [5, 5], ws_bytes=need2 - 1), NOMEM, b"workspace")]
    for what, fn, status, text in cases:
        got = fn()
        msg = lib.ia2p_llm_last_error(lm._h)
        assert got == status, f"{what}: status {got}, expected {status} ({msg})"
        assert text in msg, f"{what}: {msg}"
        assert [lm.slot_position(s) for s in range(6)] == want, what
    assert call([0, 1], [5, 5], ws_bytes=need2) == OK           # the size the library asks for is enough
    torch.cuda.synchronize()
    assert [lm.slot_position(s) for s in range(6)] == [5, 8, 0, 0, 64, 0]
    with pytest.raises(ValueError):
        lm.reset_slot(6)
    assert lm.slot_position(6) == -1


# ---- generate_batch -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    """tiny model with two slots (a third request makes a second group) and the stub tokenizer; slot 0 on the single-sequence path is the yardstick"""
    from stub_llm_tokenizer import StubLlamaTokenizer
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
    cfg = tiny_llm()
    sd = synthetic_state_dict(llm_param_specs(cfg, cfg.embed_dim, "linear"), seed=21)
    return _make(cfg, sd, "fp16", 256, 2), StubLlamaTokenizer(503)


def _same_output(a, b):
    return torch.equal(a.sequences, b.sequences) and len(a.hidden_states) == len(b.hidden_states) and all(
        torch.equal(x[-1][:, -1:], y[-1][:, -1:]) for x, y in zip(a.hidden_states, b.hidden_states))


def test_generate_batch_greedy_is_the_serial_result(pair):
    from instructany2pix_amd.llm import KeywordsStoppingCriteria
    lm, tok = pair
    prompts = [_ids(T, 503, 80 + T)[None] for T in (7, 12, 20)]
    serial = [lm.generate(p, do_sample=False, max_new_tokens=24) for p in prompts]
    outs = lm.generate_batch(prompts, do_sample=False, max_new_tokens=24)
    assert len(outs) == 3
    for i, (o, s) in enumerate(zip(outs, serial)):
        assert o.sequences.shape == (1, prompts[i].shape[1] + 24) and len(o.hidden_states) == 24
        assert o.hidden_states[0][-1][:, -1:].shape == (1, 1, 512)
        assert _same_output(o, s), f"request {i} differs from generate(do_sample=False)"
    # request 1 once more with a keyword that the serial run produces among its first new tokens: it ends there, the others run on
    words = [tok.batch_decode(serial[1].sequences[:, 12 + k:12 + k + 1], skip_special_tokens=True)[0] for k in range(2, 12)]
    k, word = next((2 + i, w) for i, w in enumerate(words) if w)
    crit = lambda: [KeywordsStoppingCriteria([word], tok, prompts[1])]      # noqa: E731
    early = lm.generate(prompts[1], do_sample=False, max_new_tokens=24, stopping_criteria=crit())
    assert early.sequences.shape[1] <= 12 + k + 1 < 12 + 24
    outs = lm.generate_batch(prompts, do_sample=False, max_new_tokens=24, stopping_criteria=[None, crit(), None])
    assert _same_output(outs[1], early) and _same_output(outs[0], serial[0]) and _same_output(outs[2], serial[2])


def test_generate_batch_sampling_is_reproducible_for_a_seed(pair):
    lm, _ = pair
    prompts = [_ids(T, 503, 90 + T)[None] for T in (6, 9, 15)]
    torch.manual_seed(17)
    a = lm.generate_batch(prompts, do_sample=True, temperature=0.3, max_new_tokens=8)
    torch.manual_seed(17)
    b = lm.generate_batch(prompts, do_sample=True, temperature=0.3, max_new_tokens=8)
    assert all(torch.equal(x.sequences, y.sequences) for x, y in zip(a, b))
    assert [x.sequences.shape for x in a] == [(1, 14), (1, 17), (1, 23)]


def _same_tuple(a, b):
    def same(x, y):
        if isinstance(x, torch.Tensor):
            return isinstance(y, torch.Tensor) and torch.equal(x, y)
        if isinstance(x, dict):
            return isinstance(y, dict) and x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        return x == y
    return len(a) == len(b) == 5 and all(same(x, y) for x, y in zip(a, b))


def test_forward_llm_batch_equals_forward_llm_per_request(pair, monkeypatch):
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    lm, tok = pair
    gen, gen_batch = lm.generate, lm.generate_batch
    monkeypatch.setattr(lm, "generate", lambda *a, **kw: gen(*a, **{**kw, "do_sample": False}), raising=False)
    monkeypatch.setattr(lm, "generate_batch", lambda *a, **kw: gen_batch(*a, **{**kw, "do_sample": False}), raising=False)
    pipe = InstructAny2PixPipeline(unet=object(), llm=lm, llm_tokenizer=tok)
    g = torch.Generator().manual_seed(5)
    mm1 = [{"type": "image", "fname": "fox.png", "embed": torch.randn(1024, generator=g)}]
    mm2 = [{"type": "image", "fname": "owl.png", "embed": torch.randn(1024, generator=g)},
           {"type": "audio", "fname": "rain.wav", "embed": torch.randn(1024, generator=g)}]
    insts = ["turn the fox in <video> blue", "add <video> to <video> and make it night"]
    got = pipe.forward_llm_batch(insts, [mm1, mm2])
    assert isinstance(got, list) and len(got) == 2 and all(isinstance(t, tuple) and len(t) == 5 for t in got)
    assert pipe.cache is None
    for inst, mm, t in zip(insts, (mm1, mm2), got):
        assert _same_tuple(t, pipe.forward_llm(inst, mm)), inst
    with pytest.raises(ValueError):
        pipe.forward_llm_batch(insts, [mm1])
