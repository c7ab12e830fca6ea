"""Host side of the batched LLM decode, no GPU: `generate_batch`'s bookkeeping against a stand-in for the engine calls, and the pure host
functions of the slot ABI on a context created without a device."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from instructany2pix_amd.llm import HipInstructAny2PixLM

VOCAB, HIDDEN = 16, 4


class StandIn(HipInstructAny2PixLM):
    """`prefill_slot` / `decode_batch` / `prepare_inputs_embeds` from a table: the token after t is (5 t + 3) % 16, its logit 40 above the rest
    (probability 1 after the temperature), the hidden row is the token id. No library call."""

    def __init__(self, max_batch, max_positions=64):
        self.config = SimpleNamespace(num_hidden_layers=2, hidden_size=HIDDEN, vocab_size=VOCAB)
        self.max_batch, self.max_positions, self.device = max_batch, max_positions, torch.device("cpu")
        self.calls, self.last = [], {}
        self._h = None

    def _row(self, token):
        logits = torch.zeros(VOCAB)
        logits[(5 * token + 3) % VOCAB] = 40.0
        return torch.full((HIDDEN,), float(token)), logits

    def prepare_inputs_embeds(self, input_ids, extra_replacement=None):
        self.calls.append(("embeds", input_ids.reshape(-1).tolist(), extra_replacement))
        return input_ids.reshape(-1, 1).float()

    def reset_slot(self, slot):
        self.calls.append(("reset", slot))

    def prefill_slot(self, slot, inputs_embeds):
        self.calls.append(("prefill", slot, inputs_embeds.shape[0]))
        return self._row(int(inputs_embeds[-1, 0]))

    def decode_batch(self, slots, token_ids):
        self.calls.append(("decode", list(slots), list(token_ids)))
        rows = [self._row(t) for t in token_ids]
        return torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])


def chain(t, n):
    out = []
    for _ in range(n):
        t = (5 * t + 3) % VOCAB
        out.append(t)
    return out


class StopAt:
    def __init__(self, total_len):
        self.total_len = total_len

    def __call__(self, ids, scores, **kw):
        assert ids.shape[0] == 1
        return ids.shape[1] >= self.total_len


@pytest.mark.parametrize("do_sample", [False, True])
def test_generate_batch_bookkeeping(do_sample, monkeypatch):
    lm = StandIn(max_batch=2)
    prompts = [torch.tensor([[1, 2, 4]]), torch.tensor([[1, 7]]), torch.tensor([[1, 9, 9, 9, 6]])]
    reps = [None, {"tag": "r1"}, None]
    draws = []
    real = torch.multinomial
    monkeypatch.setattr(torch, "multinomial", lambda p, num_samples, **kw: (draws.append(tuple(p.shape)), real(p, num_samples, **kw))[1])
    outs = lm.generate_batch(prompts, extra_replacements=reps, do_sample=do_sample, max_new_tokens=6,
                             stopping_criteria=[[StopAt(3 + 2)], None, [StopAt(5 + 4)]])
    # shapes and contents: request 0 stops after 2 new tokens, request 1 runs to max_new_tokens, request 2 (second group) stops after 4
    new = [2, 6, 4]
    for i, (o, p) in enumerate(zip(outs, prompts)):
        assert o.sequences.shape == (1, p.shape[1] + new[i]) and o.sequences.dtype == torch.long
        assert o.sequences[0, p.shape[1]:].tolist() == chain(int(p[0, -1]), new[i])
        assert len(o.hidden_states) == new[i] and len(o.hidden_states[0]) == 3
        rows = [h[-1][:, -1:] for h in o.hidden_states]
        assert all(r.shape == (1, 1, HIDDEN) for r in rows)
        assert [float(r[0, 0, 0]) for r in rows] == [float(t) for t in [int(p[0, -1])] + chain(int(p[0, -1]), new[i] - 1)]
    # groups of max_batch in order: requests 0 and 1 in slots 0 and 1, then request 2 in slot 0
    prefills = [c for c in lm.calls if c[0] in ("reset", "prefill", "embeds")]
    assert [c[:2] for c in prefills if c[0] != "embeds"] == [("reset", 0), ("prefill", 0), ("reset", 1), ("prefill", 1), ("reset", 0), ("prefill", 0)]
    assert [c[2] for c in prefills if c[0] == "embeds"] == reps
    order = [c[0] for c in lm.calls if c[0] in ("prefill", "decode")]
    assert order == ["prefill", "prefill"] + ["decode"] * 5 + ["prefill"] + ["decode"] * 3
    decodes = [c for c in lm.calls if c[0] == "decode"]
    c0, c1, c2 = chain(4, 6), chain(7, 6), chain(6, 4)
    assert decodes[0] == ("decode", [0, 1], [c0[0], c1[0]])                       # both requests
    assert decodes[1:5] == [("decode", [1], [c1[k]]) for k in range(1, 5)]        # request 0 has left: its slot is in no later call
    assert decodes[5:] == [("decode", [0], [c2[k]]) for k in range(3)]            # second group; no decode behind the last token
    # one draw of n_active rows per step
    assert draws == ([(2, VOCAB), (2, VOCAB)] + [(1, VOCAB)] * 4 + [(1, VOCAB)] * 4 if do_sample else [])


def test_generate_batch_refuses_bad_arguments():
    lm = StandIn(max_batch=2, max_positions=10)
    with pytest.raises(ValueError, match="one entry per request"):
        lm.generate_batch([torch.tensor([[1, 2]])], extra_replacements=[None, None])
    with pytest.raises(ValueError, match="one entry per request"):
        lm.generate_batch([torch.tensor([[1, 2]]), torch.tensor([[3]])], stopping_criteria=[None])
    with pytest.raises(ValueError, match="do not fit"):
        lm.generate_batch([torch.tensor([[1, 2]]), torch.tensor([[1, 2, 3, 4, 5]])], max_new_tokens=6)
    with pytest.raises(ValueError, match=r"\[1, tokens\]"):
        lm.generate_batch([torch.tensor([1, 2])], max_new_tokens=2)
    assert lm.calls == []                                                        # refused before any engine call
    assert lm.generate_batch([], max_new_tokens=2) == []


def test_forward_llm_batch_refuses_bad_arguments():
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    pipe = InstructAny2PixPipeline(unet=object(), llm=StandIn(max_batch=1), llm_tokenizer=object())
    with pytest.raises(ValueError, match="2 instructions for 1"):
        pipe.forward_llm_batch(["a", "b"], [[]])
    with pytest.raises(ValueError, match="max_batch=1"):
        pipe.forward_llm_batch(["a", "b"], [[], []])


# ---- pure host functions of the slot ABI ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from instructany2pix_amd import build, _ffi
    from instructany2pix_amd.config import tiny_llm
    build.build(verbose=False)
    lib = _ffi.lib()
    h = C.c_void_p()
    cfg = _ffi.make_llm_config(tiny_llm())
    _ffi.check(lib.ia2p_llm_create(C.byref(cfg), C.byref(h)), None, llm=True)
    yield lib, h
    lib.ia2p_llm_destroy(h)


def test_kv_slots_bytes(ctx):
    lib, h = ctx
    for P in (1, 64, 1024, 8192):
        one = lib.ia2p_llm_kv_bytes(h, P)
        assert one == 4 * 2 * P * 512 * 2 and lib.ia2p_llm_kv_slots_bytes(h, P, 1) == one
        assert [lib.ia2p_llm_kv_slots_bytes(h, P, n) for n in (2, 3, 8, 13)] == [n * one for n in (2, 3, 8, 13)]
    assert lib.ia2p_llm_kv_slots_bytes(h, 64, 0) == 0 and lib.ia2p_llm_kv_slots_bytes(h, 64, -1) == 0
    assert lib.ia2p_llm_kv_slots_bytes(h, 0, 2) == 0 and lib.ia2p_llm_kv_slots_bytes(h, 8193, 2) == 0
    assert lib.ia2p_llm_kv_slots_bytes(None, 64, 2) == 0
    assert lib.ia2p_llm_slots(h) == 0 and lib.ia2p_llm_slot_position(h, 0) == -1          # no cache bound
    assert lib.ia2p_llm_reset_slot(h, 0) == 1


def test_batch_workspace_bytes_is_monotone(ctx):
    lib, h = ctx
    w = {(T, n): lib.ia2p_llm_batch_workspace_bytes(h, T, n) for T in (0, 1, 7, 64, 200) for n in range(1, 9)}
    assert all(v > 0 for v in w.values())
    for T in (0, 1, 7, 64, 200):
        assert all(w[(T, n)] <= w[(T, n + 1)] for n in range(1, 8))
    for n in range(1, 9):
        assert w[(0, n)] <= w[(1, n)] <= w[(7, n)] <= w[(64, n)] <= w[(200, n)]
    assert w[(0, 1)] < w[(0, 8)] and w[(1, 1)] < w[(200, 1)]
    assert w[(64, 1)] >= lib.ia2p_llm_workspace_bytes(h, 64)
    for T, n in ((-1, 1), (4, 0), (4, 9)):
        assert lib.ia2p_llm_batch_workspace_bytes(h, T, n) == 0


def test_batch_workspace_serves_every_shorter_prefill():
    """a prefill's need is not monotone in its row count (9 rows need more than 10 at full width): the batch workspace covers every T up to max_T"""
    from instructany2pix_amd import build, _ffi
    from instructany2pix_amd.config import vicuna_7b
    build.build(verbose=False)
    lib = _ffi.lib()
    cfg = vicuna_7b(32003)
    cfg.num_hidden_layers = 2
    h, c = C.c_void_p(), _ffi.make_llm_config(cfg)
    _ffi.check(lib.ia2p_llm_create(C.byref(c), C.byref(h)), None, llm=True)
    try:
        need = [lib.ia2p_llm_workspace_bytes(h, T) for T in range(1, 41)]
        assert any(a > b for a, b in zip(need, need[1:]))                      # the premise
        for T_max in (10, 33, 40):
            assert lib.ia2p_llm_batch_workspace_bytes(h, T_max, 8) >= max(need[:T_max])
    finally:
        lib.ia2p_llm_destroy(h)
