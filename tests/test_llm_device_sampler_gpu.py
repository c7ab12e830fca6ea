"""The device sampler in the LLM's host loop: `decode_batch_dev` (ids read from device memory), `generate` / `generate_batch` under `sampler="device"`.

Tiny LLaMA configuration with eight cache slots, fp16 and 4-bit weights. Every comparison is `torch.equal`: a decode row depends on its id and its slot only
(tests/test_llm_batch_gpu.py pins a batched row against the single-sequence step), and a draw on its logits row, its seed and its step only, so a request must
get the same tokens and hidden rows alone, in a batch, and in a loop driven by hand."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_llm_gpu import _ids  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMATS = ["fp16", "fp4"]
PROMPTS = (5, 12, 33, 7, 9, 20, 3, 16)          # prompt lengths of the eight slots
SEEDS = [11, 2 ** 63 + 5, 0xDEADBEEFCAFE, 7, 2 ** 40 + 3]


class Tiny:
    def __init__(self, fmt):
        from instructany2pix_amd.config import tiny_llm
        self.cfg, self.fmt = tiny_llm(), fmt
        self.lm = self.make(8)
        self.ids = [_ids(T, 503, 40 + T) for T in PROMPTS]
        self.prompts = [ids[None] for ids in self.ids]

    def make(self, max_batch):
        from instructany2pix_amd.llm import HipInstructAny2PixLM
        from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
        kw = {} if self.fmt == "fp16" else dict(load_in_4bit=True, bnb_4bit_quant_type=self.fmt)
        lm = HipInstructAny2PixLM(self.cfg, DEV, max_positions=64, video_token_id=self.cfg.vocab_size - 3, max_batch=max_batch, **kw)
        lm.load_state_dict(synthetic_state_dict(llm_param_specs(self.cfg, self.cfg.embed_dim, "linear"), seed=21))
        return lm

    def prefill_all(self):
        for slot, ids in enumerate(self.ids):
            self.lm.reset_slot(slot)
            self.lm.prefill_slot(slot, self.lm.embed_tokens(ids))


@pytest.fixture(scope="module", params=FORMATS)
def tiny(request):
    return Tiny(request.param)


def _same_output(a, b):
    return torch.equal(a.sequences, b.sequences) and len(a.hidden_states) == len(b.hidden_states) and all(
        torch.equal(x[-1][:, -1:], y[-1][:, -1:]) for x, y in zip(a.hidden_states, b.hidden_states))


@pytest.mark.parametrize("n", [1, 3, 8])
def test_decode_from_device_tokens_equals_decode_from_host_tokens(tiny, n):
    lm = tiny.lm
    slots = [5, 0, 2, 7, 1, 3, 6, 4][:n]
    ids = [int(t) for t in _ids(n, 503, 900 + n)]
    perm = torch.randperm(n + 2, generator=torch.Generator().manual_seed(n))[:n].tolist()          # where row r's id lies in the device buffer
    buf = torch.full((n + 2,), 499, dtype=torch.int32)
    for r in range(n):
        buf[perm[r]] = ids[r]
    tiny.prefill_all()
    want_h, want_l = lm.decode_batch(slots, ids)
    want_h2, want_l2 = lm.decode_batch(slots, ids[::-1])                                              # a second step, so positions matter
    tiny.prefill_all()
    dev = buf.to(DEV)
    got_h, got_l = lm.decode_batch_dev(slots, dev, perm)
    assert [lm.slot_position(s) for s in slots] == [PROMPTS[s] + 1 for s in slots]
    assert torch.equal(got_h, want_h) and torch.equal(got_l, want_l), "rows decoded from device ids differ from the rows decoded from the same host ids"
    ordered = torch.tensor(ids[::-1], dtype=torch.int32, device=DEV)
    got_h2, got_l2 = lm.decode_batch_dev(slots, ordered)                                              # token_index = None: 0 .. n-1
    assert torch.equal(got_h2, want_h2) and torch.equal(got_l2, want_l2)


def test_an_id_outside_the_vocabulary_is_clamped_by_the_kernel(tiny):
    """the sampler writes -1 for a row it cannot sample, and the look-ahead decode runs before the host has seen it: the row embeds table row 0"""
    lm, V = tiny.lm, tiny.cfg.vocab_size
    tiny.prefill_all()
    want = lm.decode_batch([0, 1, 2], [0, V - 1, 17])
    tiny.prefill_all()
    got = lm.decode_batch_dev([0, 1, 2], torch.tensor([-1, V + 5, 17], dtype=torch.int32, device=DEV))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError):
        lm.decode_batch_dev([0, 1], torch.zeros(2, dtype=torch.int32, device=DEV), [0, -1])
    with pytest.raises(ValueError):
        lm.decode_batch_dev([0, 0], torch.zeros(2, dtype=torch.int32, device=DEV))
    assert lm.slot_position(0) == PROMPTS[0] + 1


def test_greedy_is_the_host_sampler_result(tiny):
    lm = tiny.lm
    prompts = tiny.prompts[:3]
    host = [lm.generate(p, do_sample=False, max_new_tokens=12, sampler="host") for p in prompts]
    for p, h in zip(prompts, host):
        d = lm.generate(p, do_sample=False, max_new_tokens=12, sampler="device")
        assert d.sequences.shape == (1, p.shape[1] + 12) and len(d.hidden_states) == 12 and d.hidden_states[0][-1][:, -1:].shape == (1, 1, 512)
        assert _same_output(d, h), "generate(sampler='device', do_sample=False) differs from the host sampler"
    outs = lm.generate_batch(prompts, do_sample=False, max_new_tokens=12, sampler="device")
    hosts = lm.generate_batch(prompts, do_sample=False, max_new_tokens=12, sampler="host")
    assert all(_same_output(o, h) for o, h in zip(outs, host)) and all(_same_output(o, h) for o, h in zip(hosts, host))


class _StopAt:
    """a stopping criterion on the request's own sequence: done once `token` has been generated"""

    def __init__(self, token, start):
        self.token, self.start = token, start

    def __call__(self, seq, scores, **kw):
        return bool((seq[0, self.start:] == self.token).any())


def test_a_batch_gives_every_request_its_serial_tokens(tiny):
    lm = tiny.lm
    prompts = tiny.prompts[:5]                       # 5, 12, 33, 7 and 9 prompt tokens
    kw = dict(do_sample=True, temperature=1.0, top_k=50, max_new_tokens=10, sampler="device")
    free = lm.generate(prompts[1], seed=SEEDS[1], **kw)
    stop = _StopAt(int(free.sequences[0, 12 + 3]), 12)          # request 1 ends at its 4th new token at the latest, the others run on
    serial = [lm.generate(p, seed=s, stopping_criteria=[stop] if i == 1 else None, **kw) for i, (p, s) in enumerate(zip(prompts, SEEDS))]
    assert serial[1].sequences.shape[1] <= 12 + 4 and torch.equal(serial[1].sequences, free.sequences[:, :serial[1].sequences.shape[1]])
    assert len({tuple(s.sequences[0, -10:].tolist()) for i, s in enumerate(serial) if i != 1}) == 4          # different seeds, different streams
    outs = lm.generate_batch(prompts, seeds=SEEDS, stopping_criteria=[None, [stop], None, None, None], **kw)
    for i, (o, s) in enumerate(zip(outs, serial)):
        assert o.sequences.shape[1] == s.sequences.shape[1] == (prompts[i].shape[1] + 10 if i != 1 else serial[1].sequences.shape[1])
        assert len(o.hidden_states) == o.sequences.shape[1] - prompts[i].shape[1]
        assert _same_output(o, s), f"request {i} in a batch of five differs from generate(seed={SEEDS[i]})"
    # a batch of two out of the five
    two = lm.generate_batch(prompts[:2], seeds=SEEDS[:2], stopping_criteria=[None, [stop]], **kw)
    assert _same_output(two[0], serial[0]) and _same_output(two[1], serial[1])
    # two slots instead of eight: the five requests run in groups of 2, 2 and 1 (slots reused, the step counter restarting with every group), an iterator for seeds
    small = tiny.make(2)
    outs = small.generate_batch(prompts, seeds=iter(SEEDS), stopping_criteria=[None, [stop], None, None, None], **kw)
    for i, (o, s) in enumerate(zip(outs, serial)):
        assert _same_output(o, s), f"request {i} in groups of two differs from generate(seed={SEEDS[i]})"
    greedy = small.generate_batch(prompts, do_sample=False, max_new_tokens=6, sampler="device")
    assert all(_same_output(o, lm.generate(p, do_sample=False, max_new_tokens=6, sampler="host")) for o, p in zip(greedy, prompts))


def test_generate_equals_a_loop_driven_by_hand(tiny):
    """prefill -> ia2p_sample_tokens -> decode, the id read by the host after every draw"""
    from instructany2pix_amd import _ffi
    lm, lib = tiny.lm, tiny.lm._lib
    prompt, seed, new = tiny.prompts[4], 0x1234567890ABCDEF, 9
    out = lm.generate(prompt, do_sample=True, temperature=0.7, top_k=20, max_new_tokens=new, sampler="device", seed=seed)
    lm.reset()
    hid, logits = lm.prefill(lm.embed_tokens(prompt.reshape(-1)))
    tok = torch.zeros(1, dtype=torch.int32, device=DEV)
    seq, rows = prompt.reshape(-1).tolist(), []
    for step in range(new):
        rows.append(hid)
        _ffi.check(lib.ia2p_sample_tokens(_ffi.current_stream(), _ffi.ptr(logits), logits.numel(), 1, logits.numel(), 0.7, 20, 1, (C.c_uint64 * 1)(seed),
                                          (C.c_uint32 * 1)(step), _ffi.ptr(tok), None, None), None, llm=True)
        seq.append(int(tok.item()))
        if step + 1 < new:
            hid, logits = lm.decode(seq[-1])
    assert out.sequences[0].tolist() == seq
    assert all(torch.equal(h[-1][:, -1:].reshape(-1), r) for h, r in zip(out.hidden_states, rows))


def test_seeds_come_from_the_global_generator_when_none_are_given(tiny):
    lm, kw = tiny.lm, dict(do_sample=True, temperature=1.0, max_new_tokens=6, sampler="device")
    torch.manual_seed(3)
    a = lm.generate_batch(tiny.prompts[:3], **kw)
    torch.manual_seed(3)
    b = lm.generate_batch(tiny.prompts[:3], **kw)
    torch.manual_seed(3)
    seeds = [int(torch.randint(0, 2 ** 63 - 1, (1,)).item()) for _ in range(3)]
    c = lm.generate_batch(tiny.prompts[:3], seeds=seeds, **kw)
    assert all(_same_output(x, y) for x, y in zip(a, b)) and all(_same_output(x, y) for x, y in zip(a, c))


def test_a_row_without_a_token_raises_and_names_the_request(tiny, monkeypatch):
    lm = tiny.lm
    draw = lm.sample_tokens

    def spoiled(logits, *a, **kw):
        logits[1, 3] = float("nan")                # request 1's logits row
        return draw(logits, *a, **kw)

    monkeypatch.setattr(lm, "sample_tokens", spoiled, raising=False)
    with pytest.raises(RuntimeError, match="request 1"):
        lm.generate_batch(tiny.prompts[:3], do_sample=True, max_new_tokens=4, sampler="device", seeds=[1, 2, 3])
    torch.cuda.synchronize()


def test_the_host_sampler_is_what_it_was(tiny):
    """`sampler="host"` against the loop it has always been, driven by hand with `sample_next` / one `torch.multinomial` per step on the global RNG"""
    from instructany2pix_amd.llm import sample_next, sample_probs
    lm = tiny.lm
    prompt, new = tiny.prompts[0], 8
    torch.manual_seed(0)
    out = lm.generate(prompt, do_sample=True, temperature=0.3, max_new_tokens=new, sampler="host")
    torch.manual_seed(0)
    lm.reset()
    hid, logits = lm.prefill(lm.embed_tokens(prompt.reshape(-1)))
    seq, rows = prompt.reshape(-1).tolist(), []
    for step in range(new):
        rows.append(hid)
        seq.append(int(sample_next(logits.reshape(1, -1).cpu(), True, 0.3, 50)))
        if step + 1 < new:
            hid, logits = lm.decode(seq[-1])
    assert out.sequences[0].tolist() == seq and all(torch.equal(h[-1][:, -1:].reshape(-1), r) for h, r in zip(out.hidden_states, rows))

    prompts = tiny.prompts[:3]
    torch.manual_seed(0)
    outs = lm.generate_batch(prompts, do_sample=True, temperature=0.3, max_new_tokens=new, sampler="host")
    torch.manual_seed(0)
    seqs = [p.reshape(-1).tolist() for p in prompts]
    for slot, p in enumerate(prompts):
        lm.reset_slot(slot)
    first = [lm.prefill_slot(slot, lm.embed_tokens(p.reshape(-1))) for slot, p in enumerate(prompts)]
    logits = torch.stack([f[1] for f in first])
    for step in range(new):
        nxt = torch.multinomial(sample_probs(logits.cpu(), 0.3, 50), num_samples=1).squeeze(1).tolist()
        for s, t in zip(seqs, nxt):
            s.append(t)
        if step + 1 < new:
            _, logits = lm.decode_batch([0, 1, 2], nxt)
    assert [o.sequences[0].tolist() for o in outs] == seqs
