"""The LLaMA decoder on the HIP kernels (ia2p_llm_*) against the installed transformers `LlamaForCausalLM` on the CPU, loaded with the same
fp16-rounded synthetic weights.

Tolerance. The yardstick is transformers itself: the oracle runs in fp32 and once more in fp16 on the same inputs,
`e_ref = rel-L2(fp16 oracle, fp32 oracle)` over the rows a test checks (stacked: the error of the number format on this model and these inputs,
estimated over all the checked rows rather than a single one), and every checked HIP row must satisfy `rel-L2(hip, fp32 oracle) <= 2 * e_ref`
(factor 2: the sums run in another order than the CPU's). The greedy check uses `delta = 2 * max|fp16 oracle logits - fp32 oracle logits|` over
the checked steps. Every figure is printed before it is asserted (pytest -s); docs/LOG.md records a run."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def make_oracle(cfg, sd):
    from transformers import LlamaConfig, LlamaForCausalLM
    lc = LlamaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                     num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                     num_key_value_heads=cfg.num_key_value_heads, rms_norm_eps=cfg.rms_norm_eps, max_position_embeddings=2048,
                     rope_parameters={"rope_type": "default", "rope_theta": cfg.rope_theta}, tie_word_embeddings=False, attention_bias=False)
    m = LlamaForCausalLM(lc).eval()
    llama = {k: v.float() for k, v in sd.items() if "vae_pro" not in k and "vae_pre" not in k}      # p.data = p.data.half().float()
    m.load_state_dict(llama, strict=True)
    return m, copy.deepcopy(m).half()


@torch.no_grad()
def oracle_rows(model, ids=None, embeds=None):
    """-> (final-normed hidden rows [T, H], logits rows [T, V]) of one full forward, as fp32"""
    kw = dict(input_ids=ids.reshape(1, -1)) if embeds is None else dict(inputs_embeds=embeds.reshape(1, *embeds.shape[-2:]).to(model.dtype))
    out = model(**kw, output_hidden_states=True, use_cache=False)
    return out.hidden_states[-1][0].float(), out.logits[0].float()


class Bundle:
    def __init__(self, cfg, seed, projector_type="linear", max_positions=256):
        from instructany2pix_amd.llm import HipInstructAny2PixLM
        from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
        self.cfg = cfg
        self.sd = synthetic_state_dict(llm_param_specs(cfg, cfg.embed_dim, projector_type), seed=seed)
        self.o32, self.o16 = make_oracle(cfg, self.sd)
        self.lm = HipInstructAny2PixLM(cfg, DEV, max_positions=max_positions, video_token_id=cfg.vocab_size - 3)
        self.lm.load_state_dict(self.sd)

    def refs(self, ids=None, embeds=None):
        h32, l32 = oracle_rows(self.o32, ids, embeds)
        h16, l16 = oracle_rows(self.o16, ids, embeds)
        return h32, l32, h16, l16


@pytest.fixture(scope="module")
def tiny():
    from instructany2pix_amd.config import tiny_llm
    return Bundle(tiny_llm(), seed=21)


def _ids(n, vocab, seed):
    return torch.randint(3, vocab - 9, (n,), generator=torch.Generator().manual_seed(seed))


def _check(tag, hip_h, hip_l, h32, l32, eh, el):
    dh, dl = rel_l2(hip_h, h32), rel_l2(hip_l, l32)
    print(f"[llm] {tag}: hidden rel-L2 {dh:.3e} (e_ref {eh:.3e}), logits rel-L2 {dl:.3e} (e_ref {el:.3e})")
    return dh <= 2 * eh and dl <= 2 * el


def test_oracle_hidden_state_is_final_normed(tiny):
    h32, l32, _, _ = tiny.refs(_ids(9, 512, 1))
    assert torch.allclose(h32 @ tiny.o32.lm_head.weight.t(), l32, atol=1e-4)


@pytest.mark.parametrize("T", [1, 7, 40, 129])
def test_prefill_against_oracle(tiny, T):
    ids = _ids(T, 512, 100 + T)
    h32, l32, h16, l16 = tiny.refs(ids)
    tiny.lm.reset()
    hid, logits = tiny.lm.prefill(tiny.lm.embed_tokens(ids))
    assert tiny.lm.position == T
    ok = _check(f"prefill T={T}", hid, logits, h32[-1], l32[-1], rel_l2(h16[-1], h32[-1]), rel_l2(l16[-1], l32[-1]))
    assert ok


def _prefill_then_decode(lm, ids, n_prefill):
    lm.reset()
    rows = [lm.prefill(lm.embed_tokens(ids[:n_prefill]))]
    for t in ids[n_prefill:].tolist():
        rows.append(lm.decode(t))
    return torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])


def test_decode_steps_teacher_forced(tiny):
    """24 decode steps behind a 17-row prefill; step i against row 16 + i of the oracle's forward of the 41 ids (causal: that row is the
    oracle's full forward of the prefix, the `use_cache=False` computation of the reference)"""
    ids = _ids(41, 512, 7)
    h32, l32, h16, l16 = tiny.refs(ids)
    hid, logits = _prefill_then_decode(tiny.lm, ids, 17)
    assert hid.shape[0] == 25 and tiny.lm.position == 41
    eh, el = rel_l2(h16[16:], h32[16:]), rel_l2(l16[16:], l32[16:])
    oks = [_check(f"decode step {i}", hid[i], logits[i], h32[16 + i], l32[16 + i], eh, el) for i in range(25)]
    assert all(oks)


def test_one_prefill_equals_prefill_plus_decodes_within_tolerance_and_decode_is_deterministic(tiny):
    ids = _ids(41, 512, 8)
    h32, l32, h16, l16 = tiny.refs(ids)
    eh, el = rel_l2(h16[-1], h32[-1]), rel_l2(l16[-1], l32[-1])
    tiny.lm.reset()
    ph, pl = tiny.lm.prefill(tiny.lm.embed_tokens(ids))
    a_h, a_l = _prefill_then_decode(tiny.lm, ids, 17)
    b_h, b_l = _prefill_then_decode(tiny.lm, ids, 17)
    ok1 = _check("41 rows as one prefill", ph, pl, h32[-1], l32[-1], eh, el)
    ok2 = _check("prefill(17) + 24 decodes", a_h[-1], a_l[-1], h32[-1], l32[-1], eh, el)
    assert ok1 and ok2
    assert torch.equal(a_h, b_h) and torch.equal(a_l, b_l)          # run-to-run identical bits


@pytest.fixture(scope="module")
def long2():
    """two layers and 2048 cached positions: rows past position 255, where the attention's loops over the keys take a second trip and more"""
    from instructany2pix_amd.config import tiny_llm
    cfg = tiny_llm()
    cfg.num_hidden_layers = 2
    return Bundle(cfg, seed=22, max_positions=2048)


@pytest.mark.parametrize("T", [257, 1025])
def test_prefill_past_256_positions_against_oracle(long2, T):
    ids = _ids(T, 512, 200 + T)
    h32, l32, h16, l16 = long2.refs(ids)
    long2.lm.reset()
    hid, logits = long2.lm.prefill(long2.lm.embed_tokens(ids))
    assert long2.lm.position == T
    assert _check(f"2 layers, prefill T={T}", hid, logits, h32[-1], l32[-1], rel_l2(h16[-1], h32[-1]), rel_l2(l16[-1], l32[-1]))


@pytest.mark.parametrize("n_prefill,steps", [(250, 10), (1020, 8)])
def test_decode_steps_across_a_256_position_boundary(long2, n_prefill, steps):
    """teacher-forced decode steps whose positions cross 256 (250 .. 259) and 1024 (1020 .. 1027); row i of the run against row n_prefill - 1 + i of the
    oracle's forward of all the ids"""
    ids = _ids(n_prefill + steps, 512, 300 + n_prefill)
    h32, l32, h16, l16 = long2.refs(ids)
    hid, logits = _prefill_then_decode(long2.lm, ids, n_prefill)
    lo = n_prefill - 1
    assert hid.shape[0] == steps + 1 and long2.lm.position == n_prefill + steps
    eh, el = rel_l2(h16[lo:], h32[lo:]), rel_l2(l16[lo:], l32[lo:])
    oks = [_check(f"2 layers, position {lo + i}", hid[i], logits[i], h32[lo + i], l32[lo + i], eh, el) for i in range(steps + 1)]
    assert all(oks)


def test_reset_leaves_no_state(tiny):
    ids_a, ids_b = _ids(30, 512, 9), _ids(23, 512, 10)
    a_h, a_l = _prefill_then_decode(tiny.lm, ids_a, 20)
    _prefill_then_decode(tiny.lm, ids_b, 5)                         # another request in between, other lengths
    c_h, c_l = _prefill_then_decode(tiny.lm, ids_a, 20)
    assert torch.equal(a_h, c_h) and torch.equal(a_l, c_l)


def test_errors_before_any_launch(tiny):
    from instructany2pix_amd import _ffi
    lm = tiny.lm
    lm.reset()
    with pytest.raises(_ffi.IA2PError, match="before a prefill"):
        lm.decode(5)
    with pytest.raises(ValueError, match="cache holds"):
        lm.prefill(torch.zeros(257, 512))
    lm.prefill(lm.embed_tokens(_ids(4, 512, 3)))
    with pytest.raises(ValueError, match="vocabulary"):
        lm.decode(512)
    assert lm.position == 4


def _reference_inputs_embeds(table_rows, raw_input_ids, video_id, extra_replacement, projector):
    """the lines of `InstructAny2PixLMForCausalLM.forward` that build `inputs_embeds` at inference (any2pix_llama.py:277-291), operation
    for operation on [1, T, H] tensors, INPUT = 0"""
    inputs_embeds = table_rows.clone()
    extra_replacement_mask = (raw_input_ids == video_id)
    z = torch.zeros_like(inputs_embeds)
    z2 = projector(extra_replacement['data'][extra_replacement['mask'] == 0])
    a, b = torch.where(extra_replacement_mask)
    a = a[:extra_replacement['mask'].shape[0]]
    b = b[:extra_replacement['mask'].shape[0]]
    z[a[extra_replacement['mask'] == 0], b[extra_replacement['mask'] == 0]] += z2
    inputs_embeds[extra_replacement_mask][:extra_replacement['mask'].shape[0]][extra_replacement['mask'] == 0] = 0.0
    z = z + inputs_embeds
    return z


def test_video_replacement(tiny):
    lm, cfg = tiny.lm, tiny.cfg
    vid = lm.DEFAULT_VIDEO_TOKEN_IDX
    ids = _ids(20, 512, 12)
    ids[3], ids[9], ids[15] = vid, vid, vid
    g = torch.Generator().manual_seed(13)
    data = torch.randn(2, cfg.embed_dim, generator=g)
    data = data / data.norm(dim=-1, keepdim=True) * 20
    er = {"data": data, "mask": torch.zeros(2, dtype=torch.long)}
    W, bias = tiny.sd["model.vae_projector_image.weight"].float(), tiny.sd["model.vae_projector_image.bias"].float()
    table = tiny.sd["model.embed_tokens.weight"].float()
    want = _reference_inputs_embeds(table[ids][None], ids[None], vid, er, lambda x: x @ W.t() + bias)[0]
    got = lm.prepare_inputs_embeds(ids[None], er).float().cpu()
    assert torch.equal(got[15], table[vid])                          # the third <video> keeps its table embedding
    keep = torch.ones(20, dtype=torch.bool); keep[[3, 9]] = False
    assert torch.equal(got[keep], table[ids][keep])
    tol = 2 * 2.0 ** -11 * float(want[[3, 9]].abs().max())           # two fp16 roundings: the projection's output, the sum
    print(f"[llm] <video> rows: max abs error {float((got[[3, 9]] - want[[3, 9]]).abs().max()):.3e} (bound {tol:.3e})")
    assert float((got[[3, 9]] - want[[3, 9]]).abs().max()) <= tol
    h32, l32, h16, l16 = tiny.refs(embeds=want)
    lm.reset()
    hid, logits = lm.prefill(lm.prepare_inputs_embeds(ids[None], er))
    assert _check("<video> replacement prefill", hid, logits, h32[-1], l32[-1], rel_l2(h16[-1], h32[-1]), rel_l2(l16[-1], l32[-1]))
    with pytest.raises(ValueError):
        lm.prepare_inputs_embeds(ids[None], {"data": torch.randn(4, cfg.embed_dim), "mask": torch.zeros(4, dtype=torch.long)})


def test_mlp_gelu_heads():
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    from instructany2pix_amd.weights import llm_head_specs, synthetic_state_dict
    cfg = tiny_llm(vocab_size=64, mm_projector_type="mlp2x_gelu")
    cfg.num_hidden_layers = 1
    sd = synthetic_state_dict(llm_head_specs(cfg, cfg.embed_dim, "mlp2x_gelu"), seed=4)
    lm = HipInstructAny2PixLM(cfg, DEV, max_positions=8)
    lm.load_state_dict(sd, strict=False)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, cfg.embed_dim, generator=g).half()
    f = {k: v.float() for k, v in sd.items()}
    gelu = torch.nn.functional.gelu
    p = "model.vae_projector_image."
    want = gelu(x.float() @ f[p + "0.weight"].t() + f[p + "0.bias"]) @ f[p + "2.weight"].t() + f[p + "2.bias"]
    got = lm.vae_projector_image(x).cpu()
    assert got.shape == (3, 512) and rel_l2(got, want) < 2e-3        # fp16 storage between the two linears: 2^-11 per rounding, three of them
    q = "model.vae_predictor_image."
    y = torch.randn(1, 1, 512, generator=g).half()
    want = gelu(y.float() @ f[q + "0.weight"].t() + f[q + "0.bias"]) @ f[q + "2.weight"].t() + f[q + "2.bias"]
    got = lm.vae_predictor_image(y.float().to(DEV)).cpu()
    assert got.shape == (1, 1, cfg.embed_dim) and rel_l2(got, want) < 2e-3


def test_greedy_generate_against_teacher_forced_oracle(tiny):
    lm = tiny.lm
    prompt = _ids(12, 512, 14)[None]
    out = lm.generate(prompt, do_sample=False, max_new_tokens=32)
    assert out.sequences.shape == (1, 44) and len(out.hidden_states) == 32 and torch.equal(out.sequences[:, :12], prompt)
    h32, l32, h16, l16 = tiny.refs(out.sequences[0, :-1])             # row 11 + i predicted generated token i
    steps32, steps16 = l32[11:], l16[11:]
    delta = 2 * float((steps16 - steps32).abs().max())
    chosen = out.sequences[0, 12:]
    gap = steps32.max(dim=-1).values - steps32.gather(1, chosen[:, None])[:, 0]
    print(f"[llm] greedy: delta {delta:.3e}, largest gap of a chosen token to the oracle's maximum {float(gap.max()):.3e}, "
          f"tokens equal to the oracle's argmax: {int((steps32.argmax(-1) == chosen).sum())}/32")
    assert gap.shape == (32,) and bool((gap <= delta).all())
    eh = rel_l2(h16[11:], h32[11:])
    got = torch.cat([out.hidden_states[i][-1][:, -1:].reshape(1, -1) for i in range(32)])
    assert all(rel_l2(got[i], h32[11 + i]) <= 2 * eh for i in range(32))
    with pytest.raises(IndexError):
        out.hidden_states[0][0]

    class StopAfter:
        def __init__(self, n):
            self.n = n

        def __call__(self, ids, scores, **kw):
            return ids.shape[1] >= 12 + self.n

    early = lm.generate(prompt, do_sample=False, max_new_tokens=32, stopping_criteria=[StopAfter(5)])
    assert early.sequences.shape == (1, 17) and len(early.hidden_states) == 5
    assert torch.equal(early.sequences, out.sequences[:, :17])
    torch.manual_seed(3)
    s1 = lm.generate(prompt, do_sample=True, temperature=0.3, max_new_tokens=6).sequences
    torch.manual_seed(3)
    s2 = lm.generate(prompt, do_sample=True, temperature=0.3, max_new_tokens=6).sequences
    assert torch.equal(s1, s2)


def test_full_width_two_layers():
    """hidden 4096, 32 heads, intermediate 11008, vocabulary 32 003 (not a multiple of 4), 2 layers: prefill 33 + 8 decodes"""
    from instructany2pix_amd.config import vicuna_7b
    cfg = vicuna_7b(32003)
    cfg.num_hidden_layers = 2
    b = Bundle(cfg, seed=33)
    ids = _ids(41, 32003, 15)
    h32, l32, h16, l16 = b.refs(ids)
    hid, logits = _prefill_then_decode(b.lm, ids, 33)
    assert hid.shape == (9, 4096) and logits.shape == (9, 32003)
    eh, el = rel_l2(h16[32:], h32[32:]), rel_l2(l16[32:], l32[32:])
    oks = [_check(f"full width row {32 + i}", hid[i], logits[i], h32[32 + i], l32[32 + i], eh, el) for i in range(9)]
    assert all(oks)


def test_pipeline_llm_only_end_to_end(tiny):
    from stub_llm_tokenizer import StubLlamaTokenizer
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    tok = StubLlamaTokenizer(503)
    assert len(tok) == tiny.cfg.vocab_size and tok("<video>", add_special_tokens=False).input_ids[0] == tiny.lm.DEFAULT_VIDEO_TOKEN_IDX
    pipe = InstructAny2PixPipeline(unet=object(), llm=tiny.lm, llm_tokenizer=tok)
    g = torch.Generator().manual_seed(5)
    mm = [{"type": "image", "fname": "fox.png", "embed": torch.randn(1024, generator=g)},
          {"type": "audio", "fname": "rain.wav", "embed": torch.randn(1024, generator=g)}]
    torch.manual_seed(17)
    a, b, caption = pipe("add <video> to <video> and turn the fox blue", mm, llm_only=True)
    assert a is None and b is None and isinstance(caption, str)
    assert isinstance(pipe.cache, tuple) and len(pipe.cache) == 5 and pipe.cache[2] == caption
    n_prompt = tok("x", return_tensors="pt").input_ids.shape[1]
    assert 1 <= tiny.lm.position and n_prompt == 2
    assert pipe.forward_llm("anything", mm, use_cache=True) is pipe.cache
    with pytest.raises(ValueError):
        pipe.forward_llm("no entries", [])
