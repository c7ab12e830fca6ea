"""Top-p without a GPU: `sample_probs(..., top_p)` against the installed transformers warpers, the float64 oracle of tests/nucleus_ref.py against it, the new
symbol's refusals (made before any HIP call), and the generation-config plumbing of `HipInstructAny2PixLM` (keyword over loaded value over default)."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nucleus_ref as nr  # noqa: E402

CPU_VS = tuple(V for V in nr.VS if V <= 1000)


@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


@pytest.mark.parametrize("V", CPU_VS)
def test_sample_probs_is_the_transformers_chain(V):
    from transformers import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    from instructany2pix_amd.llm import sample_probs
    logits = nr.rows(V)
    ids = torch.zeros(8, 4, dtype=torch.long)
    for temperature in nr.TEMPERATURES:
        for top_k in nr.TOP_KS:
            plain = sample_probs(logits, temperature, top_k)
            for top_p in nr.TOP_PS:
                ref = TemperatureLogitsWarper(temperature)(ids, logits.clone())
                if top_k:
                    ref = TopKLogitsWarper(top_k)(ids, ref)
                if top_p < 1.0:                                    # `generate` adds the warper only then
                    ref = TopPLogitsWarper(top_p)(ids, ref)
                got = sample_probs(logits, temperature, top_k, top_p)
                assert torch.equal(got, torch.nn.functional.softmax(ref, dim=-1)), (V, temperature, top_k, top_p)
                if top_p == 1.0:
                    assert torch.equal(got.view(torch.int32), plain.view(torch.int32))
    assert torch.equal(sample_probs(logits, 0.3, 50, top_p=1.0).view(torch.int32), sample_probs(logits).view(torch.int32))


def test_sample_next_draws_from_the_nucleus():
    from instructany2pix_amd.llm import sample_next, sample_probs
    logits = nr.rows(1000)[:1]
    probs = sample_probs(logits, 0.3, 50, 0.6)
    torch.manual_seed(4)
    want = torch.multinomial(probs, num_samples=1).squeeze(1)
    torch.manual_seed(4)
    assert torch.equal(sample_next(logits, True, 0.3, 50, 0.6), want)
    assert torch.equal(sample_next(logits, False, top_p=0.6), logits.argmax(-1))
    assert 1 <= int((probs > 0).sum()) < 50


@pytest.mark.parametrize("bad", [float("nan"), 0, 0.0, -0.5, 1.5, float("inf"), None, "x"])
def test_an_invalid_top_p_raises_with_the_warpers_wording(bad):
    from instructany2pix_amd.llm import HipInstructAny2PixLM, sample_next, sample_probs
    logits = torch.zeros(1, 8)
    with pytest.raises(ValueError, match="`top_p` has to be a float > 0 and < 1"):
        sample_probs(logits, 0.3, 50, bad)
    with pytest.raises(ValueError, match="`top_p` has to be a float > 0 and < 1"):
        sample_next(logits, True, 0.3, 50, bad)
    if bad is None:                                                  # (the LM's keyword reads None as "not given")
        return
    lm = object.__new__(HipInstructAny2PixLM)                        # no engine behind it: the check comes before the first use of one
    for sampler in ("host", "device"):
        with pytest.raises(ValueError, match="top_p"):
            lm.generate(torch.tensor([[1, 5, 6]]), sampler=sampler, top_p=bad)
        with pytest.raises(ValueError, match="top_p"):
            lm.generate_batch([torch.tensor([[1, 5, 6]])], sampler=sampler, top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        lm.sample_tokens(torch.zeros(1, 8), [1], [0], top_p=bad)


@pytest.mark.parametrize("V", CPU_VS)
def test_the_oracle_agrees_with_sample_probs_where_no_scores_tie(V):
    """fp32 torch against the float64 rule: every decided entry has the support `sample_probs` gives it. Row 1 (ties at the k-th value, which the nucleus
    boundary can reach) and row 3 (all equal) are asserted the other way: the oracle keeps a tied group whole, whatever the sort did with it."""
    from instructany2pix_amd.llm import sample_probs
    logits = nr.rows(V)
    for temperature in nr.TEMPERATURES:
        for top_k in nr.TOP_KS:
            for top_p in nr.TOP_PS[:-1]:
                support = sample_probs(logits, temperature, top_k, top_p) > 0
                for r in range(8):
                    kept, dropped, undecided = nr.oracle(logits[r], temperature, top_k, top_p)
                    what = (V, temperature, top_k, top_p, r)
                    assert int(undecided.sum()) <= nr.undecided_cap(V), what
                    assert not bool((kept & dropped).any()) and bool((kept | dropped | undecided).all()) and bool(kept.any()), what
                    scores = logits[r] / temperature
                    assert bool(kept[scores == scores.max()].all()), what
                    if bool(dropped.any()):                             # closed upwards, strictly: equal scores are never split by a decision
                        assert float(scores[kept].min()) > float(scores[dropped].max()), what
                    if r in (1, 3):
                        continue
                    assert bool(support[r][kept].all()) and not bool(support[r][dropped].any()), what
    # row 3: every entry ties, the whole row is the nucleus (transformers keeps a sort-dependent part of it)
    kept, dropped, undecided = nr.oracle(logits[3], 1.0, 50, 0.25)
    assert bool(kept.all()) and not bool(dropped.any()) and not bool(undecided.any())
    assert int((sample_probs(logits[3:4], 1.0, 50, 0.25) > 0).sum()) < V
    # row 1 at top_p -> 0: the nucleus is the maximum alone; at top_p close to 1 the ties at the k-th value come in, all of them or none
    scores, K = nr.scores_and_topk(logits[1], 0.3, 50)
    ties = scores == scores[K].min()
    for top_p in (0.25, 0.6, 0.9, 0.999999):
        kept, _, undecided = nr.oracle(logits[1], 0.3, 50, top_p)
        assert int(ties.sum()) == {50: 1, 51: 2, 1000: 5}[V]
        assert bool(kept[ties].all()) or not bool((kept | undecided)[ties].any())
    kept, _, _ = nr.oracle(logits[1], 1.0, 50, 0.999999)
    assert bool(kept[ties].all()) and torch.equal(kept, K)


def test_the_cap_on_undecided_entries_holds_at_the_largest_shape():
    """the condition the GPU test puts on its inputs, at V = 32003 (rows 0-7, every temperature, top_k and top_p < 1)"""
    logits = nr.rows(32003)
    worst = 0
    for temperature in nr.TEMPERATURES:
        for top_k in nr.TOP_KS:
            for top_p in nr.TOP_PS[:-1]:
                for r in range(8):
                    worst = max(worst, int(nr.oracle(logits[r], temperature, top_k, top_p)[2].sum()))
    assert worst <= nr.undecided_cap(32003), worst


def test_library_exports_the_nucleus_sampler_and_refuses_a_bad_top_p(lib):
    assert hasattr(lib, "ia2p_sample_tokens_p")
    one = 256           # never dereferenced: every call below is refused before any HIP call
    s1, t1 = (C.c_uint64 * 1)(1), (C.c_uint32 * 1)(0)
    for top_p in (float("nan"), 0.0, -0.5, 1.5):
        for do_sample in (1, 0):
            assert lib.ia2p_sample_tokens_p(None, one, 8, 1, 8, 1.0, 0, top_p, do_sample, s1, t1, one, None, None) == 1, top_p
        assert b"top_p" in lib.ia2p_last_error(None)
    # the refusals of ia2p_sample_tokens, with a valid top_p
    assert lib.ia2p_sample_tokens_p(None, None, 8, 1, 8, 1.0, 0, 0.6, 1, s1, t1, one, None, None) == 1
    assert lib.ia2p_sample_tokens_p(None, one, 8, 1, 8, 1.0, 0, 0.6, 1, None, t1, one, None, None) == 1
    assert lib.ia2p_sample_tokens_p(None, one, 8, 1, 8, 0.0, 0, 0.6, 1, s1, t1, one, None, None) == 1
    assert lib.ia2p_sample_tokens_p(None, one, 8, 1, 8, 1.0, 0, 0.6, 2, s1, t1, one, None, None) == 1
    assert lib.ia2p_sample_tokens_p(None, one, 8, 0, 8, 1.0, 0, 0.6, 1, s1, t1, one, None, None) == 2
    assert lib.ia2p_sample_tokens_p(None, one, 8, 4097, 8, 1.0, 0, 1.0, 0, None, None, one, None, None) == 2
    assert lib.ia2p_sample_tokens_p(None, one, 8, 1, (1 << 20) + 1, 1.0, 0, 0.6, 1, s1, t1, one, None, None) == 2
    assert lib.ia2p_sample_tokens_p(None, one, 7, 2, 8, 1.0, 0, 0.6, 1, s1, t1, one, None, None) == 2
    assert lib.ia2p_sample_tokens_p(None, one + 2, 8, 1, 8, 1.0, 0, 0.6, 1, s1, t1, one, None, None) == 1          # misaligned


# ---- generation config ----------------------------------------------------------------------------------------------------------------------------------

def _standin():
    """`generate` / `generate_batch` on a table instead of an engine (the stand-in of tests/test_llm_batch_cpu.py, restated): logits that put all weight on
    one token, a `sample_tokens` that records its keywords and names that token"""
    from types import SimpleNamespace
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    VOCAB = 16

    class StandIn(HipInstructAny2PixLM):
        def __init__(self):
            self.config = SimpleNamespace(num_hidden_layers=2, hidden_size=4, vocab_size=VOCAB)
            self.max_batch, self.max_positions, self.device = 2, 64, torch.device("cpu")
            self.seen = []
            self._tok_dev = torch.zeros(8, dtype=torch.int32)
            self._tok_host = torch.zeros(8, dtype=torch.int32)

        def _row(self, token):
            logits = torch.zeros(VOCAB)
            logits[(5 * int(token) + 3) % VOCAB] = 40.0
            return torch.full((4,), float(token)), logits

        def prepare_inputs_embeds(self, input_ids, extra_replacement=None):
            return input_ids.reshape(-1, 1).float()

        def reset(self):
            pass

        def reset_slot(self, slot):
            pass

        def prefill(self, emb):
            return self._row(emb[-1, 0])

        def prefill_slot(self, slot, emb):
            return self._row(emb[-1, 0])

        def decode(self, token):
            return self._row(token)

        def decode_batch(self, slots, token_ids):
            r = [self._row(t) for t in token_ids]
            return torch.stack([x[0] for x in r]), torch.stack([x[1] for x in r])

        def decode_batch_dev(self, slots, dev_tokens, token_index=None):
            index = range(len(slots)) if token_index is None else token_index
            return self.decode_batch(slots, [int(dev_tokens[i]) for i in index])

    return StandIn()


def test_load_generation_config_takes_a_dict_a_file_and_a_folder(tmp_path):
    from instructany2pix_amd.llm import HipInstructAny2PixLM, read_generation_config
    lm = _standin()
    assert lm.generation_defaults == {"top_k": 50, "top_p": 1.0} == HipInstructAny2PixLM.generation_defaults
    vicuna = {"_from_model_config": True, "bos_token_id": 1, "eos_token_id": 2, "max_length": 4096, "pad_token_id": 0, "temperature": 0.9, "top_p": 0.6,
              "transformers_version": "4.31.0"}
    assert lm.load_generation_config(vicuna) == {"top_k": 50, "top_p": 0.6, "temperature": 0.9} == lm.generation_defaults
    assert HipInstructAny2PixLM.generation_defaults == {"top_k": 50, "top_p": 1.0}, "loading into one LM changed the class's defaults"
    folder = tmp_path / "llm-retrained"
    folder.mkdir()
    (folder / "generation_config.json").write_text(json.dumps({"top_p": 0.25, "top_k": 20, "do_sample": True}))
    for where in (folder, str(folder), folder / "generation_config.json"):
        lm = _standin()
        assert lm.load_generation_config(where) == {"top_k": 20, "top_p": 0.25}
    assert read_generation_config({"top_k": 0}) == {"top_k": None} and read_generation_config({"max_length": 5}) == {}
    for bad in ({"top_p": 0.0}, {"top_p": 1.5}, {"top_p": float("nan")}, {"top_p": "much"}, {"top_k": -1}, {"top_k": 2.5}, {"temperature": 0.0}):
        lm = _standin()
        with pytest.raises(ValueError):
            lm.load_generation_config(bad)
        assert lm.generation_defaults == {"top_k": 50, "top_p": 1.0}
    with pytest.raises(OSError):
        lm.load_generation_config(tmp_path)                          # a folder without the file


def test_a_top_p_keyword_reaches_the_sampler_and_wins_over_the_loaded_value(monkeypatch):
    """spies on `sample_next` / `sample_probs` (host) and `sample_tokens` (device): keyword over loaded value over 1.0"""
    from instructany2pix_amd import llm as L
    seen = []
    real_next, real_probs = L.sample_next, L.sample_probs

    def spy_next(logits, do_sample=True, temperature=0.3, top_k=50, top_p=1.0):
        seen.append(("next", top_k, top_p))
        return real_next(logits, do_sample, temperature, top_k, top_p)

    def spy_probs(logits, temperature=0.3, top_k=50, top_p=1.0):
        seen.append(("probs", top_k, top_p))
        return real_probs(logits, temperature, top_k, top_p)

    monkeypatch.setattr(L, "sample_next", spy_next)
    monkeypatch.setattr(L, "sample_probs", spy_probs)
    monkeypatch.setattr(torch.cuda, "Event", lambda: type("E", (), {"record": lambda s: None, "synchronize": lambda s: None})())
    lm = _standin()

    def spy_tokens(logits, seeds, steps, do_sample=True, temperature=0.3, top_k=50, out=None, top_p=None):
        seen.append(("tokens", top_k, lm._resolve_top_p(top_p)))
        out[:logits.shape[0]] = logits.argmax(-1).int()
        return out[:logits.shape[0]]

    lm.sample_tokens = spy_tokens
    prompt = torch.tensor([[1, 2, 4]])

    def run(**kw):
        del seen[:]
        a = lm.generate(prompt, max_new_tokens=2, sampler="host", **kw)
        b = lm.generate_batch([prompt, prompt], max_new_tokens=2, sampler="host", **kw)
        c = lm.generate(prompt, max_new_tokens=2, sampler="device", seed=1, **kw)
        d = lm.generate_batch([prompt, prompt], max_new_tokens=2, sampler="device", seeds=[1, 2], **kw)
        assert all(torch.equal(x.sequences, a.sequences) for x in (b[0], b[1], c, d[0], d[1]))
        assert {s[0] for s in seen} == {"next", "probs", "tokens"}
        return {s[2] for s in seen}, {s[1] for s in seen}

    assert run() == ({1.0}, {50})
    assert run(top_p=0.6) == ({0.6}, {50})
    lm.load_generation_config({"top_p": 0.25, "temperature": 0.9})
    assert run() == ({0.25}, {50})
    assert run(top_p=0.9, top_k=7) == ({0.9}, {7})
    assert run(top_p=1.0) == ({1.0}, {50})


def test_the_pipeline_loads_the_generation_config_of_the_llm_folder(tmp_path):
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    (tmp_path / "llm-retrained").mkdir()
    lm = _standin()
    InstructAny2PixPipeline(str(tmp_path), unet=object(), llm=lm, llm_tokenizer=object())
    assert lm.generation_defaults == {"top_k": 50, "top_p": 1.0}
    (tmp_path / "llm-retrained" / "generation_config.json").write_text(json.dumps({"temperature": 0.9, "top_p": 0.6}))
    InstructAny2PixPipeline(str(tmp_path), unet=object(), llm=lm, llm_tokenizer=object())
    assert lm.generation_defaults == {"top_k": 50, "top_p": 0.6, "temperature": 0.9}
