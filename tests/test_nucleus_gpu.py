"""`ia2p_sample_tokens_p` against the float64 rule of tests/nucleus_ref.py, and top-p through `generate` / `generate_batch` on the tiny LLaMA configuration.

The nucleus the kernel kept is read from `probs_out > 0`. It must agree with the oracle on every decided entry (an entry within BAND = 2 * (d + 2) * 2^-24 of the
boundary, d = 1 the kernel's summation depth, may fall either way; the inputs have at most 8 such entries per row at V >= 1000 and none at V <= 51, which is
asserted of the inputs before a result is looked at), and be closed upwards in score. The draw and `probs_out` are then judged against the float64 distribution
over THAT set, as tests/test_sampler_gpu.py judges them: u is the Philox restatement's bit for bit and falls into the token's interval of the cdf within
4 * K * 2^-24, `probs_out` is within 1e-5 relative. top_p = 1.0 is judged by what defines it: the bits of `ia2p_sample_tokens`."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucleus_ref as nr  # noqa: E402
import sampler_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG = nr.NEG


def _lib():
    from instructany2pix_amd import _ffi
    return _ffi, _ffi.lib()


def _sample(block, M, V, temperature, top_k, top_p, seeds, steps, ld=None, do_sample=1, probs=True):
    """block: device tensor whose data pointer is row 0 -> (tokens [M], u [M], probs [M, V] or None) on the host; top_p None: `ia2p_sample_tokens`"""
    ffi, lib = _lib()
    tokens = torch.full((M,), -7, dtype=torch.int32, device=DEV)
    u = torch.full((M,), -1.0, device=DEV)
    p = torch.full((M, V), float("nan"), device=DEV) if probs else None
    sd, st = (C.c_uint64 * M)(*seeds) if seeds else None, (C.c_uint32 * M)(*steps) if steps else None
    ld = V if ld is None else ld
    if top_p is None:
        status = lib.ia2p_sample_tokens(ffi.current_stream(), C.c_void_p(block.data_ptr()), ld, M, V, temperature, top_k, do_sample, sd, st, ffi.ptr(tokens), ffi.ptr(p),
                                        ffi.ptr(u))
    else:
        status = lib.ia2p_sample_tokens_p(ffi.current_stream(), C.c_void_p(block.data_ptr()), ld, M, V, temperature, top_k, top_p, do_sample, sd, st, ffi.ptr(tokens),
                                          ffi.ptr(p), ffi.ptr(u))
    ffi.check(status, None, llm=True)
    torch.cuda.synchronize()
    return tokens.cpu(), u.cpu(), None if p is None else p.cpu()


_ORACLE = {}


def _oracle(V, r, temperature, top_k, top_p):
    key = (V, r, temperature, top_k, top_p)
    if key not in _ORACLE:
        _ORACLE[key] = nr.oracle(nr.rows(V)[r], temperature, top_k, top_p)
    return _ORACLE[key]


def _same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and (
        (a[2] is None and b[2] is None) or torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)))


def _judge_set(what, row, temperature, got, oracle):
    """got: bool [V], the kernel's nucleus -> its float64 (probs, cdf), after the set itself has been checked"""
    kept, dropped, _ = oracle
    assert bool(got[kept].all()), f"{what}: {int((~got[kept]).sum())} entries of the nucleus are missing"
    assert not bool(got[dropped].any()), f"{what}: {int(got[dropped].sum())} entries outside the nucleus carry weight"
    scores = row.float() / temperature
    if not bool(got.all()):
        assert float(scores[got].min()) > float(scores[~got].max()), f"{what}: a dropped score is not below every kept one"
    return nr.distribution(row, temperature, got)


def _judge_draw(what, t, u, got, cdf, seed, step):
    """tests/test_sampler_gpu.py::_judge on the kernel's own kept set"""
    assert float(u) == float(sampler_ref.uniform(seed, step)), f"{what}: u = {float(u)!r}, the restatement gives {float(sampler_ref.uniform(seed, step))!r}"
    assert 0 <= t < got.numel() and bool(got[t]), f"{what}: token {t} is outside the kept set"
    rank = int(got[:t].sum())
    lo, hi = (float(cdf[rank - 1]) if rank else 0.0), float(cdf[rank])
    tol = 4 * cdf.numel() * 2.0 ** -24
    assert lo - tol <= float(u) < hi + tol, f"{what}: u = {float(u)} outside [{lo}, {hi}) of token {t} (tol {tol})"


def _judge_probs(what, p, got, want):
    assert bool((p[~got] == 0).all()), f"{what}: weight outside the kept set"
    assert bool(((p - want).abs() <= 1e-5 * want)[got].all()), f"{what}: probs_out off by {float(((p - want).abs() / want)[got].max())} relative"


@pytest.mark.parametrize("V", nr.VS)
def test_the_kept_set_is_the_nucleus_and_every_draw_inverts_its_cdf(V):
    rows = nr.rows(V)
    for temperature in nr.TEMPERATURES:                  # the condition on the inputs, before any result
        for top_k in nr.TOP_KS:
            for top_p in nr.TOP_PS[:-1]:
                for r in range(8):
                    n = int(_oracle(V, r, temperature, top_k, top_p)[2].sum())
                    assert n <= nr.undecided_cap(V), f"V={V} top_k={top_k} T={temperature} top_p={top_p} row {r}: {n} undecided entries"
    buf = torch.empty(8 * V + 1, device=DEV)
    for off in (0, 1):                                   # row 0 at a 16-byte boundary, and one float past it
        block = buf[off:off + 8 * V]
        assert block.data_ptr() % 16 == 4 * off
        block.copy_(rows.reshape(-1))
        for M in nr.MS:
            seeds = [(0x9E3779B97F4A7C15 * (r + 1) + V) % 2 ** 64 for r in range(M)]
            steps = [3 * r + M for r in range(M)]
            for top_k in nr.TOP_KS:
                for temperature in nr.TEMPERATURES:
                    plain = _sample(block, M, V, temperature, top_k, None, seeds, steps)
                    for top_p in nr.TOP_PS:
                        out = _sample(block, M, V, temperature, top_k, top_p, seeds, steps)
                        if top_p == 1.0:                 # no nucleus: ia2p_sample_tokens, bit for bit
                            assert _same_bits(out, plain), f"V={V} off={off} M={M} top_k={top_k} T={temperature}: top_p = 1 is not ia2p_sample_tokens"
                            continue
                        tokens, u, probs = out
                        for r in range(M):
                            what = f"V={V} off={off} M={M} top_k={top_k} T={temperature} top_p={top_p} row {r}"
                            got = probs[r] > 0
                            want, cdf = _judge_set(what, rows[r], temperature, got, _oracle(V, r, temperature, top_k, top_p))
                            _judge_draw(what, int(tokens[r]), u[r], got, cdf, seeds[r], steps[r])
                            _judge_probs(what, probs[r].double(), got, want)


def _row_of(masses, V):
    """a logits row whose softmax at temperature 1 is `masses` on its first entries and 0 on the rest"""
    row = torch.full((V,), NEG)
    row[:len(masses)] = torch.log(torch.tensor(masses, dtype=torch.float64)).float()
    return row


def test_a_tied_group_that_straddles_the_boundary_is_kept_whole():
    """0.5, then five entries of 0.1: at top_p = 0.75 the cumulative sum from below passes 0.25 inside the tied group. transformers keeps the part of the group its
    sort put last; the rule keeps all five. At top_p = 0.45 the group as a whole stays under 0.55 and goes as a whole."""
    from instructany2pix_amd.llm import sample_probs
    V = 1000
    row = _row_of([0.5] + [0.1] * 5, V)
    row = row[torch.randperm(V, generator=torch.Generator().manual_seed(1))]
    ties, top = row == row[row > NEG].min(), row == row.max()
    assert int(ties.sum()) == 5 and int(top.sum()) == 1
    assert int((sample_probs(row[None], 1.0, 50, 0.75) > 0).sum()) == 4         # transformers: the maximum and three of the five
    for top_k in (50, 0, 3):                             # 3: the third largest value is the tied one, top-k keeps the group too
        kept, dropped, undecided = nr.oracle(row, 1.0, top_k, 0.75)
        assert torch.equal(kept, ties | top) and not bool(undecided.any())
        tokens, u, probs = _sample(row.to(DEV), 8, V, 1.0, top_k, 0.75, list(range(8)), [0] * 8, ld=0)
        assert torch.equal(probs[0] > 0, ties | top), f"top_k={top_k}: {int((probs[0] > 0).sum())} entries kept, 6 form the nucleus"
        assert torch.allclose(probs[0][ties], torch.full((5,), 0.1)) and abs(float(probs[0][top]) - 0.5) < 1e-6
        _, cdf = nr.distribution(row, 1.0, ties | top)
        for r in range(8):
            _judge_draw(f"top_k={top_k} draw {r}", int(tokens[r]), u[r], ties | top, cdf, r, 0)
        _, _, probs = _sample(row.to(DEV), 1, V, 1.0, top_k, 0.45, [1], [0])
        assert torch.equal(probs[0] > 0, top) and float(probs[0][top]) == 1.0
    # five equal scores and nothing else: the first member alone would close any nucleus, all five stay
    row = _row_of([0.2] * 5, V)
    _, _, probs = _sample(row.to(DEV), 1, V, 1.0, 50, 0.1, [1], [0])
    assert torch.equal(probs[0] > 0, row > NEG) and bool((probs[0][:5] == probs[0][0]).all())


def test_a_dominant_token_is_the_whole_nucleus():
    """two tied maxima of 0.45 each, the rest 0.1 spread over 40 entries: at top_p = 0.6 everything below the maxima sums to 0.1 <= 0.4 and is dropped"""
    V, M = 1000, 256
    row = _row_of([0.45, 0.45] + [0.0025] * 40, V).flip(0).contiguous()
    top = row == row.max()
    kept, _, undecided = nr.oracle(row, 1.0, 50, 0.6)
    assert torch.equal(kept, top) and int(top.sum()) == 2 and not bool(undecided.any())
    for top_k in (50, 0):
        tokens, u, probs = _sample(row.to(DEV), M, V, 1.0, top_k, 0.6, [77] * M, list(range(M)), ld=0)
        assert torch.equal(probs[0] > 0, top) and bool((probs[0][top] == 0.5).all())
        assert set(tokens.tolist()) == {V - 2, V - 1}, f"top_k={top_k}: tokens {sorted(set(tokens.tolist()))}"
        want = torch.tensor([V - 2 if float(sampler_ref.uniform(77, s)) < 0.5 else V - 1 for s in range(M)], dtype=torch.int32)
        assert torch.equal(tokens, want)


def test_the_nucleus_is_taken_after_top_k():
    """0.3, 49 distinct entries of about 0.004 (0.196 together), 950 entries sharing the other 0.504. Of the whole row, top_p = 0.5 keeps everything above
    a boundary inside the 950; of the renormalised top-50 set the 49 are 0.395 <= 0.5 and only the maximum stays. TopK runs first."""
    V = 1000
    small = [0.004 * (1 + 1e-3 * (i - 24)) for i in range(49)]
    rest = (1 - 0.3 - sum(small)) / 950
    row = _row_of([0.3] + small + [rest * (1 + 1e-4 * (i - 475)) for i in range(950)], V)
    row = row[torch.randperm(V, generator=torch.Generator().manual_seed(2))]
    after, _, und_a = nr.oracle(row, 1.0, 50, 0.5)
    whole, _, und_w = nr.oracle(row, 1.0, 0, 0.5)
    assert int(after.sum()) == 1 and int(whole.sum()) > 50 and not bool(und_a.any()) and int(und_w.sum()) <= 1
    _, _, probs = _sample(row.to(DEV), 1, V, 1.0, 50, 0.5, [3], [0])
    assert torch.equal(probs[0] > 0, after) and float(probs[0].max()) == 1.0
    _, _, probs = _sample(row.to(DEV), 1, V, 1.0, 0, 0.5, [3], [0])
    _judge_set("top_k=0", row, 1.0, probs[0] > 0, nr.oracle(row, 1.0, 0, 0.5))


def test_both_ways_to_the_nucleus_meet_at_their_threshold():
    """up to 256 weighted survivors of top-k the kernel finds the nucleus among them in LDS, from 257 on by its passes over the row: 255, 256 and 257 survivors
    by top-k (distinct scores, V = 300) and by the row's length (top_k = 0), and a row whose 300 entries all tie at the k-th value"""
    g = torch.Generator().manual_seed(9)
    cases = [(300, top_k) for top_k in (255, 256, 257)] + [(V, 0) for V in (255, 256, 257)]
    for V, top_k in cases:
        row = torch.randn(V, generator=g)
        assert row.unique().numel() == V
        for top_p in (0.25, 0.6, 0.9):
            oracle = nr.oracle(row, 1.0, top_k, top_p)
            assert int(oracle[2].sum()) <= 1
            tokens, u, probs = _sample(row.to(DEV), 8, V, 1.0, top_k, top_p, list(range(8)), [V] * 8, ld=0)
            what = f"V={V} top_k={top_k} top_p={top_p}"
            got = probs[0] > 0
            want, cdf = _judge_set(what, row, 1.0, got, oracle)
            _judge_probs(what, probs[0].double(), got, want)
            for r in range(8):
                _judge_draw(f"{what} draw {r}", int(tokens[r]), u[r], got, cdf, r, V)
    row = torch.full((300,), -1.5)
    _, _, probs = _sample(row.to(DEV), 1, 300, 1.0, 50, 0.25, [1], [0])
    assert bool((probs[0] == probs[0, 0]).all()) and abs(float(probs[0, 0]) * 300 - 1) < 1e-6


def test_edge_rows():
    V = 1000
    rows = nr.rows(V)
    block = rows[2].to(DEV)                              # a third of the row is -inf
    for top_k in (0, 50, 900):                           # 900 > the finite entries: top-k keeps everything, at weight 0
        tokens, u, probs = _sample(block, 8, V, 1.0, top_k, 0.6, list(range(40, 48)), [0] * 8, ld=0)
        got = probs[0] > 0
        want, cdf = _judge_set(f"top_k={top_k}", rows[2], 1.0, got, nr.oracle(rows[2], 1.0, top_k, 0.6))
        assert not bool(got[rows[2] == NEG].any())
        for r in range(8):
            assert rows[2][int(tokens[r])] != NEG
            _judge_draw(f"top_k={top_k} draw {r}", int(tokens[r]), u[r], got, cdf, 40 + r, 0)
    bad = rows.clone()
    bad[1, 999] = float("nan")
    bad[3, 0] = float("inf")
    bad[5] = NEG
    bad[6, 500] = float("nan")
    bad[6, 501] = float("inf")
    for do_sample in (1, 0):
        tokens, _, _ = _sample(bad.to(DEV), 8, V, 0.3, 50, 0.6, list(range(8)), [0] * 8, do_sample=do_sample, probs=False)
        assert [int(t) for t in tokens[[1, 3, 5, 6]]] == [-1] * 4 and all(int(t) >= 0 for t in tokens[[0, 2, 4, 7]]), tokens
    # argmax ignores top_p
    greedy = _sample(rows.to(DEV), 8, V, 1.0, 50, 0.25, None, None, do_sample=0, probs=False)
    assert _same_bits(greedy, _sample(rows.to(DEV), 8, V, 1.0, 50, None, None, None, do_sample=0, probs=False))
    assert greedy[0].tolist() == [0 if r == 3 else int(rows[r].argmax()) for r in range(8)]          # (row 3: all equal, the lowest index)


def test_the_nucleus_does_not_depend_on_launch_batch_or_alignment():
    for V in (51, 32003):
        rows = nr.rows(V)
        buf = torch.empty(8 * V + 1, device=DEV)
        for top_k in (50, 0):
            outs = []
            for off in (0, 1):
                block = buf[off:off + 8 * V]
                block.copy_(rows.reshape(-1))
                a = _sample(block, 8, V, 0.3, top_k, 0.6, list(range(1, 9)), list(range(8)))
                b = _sample(block, 8, V, 0.3, top_k, 0.6, list(range(1, 9)), list(range(8)))
                assert _same_bits(a, b), f"V={V} top_k={top_k} off={off}: two launches differ"
                outs.append(a)
                for r in (1, 5):                         # a row alone: another workgroup index, M = 1
                    alone = _sample(block[r * V:(r + 1) * V], 1, V, 0.3, top_k, 0.6, [r + 1], [r])
                    assert int(alone[0][0]) == int(a[0][r]) and torch.equal(alone[2][0].view(torch.int32), a[2][r].view(torch.int32)), (V, top_k, off, r)
            assert _same_bits(outs[0], outs[1]), f"V={V} top_k={top_k}: the result depends on the alignment of the block"


def test_4096_draws_of_one_row_in_one_launch():
    V, M, seed = 1000, 4096, 0xC0FFEE123456789
    row = nr.rows(V)[0]
    block = row.to(DEV)
    _, _, one = _sample(block, 1, V, 1.0, 50, 0.6, [seed], [0])
    got = one[0] > 0
    probs, cdf = _judge_set("row 0", row, 1.0, got, _oracle(V, 0, 1.0, 50, 0.6))
    tokens, u, _ = _sample(block, M, V, 1.0, 50, 0.6, [seed] * M, list(range(M)), ld=0, probs=False)
    for r in range(M):
        _judge_draw(f"draw {r}", int(tokens[r]), u[r], got, cdf, seed, r)
    first = _sample(block, 8, V, 1.0, 50, 0.6, [seed] * 8, list(range(8)), ld=0, probs=False)
    assert torch.equal(first[0], tokens[:8]) and torch.equal(first[1], u[:8])
    counts = torch.bincount(tokens.long(), minlength=V).double()
    assert float(((counts / M - probs) ** 2).sum()) < 4.0 / M and int((counts > 0).sum()) <= int(got.sum()) < 50


# ---- on the tiny LLaMA configuration ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    from instructany2pix_amd.weights import llm_param_specs, synthetic_state_dict
    from test_llm_gpu import _ids
    cfg = tiny_llm()
    lm = HipInstructAny2PixLM(cfg, DEV, max_positions=128, video_token_id=cfg.vocab_size - 3, max_batch=4)
    lm.load_state_dict(synthetic_state_dict(llm_param_specs(cfg, cfg.embed_dim, "linear"), seed=21))
    lm.prompts = [_ids(T, 503, 40 + T)[None] for T in (5, 12, 33, 7)]
    return lm


def _same_output(a, b):
    return torch.equal(a.sequences, b.sequences) and len(a.hidden_states) == len(b.hidden_states) and all(
        torch.equal(x[-1][:, -1:], y[-1][:, -1:]) for x, y in zip(a.hidden_states, b.hidden_states))


def test_generate_equals_a_loop_driven_through_the_nucleus_sampler(tiny):
    from instructany2pix_amd import _ffi
    lm, lib = tiny, tiny._lib
    prompt, seed, new = lm.prompts[1], 0x1234567890ABCDEF, 9
    out = lm.generate(prompt, do_sample=True, temperature=1.0, top_k=20, top_p=0.6, max_new_tokens=new, sampler="device", seed=seed)
    lm.reset()
    hid, logits = lm.prefill(lm.embed_tokens(prompt.reshape(-1)))
    tok = torch.zeros(1, dtype=torch.int32, device=DEV)
    seq, rows = prompt.reshape(-1).tolist(), []
    for step in range(new):
        rows.append(hid)
        _ffi.check(lib.ia2p_sample_tokens_p(_ffi.current_stream(), _ffi.ptr(logits), logits.numel(), 1, logits.numel(), 1.0, 20, 0.6, 1, (C.c_uint64 * 1)(seed),
                                            (C.c_uint32 * 1)(step), _ffi.ptr(tok), None, None), None, llm=True)
        seq.append(int(tok.item()))
        if step + 1 < new:
            hid, logits = lm.decode(seq[-1])
    assert out.sequences[0].tolist() == seq
    assert all(torch.equal(h[-1][:, -1:].reshape(-1), r) for h, r in zip(out.hidden_states, rows))
    plain = lm.generate(prompt, do_sample=True, temperature=1.0, top_k=20, max_new_tokens=new, sampler="device", seed=seed)
    assert _same_output(plain, lm.generate(prompt, do_sample=True, temperature=1.0, top_k=20, top_p=1.0, max_new_tokens=new, sampler="device", seed=seed))


def test_a_batch_gives_every_request_its_serial_tokens_under_top_p(tiny):
    lm, seeds = tiny, [11, 2 ** 63 + 5, 0xDEADBEEFCAFE, 7]
    kw = dict(do_sample=True, temperature=1.0, top_k=50, top_p=0.6, max_new_tokens=10, sampler="device")
    serial = [lm.generate(p, seed=s, **kw) for p, s in zip(lm.prompts, seeds)]
    outs = lm.generate_batch(lm.prompts, seeds=seeds, **kw)
    for i, (o, s) in enumerate(zip(outs, serial)):
        assert _same_output(o, s), f"request {i} in a batch of four differs from generate(seed={seeds[i]}, top_p=0.6)"


def test_the_host_sampler_stays_inside_the_nucleus(tiny, monkeypatch):
    from instructany2pix_amd import llm as L
    lm, seen = tiny, []
    real = L.sample_next

    def spy(logits, do_sample=True, temperature=0.3, top_k=50, top_p=1.0):
        t = real(logits, do_sample, temperature, top_k, top_p)
        seen.append((logits.reshape(-1).clone(), int(t), temperature, top_k, top_p))
        return t

    monkeypatch.setattr(L, "sample_next", spy)
    torch.manual_seed(0)
    out = lm.generate(lm.prompts[0], do_sample=True, temperature=1.0, top_k=50, top_p=0.25, max_new_tokens=64, sampler="host")
    assert len(seen) == 64 and out.sequences.shape[1] == lm.prompts[0].shape[1] + 64
    sizes = []
    for step, (row, t, temperature, top_k, top_p) in enumerate(seen):
        assert (temperature, top_k, top_p) == (1.0, 50, 0.25)
        kept, dropped, _ = nr.oracle(row, temperature, top_k, top_p)
        assert not bool(dropped[t]), f"step {step}: token {t} lies outside the nucleus"
        sizes.append(int(kept.sum()))
    assert max(sizes) < 50, "top_p = 0.25 never narrowed the 50 candidates of top-k"


def test_a_loaded_generation_config_is_used_when_the_call_passes_no_top_p(tiny, monkeypatch):
    lm = tiny
    kw = dict(do_sample=True, temperature=1.0, max_new_tokens=12, sampler="device", seed=5)
    plain, narrow = lm.generate(lm.prompts[2], **kw), lm.generate(lm.prompts[2], top_p=0.25, **kw)
    assert not torch.equal(plain.sequences, narrow.sequences), "top_p = 0.25 drew the tokens of top_p = 1 (choose another seed: the test needs them to differ)"
    monkeypatch.setattr(lm, "generation_defaults", dict(lm.generation_defaults))
    lm.load_generation_config({"temperature": 0.9, "top_p": 0.25})
    assert _same_output(lm.generate(lm.prompts[2], **kw), narrow)
    assert _same_output(lm.generate(lm.prompts[2], top_p=1.0, **kw), plain)            # the keyword wins
    assert _same_output(lm.generate_batch([lm.prompts[2]], do_sample=True, temperature=1.0, max_new_tokens=12, sampler="device", seeds=[5])[0], narrow)
