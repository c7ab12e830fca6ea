"""`ia2p_sample_tokens` against `llm.sample_probs` and the Philox restatement of tests/sampler_ref.py.

A draw cannot be compared token for token with torch (another generator, another summation order), so every draw is judged by what defines it: the token
lies in the kept set of `sample_probs`, and the row's uniform u falls into the token's interval of the float64 cumulative distribution,
`cdf[t-1] - tol <= u < cdf[t] + tol` with tol = 4 * K_kept * 2^-24 (the bound on an fp32 sum of K_kept terms in any association, the error of `exp` inside
it). u itself must be the restatement's, bit for bit, and `probs_out` exactly 0 outside the kept set and within 1e-5 relative inside it."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VS = (50, 51, 1000, 32003)
MS = (1, 3, 8)
TOP_KS = (50, 0, None)          # None stands for V + 7
TEMPERATURES = (0.3, 1.0)
NEG = -float("inf")


def _lib():
    from instructany2pix_amd import _ffi
    return _ffi, _ffi.lib()


def _rows(V):
    """8 logits rows: 0 random normal, 1 with its 50th to 54th largest values equal, 2 with -inf entries, 3 all equal, 4-7 random normal at other scales"""
    g = torch.Generator().manual_seed(100 + V)
    rows = torch.randn(8, V, generator=g) * torch.tensor([1.0, 1.0, 1.0, 0.0, 0.5, 1.5, 0.25, 1.25])[:, None]
    order = torch.argsort(rows[1], descending=True)
    rows[1, order[49:min(54, V)]] = float(rows[1, order[49]])
    rows[2, torch.randperm(V, generator=g)[:V // 3]] = NEG
    rows[3] = 0.625
    return rows.contiguous()


def _sample(block, M, V, temperature, top_k, seeds, steps, ld=None, do_sample=1, probs=True):
    """block: device tensor whose data pointer is row 0 -> (tokens [M], u [M], probs [M, V] or None) on the host"""
    ffi, lib = _lib()
    tokens = torch.full((M,), -7, dtype=torch.int32, device=DEV)
    u = torch.full((M,), -1.0, device=DEV)
    p = torch.full((M, V), float("nan"), device=DEV) if probs else None
    st = lib.ia2p_sample_tokens(ffi.current_stream(), C.c_void_p(block.data_ptr()), V if ld is None else ld, M, V, temperature, top_k, do_sample,
                                (C.c_uint64 * M)(*seeds) if seeds else None, (C.c_uint32 * M)(*steps) if steps else None, ffi.ptr(tokens), ffi.ptr(p), ffi.ptr(u))
    ffi.check(st, None, llm=True)
    torch.cuda.synchronize()
    return tokens.cpu(), u.cpu(), None if p is None else p.cpu()


_ORACLE = {}


def _oracle(V, r, temperature, top_k):
    key = (V, r, temperature, top_k)
    if key not in _ORACLE:
        _ORACLE[key] = sampler_ref.oracle(_rows(V)[r], temperature, top_k)
    return _ORACLE[key]


def _judge(what, t, u, kept, cdf, seed, step):
    assert float(u) == float(sampler_ref.uniform(seed, step)), f"{what}: u = {float(u)!r}, the restatement gives {float(sampler_ref.uniform(seed, step))!r}"
    assert 0 <= t < kept.numel() and bool(kept[t]), f"{what}: token {t} is outside the kept set"
    rank = int(kept[:t].sum())
    lo, hi = (float(cdf[rank - 1]) if rank else 0.0), float(cdf[rank])
    tol = 4 * cdf.numel() * 2.0 ** -24
    assert lo - tol <= float(u) < hi + tol, f"{what}: u = {float(u)} outside [{lo}, {hi}) of token {t} (tol {tol})"


@pytest.mark.parametrize("V", VS)
def test_every_draw_inverts_the_float64_cdf(V):
    rows = _rows(V)
    buf = torch.empty(8 * V + 1, device=DEV)
    for off in (0, 1):                                   # row 0 at a 16-byte boundary, and one float past it
        block = buf[off:off + 8 * V]
        assert block.data_ptr() % 16 == 4 * off
        block.copy_(rows.reshape(-1))
        for M in MS:
            for tk in TOP_KS:
                top_k = V + 7 if tk is None else tk
                for temperature in TEMPERATURES:
                    seeds = [(0x9E3779B97F4A7C15 * (r + 1) + V) % 2 ** 64 for r in range(M)]
                    steps = [3 * r + M for r in range(M)]
                    tokens, u, probs = _sample(block, M, V, temperature, top_k, seeds, steps)
                    for r in range(M):
                        kept, want, cdf = _oracle(V, r, temperature, top_k)
                        what = f"V={V} off={off} M={M} top_k={top_k} T={temperature} row {r}"
                        _judge(what, int(tokens[r]), u[r], kept, cdf, seeds[r], steps[r])
                        got = probs[r].double()
                        assert bool((got[~kept] == 0).all()), f"{what}: weight outside the kept set"
                        assert bool(((got - want).abs() <= 1e-5 * want)[kept].all()), f"{what}: probs_out off by {float(((got - want).abs() / want)[kept & (want > 0)].max())} relative"


def test_ties_at_the_kth_value_are_all_kept():
    for V, n in ((51, 51), (1000, 54), (32003, 54)):
        kept, _, _ = _oracle(V, 1, 0.3, 50)
        assert int(kept.sum()) == n                        # the oracle's own count (TopKLogitsWarper removes nothing equal to the k-th value)
        _, _, probs = _sample(_rows(V)[1].to(DEV), 1, V, 0.3, 50, [5], [0])
        assert int((probs[0] > 0).sum()) == n, f"V={V}: {int((probs[0] > 0).sum())} entries kept, {n} tie at or above the 50th value"
        assert torch.equal(probs[0] > 0, kept)
    kept, _, _ = _oracle(1000, 3, 1.0, 50)                 # all equal: every entry ties with the 50th
    _, _, probs = _sample(_rows(1000)[3].to(DEV), 1, 1000, 1.0, 50, [5], [0])
    assert int(kept.sum()) == 1000 and bool((probs[0] == probs[0, 0]).all()) and abs(float(probs[0, 0]) - 1e-3) < 1e-8


def test_minus_infinity_is_never_drawn():
    V = 1000
    row = _rows(V)[2]
    block = row.to(DEV)
    for top_k in (0, 50, 900):                             # 900 > the finite entries: the 900th largest value is -inf, everything is kept at weight 0
        kept, _, cdf = _oracle(V, 2, 1.0, top_k)
        tokens, u, probs = _sample(block, 8, V, 1.0, top_k, list(range(40, 48)), [0] * 8, ld=0)
        assert bool((probs[0][row == NEG] == 0).all())
        for r in range(8):
            assert row[int(tokens[r])] != NEG
            _judge(f"top_k={top_k} draw {r}", int(tokens[r]), u[r], kept, cdf, 40 + r, 0)


def test_a_draw_at_the_top_of_the_unit_interval_takes_the_last_entry_with_weight():
    """u = 1 - 2^-23 (seed 2024, counter 6020551, found by running the restatement over the counters) on a row of ten finite entries followed by 990 kept -inf
    entries (top_k = 0 keeps everything). Entry 9 carries 2^-21 of the weight: u lies in its interval and it must be drawn, by the cumulative sum or by the
    rule for a sum that rounding leaves short -- never one of the -inf entries behind it. With 2^-30 on entry 9 instead, u lies in entry 8's interval."""
    import math
    V, seed, step = 1000, 2024, 6020551
    assert float(sampler_ref.uniform(seed, step)) == 1.0 - 2.0 ** -23
    for weight, want in ((2.0 ** -21, 9), (2.0 ** -30, 8)):
        row = torch.full((V,), NEG)
        row[:9] = 0.0
        row[9] = math.log(9 * weight / (1 - weight))
        kept, probs, cdf = sampler_ref.oracle(row, 1.0, 0)
        assert int(kept.sum()) == V and abs(float(probs[9]) / weight - 1) < 1e-6
        for top_k in (0, 5):                                 # 5: the 5th largest value is 0.0, entries 0..8 tie with it and entry 9 falls out
            tokens, u, p = _sample(row.to(DEV), 1, V, 1.0, top_k, [seed], [step])
            t = int(tokens[0])
            assert float(u[0]) == 1.0 - 2.0 ** -23 and row[t] != NEG and bool((p[0][10:] == 0).all())
            assert t == (want if top_k == 0 else 8), f"weight {weight}, top_k {top_k}: token {t}"


def test_misaligned_outputs_are_refused():
    ffi, lib = _lib()
    x, t, f = torch.zeros(16, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(64, device=DEV)
    s1, t1 = (C.c_uint64 * 1)(1), (C.c_uint32 * 1)(0)
    for probs, u in ((f.data_ptr() + 2, None), (None, f.data_ptr() + 1)):
        assert lib.ia2p_sample_tokens(ffi.current_stream(), ffi.ptr(x), 16, 1, 16, 1.0, 0, 1, s1, t1, ffi.ptr(t), probs, u) == 1
    assert lib.ia2p_sample_tokens(ffi.current_stream(), ffi.ptr(x), 16, 1, 16, 1.0, 0, 1, s1, t1, ffi.ptr(t), ffi.ptr(f), ffi.ptr(f[32:])) == 0
    torch.cuda.synchronize()


def test_4096_draws_of_one_row_in_one_launch():
    """ld = 0: every workgroup reads the same row; seeds and steps of 4096 rows go through the launcher's staging copy. The first eight draws are also made
    by a launch of eight rows (ids by value): the two paths give the same tokens."""
    V, M, seed = 1000, 4096, 0xC0FFEE123456789
    block = _rows(V)[0].to(DEV)
    kept, probs, cdf = _oracle(V, 0, 1.0, 50)
    tokens, u, _ = _sample(block, M, V, 1.0, 50, [seed] * M, list(range(M)), ld=0, probs=False)
    for r in range(M):
        _judge(f"draw {r}", int(tokens[r]), u[r], kept, cdf, seed, r)
    first, u8, _ = _sample(block, 8, V, 1.0, 50, [seed] * 8, list(range(8)), ld=0, probs=False)
    assert torch.equal(first, tokens[:8]) and torch.equal(u8, u[:8])
    # 4096 inversions of the cdf: the counts follow the distribution (50 kept tokens; a wrong interval map would not)
    counts = torch.bincount(tokens.long(), minlength=V).double()
    assert float(((counts / M - probs) ** 2).sum()) < 4.0 / M and int((counts > 0).sum()) <= 50


def test_two_launches_give_the_same_bits():
    for V in (51, 32003):
        block = _rows(V).to(DEV)
        for top_k in (50, 0):
            a = _sample(block, 8, V, 0.3, top_k, list(range(1, 9)), list(range(8)))
            b = _sample(block, 8, V, 0.3, top_k, list(range(1, 9)), list(range(8)))
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
            # a row alone (16-byte aligned, another workgroup index) draws what it draws inside the block
            for r in (1, 5):
                alone = _sample(block[r].clone(), 1, V, 0.3, top_k, [r + 1], [r])
                assert int(alone[0][0]) == int(a[0][r]) and torch.equal(alone[2][0].view(torch.int32), a[2][r].view(torch.int32)), (V, top_k, r)


def test_argmax_takes_the_lowest_index_of_a_duplicated_maximum():
    for V in VS:
        rows = _rows(V)
        top = float(rows.max()) + 1.0
        rows[0, [V - 1, V // 2, 7]] = top                  # three maxima: index 7 is the answer
        rows[1, V - 1] = top
        rows[2, [V - 2, V - 1]] = top
        tokens, _, _ = _sample(rows.to(DEV), 8, V, 1.0, 50, None, None, do_sample=0, probs=False)
        want = [7, V - 1, V - 2, 0] + [int(rows[r].argmax()) for r in range(4, 8)]
        assert tokens.tolist() == want, f"V={V}"


def test_rows_that_cannot_be_sampled_give_minus_one():
    V = 1000
    rows = _rows(V)
    rows[1, 999] = float("nan")
    rows[3, 0] = float("inf")
    rows[5] = NEG
    rows[6, 500] = float("nan")
    rows[6, 501] = float("inf")
    for do_sample in (1, 0):
        tokens, _, _ = _sample(rows.to(DEV), 8, V, 0.3, 50, list(range(8)), [0] * 8, do_sample=do_sample, probs=False)
        assert [int(t) < 0 for t in tokens] == [False, True, False, True, False, True, True, False], tokens
        assert all(int(t) == -1 for t in tokens[[1, 3, 5, 6]])
