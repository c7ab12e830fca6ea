"""Float64 reference of the nucleus rule of `ia2p_sample_tokens_p` (include/ia2p.h), and the inputs the nucleus tests share.

The rule: K = the set top-k keeps (ties included), e_i = exp(score_i - max) over K, Z their sum, T(v) = the sum of e_i over the i in K with score_i <= v; index i
is in the nucleus iff e_i > 0 and T(score_i) > (1 - top_p) * Z. The scores and K are fp32 torch's (`logits / temperature`, `scores >= the k-th largest`), as in
tests/sampler_ref.py; everything after them is float64. The kernel sums its terms as integers (no summation order, depth D = 1: each term is rounded once, see the
header of csrc/sample.hip), so what separates its T / Z from this one is the error of its fp32 terms: an entry with |T / Z - (1 - top_p)| <= BAND is left
undecided, BAND = 2 * (D + 2) * 2^-24, and either answer is accepted for it; every other entry is decided."""
import torch

D = 1                                    # summation depth of the kernel's nucleus sums (csrc/sample.hip, header comment)
BAND = 2 * (D + 2) * 2.0 ** -24
NEG = -float("inf")
VS = (50, 51, 1000, 32003)
MS = (1, 3, 8)
TOP_KS = (50, 0)
TEMPERATURES = (0.3, 1.0)
TOP_PS = (0.25, 0.6, 0.9, 1.0)


def rows(V):
    """the rows of tests/test_sampler_gpu.py::_rows, restated: 0 random normal, 1 with its 50th to 54th largest values equal, 2 with -inf entries, 3 all equal,
    4-7 random normal at other scales"""
    g = torch.Generator().manual_seed(100 + V)
    out = torch.randn(8, V, generator=g) * torch.tensor([1.0, 1.0, 1.0, 0.0, 0.5, 1.5, 0.25, 1.25])[:, None]
    order = torch.argsort(out[1], descending=True)
    out[1, order[49:min(54, V)]] = float(out[1, order[49]])
    out[2, torch.randperm(V, generator=g)[:V // 3]] = NEG
    out[3] = 0.625
    return out.contiguous()


def scores_and_topk(row, temperature, top_k):
    """-> (fp32 scores [V], bool [V]: the set top-k keeps), both as `llm.sample_probs` has them"""
    row = row.detach().float().cpu().reshape(-1)
    scores = row / temperature
    k = int(top_k) if top_k and 0 < int(top_k) < row.numel() else None
    return scores, (torch.ones_like(scores, dtype=torch.bool) if k is None else scores >= torch.topk(scores, k)[0][-1])


def ratio(row, temperature, top_k):
    """-> (scores, K, e float64 [V] (0 outside K), T(score_i) / Z float64 [V] (0 outside K))"""
    scores, K = scores_and_topk(row, temperature, top_k)
    s64 = scores.double()
    e = torch.where(K, torch.exp(s64 - s64[K].max()), torch.zeros_like(s64))
    order = torch.argsort(scores, stable=True)                        # ascending; entries outside K carry 0 and move nothing
    cum = torch.cumsum(e[order], 0)
    _, inverse, counts = torch.unique_consecutive(scores[order], return_inverse=True, return_counts=True)
    last = torch.cumsum(counts, 0) - 1                                # the last sorted position of every group of equal scores: T takes the whole group in
    T = torch.empty_like(e)
    T[order] = cum[last[inverse]]
    return scores, K, e, torch.where(K, T / e.sum(), torch.zeros_like(T))


def oracle(row, temperature, top_k, top_p, band=BAND):
    """one fp32 logits row -> (kept, dropped, undecided), bool [V] each and disjoint: the entries decided to be in the nucleus, decided to be outside it (everything
    top-k removes and every entry of weight 0 included), and those within `band` of the boundary"""
    _, K, e, r = ratio(row, temperature, top_k)
    live = K & (e > 0)
    gap = r - (1.0 - float(top_p))
    undecided = live & (gap.abs() <= band)
    kept = live & (gap > band)
    return kept, ~(kept | undecided), undecided


def distribution(row, temperature, kept):
    """the float64 softmax of the fp32 scores over a given kept set -> (probs float64 [V], cdf over the kept entries in index order [K])"""
    scores = row.detach().float().cpu().reshape(-1) / temperature
    s64 = scores.double()
    e = torch.where(kept, torch.exp(s64 - s64[kept].max()), torch.zeros_like(s64))
    probs = e / e.sum()
    return probs, torch.cumsum(probs[kept], 0)


def undecided_cap(V):
    """how many undecided entries a row of the shared inputs may have: a condition on the inputs, asserted before any result is looked at"""
    return 0 if V <= 51 else 8
