"""fp64 reference of the automatic edit mask (include/ia2p.h, "Automatic edit mask", steps 5 - 7), in numpy: the written-out rule, nothing of the code under test.
Shared by tests/test_auto_mask_cpu.py (hand cases, mutants, the bound itself) and tests/test_auto_mask_gpu.py (against the HIP kernels).

The error bound, from the operations read in csrc/auto_mask.hip, u = 2^-24 per fp32 operation, gamma_k = k u / (1 - k u):
  map   one __fsub_rn of two fp16 values (their exact difference can need more than 24 bits), fabsf (exact), n C sequential __fadd_rn (the first, onto 0, is exact; counted
        anyway), the host's fp32(1 / (n C)) and one __fmul_rn by it:                                   |map - map_ref| <= gamma_(n C + 3) map_ref
  mean  the sum of the computed map values over the kernel's own tree -- 4 ceil(HW / 4096) sequential additions per thread, 6 butterfly levels, 15 additions of the wave
        totals: depth D(HW) -- of non-negative terms, fp32(HW) (exact below 2^24; counted) and one __fdiv_rn:   |mean - mean_ref| <= gamma_(n C + 3 + D + 2) mean_ref
  tau   0.5 rho is exact, one __fmul_rn:                                                               |tau - tau_ref| <= gamma_(n C + D + 6) tau_ref
A cell is decision-certain when |map_ref - tau_ref| exceeds the sum of the map's and tau's bounds: there every correctly rounded evaluation in the kernel's order decides
as the reference does."""
import math

import numpy as np

U = 2.0 ** -24

# (B, n, C, h, w) of the real-valued cases: the issue's six, then the sizes at which the kernels first take another path --
#   HW = 2049: the second workgroup of a row in the map kernel (256 threads x 8 pixels);
#   HW = 4097 = 17 x 241: the second iteration of the mean's per-thread loop (1024 threads x 4 values per pass), at B = 2 with row 1 off the 16-byte grid;
#   HW = 8193 = 3 x 2731: the second iteration of the mask kernel's output loop (1024 threads x 8 cells per pass)
REAL_CASES = ((1, 1, 1, 1, 2), (1, 2, 4, 1, 63), (1, 3, 4, 1, 65), (2, 4, 4, 16, 16), (3, 8, 4, 33, 33), (2, 8, 4, 64, 64),
              (1, 1, 2, 1, 2049), (2, 1, 2, 17, 241), (1, 1, 1, 3, 2731))
LATTICE_CASES = ((1, 2, 4, 8, 8), (2, 8, 4, 8, 8), (1, 2, 4, 16, 16), (3, 8, 4, 16, 16), (1, 2, 4, 64, 64), (2, 8, 4, 64, 64))      # n C in {8, 32}, HW in {64, 256, 4096}


def gamma(k):
    return k * U / (1.0 - k * U)


def reduction_depth(HW):
    """additions on the longest path of the mean's tree in contrast_mask_kernel"""
    return 4 * math.ceil(HW / 4096) + 6 + 15


def contrast_map_ref(tgt, src):
    """[B, n, C, h, w] x 2 -> float64 [B, h, w]: (1 / (n C)) sum_k sum_c |tgt - src|"""
    t, s = np.asarray(tgt, np.float64), np.asarray(src, np.float64)
    return np.abs(t - s).sum(axis=(1, 2)) / (t.shape[1] * t.shape[2])


def threshold_ref(cmap, ratio):
    """float64 [B, h, w], one ratio per request -> (stats float64 [B, 2] = (mean, tau), m bool [B, h, w]); the ratio is the fp32 value the launch carries; strict"""
    cmap = np.asarray(cmap, np.float64)
    B = cmap.shape[0]
    rho = np.broadcast_to(np.asarray(ratio, np.float32), (B,)).astype(np.float64)
    mean = cmap.reshape(B, -1).sum(axis=1) / (cmap.shape[1] * cmap.shape[2])
    tau = 0.5 * rho * mean
    return np.stack([mean, tau], axis=1), cmap > tau[:, None, None]


def dilate_ref(m, d):
    """bool [B, h, w], one d per request -> bool: the max over |dy|, |dx| <= d; cells outside the grid count 0, no wrap"""
    m = np.asarray(m, bool)
    B, h, w = m.shape
    ds = np.broadcast_to(np.asarray(d, np.int64), (B,))
    out = np.zeros_like(m)
    for b in range(B):
        r = int(ds[b])
        pad = np.zeros((h + 2 * r, w + 2 * r), bool)
        pad[r:r + h, r:r + w] = m[b]
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                out[b] |= pad[dy:dy + h, dx:dx + w]
    return out


def auto_mask_ref(tgt, src, ratio=3.0, dilate=1):
    """-> (map float64 [B, h, w], stats float64 [B, 2], m bool (before dilation), mask float16 [B, 1, h, w])"""
    cmap = contrast_map_ref(tgt, src)
    stats, m = threshold_ref(cmap, ratio)
    return cmap, stats, m, dilate_ref(m, dilate).astype(np.float16)[:, None]


def bounds(cmap, stats, nC):
    """-> (map bound [B, h, w], mean bound [B], tau bound [B]) for real-valued inputs, as derived in the module docstring"""
    HW = cmap.shape[1] * cmap.shape[2]
    D = reduction_depth(HW)
    return gamma(nC + 3) * np.abs(cmap), gamma(nC + D + 5) * np.abs(stats[:, 0]), gamma(nC + D + 6) * np.abs(stats[:, 1])


def certain(cmap, stats, nC):
    """bool [B, h, w]: the cells whose decision no rounding within the bounds can change"""
    bm, _, bt = bounds(cmap, stats, nC)
    return np.abs(cmap - stats[:, 1][:, None, None]) > bm + bt[:, None, None]


def max_uncertain(HW):
    return max(1, HW // 1000)


def real_case(B, n, C, h, w, seed):
    """the issue's inputs: a = randn.half(), b = (a + amp randn).half(), amp uniform in [0, 4] per pixel -> (tgt, src) float16 [B, n, C, h, w]"""
    g = np.random.default_rng(seed)
    a = g.standard_normal((B, n, C, h, w)).astype(np.float16)
    amp = g.uniform(0.0, 4.0, (B, 1, 1, h, w))
    b = (a.astype(np.float64) + amp * g.standard_normal((B, n, C, h, w))).astype(np.float16)
    return b, a


def lattice_case(B, n, C, h, w, seed):
    """integers in [-3, 3] times 2^-2: every sum of the rule is exact in fp32 (|diff| <= 1.5 in units of 2^-2, at most 32 of them; the map in units of 2^-7, at most 4096
    values below 2^8 units; mean and tau = 1.5 mean keep fewer than 24 bits)"""
    g = np.random.default_rng(seed)
    mk = lambda: (g.integers(-3, 4, (B, n, C, h, w)) * 0.25).astype(np.float16)
    tgt, src = mk(), mk()
    same = g.random((B, 1, 1, h, w)) < 0.7                     # the predictions agree on 70 % of the pixels: the rest stands out above 1.5 x the mean
    return np.where(same, src, tgt), src


def tie_case(n, C, h, w):
    """a lattice case built to hold ties at tau: src = 0, tgt = v[p] on every (k, c), v cycling through (0, 0, 0, 0.25, 0.75, 0.75, 0.75, 1.5): the map is v, its mean 0.5,
    tau = 1.5 * 0.5 = 0.75 at ratio 3 -- the cells at 0.75 tie (0, strictly), the cells at 1.5 are on"""
    v = np.resize(np.array([0, 0, 0, 0.25, 0.75, 0.75, 0.75, 1.5]), h * w).reshape(h, w)
    assert (h * w) % 8 == 0
    tgt = np.broadcast_to(v, (1, n, C, h, w)).astype(np.float16)
    return tgt, np.zeros_like(tgt)


def kernel_order_fp32(tgt, src, ratio):
    """The kernels' own evaluation order replayed in numpy float32 (every operation rounded once): -> (map float32 [B, h, w], stats float32 [B, 2]). What the bound has to
    cover; tests/test_auto_mask_cpu.py holds it against the reference without a GPU."""
    f = np.float32
    t, s = np.asarray(tgt, np.float32), np.asarray(src, np.float32)
    B, n, C, h, w = t.shape
    acc = np.zeros((B, h, w), f)
    for k in range(n):
        for c in range(C):
            acc = (acc + np.abs((t[:, k, c] - s[:, k, c]).astype(f))).astype(f)
    cmap = (acc * f(f(1.0) / f(n * C))).astype(f)
    HW = h * w
    stats = np.zeros((B, 2), f)
    for b in range(B):
        row = np.zeros(math.ceil(HW / 4096) * 4096, f)
        row[:HW] = cmap[b].reshape(-1)
        part = np.zeros(1024, f)
        for j in range(len(row) // 4096):                      # thread t: the groups of 4 at (j 1024 + t) 4, in index order
            blk = row[j * 4096:(j + 1) * 4096].reshape(1024, 4)
            for e in range(4):
                part = (part + blk[:, e]).astype(f)
        lanes = part.reshape(16, 64)
        for o in (32, 16, 8, 4, 2, 1):                         # xor-butterfly: every lane ends with the wave's total
            lanes = (lanes + lanes[:, np.arange(64) ^ o]).astype(f)
        total = lanes[0, 0]
        for wv in range(1, 16):
            total = f(total + lanes[wv, 0])
        mean = f(total / f(HW))
        stats[b] = (mean, f(f(f(0.5) * f(np.broadcast_to(np.asarray(ratio, f), (B,))[b])) * mean))
    return cmap, stats
