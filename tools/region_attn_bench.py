"""`ia2p_attention_regions` against its yardstick at SDXL's two cross-attention shapes of a 1024 x 1024 request under CFG (B = 2: 10 heads x 4096 queries, 20 heads x 1024
queries; 77 text keys) for G in {1, 3, 8} token groups. The yardstick is the two-segment `ia2p_attention` at n1 = 4 G with the scale carried in w1: the same K / V
traffic and the same MFMA work (what it lacks: the [B, G, Nq] mask weights, the per-group softmaxes and coefficients). The two launches alternate train by train in
this one process: microseconds per launch between two device events around TRAIN back-to-back launches (the Python call included), median (min, max) of REPS trains
each, after a warm-up of both. The outputs of the two agree where every mask is 1 and G = 1 (checked before the clock: the formulas coincide there).

    python tools/region_attn_bench.py [--train 200] [--reps 7]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instructany2pix_amd import _ffi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--train", type=int, default=200)
ap.add_argument("--reps", type=int, default=7)
A = ap.parse_args()
DEV = "cuda:0"
L = _ffi.lib()
s = _ffi.current_stream()
p = lambda t, off=0: C.c_void_p(t.data_ptr() + 2 * off)      # noqa: E731
g = torch.Generator().manual_seed(5)
rn = lambda *sh: torch.randn(*sh, generator=g).half().to(DEV)      # noqa: E731


def train(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(A.train):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / A.train


print(f"# B = 2, 77 text keys, IP scale 0.8; us per launch incl. the Python call, median (min, max) of {A.reps} alternating trains of {A.train}", flush=True)
for heads, Nq in ((10, 4096), (20, 1024)):
    B, Cc, n0 = 2, heads * 64, 77
    q, kv0, o1, o2 = rn(B, Nq, Cc), rn(B, n0, 2 * Cc), torch.empty(B, Nq, Cc, dtype=torch.half, device=DEV), torch.empty(B, Nq, Cc, dtype=torch.half, device=DEV)
    for G in (1, 3, 8):
        kv1 = rn(B, 4 * G, 2 * Cc)
        m = (torch.rand(B, G, Nq, generator=g) < 0.5).half().to(DEV)
        regions = lambda m=m: _ffi.check(L.ia2p_attention_regions(s, p(q), Cc, p(o1), Cc, B, heads, Nq, 2, p(kv0), p(kv0, Cc), 2 * Cc, n0, 1.0,      # noqa: E731
                                                                  p(kv1), p(kv1, Cc), 2 * Cc, 4 * G, 0.8, p(m), G, None))
        plain = lambda: _ffi.check(L.ia2p_attention(s, p(q), Cc, p(o2), Cc, B, heads, Nq, 2, p(kv0), p(kv0, Cc), 2 * Cc, n0, 1.0, p(kv1), p(kv1, Cc), 2 * Cc, 4 * G, 0.8))      # noqa: E731
        if G == 1:
            regions(torch.ones_like(m)), plain()
            torch.cuda.synchronize()
            d = float((o1.float() - o2.float()).abs().max())
            assert d <= 4e-3 * float(o2.float().abs().max()), d
        for _ in range(20):
            regions(), plain()
        us = {"regions": [], "two-segment": []}
        for _ in range(A.reps):
            us["regions"].append(train(regions))
            us["two-segment"].append(train(plain))
        med = {k: statistics.median(v) for k, v in us.items()}
        print(f"heads {heads} Nq {Nq} G {G}: " + ", ".join(f"{k} {med[k]:.1f} ({min(v):.1f}, {max(v):.1f})" for k, v in us.items())
              + f"; regions / two-segment {med['regions'] / med['two-segment']:.3f}", flush=True)
