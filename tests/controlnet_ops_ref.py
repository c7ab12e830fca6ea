"""fp64 references of the ControlNet path's launches -- the narrow 3x3 convolution (`ia2p_conv3x3_narrow`, and `ia2p_conv_in_act` for the 3 -> 16 convolution), the zero
convolution with its per-image scale (`ia2p_gemm_rowscale`) and the residual injection with GroupNorm column sums (`ia2p_residual_add_gnstats`) -- and the bound each
kernel must meet (None: the exact bits), in the manner of unet_ops_ref.py, whose helpers and notation this file uses.

  lattice      operands are integers in [-3, 3] times a power of two, so every fp32 accumulation is exact in any order (`R.exactness(case)` < 2^24, asserted for every
               case in test_controlnet_ops_cpu.py). What is left are the roundings the reference's fp16 tensors make, which the references apply (round16).
  convolution  r = fp16(acc + bias): the exact bits. With SiLU: out = fp16(silu(r)) on an exact r -- `R.silu_bound(r, 0)` (the native exponential modelled, its share of
               the bound below a tenth) and the fp16 store.
  zero conv    r = fp16(acc + bias); res = fp16(s_b r) with s_b in {0, 0.5, 0.75, 1, 1.5}: s_b r has at most 13 significant bits, exact in fp32; the exact bits.
  injection    y = fp16(x + r): the sum of two lattice values is exact in fp32, the store rounds (one row of every run of 16 sits at +-1024, where fp16 steps by 1 and
               the quarter steps of r are rounded away, ties included). Column sums: fp32 over runs of 16 rows, fp64 from there on -- exact where
               `R.colstats_exactness(y, 0.5)` stays below 2^24, so they equal `R.colstats_ref(y)` and, bit for bit, what ia2p_gn_colstats returns for y.
"""
import torch

import unet_ops_ref as R
from unet_ops_ref import f64, round16, with_store16  # noqa: F401

NARROW_SHAPES = ((2, 17, 23, 16, 16, 1), (1, 18, 22, 16, 32, 2), (2, 17, 23, 32, 96, 2), (1, 16, 24, 96, 96, 1), (1, 17, 19, 96, 256, 2))      # B, H, W, Cin, Co, stride
CONV_IN_ACT_SHAPES = ((2, 3, 17, 23, 16),)                                                                                                       # B, Cin, H, W, Co
ROWSCALE_SHAPES = ((3, 80, 64), (2, 64, 320), (2, 16, 256))                                                                                      # B, HW, C
ROWSCALE_SCALES = (0.0, 0.75, 1.5)
SCALES = (0.0, 0.5, 0.75, 1.0, 1.5)
INJECT_SHAPES = ((2, 64, 64), (1, 256, 320), (3, 16, 256), (1, 32, 72))       # B, HW, C; the last: a width that is no multiple of 64 (a partly idle last span)
INJECT_ROWS = {(2, 64, 64): (64, 16), (1, 256, 320): (256, 64), (3, 16, 256): (16,), (1, 32, 72): (32, 16)}
INJECT_UNIT = 0.5


def narrow_case(B, H, W, Cin, Co, stride):
    c = R.conv_case(B, H, W, Cin, Co, stride)
    c.update(tv=None, res=None)
    return c


def narrow_ref(c, silu):
    """-> (ref [B, Ho, Wo, Co], bound or None, the modelled exponential's share)"""
    r = round16(R.conv3x3_sum(c["x"], c["w"], c["stride"]) + f64(c["bias"]))
    if not silu:
        return r, None, 0.0
    out, Bf, X = R.silu_bound(r, torch.zeros_like(r))
    total = with_store16(out, Bf)
    return out, total, float((X / total).max())


def conv_in_act_case(B, Cin, H, W, Co):
    return R.boundary_case("in", B, Cin, H, W, Co)


def rowscale_case(B, HW, C, scales=None):
    c = R.gemm_case(B * HW, C, C)
    s = torch.tensor([(scales or ROWSCALE_SCALES)[b % len(scales or ROWSCALE_SCALES)] for b in range(B)], dtype=torch.float64)
    c.update(res=None, B=B, HW=HW, scales=s.float())
    return c


def rowscale_ref(c):
    r = round16(f64(c["A"]) @ f64(c["W"]).t() + f64(c["bias"]))
    s = f64(c["scales"]).repeat_interleave(c["HW"]).reshape(-1, 1)
    p = r * s
    assert torch.equal(p, torch.from_numpy(p.numpy().astype("float32").astype("float64"))), "s r must be exact in fp32"
    return round16(p), None


def inject_case(B, HW, C):
    """x, r [B HW, C] fp16: multiples of 1/2 in [-1.5, 1.5] each; row 5 of every run of 16 rows holds x = +-1024 + k, r = j / 4 (the store rounds to integers)"""
    g = R.gen(9100 + B + HW + C)
    M = B * HW
    x, r = R.ints((M, C), g) * 0.5, R.ints((M, C), g) * 0.5
    big = torch.arange(M) % 16 == 5
    sign = torch.where((torch.arange(M) // 16) % 2 == 0, 1.0, -1.0).double().reshape(M, 1)
    x[big] = (sign * 1024.0 + R.ints((M, C), g))[big]
    r[big] = (R.ints((M, C), g, -7, 7) * 0.25)[big]
    return dict(B=B, HW=HW, C=C, M=M, x=x.half(), r=r.half())


def inject_ref(c):
    s = f64(c["x"]) + f64(c["r"])
    assert torch.equal(s, torch.from_numpy(s.numpy().astype("float32").astype("float64")))
    return round16(s)
