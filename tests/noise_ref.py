"""CPU reference of the seeded noise launches (include/ia2p.h, "Seeded noise"): a numpy restatement of the noise rule in float64, of the posterior sample and of
the polar mixing, and the error bound each launch is held to. The bounds are counted from the operations, the way tests/llm_ops_ref.py does it; none is fitted.

Philox: `philox_blocks` is a vectorised twin of tests/sampler_ref.py::philox4x32_10 (tests/test_noise_cpu.py checks one against the other and against
Random123's known answers).

Units: u = 2^-24 is half an fp32 ulp, relative (one correctly rounded operation errs by at most u |result|; an operation documented at "1 ulp" by at most
2 u |result|).

Bound of a normal, K_NORMAL. The kernel computes z = fl(r * t), r = sqrtf(-2 logf(u1)), t = cospi / sinpi (2 u2) from sincospif. u1, u2, the factor -2 and the
argument 2 u2 are exact. HIP's device math functions are documented at: logf 1 ulp, sqrtf 1 ulp (correctly rounded in the default build: counted at 1 ulp all
the same), sincospif 1 ulp (ROCm HIP math API, "single precision mathematical functions" table).
    L = logf(u1):            relative error <= 2 u                      (u1 = 1 gives L = 0 and r = 0 exactly)
    r = sqrtf(-2 L):         half the argument's relative error, plus the function's own: <= u + 2 u = 3 u
    t = sincospif:           |dt| <= 2 u |t| <= 2 u
    z = fl(r t):             |dz| <= r |dt| + |t| |dr| + u |z|  <=  r (2 u + 3 u + u)  =  6 u r  =  3 * 2^-23 * r
and the second-order products are below (6 u)^2 r < 2^-40 r: K_NORMAL = 3 (1 + 2^-16) covers them. The bound is k * 2^-23 * r(u1), per element.
"""
import numpy as np

from sampler_ref import MASK, M0, M1, W0, W1

U = 2.0 ** -24
K_NORMAL = 3.0 * (1.0 + 2.0 ** -16)


def philox_blocks(c0, c1, c2, c3, key):
    """vectorised Philox4x32-10: c0 an array of first counter words, c1..c3 scalars, key = (k0, k1) -> uint64 array [4, n] holding the four 32-bit words of every block"""
    c = [np.asarray(c0, dtype=np.uint64) & np.uint64(MASK)] + [np.full(np.shape(c0), int(x) & MASK, dtype=np.uint64) for x in (c1, c2, c3)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    m = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m, p1 >> np.uint64(32), p1 & m
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c)


def words(seed: int, draw: int, first: int, n: int):
    """the Philox words behind elements first .. first + n - 1 of stream (seed, draw): (w_even, w_odd), each [n] uint64 -- w[2p], w[2p + 1] of every element's pair"""
    e = np.arange(first, first + n, dtype=np.uint64)
    j = e >> np.uint64(2)
    j0 = int(j[0])
    blocks = philox_blocks(np.arange(j0, int(j[-1]) + 1, dtype=np.uint64), draw, 0, 1, (seed & MASK, (seed >> 32) & MASK))      # counter (j, draw, 0, 1)
    col = (j - np.uint64(j0)).astype(np.int64)
    p = ((e & np.uint64(3)) >> np.uint64(1)).astype(np.int64)
    return blocks[2 * p, col], blocks[2 * p + 1, col]


def normals(seed: int, draw: int, n: int, first: int = 0):
    """float64 values of elements first .. first + n - 1 of stream (seed, draw) -> (z [n], r [n]); r is what the error bound scales with"""
    wa, wb = words(seed, draw, first, n)
    u1 = ((wa >> np.uint64(8)).astype(np.float64) + 1.0) * U
    u2 = (wb >> np.uint64(8)).astype(np.float64) * U
    r = np.sqrt(-2.0 * np.log(u1))
    odd = (np.arange(first, first + n) & 1).astype(bool)
    # cospi / sinpi of an exact argument: reduce 2 u2 in [0, 2) exactly before multiplying by pi, so that the float64 value is good to its last bits
    x = 2.0 * u2
    t = np.where(odd, _sinpi(x), _cospi(x))
    return r * t, r


def _sinpi(x):
    x = np.where(x >= 1.0, x - 2.0, x)                        # [-1, 1), exact
    x = np.where(x > 0.5, 1.0 - x, np.where(x < -0.5, -1.0 - x, x))      # sin(pi x) = sin(pi (1 - x)): [-0.5, 0.5], exact
    return np.sin(np.pi * x)


def _cospi(x):
    return _sinpi(x + 0.5 - np.where(x + 0.5 >= 2.0, 2.0, 0.0))          # cos(pi x) = sin(pi (x + 1/2)); x + 1/2 is exact (multiples of 2^-23 below 4)


def normal_bound(r):
    return K_NORMAL * 2.0 ** -23 * r


def half_ulp16(v):
    """half an fp16 ulp at |v| (subnormal spacing 2^-24 below 2^-14)"""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -14)
    return 0.5 * 2.0 ** (np.floor(np.log2(a)) - 10)


F16_MAX = 65504.0


def posterior(moments, seeds, draw, scaling_factor):
    """float64 posterior sample of fp16 moments [B, 2 C, HW] -> (x64 [B, C, HW] before any rounding, bound on |out - x64 * sf| [B, C, HW]).
    Operations of one element, with s = exp(0.5 clamp(logvar)) and z the normal (error dz <= normal_bound):
        h = 0.5 lv                 exact (lv is an fp16 value, the clamp bounds are fp32 numbers)
        s = expf(h)                1 ulp: 2 u s
        a = fmaf(s, z, mean)       one rounding: |da| <= s dz + 2 u s |z| + u |a|
        x = fp16(a)                half an fp16 ulp of x
        o = fl(x * sf)             u |o|, then fp16(o): half an fp16 ulp of o
    so |out - x64 sf| <= sf (s dz + 2 u s |z| + u |x64| + hulp16(x64)) + u |x64 sf| + hulp16(x64 sf), the half ulps taken one binade up where the value
    could cross into it (factor 2: never too small)."""
    m = np.asarray(moments, dtype=np.float64)
    B, C2, HW = m.shape
    Cc = C2 // 2
    mean, lv = m[:, :Cc], np.clip(m[:, Cc:], -30.0, 20.0)
    s = np.exp(0.5 * lv)
    z = np.empty((B, Cc * HW))
    r = np.empty((B, Cc * HW))
    for b in range(B):
        z[b], r[b] = normals(int(seeds[b]), draw, Cc * HW)
    z, r = z.reshape(B, Cc, HW), r.reshape(B, Cc, HW)
    sf = float(np.float32(scaling_factor))
    x = mean + s * z
    bound = sf * (s * normal_bound(r) + 2 * U * s * np.abs(z) + U * np.abs(x) + 2 * half_ulp16(x)) + U * np.abs(x * sf) + 2 * half_ulp16(x * sf)
    return x, bound


def polar(x, y, alpha):
    """float64 `polar_intrtpolate` of one request's fp16 x, y (flat) at an fp32 alpha -> (out64, bound on |out - out64|).
    The kernel's sums of squares: thread t chains the squares of its groups of 8 (8 ceil(per / 8192) fused multiply-adds), 6 butterfly additions fold the lanes,
    15 additions fold the waves: every term passes through at most d = 8 ceil(per / 8192) + 21 roundings, all terms are non-negative, so a sum is off by at most
    d u relatively and its square root (1 ulp) by d u / 2 + 2 u =: e_n.
        b1 = fl(1 - a)                                 u
        ll_i = fl(fl(a x_i) + fl(b1 y_i))              |dll_i| <= u (2 |a x_i| + 3 |b1 y_i|) =: t_i   (two products, b1's own error, one sum)
        nl                                             |dnl| <= e_n nl + |t|_2
        num = fl(fl(a n0) + fl(b1 n1))                 relative <= e_n + 3 u
        scale = num / nl (correctly rounded: u)        relative <= e_n + 4 u + e_n + |t|_2 / nl =: e_s
        out_i = fp16(fl(ll_i scale))                   |dout_i| <= scale t_i + |ll_i scale| (e_s + u) + half an fp16 ulp of the result (one binade up: factor 2)"""
    a = float(np.float32(alpha))
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    per = x.size
    b1 = 1.0 - a
    ll = a * x + b1 * y
    n0, n1, nl = np.sqrt((x * x).sum()), np.sqrt((y * y).sum()), np.sqrt((ll * ll).sum())
    scale = (a * n0 + b1 * n1) / nl
    out = ll * scale
    d = 8 * -(-per // 8192) + 21
    e_n = d * U / 2 + 2 * U
    t = U * (2 * np.abs(a * x) + 3 * np.abs(b1 * y))
    e_s = 2 * e_n + 4 * U + np.sqrt((t * t).sum()) / nl
    bound = scale * t + np.abs(out) * (e_s + U) + 2 * half_ulp16(out)
    return out, bound


def moments4(z):
    """(mean, variance, skewness, excess kurtosis, max |z|) of a sample, float64"""
    z = np.asarray(z, dtype=np.float64)
    m = z.mean()
    c = z - m
    v = (c * c).mean()
    return m, v, (c ** 3).mean() / v ** 1.5, (c ** 4).mean() / v ** 2 - 3.0, np.abs(z).max()


def moment_caps(n):
    """six standard errors of each estimate under N(0, 1) at n samples, and the rule's own |z| ceiling"""
    return 6 / np.sqrt(n), 6 * np.sqrt(2 / n), 6 * np.sqrt(6 / n), 6 * np.sqrt(24 / n), 5.77
