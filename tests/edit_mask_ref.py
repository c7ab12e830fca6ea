"""Integer references for the edit-mask kernels (include/ia2p.h, "edit mask"), in numpy: the written-out rules, nothing of the code under test.
Shared by tests/test_edit_mask_cpu.py (against hand cases) and tests/test_edit_mask_gpu.py (against the HIP kernels, exact comparisons)."""
import numpy as np

# (H, W). The first four have W % 16 != 0 and W / 8 odd: the scalar paths of the mask kernels (short last chunks, one latent cell per thread). The last two have
# W % 16 == 0 and W / 8 even: their 16-byte paths (whole chunks; two cells per thread at f = 8), the ones a 1024 x 1024 image takes.
SIZES = ((8, 8), (16, 24), (8, 40), (40, 56), (16, 32), (24, 64))
VECTOR_SIZES = tuple(s for s in SIZES if s[1] % 16 == 0 and (s[1] // 8) % 2 == 0)
COMPOSITE_SIZES = SIZES + ((5, 7), (3, 11))          # B * H * W no multiple of 16 at B = 1 and 3: the scalar path of the composite and its short last chunk
RADII = (0, 1, 3, 9)                                 # 9 exceeds H / 2 at H = 8 and 16: the clamped window covers the whole column


def binarize(mask):
    return np.where(np.asarray(mask) >= 128, 255, 0).astype(np.int64)


def mask_to_latent_ref(mask, f):
    """u8 [B, H, W] -> float16 [B, 1, H / f, W / f]: 1 where any pixel of the f x f block is >= 128"""
    B, H, W = mask.shape
    assert H % f == 0 and W % f == 0
    on = (np.asarray(mask) >= 128).reshape(B, H // f, f, W // f, f)
    return on.any(axis=(2, 4)).astype(np.float16)[:, None]


def mask_feather_ref(mask, r):
    """u8 [B, H, W] -> u8: min(bin, (S + A / 2) / A), S the sum of bin over the (2 r + 1)^2 window with clamped coordinates, A = (2 r + 1)^2"""
    b = binarize(mask)
    B, H, W = b.shape
    S = np.zeros_like(b)
    ys, xs = np.arange(H), np.arange(W)
    for dy in range(-r, r + 1):
        yy = np.clip(ys + dy, 0, H - 1)
        for dx in range(-r, r + 1):
            S += b[:, yy][:, :, np.clip(xs + dx, 0, W - 1)]
    A = (2 * r + 1) ** 2
    return np.minimum(b, (S + A // 2) // A).astype(np.uint8)


def image_composite_ref(edited, base, alpha):
    """u8 [B, H, W, C] x 2, alpha u8 [B, H, W] -> (a e + (255 - a) b + 127) / 255"""
    a = np.asarray(alpha).astype(np.int64)[..., None]
    return ((a * np.asarray(edited).astype(np.int64) + (255 - a) * np.asarray(base).astype(np.int64) + 127) // 255).astype(np.uint8)


def masks(B, H, W, seed):
    """name -> u8 [B, H, W]: all 0, all 255, a single pixel, a border stripe, random codes (not only 0 / 255: the kernels binarise at 128)"""
    g = np.random.default_rng(seed)
    one = np.zeros((B, H, W), np.uint8)
    one[:, H // 2, W // 3] = 200
    stripe = np.zeros((B, H, W), np.uint8)
    stripe[:, :, :3] = 255
    stripe[:, -2:, :] = 128
    return {"zeros": np.zeros((B, H, W), np.uint8), "ones": np.full((B, H, W), 255, np.uint8), "pixel": one, "stripe": stripe,
            "random": g.integers(0, 256, (B, H, W), dtype=np.uint8)}


def known_levels_ref(steps):
    """[iterations + 1][requests]: row 0 the start level N_r, row i + 1 the level after sampling step i"""
    n = max(steps)
    return [list(steps)] + [[max(s - 1 - i, 0) for s in steps] for i in range(n)]
