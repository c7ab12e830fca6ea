"""The condition-map rules of include/ia2p.h ("condition maps") restated in integer numpy, independent of the product: grey, the separable Gaussian with given
taps, Canny (OpenCV's cv::Canny, 8-bit input, aperture 3, as restated there -- OpenCV is not installed here, so parity with it is restated, not pinned) with its
hysteresis as a plain stack-based flood from the strong pixels, and the / 255 conversion. Everything but the last is integer: comparisons are exact."""
import numpy as np

OFF, WEAK, STRONG = 0, 1, 2


def grey_ref(rgb):
    """uint8 [..., 3] -> uint8 [...]: (4899 R + 9617 G + 1868 B + 8192) >> 14"""
    v = rgb.astype(np.int64)
    return ((4899 * v[..., 0] + 9617 * v[..., 1] + 1868 * v[..., 2] + 8192) >> 14).astype(np.uint8)


def gauss_ref(src, taps):
    """uint8 [B, H, W, C], taps q_0 .. q_r (centre first, q_0 + 2 sum q_i == 4096) -> uint8 [B, H, W, C]; replicated border"""
    q = [int(t) for t in taps]
    r = len(q) - 1
    assert q[0] + 2 * sum(q[1:]) == 4096
    B, H, W, C = src.shape
    p = np.pad(src.astype(np.int64), ((0, 0), (0, 0), (r, r), (0, 0)), mode="edge")
    row = sum(q[abs(i)] * p[:, :, r + i:r + i + W, :] for i in range(-r, r + 1))
    assert int(row.max()) <= 255 * 4096
    p = np.pad(row, ((0, 0), (r, r), (0, 0), (0, 0)), mode="edge")
    acc = sum(q[abs(j)] * p[:, r + j:r + j + H, :, :] for j in range(-r, r + 1))
    assert int(acc.max()) <= 255 << 24
    return ((acc + (1 << 23)) >> 24).astype(np.uint8)


def sobel_ref(grey):
    """uint8 [H, W] -> (dx, dy) int64 [H, W]: [-1 0 1; -2 0 2; -1 0 1] and its transpose, replicated border"""
    g = np.pad(grey.astype(np.int64), 1, mode="edge")
    a, b, c = g[:-2, :-2], g[:-2, 1:-1], g[:-2, 2:]
    d, f = g[1:-1, :-2], g[1:-1, 2:]
    p, q, t = g[2:, :-2], g[2:, 1:-1], g[2:, 2:]
    return (c + 2 * f + t) - (a + 2 * d + p), (p + 2 * q + t) - (a + 2 * b + c)


def thresholds_ref(low, high, l2):
    if low > high:
        low, high = high, low
    lo, hi = int(np.floor(low)), int(np.floor(high))
    return (lo * lo, hi * hi) if l2 else (lo, hi)


def nms_state_ref(dx, dy, lo, hi, l2):
    """gradients int [H, W] and the integer thresholds -> state uint8 [H, W] (0 off, 1 weak, 2 strong)"""
    dx, dy = dx.astype(np.int64), dy.astype(np.int64)
    H, W = dx.shape
    m = dx * dx + dy * dy if l2 else np.abs(dx) + np.abs(dy)
    M = np.pad(m, 1)                                                        # 0 outside the image

    def at(oy, ox):
        return M[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]

    x, y = np.abs(dx), np.abs(dy) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    horizontal = y < t22
    vertical = ~horizontal & (y > t67)
    negative = (dx ^ dy) < 0
    keep_h = (m > at(0, -1)) & (m >= at(0, 1))
    keep_v = (m > at(-1, 0)) & (m >= at(1, 0))
    keep_d = np.where(negative, (m > at(-1, 1)) & (m > at(1, -1)), (m > at(-1, -1)) & (m > at(1, 1)))
    keep = np.where(horizontal, keep_h, np.where(vertical, keep_v, keep_d)) & (m > lo)
    return np.where(keep, np.where(m > hi, STRONG, WEAK), OFF).astype(np.uint8)


def canny_state_ref(grey, low, high, l2=False):
    dx, dy = sobel_ref(grey)
    lo, hi = thresholds_ref(low, high, l2)
    return nms_state_ref(dx, dy, lo, hi, l2)


def hysteresis_ref(state):
    """state uint8 [H, W] -> uint8 [H, W] in {0, 255}: a plain stack-based flood from the strong pixels through weak ones, 8-connected"""
    H, W = state.shape
    out = np.zeros((H, W), dtype=np.uint8)
    stack = [(int(y), int(x)) for y, x in zip(*np.nonzero(state == STRONG))]
    for y, x in stack:
        out[y, x] = 255
    while stack:
        y, x = stack.pop()
        for ny in range(max(y - 1, 0), min(y + 2, H)):
            for nx in range(max(x - 1, 0), min(x + 2, W)):
                if state[ny, nx] == WEAK and out[ny, nx] == 0:
                    out[ny, nx] = 255
                    stack.append((ny, nx))
    return out


def canny_ref(grey, low, high, l2=False):
    """uint8 [H, W] -> uint8 [H, W] in {0, 255}"""
    return hysteresis_ref(canny_state_ref(grey, low, high, l2))


def condition_ref(map_u8):
    """uint8 [B, H, W] or [B, H, W, 3] -> float16 [B, 3, H, W]: q / 255 in float32 (one rounding), then one rounding to float16"""
    m = map_u8 if map_u8.ndim == 4 else np.repeat(map_u8[..., None], 3, axis=-1)
    v = m.astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(v.astype(np.float16).transpose(0, 3, 1, 2))


# ---- the inputs the tests share ------------------------------------------------------------------------------------------------------------------------------
def noise_image(H, W, seed, B=1):
    return np.random.default_rng(seed).integers(0, 256, size=(B, H, W), dtype=np.uint8)


def ramp_steps_image(H, W):
    """a smooth horizontal ramp plus vertical and horizontal steps: flat runs and equal neighbours give the exact ties of the non-maximum suppression"""
    y, x = np.mgrid[0:H, 0:W]
    g = (x * 2) % 256
    g = np.where(x >= W // 2, g // 2 + 100, g)
    g = np.where((y >= H // 3) & (y < H // 3 + 4), 255 - g, g)
    g = np.where((y + x) % 29 < 3, 40, g)
    return np.clip(g, 0, 255).astype(np.uint8)


def border_image(H, W):
    """structure that touches all four borders only: bright bars on every border row / column and the corners, flat inside"""
    g = np.full((H, W), 60, dtype=np.uint8)
    g[0, ::3] = 250
    g[-1, 1::4] = 240
    g[::5, 0] = 230
    g[2::3, -1] = 220
    g[0, 0] = g[0, -1] = g[-1, 0] = g[-1, -1] = 255
    return g


def serpentine_state(H, W, pitch=6, strong=True):
    """a one-pixel-wide weak line that runs along every `pitch`-th row from column 1 to W - 2 and steps down alternately at the right and at the left end: one
    8-connected chain that crosses every vertical tile border once per row and every horizontal one on its way down; `strong`: its first pixel is strong"""
    s = np.zeros((H, W), dtype=np.uint8)
    rows = list(range(2, H - 1, pitch))
    for k, y in enumerate(rows):
        s[y, 1:W - 1] = WEAK
        if k + 1 < len(rows):
            s[y:rows[k + 1], W - 2 if k % 2 == 0 else 1] = WEAK
    if strong:
        s[rows[0], 1] = STRONG
    return s


def tile_border_state(H, W):
    """diagonal-only chains through the tile corner at (64, 64) in both directions, weak pixels whose only strong neighbour lies across row 63 / 64 or column
    63 / 64, and weak pixels with no strong pixel anywhere near"""
    s = np.zeros((H, W), dtype=np.uint8)
    for i in range(40, 90):
        s[i, i] = WEAK                                                      # (63, 63) -> (64, 64): through the corner
    s[40, 40] = STRONG
    for y in range(45, 85):
        s[y, 191 - y] = WEAK                                                # anti-diagonal through the corner at (64, 128): (63, 128) -> (64, 127)
    s[84, 191 - 84] = STRONG
    s[63, 10], s[64, 10] = WEAK, STRONG
    s[64, 20], s[63, 20] = WEAK, STRONG
    s[10, 63], s[10, 64] = WEAK, STRONG
    s[20, 64], s[20, 63] = WEAK, STRONG
    s[100, 100:110] = WEAK                                                  # a weak run with no strong pixel: dropped
    s[63:66, 150] = WEAK
    return s
