"""The condition-map launches on the MI355X against tests/canny_ref.py, on the bytes: grey, the Gaussian, Canny, the hysteresis on hand-made state maps (chains that
cross tile borders, there and back), the fp16 conversion, determinism and the refusals. Everything is integer arithmetic: no tolerance anywhere."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import canny_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from instructany2pix_amd import _ffi
    return _ffi, _ffi.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def grey_gpu(rgb):
    ffi, lib = _lib()
    x = dev(rgb)
    B, H, W, _ = x.shape
    out = torch.empty(B, H, W, dtype=torch.uint8, device=DEV)
    ffi.check(lib.ia2p_image_grey_u8(ffi.current_stream(), ffi.ptr(x), ffi.ptr(out), B, H, W))
    return out.cpu().numpy()


def gauss_gpu(src, taps, in_place=False):
    ffi, lib = _lib()
    x = dev(src)
    B, H, W, Ch = x.shape
    out = x if in_place else torch.empty_like(x)
    ws = torch.empty(lib.ia2p_image_gauss_workspace_bytes(B, H, W, Ch) // 4, dtype=torch.int32, device=DEV)
    q = (C.c_uint16 * len(taps))(*[int(t) for t in taps])
    ffi.check(lib.ia2p_image_gauss_u8(ffi.current_stream(), ffi.ptr(x), ffi.ptr(out), ffi.ptr(ws), B, H, W, Ch, q, len(taps) - 1))
    return out.cpu().numpy()


def _canny_ws(B, H, W):
    _, lib = _lib()
    return torch.empty((lib.ia2p_canny_workspace_bytes(B, H, W) + 3) // 4, dtype=torch.int32, device=DEV)


def canny_gpu(grey, low, high, l2=False):
    ffi, lib = _lib()
    g = dev(grey)
    B, H, W = g.shape
    out, ws, rounds = torch.empty_like(g), _canny_ws(B, H, W), C.c_int(-1)
    ffi.check(lib.ia2p_canny_u8(ffi.current_stream(), ffi.ptr(g), ffi.ptr(out), ffi.ptr(ws), ws.numel() * 4, B, H, W, float(low), float(high), int(l2), C.byref(rounds)))
    return out.cpu().numpy(), rounds.value


def hysteresis_gpu(state):
    ffi, lib = _lib()
    s = dev(state)
    B, H, W = s.shape
    out, ws, rounds = torch.empty_like(s), _canny_ws(B, H, W), C.c_int(-1)
    ffi.check(lib.ia2p_canny_hysteresis_u8(ffi.current_stream(), ffi.ptr(s), ffi.ptr(out), ffi.ptr(ws), ws.numel() * 4, B, H, W, C.byref(rounds)))
    assert torch.equal(s.cpu(), torch.from_numpy(state)), "the caller's state map was changed"
    return out.cpu().numpy(), rounds.value


def taps_of_radius(r):
    """some bell with q_0 + 2 sum q_i == 4096 and every tap of radius r non-zero"""
    if r == 0:
        return [4096]
    w = np.exp(-np.arange(r + 1) ** 2 / (2.0 * (0.6 * r + 0.5) ** 2))
    q = np.maximum(np.rint(4096 * w / (w[0] + 2 * w[1:].sum())), 1).astype(np.int64)
    q[0] = 4096 - 2 * int(q[1:].sum())
    assert q[0] > 0
    return [int(v) for v in q]


SHAPES = [(1, 1, 1), (1, 1, 17), (1, 17, 1), (2, 67, 131)]


@functools.lru_cache(maxsize=None)
def rgb_image(B, H, W):
    return np.random.default_rng(100 * H + W).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)


# ---- grey, Gaussian, conversion ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(1, 16, 64), (3, 5, 7)])
def test_grey_on_the_bytes(shape):
    rgb = rgb_image(*shape)
    assert np.array_equal(grey_gpu(rgb), R.grey_ref(rgb))


def test_grey_every_code_of_each_channel():
    px = [[v if k == ch else other for k in range(3)] for ch in range(3) for other in (0, 128, 255) for v in range(256)]
    rgb = np.array(px, dtype=np.uint8).reshape(1, 9, 256, 3)
    want = R.grey_ref(rgb)
    assert want.min() == 0 and want.max() == 255
    assert np.array_equal(grey_gpu(rgb), want)
    odd = rgb.reshape(1, 1, -1, 3)[:, :, :2301]                                                    # a pixel count that is no multiple of four
    assert np.array_equal(grey_gpu(odd), R.grey_ref(odd))


@pytest.mark.parametrize("Ch", [1, 3])
@pytest.mark.parametrize("r", [0, 1, 7, 32])
@pytest.mark.parametrize("shape", SHAPES)
def test_gauss_on_the_bytes(shape, r, Ch):
    src = np.ascontiguousarray(rgb_image(*shape)[..., :Ch])
    taps = taps_of_radius(r)
    want = R.gauss_ref(src, taps)
    assert np.array_equal(gauss_gpu(src, taps), want)                                              # (r = 32 on a 1 x 17 image: the replicated border does all the work)
    if r == 0:
        assert np.array_equal(want, src)
    if r == 7 and shape == SHAPES[-1]:
        assert np.array_equal(gauss_gpu(src, taps, in_place=True), want)                           # dst == src
        assert not np.array_equal(want, src)


def test_gauss_taps_of_the_package_drive_the_same_kernel():
    from instructany2pix_amd import condition
    img = rgb_image(2, 67, 131)
    for sigma in (0.0, 0.8, 1.4, 3.0):
        got = condition.blur(dev(img), sigma).cpu().numpy()
        assert np.array_equal(got, R.gauss_ref(img, condition.gauss_taps(sigma))), sigma
    one = condition.blur(dev(img[0]), 1.4)
    assert tuple(one.shape) == (67, 131, 3) and np.array_equal(one.cpu().numpy(), R.gauss_ref(img[:1], condition.gauss_taps(1.4))[0])
    assert np.array_equal(condition.grey(dev(img)).cpu().numpy(), R.grey_ref(img))


@pytest.mark.parametrize("Ch", [1, 3])
@pytest.mark.parametrize("shape", SHAPES + [(1, 16, 16)])
def test_condition_conversion_on_the_fp16_bits(shape, Ch):
    from instructany2pix_amd import condition
    from instructany2pix_amd.image_processor import image_from_u8
    B, H, W = shape
    m = rgb_image(*shape)[..., :Ch].copy()
    if H * W >= 256:
        m.reshape(B, -1, Ch)[0, :256, 0] = np.arange(256)                                          # every code
    got = condition.to_condition(dev(m))
    want = image_from_u8(dev(np.repeat(m, 3, axis=-1) if Ch == 1 else m), normalize=False)
    assert got.dtype == torch.float16 and tuple(got.shape) == (B, 3, H, W)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert np.array_equal(got.cpu().numpy().view(np.int16), R.condition_ref(m[..., 0] if Ch == 1 else m).view(np.int16))


# ---- Canny ---------------------------------------------------------------------------------------------------------------------------------------------------------
def census(state, out):
    return int((state == R.STRONG).sum()), int(((state == R.WEAK) & (out == 255)).sum()), int(((state == R.WEAK) & (out == 0)).sum())


@functools.lru_cache(maxsize=None)
def canny_case(name):
    """-> (grey [B, H, W], low, high, l2, reference edges [B, H, W], per-image census)"""
    grey, low, high, l2 = {
        "noise_l1": lambda: (R.noise_image(67, 131, 7, B=2), 400, 800, False),
        "noise_l2": lambda: (R.noise_image(67, 131, 7, B=2), 300, 600, True),
        "ramp": lambda: (R.ramp_steps_image(67, 131)[None], 5, 300, False),
        "ramp_l2": lambda: (R.ramp_steps_image(67, 131)[None], 5, 300, True),
        "border": lambda: (R.border_image(40, 70)[None], 50, 400, False),
        "border_wide": lambda: (R.border_image(70, 140)[None], 50, 400, True),
        "row": lambda: (R.noise_image(1, 17, 3), 50, 150, False),
        "column": lambda: (R.noise_image(17, 1, 3), 50, 150, False),
        "three": lambda: (R.noise_image(3, 3, 3), 50, 150, False),
        "one": lambda: (R.noise_image(1, 1, 3), 0, 0, False),
        "swapped": lambda: (R.noise_image(67, 131, 7, B=2), 800, 400, False),
        "fractional": lambda: (R.noise_image(67, 131, 8, B=1), 399.9, 800.99, False),
        "zero_thresholds": lambda: (R.noise_image(20, 33, 9), 0, 0, False),
        "huge_thresholds": lambda: (R.noise_image(20, 33, 9), 1e9, 3e38, True),
    }[name]()
    states = [R.canny_state_ref(g, low, high, l2) for g in grey]
    want = np.stack([R.hysteresis_ref(s) for s in states])
    return grey, low, high, l2, want, [census(s, w) for s, w in zip(states, want)]


@pytest.mark.parametrize("name", ["noise_l1", "noise_l2", "ramp", "ramp_l2", "border", "border_wide", "row", "column", "three", "one", "swapped", "fractional",
                                  "zero_thresholds", "huge_thresholds"])
def test_canny_on_the_bytes(name):
    grey, low, high, l2, want, counts = canny_case(name)
    if name in ("noise_l1", "noise_l2", "swapped", "ramp"):
        for strong, kept, dropped in counts:                                                       # the reference's map has all three kinds: the test cannot pass vacuously
            assert strong > 50 and kept > 50 and dropped > 50, counts
    if name == "swapped":
        assert np.array_equal(want, canny_case("noise_l1")[4])
    if name == "ramp":
        dx, dy = R.sobel_ref(grey[0])
        m = np.abs(dx) + np.abs(dy)
        assert int(((m[:, 1:] == m[:, :-1]) & (m[:, 1:] > 5)).sum()) > 1000 and int(((m[1:] == m[:-1]) & (m[1:] > 5)).sum()) > 1000      # exact ties on both axes
    if name.startswith("border"):
        e = want[0]
        assert e[0].any() and e[-1].any() and e[:, 0].any() and e[:, -1].any() and not e[3:-3, 3:-3].any()      # edges on all four borders and nowhere inside
    if name == "huge_thresholds":
        assert not want.any()
    got, rounds = canny_gpu(grey, low, high, l2)
    print(f"[canny] {name}: census {counts}, rounds {rounds}")
    assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert 1 <= rounds <= _lib()[1].ia2p_canny_max_rounds(*grey.shape)


def test_canny_of_the_package_blur_then_detect():
    from instructany2pix_amd import condition
    img = rgb_image(2, 67, 131)
    g = R.grey_ref(img)
    got, rounds = condition.canny(dev(img), 400, 800, return_rounds=True)
    assert rounds >= 1 and np.array_equal(got.cpu().numpy(), np.stack([R.canny_ref(x, 400, 800) for x in g]))
    b = R.gauss_ref(g[..., None], condition.gauss_taps(1.4))[..., 0]
    want = np.stack([R.canny_ref(x, 20, 60, True) for x in b])
    assert 100 < int((want > 0).sum()) < want.size // 2
    assert np.array_equal(condition.canny(dev(img), 20, 60, blur_sigma=1.4, l2_gradient=True).cpu().numpy(), want)
    assert np.array_equal(condition.make({"kind": "canny", "low": 20, "high": 60, "blur_sigma": 1.4, "l2_gradient": True}, dev(img)).cpu().numpy(), want)
    one = condition.canny(dev(g[0]), 400, 800)                                                     # a grey image, no batch
    assert tuple(one.shape) == (67, 131) and np.array_equal(one.cpu().numpy(), R.canny_ref(g[0], 400, 800))
    assert np.array_equal(condition.make("grey", dev(img[0])).cpu().numpy(), g[0])


# ---- hysteresis on hand-made state maps ---------------------------------------------------------------------------------------------------------------------------
def test_serpentine_crosses_tile_borders_there_and_back():
    on, off = R.serpentine_state(130, 200), R.serpentine_state(130, 200, strong=False)
    state = np.stack([on, off])
    want = np.stack([R.hysteresis_ref(on), R.hysteresis_ref(off)])
    assert np.array_equal(want[0] > 0, on > 0) and not want[1].any() and int((on == R.STRONG).sum()) == 1
    got, rounds = hysteresis_gpu(state)
    bound = _lib()[1].ia2p_canny_max_rounds(2, 130, 200)
    print(f"[canny] serpentine 130 x 200: {rounds} rounds, bound {bound}")
    assert np.array_equal(got, want), int((got != want).sum())
    assert 2 <= rounds < bound
    alone, r1 = hysteresis_gpu(off[None])                                                          # nothing to promote: one round
    assert not alone.any() and r1 == 1


def test_diagonal_chains_and_strong_pixels_across_tile_borders():
    s = R.tile_border_state(130, 200)
    want = R.hysteresis_ref(s)
    got, rounds = hysteresis_gpu(s[None])
    assert np.array_equal(got[0], want), np.argwhere(got[0] != want)[:8]
    assert rounds >= 2
    # a full tile of weak pixels lit from one corner, and the same with the far pixel cut off
    full = np.full((1, 64, 64), R.WEAK, dtype=np.uint8)
    full[0, 63, 63] = R.STRONG
    assert (hysteresis_gpu(full)[0] == 255).all()
    full[0, 0:2, 0:2] = [[R.WEAK, 0], [0, 0]]
    out = hysteresis_gpu(full)[0]
    assert out[0, 0, 0] == 0 and int((out == 255).sum()) == 64 * 64 - 4
    junk = np.array([[[3, 1, 2, 1, 255, 1, 0, 1]]], dtype=np.uint8)                                # values other than 1 and 2 count as off
    assert hysteresis_gpu(junk)[0].tolist() == [[[0, 255, 255, 255, 0, 0, 0, 0]]]


def test_the_same_input_three_times_gives_the_same_bytes():
    grey, low, high, l2, want, _ = canny_case("noise_l1")
    runs = [canny_gpu(grey, low, high, l2)[0] for _ in range(3)]
    assert all(np.array_equal(r, want) for r in runs)
    s = np.stack([R.serpentine_state(130, 200), R.tile_border_state(130, 200)])
    runs = [hysteresis_gpu(s)[0] for _ in range(3)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_real_buffers():
    ffi, lib = _lib()
    g = dev(R.noise_image(16, 16, 1))
    out, ws = torch.full_like(g, 7), _canny_ws(1, 16, 16)
    st, p, n = ffi.current_stream(), ffi.ptr, ws.numel() * 4
    INVALID, NOMEM = 1, 5
    assert lib.ia2p_canny_u8(st, None, p(out), p(ws), n, 1, 16, 16, 100.0, 200.0, 0, None) == INVALID
    assert lib.ia2p_canny_u8(st, p(g), p(g), p(ws), n, 1, 16, 16, 100.0, 200.0, 0, None) == INVALID           # edges == grey
    assert lib.ia2p_canny_u8(st, p(g), p(out), p(ws), n - 1, 1, 16, 16, 100.0, 200.0, 0, None) == NOMEM
    assert lib.ia2p_canny_u8(st, p(g), p(out), p(ws), n, 1, 16, 16, -1.0, 200.0, 0, None) == INVALID
    assert lib.ia2p_canny_u8(st, p(g), p(out), p(ws), n, 1, 16, 16, 100.0, float("nan"), 0, None) == INVALID
    torch.cuda.synchronize()
    assert bool((out == 7).all()), "a refused call wrote to its output"
    from instructany2pix_amd import condition
    with pytest.raises(ValueError):
        condition.canny(g, low=-3)
    with pytest.raises(ValueError):
        condition.canny(torch.zeros(2, 5, 7, 2, dtype=torch.uint8, device=DEV))                    # two channels
    with pytest.raises(TypeError):
        condition.grey(torch.zeros(5, 7, 3, device=DEV))                                           # floats
