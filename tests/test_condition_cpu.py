"""Condition maps without a device: tests/canny_ref.py against independent statements of its rules, the Gaussian taps, the refusals of the pipeline surface that
come before any device call, the new ABI names, and the argument refusals of the entries (all of them before any HIP call)."""
import ctypes as C
import inspect
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import canny_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("ia2p_image_grey_u8", "ia2p_image_gauss_workspace_bytes", "ia2p_image_gauss_u8", "ia2p_canny_workspace_bytes", "ia2p_canny_max_rounds", "ia2p_canny_u8",
             "ia2p_canny_hysteresis_u8", "ia2p_condition_from_u8")


# ---- the reference against independent statements -------------------------------------------------------------------------------------------------------------
def _label_hysteresis(state):
    """components of state > 0 under the 3 x 3 structure, kept iff they hold a strong pixel"""
    import scipy.ndimage as ndi
    lab, n = ndi.label(state > 0, structure=np.ones((3, 3), dtype=int))
    keep = np.zeros(n + 1, dtype=bool)
    keep[np.unique(lab[state == R.STRONG])] = True
    keep[0] = False
    return np.where(keep[lab], 255, 0).astype(np.uint8)


@pytest.mark.parametrize("case", ["noise_l1", "noise_l2", "ramp", "border", "serpentine", "serpentine_off", "tile_border"])
def test_flood_hysteresis_is_the_labelled_components_that_hold_a_strong_pixel(case):
    state = {"noise_l1": lambda: R.canny_state_ref(R.noise_image(67, 131, 7)[0], 400, 800, False),
             "noise_l2": lambda: R.canny_state_ref(R.noise_image(67, 131, 7)[0], 300, 600, True),
             "ramp": lambda: R.canny_state_ref(R.ramp_steps_image(67, 131), 5, 300),
             "border": lambda: R.canny_state_ref(R.border_image(40, 70), 50, 400),
             "serpentine": lambda: R.serpentine_state(130, 200),
             "serpentine_off": lambda: R.serpentine_state(130, 200, strong=False),
             "tile_border": lambda: R.tile_border_state(130, 200)}[case]()
    out = R.hysteresis_ref(state)
    assert np.array_equal(out, _label_hysteresis(state))
    assert set(np.unique(out)) <= {0, 255} and bool((out[state == R.STRONG] == 255).all()) and not bool(out[state == R.OFF].any())
    if case == "serpentine":
        assert np.array_equal(out > 0, state > 0) and int((state == R.STRONG).sum()) == 1          # one chain, lit from one end
    if case == "serpentine_off":
        assert not out.any() and int((state == R.WEAK).sum()) > 4000
    if case == "tile_border":
        assert out[63, 63] == out[64, 64] == 255 and out[63, 128] == out[64, 127] == 255             # through both tile corners
        assert out[63, 10] == out[64, 20] == out[10, 63] == out[20, 64] == 255                       # lit from across row / column 63 | 64
        assert not out[100, 100:110].any() and not out[63:66, 150].any()


def test_sobel_is_the_plain_loop():
    g = R.noise_image(9, 11, 5)[0]
    dx, dy = R.sobel_ref(g)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
    for y in range(9):
        for x in range(11):
            win = np.array([[int(g[min(max(y + j, 0), 8), min(max(x + i, 0), 10)]) for i in (-1, 0, 1)] for j in (-1, 0, 1)])
            assert dx[y, x] == int((win * kx).sum()) and dy[y, x] == int((win * kx.T).sum())
    flat = np.full((5, 7), 200, dtype=np.uint8)
    assert not R.sobel_ref(flat)[0].any() and not R.sobel_ref(flat)[1].any()                       # the replicated border adds no edge


def _field(dx, dy, shape=(5, 5)):
    return np.full(shape, dx, dtype=np.int64), np.full(shape, dy, dtype=np.int64)


def test_nms_direction_sectors_and_ties():
    W, S = R.WEAK, R.STRONG
    # horizontal gradient (dy = 0): compared along the row; `>` to the left, `>=` to the right
    dx = np.array([[10, 20, 20, 10, 0]] * 3)
    st = R.nms_state_ref(dx, np.zeros_like(dx), 5, 100, False)
    assert st[1].tolist() == [0, W, 0, 0, 0]                                                       # of the tie 20 | 20 the LEFT one survives (20 > 10 and 20 >= 20)
    st = R.nms_state_ref(dx, np.zeros_like(dx), 5, 15, False)
    assert st[1].tolist() == [0, S, 0, 0, 0]
    st = R.nms_state_ref(dx[:, ::-1], np.zeros_like(dx), 5, 100, False)                            # mirrored: the tie's left one again, which was the right one
    assert st[1].tolist() == [0, 0, W, 0, 0]
    # vertical gradient (dx = 0): compared along the column; `>` above, `>=` below
    st = R.nms_state_ref(np.zeros_like(dx.T), dx.T, 5, 100, False)
    assert st[:, 1].tolist() == [0, W, 0, 0, 0]
    # diagonals: dx, dy of one sign compare (y-1, x-1) and (y+1, x+1); of opposite signs (y-1, x+1) and (y+1, x-1); both strictly
    m = np.zeros((5, 5), dtype=np.int64)
    m[2, 2], m[1, 1], m[3, 3], m[1, 3], m[3, 1] = 10, 10, 3, 3, 3
    st = R.nms_state_ref(m, m, 1, 100, False)                                                      # same sign: (1, 1) ties with (2, 2) -> both dropped along the main diagonal
    assert st[2, 2] == 0 and st[1, 1] == 0 and st[3, 3] == 0 and st[1, 3] == W and st[3, 1] == W
    st = R.nms_state_ref(m, -m, 1, 100, False)                                                     # opposite signs: the anti-diagonal neighbours (1, 3), (3, 1) are smaller
    assert st[2, 2] == W and st[1, 1] == W and st[3, 3] == W and st[1, 3] == 0
    # the sector borders: tan 22.5 = 13573 / 32768 and tan 67.5 = that + 2, in 15-bit fixed point
    x = 32768
    for dy, sector in ((13572, "h"), (13573, "d"), (13573 + 65536, "d"), (13573 + 65536 + 1, "v")):
        ddx, ddy = _field(x, dy, (3, 3))
        centre = x + dy
        # make every neighbour but one pair larger than the centre: the pixel survives iff its sector looks at the smaller pair
        gx, gy = ddx.copy(), ddy.copy()
        for (py, px), kind in {(1, 0): "h", (1, 2): "h", (0, 1): "v", (2, 1): "v", (0, 0): "d", (2, 2): "d", (0, 2): "x", (2, 0): "x"}.items():
            gx[py, px] = x // 2 if kind == sector else 2 * x
        st = R.nms_state_ref(gx, gy, 1, 10 * centre, False)
        assert st[1, 1] == W, (dy, sector)
    # nothing at or below lo, strong strictly above hi, L2 uses the squared thresholds
    dx1 = np.array([[0, 7, 0]] * 3)
    assert R.nms_state_ref(dx1, np.zeros_like(dx1), 7, 100, False)[1, 1] == 0 and R.nms_state_ref(dx1, np.zeros_like(dx1), 6, 7, False)[1, 1] == W
    assert R.nms_state_ref(dx1, np.zeros_like(dx1), *R.thresholds_ref(6.9, 6.2, True), True)[1, 1] == S      # swapped, floored: 49 > 36
    assert R.thresholds_ref(200, 100.7, False) == (100, 200)
    # the magnitude outside the image is 0: a one-pixel image keeps its pixel
    assert R.nms_state_ref(np.array([[4]]), np.array([[0]]), 1, 2, False)[0, 0] == S


def test_grey_gauss_and_conversion_rules():
    assert R.grey_ref(np.array([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=np.uint8)).tolist() == [255, 0, 76, 150, 29]
    src = R.noise_image(6, 7, 2, B=2)[..., None]
    assert np.array_equal(R.gauss_ref(src, [4096]), src)                                           # r = 0 copies
    flat = np.full((1, 3, 4, 3), 77, dtype=np.uint8)
    assert np.array_equal(R.gauss_ref(flat, [1366, 1365]), flat)                                   # a flat image stays flat under any taps, any radius
    c = R.condition_ref(np.arange(256, dtype=np.uint8).reshape(1, 16, 16))
    assert c.shape == (1, 3, 16, 16) and c.dtype == np.float16 and c[0, 0, 0, 0] == 0 and c[0, 2, 15, 15] == 1 and np.array_equal(c[0, 0], c[0, 1])


# ---- the host side of the product ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.0, -1.0, 0.1, 0.3, 0.5, 0.8, 1.0, 1.4, 2.0, 3.0, 5.0, 7.77, 10.6, 10.7, 11.0, 25.0, 1000.0])
def test_gauss_taps_sum_to_4096(sigma):
    from instructany2pix_amd.condition import gauss_taps
    q = gauss_taps(sigma)
    r = len(q) - 1
    assert q.dtype == np.uint16 and int(q[0]) + 2 * int(q[1:].astype(np.int64).sum()) == 4096
    assert r == (0 if sigma <= 0 else min(32, int(np.ceil(3 * sigma))))
    assert all(int(q[i]) >= int(q[i + 1]) for i in range(1, r)) and int(q[0]) > 0                  # a bell; the centre takes what the rounding of the others leaves
    if r:
        i = np.arange(r + 1, dtype=np.float64)
        w = np.exp(-i * i / (2 * sigma * sigma))
        w /= w[0] + 2 * w[1:].sum()
        assert np.array_equal(q[1:], np.rint(4096 * w[1:]).astype(np.uint16))


def test_condition_specs_resolve_or_refuse():
    from instructany2pix_amd.condition import Condition, resolve
    assert resolve("canny") == Condition() and resolve("grey").kind == "grey" and resolve(Condition(kind="blur", sigma=2)).sigma == 2
    c = resolve({"kind": "canny", "low": 50, "high": 150, "blur_sigma": 1.4})
    assert (c.low, c.high, c.blur_sigma, c.l2_gradient) == (50, 150, 1.4, False)
    for bad in ("depth", {"low": 3}, {"kind": "hed"}, {"kind": "grey", "sigma": 2}, {"kind": "blur", "low": 1}, 7, None,
                {"kind": "canny", "low": -1}, {"kind": "canny", "high": float("nan")}, {"kind": "blur", "sigma": float("inf")}, {"kind": "canny", "low": "3"}):
        with pytest.raises(ValueError):
            resolve(bad)


def test_pipeline_refusals_come_before_any_device_call():
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline, check_control_from
    call = InstructAny2PixPipeline.__call__
    bare, with_cn = SimpleNamespace(controlnet=None), SimpleNamespace(controlnet=object())         # nothing else exists: whatever else the call touched would raise AttributeError
    with pytest.raises(ValueError, match="controlnet="):
        call(bare, "edit", [], control_from="canny")
    with pytest.raises(ValueError, match="one of the two"):
        call(with_cn, "edit", [], control_from="canny", control_image=np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="kind"):
        call(with_cn, "edit", [], control_from="depth")
    with pytest.raises(ValueError, match="no \\['sigma'\\]"):
        call(with_cn, "edit", [], control_from={"kind": "canny", "sigma": 2.0})
    assert check_control_from(with_cn, {"kind": "blur", "sigma": 1.5}, None).sigma == 1.5
    with pytest.raises(ValueError, match="base latents only"):
        InstructAny2PixPipeline.control_map(with_cn, check_control_from(with_cn, "canny", None), None)
    # control is not in the batch paths: the keyword does not appear there half-built
    for name in ("edit_batch", "denoise_batch", "inpaint_batch"):
        fn = getattr(InstructAny2PixPipeline, name, None)
        assert fn is None or "control_from" not in inspect.signature(fn).parameters
    for name in ("__call__", "denoise"):
        assert inspect.signature(getattr(InstructAny2PixPipeline, name)).parameters["control_from"].default is None


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def test_new_names_are_declared_bound_and_exported(lib):
    from instructany2pix_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "ia2p.h")).read()
    declared = set(re.findall(r"\b(ia2p_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_NAMES:
        assert name in declared and name in _ffi.SIGNATURES and hasattr(lib, name), name
    assert "condition.hip" in __import__("instructany2pix_amd.build", fromlist=["SOURCES"]).SOURCES


def test_workspace_sizes_and_the_round_bound(lib):
    assert lib.ia2p_image_gauss_workspace_bytes(2, 67, 131, 3) == 2 * 67 * 131 * 3 * 4 and lib.ia2p_image_gauss_workspace_bytes(0, 4, 4, 1) == 0
    assert lib.ia2p_canny_workspace_bytes(1, 64, 64) == 4096 + 16 and lib.ia2p_canny_workspace_bytes(2, 67, 131) == ((2 * 67 * 131 + 15) // 16) * 16 + 16
    assert lib.ia2p_canny_workspace_bytes(1, 0, 5) == 0

    def bound(B, H, W):                                                                            # 2 B ring + 2, ring = the pixels on the outermost ring of their 64 x 64 tile
        inner = lambda n: sum(max(min(64, n - o) - 2, 0) for o in range(0, n, 64))                 # noqa: E731
        return 2 * B * (H * W - inner(H) * inner(W)) + 2
    for shape in ((1, 64, 64), (1, 1, 17), (1, 17, 1), (1, 3, 3), (2, 67, 131), (2, 130, 200), (1, 1024, 1024)):
        assert lib.ia2p_canny_max_rounds(*shape) == bound(*shape), shape
    assert lib.ia2p_canny_max_rounds(1, 64, 64) == 2 * 252 + 2 and lib.ia2p_canny_max_rounds(1, 1, 17) == 36


def test_refusals_come_before_any_hip_call(lib):
    INVALID, SHAPE, NOMEM = 1, 2, 5
    a, b, w = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)
    taps = (C.c_uint16 * 33)(*([4096] + [0] * 32))
    t3 = (C.c_uint16 * 2)(1366, 1365)
    bad = (C.c_uint16 * 2)(1366, 1366)
    big = 1 << 20
    nan, inf = float("nan"), float("inf")
    cases = [
        (INVALID, lib.ia2p_image_grey_u8(None, None, b, 1, 8, 8)),
        (INVALID, lib.ia2p_image_grey_u8(None, a, None, 1, 8, 8)),
        (INVALID, lib.ia2p_image_grey_u8(None, a, a, 1, 8, 8)),                                    # aliased
        (INVALID, lib.ia2p_image_grey_u8(None, a, C.c_void_p((1 << 20) + 100), 1, 8, 8)),          # overlapping
        (INVALID, lib.ia2p_image_grey_u8(None, a, b, 1, -8, 8)),
        (SHAPE, lib.ia2p_image_grey_u8(None, a, b, 0, 8, 8)),
        (SHAPE, lib.ia2p_image_grey_u8(None, a, b, 1, 1 << 15, 1 << 15)),                          # B H W 3 >= 2^31
        (INVALID, lib.ia2p_image_gauss_u8(None, a, b, w, 1, 8, 8, 3, None, 0)),
        (INVALID, lib.ia2p_image_gauss_u8(None, a, b, None, 1, 8, 8, 3, taps, 0)),
        (INVALID, lib.ia2p_image_gauss_u8(None, a, b, C.c_void_p((3 << 20) + 2), 1, 8, 8, 3, taps, 0)),     # 32-bit sums off the 4-byte grid
        (SHAPE, lib.ia2p_image_gauss_u8(None, a, b, w, 1, 8, 8, 2, taps, 0)),
        (SHAPE, lib.ia2p_image_gauss_u8(None, a, b, w, 1, 0, 8, 3, taps, 0)),
        (INVALID, lib.ia2p_image_gauss_u8(None, a, b, w, 1, 8, 8, 3, taps, 33)),
        (INVALID, lib.ia2p_image_gauss_u8(None, a, b, w, 1, 8, 8, 3, taps, -1)),
        (INVALID, lib.ia2p_image_gauss_u8(None, a, b, w, 1, 8, 8, 3, bad, 1)),                     # taps that do not sum to 4096
        (INVALID, lib.ia2p_image_gauss_u8(None, a, b, a, 1, 8, 8, 3, t3, 1)),                      # the workspace is the source
        (INVALID, lib.ia2p_image_gauss_u8(None, a, C.c_void_p((1 << 20) + 8), w, 1, 8, 8, 3, t3, 1)),      # dst overlaps src without being src
        (INVALID, lib.ia2p_canny_u8(None, None, b, w, big, 1, 8, 8, 100.0, 200.0, 0, None)),
        (INVALID, lib.ia2p_canny_u8(None, a, None, w, big, 1, 8, 8, 100.0, 200.0, 0, None)),
        (INVALID, lib.ia2p_canny_u8(None, a, b, None, big, 1, 8, 8, 100.0, 200.0, 0, None)),
        (INVALID, lib.ia2p_canny_u8(None, a, a, w, big, 1, 8, 8, 100.0, 200.0, 0, None)),          # edges == grey
        (INVALID, lib.ia2p_canny_u8(None, a, b, C.c_void_p((3 << 20) + 1), big, 1, 8, 8, 100.0, 200.0, 0, None)),
        (NOMEM, lib.ia2p_canny_u8(None, a, b, w, 64 + 15, 1, 8, 8, 100.0, 200.0, 0, None)),        # 64 state bytes + 16 flag bytes are needed
        (INVALID, lib.ia2p_canny_u8(None, a, b, a, big, 1, 8, 8, 100.0, 200.0, 0, None)),          # the workspace is the image
        (INVALID, lib.ia2p_canny_u8(None, a, b, w, big, 1, 8, 8, -1.0, 200.0, 0, None)),
        (INVALID, lib.ia2p_canny_u8(None, a, b, w, big, 1, 8, 8, 100.0, -0.5, 0, None)),
        (INVALID, lib.ia2p_canny_u8(None, a, b, w, big, 1, 8, 8, nan, 200.0, 0, None)),
        (INVALID, lib.ia2p_canny_u8(None, a, b, w, big, 1, 8, 8, 100.0, nan, 0, None)),
        (INVALID, lib.ia2p_canny_u8(None, a, b, w, big, 1, 8, 8, 100.0, inf, 0, None)),
        (INVALID, lib.ia2p_canny_u8(None, a, b, w, big, 1, 8, 8, 100.0, 200.0, 2, None)),
        (SHAPE, lib.ia2p_canny_u8(None, a, b, w, big, 1, 8, 0, 100.0, 200.0, 0, None)),
        (INVALID, lib.ia2p_canny_hysteresis_u8(None, None, b, w, big, 1, 8, 8, None)),
        (INVALID, lib.ia2p_canny_hysteresis_u8(None, a, a, w, big, 1, 8, 8, None)),
        (NOMEM, lib.ia2p_canny_hysteresis_u8(None, a, b, w, 0, 1, 8, 8, None)),
        (INVALID, lib.ia2p_condition_from_u8(None, None, b, 1, 8, 8, 1)),
        (INVALID, lib.ia2p_condition_from_u8(None, a, None, 1, 8, 8, 3)),
        (INVALID, lib.ia2p_condition_from_u8(None, a, C.c_void_p((2 << 20) + 1), 1, 8, 8, 1)),     # halfs off the 2-byte grid
        (INVALID, lib.ia2p_condition_from_u8(None, a, a, 1, 8, 8, 1)),
        (SHAPE, lib.ia2p_condition_from_u8(None, a, b, 1, 8, 8, 2)),
        (SHAPE, lib.ia2p_condition_from_u8(None, a, b, 1, 8, 0, 1)),
    ]
    for i, (want, got) in enumerate(cases):
        assert got == want, (i, want, got)
    rounds = C.c_int(7)
    assert lib.ia2p_canny_u8(None, a, a, w, big, 1, 8, 8, 100.0, 200.0, 0, C.byref(rounds)) == INVALID and rounds.value == 0
