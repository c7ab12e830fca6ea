"""Condition maps from the base image, on the device (csrc/condition.hip; include/ia2p.h, "condition maps").

A ControlNet is guided by a map of the structure that must survive the edit. The map almost always comes from the base image the pipeline already holds; the
three detectors that need no weights are made here, as integer HIP kernels:

  canny   OpenCV's `cv::Canny` (8-bit input, aperture 3) on the grey image, optionally after a Gaussian blur ("blur, then Canny"), edges 255 on 0
  blur    a separable Gaussian blur of the image (the blur / tile control models)
  grey    OpenCV's 8-bit RGB2GRAY rule (the recolor control models)

Images are uint8 tensors on the device, [H, W, 3] or [B, H, W, 3], or one channel as [H, W], [B, H, W] or [B, H, W, 1] (a three-dimensional tensor whose last
size is 3 is one RGB image; any other three-dimensional tensor is a batch of one-channel images). PIL images, numpy uint8 arrays and paths are taken as
`pipeline.control_tensor` takes them (`convert("RGB")`, then the 8-bit upload). The maps keep the batch form of their input. `to_condition` turns a map into the fp16
[B, 3, H, W] tensor in [0, 1] that `HipControlNetModel.embed_condition` takes.

OpenCV is not installed next to this package: parity with it is restated (tests/canny_ref.py), not pinned.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os

import numpy as np
import PIL.Image
import torch

from . import _ffi

KINDS = ("canny", "blur", "grey")
GAUSS_MAX_RADIUS = 32


def gauss_taps(sigma) -> np.ndarray:
    """The integer taps q_0 .. q_r of the Gaussian (centre first; uint16, q_0 + 2 sum_{i>=1} q_i == 4096): r = min(32, ceil(3 sigma)),
    w_i = exp(-i^2 / (2 sigma^2)) in float64 normalised over the 2 r + 1 taps, q_i = rint(4096 w_i) for i >= 1 and q_0 takes the rest. sigma <= 0: r = 0, no blur."""
    sigma = float(sigma)
    if not math.isfinite(sigma):
        raise ValueError(f"sigma must be finite, got {sigma!r}")
    if sigma <= 0:
        return np.array([4096], dtype=np.uint16)
    r = min(GAUSS_MAX_RADIUS, int(math.ceil(3.0 * sigma)))
    i = np.arange(r + 1, dtype=np.float64)
    w = np.exp(-(i * i) / (2.0 * sigma * sigma))
    w /= w[0] + 2.0 * w[1:].sum()
    q = np.rint(4096.0 * w).astype(np.int64)
    q[0] = 4096 - 2 * int(q[1:].sum())
    assert 0 < q[0] <= 4096
    return q.astype(np.uint16)


@dataclasses.dataclass(frozen=True)
class Condition:
    """What map to make: `kind` and the knobs of that kind. canny: `low`, `high` (thresholds on the gradient magnitude, swapped when low > high), `blur_sigma`
    (> 0: a Gaussian blur of the grey image before the Sobel; `cv::Canny` itself does not blur), `l2_gradient`. blur: `sigma` (3.0 is a design choice). grey: none."""
    kind: str = "canny"
    low: float = 100.0
    high: float = 200.0
    blur_sigma: float = 0.0
    l2_gradient: bool = False
    sigma: float = 3.0

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"condition kind must be one of {KINDS}, got {self.kind!r}")
        for name in ("low", "high", "blur_sigma", "sigma"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
                raise ValueError(f"condition {name} must be a finite number, got {v!r}")
        if self.low < 0 or self.high < 0:
            raise ValueError(f"canny thresholds must be >= 0, got low={self.low!r} high={self.high!r}")


_KNOBS = {"canny": ("low", "high", "blur_sigma", "l2_gradient"), "blur": ("sigma",), "grey": ()}


def resolve(spec) -> Condition:
    """"canny" / "blur" / "grey", a dict such as {"kind": "canny", "low": 50, "high": 150, "blur_sigma": 1.4}, or a `Condition` -> a `Condition`. An unknown kind, or
    a knob the kind does not have, is a ValueError; nothing touches the device."""
    if isinstance(spec, Condition):
        return spec
    if isinstance(spec, str):
        return Condition(kind=spec)
    if isinstance(spec, dict):
        d = dict(spec)
        kind = d.pop("kind", None)
        if kind not in KINDS:
            raise ValueError(f"condition kind must be one of {KINDS}, got {kind!r}")
        unknown = sorted(set(d) - set(_KNOBS[kind]))
        if unknown:
            raise ValueError(f"a {kind!r} condition has no {unknown} (its knobs: {list(_KNOBS[kind])})")
        return Condition(kind=kind, **d)
    raise ValueError(f"a condition is one of {KINDS}, a dict with 'kind' or a Condition, got {type(spec).__name__}")


# ---- images in -------------------------------------------------------------------------------------------------------------------------------------------
def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def as_u8(image, device=None):
    """-> (uint8 [B, H, W, C] contiguous on the device, C in (1, 3); whether the input carried a batch dimension)"""
    if isinstance(image, (str, os.PathLike)):
        image = PIL.Image.open(image)
    if isinstance(image, PIL.Image.Image):
        image = np.asarray(image.convert("RGB"))
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise TypeError(f"a condition is made from 8-bit pixels; got a {image.dtype} array")
        image = torch.from_numpy(np.ascontiguousarray(image))
    if not torch.is_tensor(image) or image.dtype != torch.uint8:
        raise TypeError("a condition is made from a uint8 tensor, a uint8 array, a PIL image or a path")
    t, batched = image, image.ndim == 4 or (image.ndim == 3 and image.shape[-1] != 3)
    if t.ndim == 2:
        t = t[None, :, :, None]
    elif t.ndim == 3:
        t = t[None] if t.shape[-1] == 3 else t[..., None]
    elif t.ndim != 4 or t.shape[-1] not in (1, 3):
        raise ValueError(f"an image is [H, W, 3], [B, H, W, 3], [H, W], [B, H, W] or [B, H, W, 1]; got {tuple(image.shape)}")
    if min(t.shape) < 1:
        raise ValueError(f"empty image {tuple(image.shape)}")
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    return t.contiguous(), batched


def _grey4(t):
    """uint8 [B, H, W, C] -> grey uint8 [B, H, W] (one launch for C = 3; a view for C = 1)"""
    B, H, W, Ch = t.shape
    if Ch == 1:
        return t.reshape(B, H, W)
    out = torch.empty(B, H, W, dtype=torch.uint8, device=t.device)
    with torch.cuda.device(t.device):
        _ffi.check(_ffi.lib().ia2p_image_grey_u8(_stream(t.device), _ffi.ptr(t), _ffi.ptr(out), B, H, W))
    return out


def _blur4(t, sigma):
    """uint8 [B, H, W, C] -> the same shape, blurred (sigma <= 0: the input itself)"""
    taps = gauss_taps(sigma)
    r = len(taps) - 1
    if r == 0:
        return t
    B, H, W, Ch = t.shape
    lib = _ffi.lib()
    out = torch.empty_like(t)
    ws = torch.empty(lib.ia2p_image_gauss_workspace_bytes(B, H, W, Ch) // 4, dtype=torch.int32, device=t.device)
    q = (C.c_uint16 * (r + 1))(*[int(v) for v in taps])
    with torch.cuda.device(t.device):
        _ffi.check(lib.ia2p_image_gauss_u8(_stream(t.device), _ffi.ptr(t), _ffi.ptr(out), _ffi.ptr(ws), B, H, W, Ch, q, r))
    return out


def _canny3(g, low, high, l2_gradient):
    """grey uint8 [B, H, W] -> (edges uint8 [B, H, W] in {0, 255}, hysteresis rounds)"""
    B, H, W = g.shape
    lib = _ffi.lib()
    out = torch.empty_like(g)
    ws = torch.empty((lib.ia2p_canny_workspace_bytes(B, H, W) + 3) // 4, dtype=torch.int32, device=g.device)
    rounds = C.c_int(0)
    with torch.cuda.device(g.device):
        _ffi.check(lib.ia2p_canny_u8(_stream(g.device), _ffi.ptr(g), _ffi.ptr(out), _ffi.ptr(ws), ws.numel() * 4, B, H, W, float(low), float(high),
                                     int(bool(l2_gradient)), C.byref(rounds)))
    return out, rounds.value


# ---- the maps ----------------------------------------------------------------------------------------------------------------------------------------------
def grey(image):
    """-> uint8 [H, W] or [B, H, W]: Y = (4899 R + 9617 G + 1868 B + 8192) >> 14"""
    t, batched = as_u8(image)
    out = _grey4(t)
    return out if batched else out[0]


def blur(image, sigma):
    """-> the image's own shape (channels kept): separable Gaussian blur by `gauss_taps(sigma)`, replicated border"""
    t, batched = as_u8(image)
    out = _blur4(t, sigma)
    return out if batched else out[0]


def canny(image, low=100, high=200, blur_sigma=0.0, l2_gradient=False, return_rounds=False):
    """-> uint8 [H, W] or [B, H, W] in {0, 255} (with `return_rounds`: and the number of hysteresis rounds the call took): grey, the optional blur, the detector."""
    c = Condition(kind="canny", low=low, high=high, blur_sigma=blur_sigma, l2_gradient=l2_gradient)
    t, batched = as_u8(image)
    g = _grey4(t)
    g = _blur4(g[..., None], c.blur_sigma)[..., 0] if c.blur_sigma > 0 else g
    out, rounds = _canny3(g.contiguous(), c.low, c.high, c.l2_gradient)
    out = out if batched else out[0]
    return (out, rounds) if return_rounds else out


def make(spec, image_u8):
    """the map `spec` (`resolve`) asks for, of `image_u8`"""
    c = resolve(spec)
    if c.kind == "canny":
        return canny(image_u8, c.low, c.high, c.blur_sigma, c.l2_gradient)
    if c.kind == "blur":
        return blur(image_u8, c.sigma)
    return grey(image_u8)


def to_condition(map_u8) -> torch.Tensor:
    """a map (any form `as_u8` takes) -> fp16 [B, 3, H, W] in [0, 1]: q / 255 with one rounding, a one-channel map replicated to three -- the bits
    `image_processor.image_from_u8(normalize=False)` gives for the same bytes"""
    t, _ = as_u8(map_u8)
    B, H, W, Ch = t.shape
    out = torch.empty(B, 3, H, W, dtype=torch.float16, device=t.device)
    with torch.cuda.device(t.device):
        _ffi.check(_ffi.lib().ia2p_condition_from_u8(_stream(t.device), _ffi.ptr(t), _ffi.ptr(out), B, H, W, Ch))
    return out
