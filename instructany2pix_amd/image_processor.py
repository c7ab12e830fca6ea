"""Images in and out of the pipelines: diffusers 0.26.3 `VaeImageProcessor` with the per-pixel work on the HIP codec (csrc/image.hip).

The reference loads a base image file, hands it to `image_processor.preprocess` before the VAE encode (instructany2pix/ddim/pnp_pipeline.py:190-204)
and returns what `image_processor.postprocess(image, output_type="pil")` makes of the decode (ddim/sdxl_pipeline.py:859-880). Here:

  preprocess   PIL / list of PIL / uint8 HWC ndarray -> resize on the host in PIL (exactly the reference's resampling) -> uint8 to the device ->
               `ia2p_image_from_u8` (q / 255, 2 v - 1, HWC -> NCHW, fp16).  Float [0, 1] arrays / tensors follow diffusers' float branch;
               float tensors in [-1, 1] and 4-channel latents pass through.
  postprocess  fp16 [-1, 1] NCHW on the device -> "pil": `ia2p_image_to_u8` (only uint8 comes back to the host), "np" / "pt": `ia2p_image_to_f32`,
               "latent": unchanged.

Both directions equal diffusers' numpy / torch arithmetic bit for bit (tests/test_image_io_gpu.py checks every 8-bit code and every fp16 pattern).

Editing inside a mask adds the mask's side: `load_edit_mask` (forms and sizes of a user's mask, on the host), `mask_to_latent`, `mask_feather`
and `image_composite` (integer HIP kernels of csrc/image.hip: the latent mask, the inward seam feather, the 8-bit composite with the base image).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import List, Union

import numpy as np
import PIL.Image
import torch

from . import _ffi

OUTPUT_TYPES = ("latent", "pt", "np", "pil")
PIL_INTERPOLATION = {"linear": PIL.Image.Resampling.BILINEAR, "bilinear": PIL.Image.Resampling.BILINEAR, "bicubic": PIL.Image.Resampling.BICUBIC,
                     "lanczos": PIL.Image.Resampling.LANCZOS, "nearest": PIL.Image.Resampling.NEAREST}


# ---- the HIP codec (include/ia2p.h, "image codec") ---------------------------------------------------------------------------------------------
def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _device_tensor(t, dtype, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise TypeError(f"{what} expects a contiguous {dtype} tensor on the GPU")
    return t


def image_from_u8(u8: torch.Tensor, normalize: bool = True) -> torch.Tensor:
    """uint8 [B,H,W,C] on the device -> fp16 [B,C,H,W]: 2 q / 255 - 1 (normalize) or q / 255."""
    _device_tensor(u8, torch.uint8, "image_from_u8")
    if u8.ndim != 4:
        raise ValueError(f"image_from_u8 expects [B,H,W,C], got {tuple(u8.shape)}")
    B, H, W, Ch = u8.shape
    out = torch.empty(B, Ch, H, W, dtype=torch.float16, device=u8.device)
    with torch.cuda.device(u8.device):
        _ffi.check(_ffi.lib().ia2p_image_from_u8(_stream(u8.device), _ffi.ptr(u8), _ffi.ptr(out), B, H, W, Ch, int(bool(normalize))))
    return out


def image_to_u8(x: torch.Tensor) -> torch.Tensor:
    """fp16 [B,C,H,W] in [-1, 1] on the device -> uint8 [B,H,W,C]: rint(clamp(x / 2 + 0.5, 0, 1) * 255), NaN -> 0."""
    _device_tensor(x, torch.float16, "image_to_u8")
    B, Ch, H, W = x.shape
    out = torch.empty(B, H, W, Ch, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _ffi.check(_ffi.lib().ia2p_image_to_u8(_stream(x.device), _ffi.ptr(x), _ffi.ptr(out), B, H, W, Ch))
    return out


def image_to_f32(x: torch.Tensor, nhwc: bool) -> torch.Tensor:
    """fp16 [B,C,H,W] on the device -> float32 clamp(x / 2 + 0.5, 0, 1) as [B,H,W,C] (nhwc) or [B,C,H,W]."""
    _device_tensor(x, torch.float16, "image_to_f32")
    B, Ch, H, W = x.shape
    out = torch.empty((B, H, W, Ch) if nhwc else (B, Ch, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _ffi.check(_ffi.lib().ia2p_image_to_f32(_stream(x.device), _ffi.ptr(x), _ffi.ptr(out), B, H, W, Ch, int(bool(nhwc))))
    return out


def requantize(x: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """The 8-bit round trip of an fp16 image in [-1, 1] in one launch: equals `pipeline.to_8bit_image` bit for bit. `out` may be `x`."""
    _device_tensor(x, torch.float16, "requantize")
    out = torch.empty_like(x) if out is None else _device_tensor(out, torch.float16, "requantize")
    if out.shape != x.shape:
        raise ValueError("requantize: out must have the shape of x")
    with torch.cuda.device(x.device):
        _ffi.check(_ffi.lib().ia2p_image_requantize(_stream(x.device), _ffi.ptr(x), _ffi.ptr(out), x.numel()))
    return out


# ---- editing inside a mask (include/ia2p.h, "edit mask") -------------------------------------------------------------------------------------------------
EDIT_FEATHER_MAX = 64


def check_edit_feather(r) -> int:
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= int(r) <= EDIT_FEATHER_MAX:
        raise ValueError(f"edit_feather must be an integer radius of 0 .. {EDIT_FEATHER_MAX} pixels, got {r!r}")
    return int(r)


def mask_to_latent(mask_u8: torch.Tensor, f: int) -> torch.Tensor:
    """uint8 [B, H, W] on the device -> fp16 [B, 1, H / f, W / f]: 1.0 where any pixel of the cell's f x f block is >= 128."""
    _device_tensor(mask_u8, torch.uint8, "mask_to_latent")
    if mask_u8.ndim != 3:
        raise ValueError(f"mask_to_latent expects [B,H,W], got {tuple(mask_u8.shape)}")
    B, H, W = mask_u8.shape
    f = int(f)
    out = torch.empty(B, 1, H // max(f, 1), W // max(f, 1), dtype=torch.float16, device=mask_u8.device)
    with torch.cuda.device(mask_u8.device):
        _ffi.check(_ffi.lib().ia2p_mask_to_latent(_stream(mask_u8.device), _ffi.ptr(mask_u8), _ffi.ptr(out), B, H, W, f))
    return out


def mask_feather(mask_u8: torch.Tensor, r: int) -> torch.Tensor:
    """uint8 [B, H, W] on the device -> the compositing alpha, uint8 [B, H, W]: min(bin, box mean of bin over (2 r + 1)^2, edge replicate, rounded) with
    bin = 255 where the mask is >= 128. The ramp lies inside the mask: alpha is 0 wherever the mask is 0."""
    _device_tensor(mask_u8, torch.uint8, "mask_feather")
    if mask_u8.ndim != 3:
        raise ValueError(f"mask_feather expects [B,H,W], got {tuple(mask_u8.shape)}")
    B, H, W = mask_u8.shape
    out, ws = torch.empty_like(mask_u8), torch.empty(B, H, W, dtype=torch.int16, device=mask_u8.device)
    with torch.cuda.device(mask_u8.device):
        _ffi.check(_ffi.lib().ia2p_mask_feather_u8(_stream(mask_u8.device), _ffi.ptr(mask_u8), _ffi.ptr(out), _ffi.ptr(ws), B, H, W, int(r)))
    return out


def image_composite(edited: torch.Tensor, base: torch.Tensor, alpha: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """uint8 [B, H, W, C] images and uint8 [B, H, W] alpha on the device -> (a e + (255 - a) b + 127) / 255 per byte. `out` may be `edited`."""
    for t in (edited, base, alpha):
        _device_tensor(t, torch.uint8, "image_composite")
    out = torch.empty_like(edited) if out is None else _device_tensor(out, torch.uint8, "image_composite")
    if edited.ndim != 4 or base.shape != edited.shape or out.shape != edited.shape or tuple(alpha.shape) != tuple(edited.shape[:3]):
        raise ValueError(f"image_composite expects [B,H,W,C] images of one shape and a [B,H,W] alpha, got {tuple(edited.shape)}, {tuple(base.shape)}, {tuple(alpha.shape)}")
    B, H, W, Ch = edited.shape
    with torch.cuda.device(edited.device):
        _ffi.check(_ffi.lib().ia2p_image_composite_u8(_stream(edited.device), _ffi.ptr(edited), _ffi.ptr(base), _ffi.ptr(alpha), _ffi.ptr(out), B, H, W, Ch))
    return out


def fit_edit_mask(mask: PIL.Image.Image, size: int) -> PIL.Image.Image:
    """a mask of the base image FILE's size through what `loas_base_img` does to the image: the geometry of `resize_and_crop(..., 'middle')` (scaled side
    truncated to an int, float crop box) and the final resize, every resampling NEAREST, so that it stays registered with the image and stays binary"""
    near = PIL.Image.Resampling.NEAREST
    w, h = mask.size
    if w > h:                                       # relatively wider than the square: fit the height, crop columns
        mask = mask.resize((int(size * w / h), size), near)
        lo = (mask.size[0] - size) / 2
        mask = mask.crop((lo, 0, lo + size, mask.size[1]))
    elif w < h:                                     # relatively taller: fit the width, crop rows
        mask = mask.resize((size, int(size * h / w)), near)
        lo = (mask.size[1] - size) / 2
        mask = mask.crop((0, lo, mask.size[0], lo + size))
    return mask.resize((size, size), near)


def load_edit_mask(mask, height: int, width: int, file_size=None) -> np.ndarray:
    """The mask-loading rule of an edit inside a mask -> uint8 [height, width] in {0, 255}, 255 = "may change".
    Forms: a PIL image of any mode (converted to "L"), a file path, a numpy uint8 / bool / float [H, W] array; binarised at 128 (floats at 0.5).
    Sizes: height x width (the pixels the base latents stand for: `base_image_size` squared for a loaded base image file, vae_scale_factor x the latent
    grid for latent-only callers) is used as is; `file_size` = (width, height) of the base image FILE goes through `fit_edit_mask`. Any other size raises."""
    if isinstance(mask, (str, bytes)) or hasattr(mask, "__fspath__"):
        mask = PIL.Image.open(mask)
    if isinstance(mask, PIL.Image.Image):
        a = np.asarray(mask.convert("L"))
    elif isinstance(mask, np.ndarray):
        a = mask
    else:
        raise TypeError(f"edit_mask must be a PIL image, a numpy [H, W] array or a file path, got {type(mask)}")
    if a.ndim != 2:
        raise ValueError(f"edit_mask must be one [H, W] plane, got shape {tuple(a.shape)}")
    if a.dtype == np.bool_:
        on = a
    elif a.dtype == np.uint8:
        on = a >= 128
    elif np.issubdtype(a.dtype, np.floating):
        on = a >= 0.5
    else:
        raise TypeError(f"edit_mask arrays must be uint8, bool or float, got {a.dtype}")
    u8 = np.where(on, 255, 0).astype(np.uint8)
    if u8.shape == (height, width):
        return np.ascontiguousarray(u8)
    if file_size is not None and (u8.shape[1], u8.shape[0]) == tuple(file_size) and height == width:
        return np.ascontiguousarray(np.asarray(fit_edit_mask(PIL.Image.fromarray(u8), height)))
    sizes = f"{height} x {width} (height x width of the base image as the pipeline holds it)"
    if file_size is not None:
        sizes += f" or {file_size[1]} x {file_size[0]} (the base image file)"
    raise ValueError(f"edit_mask is {u8.shape[0]} x {u8.shape[1]}: expected {sizes}")


def _binarize_lut(normalize: bool) -> np.ndarray:
    v = np.arange(256, dtype=np.float32) / np.float32(255.0)
    return (2.0 * v - 1.0 if normalize else v) >= 0.5


# ---- diffusers' image processor -------------------------------------------------------------------------------------------------------------------
class VaeImageProcessor:
    """diffusers 0.26.3 `VaeImageProcessor` (same constructor options, same `preprocess` / `postprocess` meaning). `device`: where preprocess
    leaves its fp16 tensor (the VAE's device). Non-RGB PIL images are converted with `convert("RGB")` (unless do_convert_grayscale)."""

    def __init__(self, do_resize: bool = True, vae_scale_factor: int = 8, resample: str = "lanczos", do_normalize: bool = True,
                 do_binarize: bool = False, do_convert_rgb: bool = False, do_convert_grayscale: bool = False, device="cuda:0"):
        if do_convert_rgb and do_convert_grayscale:
            raise ValueError("`do_convert_rgb` and `do_convert_grayscale` can not both be set to `True`")
        if resample not in PIL_INTERPOLATION:
            raise ValueError(f"resample must be one of {sorted(PIL_INTERPOLATION)}")
        self.config = SimpleNamespace(do_resize=do_resize, vae_scale_factor=vae_scale_factor, resample=resample, do_normalize=do_normalize,
                                      do_binarize=do_binarize, do_convert_rgb=do_convert_rgb, do_convert_grayscale=do_convert_grayscale)
        self.device = torch.device(device)

    # -- diffusers' static helpers (host side, for callers that want them) --
    @staticmethod
    def numpy_to_pil(images: np.ndarray) -> List[PIL.Image.Image]:
        if images.ndim == 3:
            images = images[None, ...]
        images = (images * 255).round().astype("uint8")
        if images.shape[-1] == 1:
            return [PIL.Image.fromarray(image.squeeze()) for image in images]           # 2-D uint8: mode "L"
        return [PIL.Image.fromarray(image) for image in images]

    @staticmethod
    def pil_to_numpy(images) -> np.ndarray:
        if not isinstance(images, list):
            images = [images]
        return np.stack([np.array(image).astype(np.float32) / 255.0 for image in images], axis=0)

    @staticmethod
    def normalize(images):
        return 2.0 * images - 1.0

    @staticmethod
    def denormalize(images):
        return (images / 2 + 0.5).clamp(0, 1)

    @staticmethod
    def binarize(image):
        image[image < 0.5] = 0
        image[image >= 0.5] = 1
        return image

    def get_default_height_width(self, image, height=None, width=None):
        """the image's own size where height / width are not given, rounded down to multiples of vae_scale_factor"""
        if height is None:
            height = image.height if isinstance(image, PIL.Image.Image) else image.shape[2] if torch.is_tensor(image) else image.shape[1]
        if width is None:
            width = image.width if isinstance(image, PIL.Image.Image) else image.shape[3] if torch.is_tensor(image) else image.shape[2]
        f = self.config.vae_scale_factor
        return height - height % f, width - width % f

    def resize(self, image, height: int, width: int):
        if isinstance(image, PIL.Image.Image):
            return image.resize((width, height), resample=PIL_INTERPOLATION[self.config.resample])
        if torch.is_tensor(image):
            return torch.nn.functional.interpolate(image, size=(height, width))
        return self.resize(torch.from_numpy(image.transpose(0, 3, 1, 2)), height, width).numpy().transpose(0, 2, 3, 1)

    def _convert(self, image: PIL.Image.Image) -> PIL.Image.Image:
        want = "L" if self.config.do_convert_grayscale else "RGB"
        return image if image.mode == want else image.convert(want)

    # -- preprocess --
    def pil_to_u8(self, images: List[PIL.Image.Image], height=None, width=None):
        """The host half of `preprocess` for PIL images: resize (PIL), convert the mode, stack -> (uint8 [B, H, W, C] contiguous, normalize flag
        for ia2p_image_from_u8). A binarising processor decides 0 / 1 per 8-bit code here and uploads 0 / 255."""
        if self.config.do_resize:
            height, width = self.get_default_height_width(images[0], height, width)
            images = [i if i.size == (width, height) else self.resize(i, height, width) for i in images]
        u8 = np.stack([np.asarray(self._convert(i)) for i in images])
        if u8.ndim == 3:
            u8 = u8[..., None]                                           # grayscale: [B, H, W, 1]
        normalize = self.config.do_normalize
        if self.config.do_binarize:                  # binarize(normalize(q / 255)) in {0, 1}, decided per code (q >= 128 for a mask processor)
            u8 = np.where(_binarize_lut(normalize)[u8], 255, 0).astype(np.uint8)
            normalize = False
        return np.ascontiguousarray(u8), normalize

    def preprocess(self, image, height=None, width=None) -> torch.Tensor:
        """-> fp16 [B, C, H, W] on `self.device`: in [-1, 1] (do_normalize), or {0, 1} for a binarising mask processor."""
        supported = (PIL.Image.Image, np.ndarray, torch.Tensor)
        if isinstance(image, supported):
            image = [image]
        elif not (isinstance(image, list) and image and all(isinstance(i, supported) for i in image)):
            raise ValueError(f"Input is in incorrect format: {[type(i) for i in image] if isinstance(image, list) else type(image)}. "
                             f"Currently, we only support {', '.join(str(t) for t in supported)}")
        if isinstance(image[0], np.ndarray) and image[0].dtype == np.uint8:
            # 8-bit pixels: through PIL, so that they resize and convert exactly as PIL images do
            arrs = [a for i in image for a in (i if i.ndim == 4 else i[None])]
            image = [PIL.Image.fromarray(a[..., 0] if a.ndim == 3 and a.shape[-1] == 1 else a) for a in arrs]
        if isinstance(image[0], PIL.Image.Image):
            u8, normalize = self.pil_to_u8(image, height, width)
            return image_from_u8(torch.from_numpy(u8).to(self.device), normalize=normalize)
        # diffusers' float branch: [0, 1] arrays / tensors (and [-1, 1] tensors, which are not normalised again)
        if isinstance(image[0], np.ndarray):
            image = np.concatenate(image, axis=0) if image[0].ndim == 4 else np.stack(image, axis=0)
            if self.config.do_convert_grayscale and image.ndim == 3:
                image = image[..., None]
            image = torch.from_numpy(image.transpose(0, 3, 1, 2))
        else:
            image = torch.cat(image, axis=0) if image[0].ndim == 4 else torch.stack(image, axis=0)
            if self.config.do_convert_grayscale and image.ndim == 3:
                image = image.unsqueeze(1)
            if image.shape[1] == 4:                                      # latents
                return image
        image = image.to(self.device)
        height, width = self.get_default_height_width(image, height, width)
        if self.config.do_resize and tuple(image.shape[-2:]) != (height, width):
            image = self.resize(image, height, width)
        if self.config.do_normalize and float(image.min()) >= 0:
            image = self.normalize(image)
        if self.config.do_binarize:
            image = self.binarize(image)
        return image.to(torch.float16).contiguous()

    # -- postprocess --
    def postprocess(self, image: torch.Tensor, output_type: str = "pil", do_denormalize=None) -> Union[torch.Tensor, np.ndarray, List[PIL.Image.Image]]:
        """decoded image [B, C, H, W] (fp16 on the device, in [-1, 1]) -> "pil" list of PIL images, "np" float32 [B,H,W,C] in [0, 1],
        "pt" float32 [B,C,H,W] in [0, 1], "latent" unchanged."""
        if not torch.is_tensor(image):
            raise ValueError(f"Input for postprocessing is in incorrect format: {type(image)}. We only support pytorch tensor")
        if output_type not in OUTPUT_TYPES:
            raise ValueError(f"output_type must be one of {OUTPUT_TYPES}, got {output_type!r}")
        if output_type == "latent":
            return image
        if do_denormalize is None:
            do_denormalize = [self.config.do_normalize] * image.shape[0]
        if not all(do_denormalize):          # images that are not in [-1, 1] (diffusers' un-normalised branch; not an output of the pipelines)
            image = torch.stack([self.denormalize(image[i]) if do_denormalize[i] else image[i] for i in range(image.shape[0])]).float()
            if output_type == "pt":
                return image
            image = image.cpu().permute(0, 2, 3, 1).numpy()
            return image if output_type == "np" else self.numpy_to_pil(image)
        x = image.to(device=image.device if image.is_cuda else self.device, dtype=torch.float16).contiguous()
        if output_type == "pt":
            return image_to_f32(x, nhwc=False)
        if output_type == "np":
            return image_to_f32(x, nhwc=True).cpu().numpy()
        u8 = image_to_u8(x).cpu().numpy()
        return [PIL.Image.fromarray(a[..., 0] if a.shape[-1] == 1 else a) for a in u8]
