"""Segment Anything on the HIP executor `ia2p_sam_*`: the subject masks of the subject-consistency pass.

  HipSamModel(config).load_state_dict(sd)   <- `sam_model_registry["vit_h"](".../sam_vit_h_4b8939.pth")` (reference gdino/lib.py:54-58); takes the
                                               checkpoint's own key names or transformers' `SamModel` names
  HipSamPredictor(model)                    <- `SamPredictor(sam)`: `set_image`, `predict(box=...)` (gdino/lib.py:33-38, :73)
  get_mask(ph, boxes, phrases, predictor)   <- gdino/lib.py:21-51: box of the phrase -> SAM mask -> erode, dilate (HIP) -> Gaussian blur (PIL)

Boxes come from the caller or an injected detector: GroundingDINO is not built here.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _ffi

PIXEL_MEAN = (123.675, 116.28, 103.53)
PIXEL_STD = (58.395, 57.12, 57.375)


@dataclass
class SamConfig:
    hidden_size: int = 1280
    num_layers: int = 32
    num_heads: int = 16
    mlp_dim: int = 5120
    image_size: int = 1024
    patch_size: int = 16
    window_size: int = 14
    global_attn_indexes: List[int] = field(default_factory=lambda: [7, 15, 23, 31])
    output_channels: int = 256
    dec_hidden: int = 256
    dec_layers: int = 2
    dec_heads: int = 8
    dec_mlp_dim: int = 2048
    dec_downsample_rate: int = 2
    layer_norm_eps: float = 1e-6
    mask_threshold: float = 0.0

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size


def sam_vit_h_config() -> SamConfig:
    return SamConfig()


def sam_tiny_config(image_size: int = 320, head_dim: int = 80) -> SamConfig:
    """4 blocks of 4 heads (global attention in blocks 1 and 3), a 20 x 20 grid at image size 320: padded windows, partial windows and both attention kinds"""
    return SamConfig(hidden_size=4 * head_dim, num_layers=4, num_heads=4, mlp_dim=640, image_size=image_size, global_attn_indexes=[1, 3], dec_mlp_dim=512)


# ---- parameter names ---------------------------------------------------------------------------------------------------------------------------
# Three spellings of one tensor: the checkpoint's (`segment_anything`, as in sam_vit_h_4b8939.pth), transformers' `SamModel`, and the executor's.
# The checkpoint's names are written from knowledge of that package's module tree: the package was not at hand where this was written.
_ATTN = {"q_proj": "q", "k_proj": "k", "v_proj": "v", "out_proj": "out"}
_HF_FIXED = {
    "vision_encoder.patch_embed.projection.weight": "patch_embed.weight", "vision_encoder.patch_embed.projection.bias": "patch_embed.bias",
    "vision_encoder.pos_embed": "pos_embed",
    "vision_encoder.neck.conv1.weight": "neck.conv1.weight", "vision_encoder.neck.conv2.weight": "neck.conv2.weight",
    "vision_encoder.neck.layer_norm1.weight": "neck.norm1.weight", "vision_encoder.neck.layer_norm1.bias": "neck.norm1.bias",
    "vision_encoder.neck.layer_norm2.weight": "neck.norm2.weight", "vision_encoder.neck.layer_norm2.bias": "neck.norm2.bias",
    "shared_image_embedding.positional_embedding": "prompt.pe_gaussian",
    "prompt_encoder.shared_embedding.positional_embedding": "prompt.pe_gaussian",      # (tied to the one above)
    "prompt_encoder.no_mask_embed.weight": "prompt.no_mask_embed",
    "prompt_encoder.point_embed.2.weight": "prompt.point_embed.2", "prompt_encoder.point_embed.3.weight": "prompt.point_embed.3",
    "mask_decoder.iou_token.weight": "decoder.iou_token", "mask_decoder.mask_tokens.weight": "decoder.mask_tokens",
    "mask_decoder.transformer.layer_norm_final_attn.weight": "decoder.norm_final.weight", "mask_decoder.transformer.layer_norm_final_attn.bias": "decoder.norm_final.bias",
    "mask_decoder.upscale_conv1.weight": "decoder.upscale1.weight", "mask_decoder.upscale_conv1.bias": "decoder.upscale1.bias",
    "mask_decoder.upscale_conv2.weight": "decoder.upscale2.weight", "mask_decoder.upscale_conv2.bias": "decoder.upscale2.bias",
    "mask_decoder.upscale_layer_norm.weight": "decoder.upscale_norm.weight", "mask_decoder.upscale_layer_norm.bias": "decoder.upscale_norm.bias",
}
_MLP3 = {"proj_in": "0", "layers.0": "1", "proj_out": "2"}
# tensors of prompts and outputs this package does not evaluate (points, mask prompts, the multimask hypernetworks): accepted, unused
_HF_UNUSED = re.compile(r"^(prompt_encoder\.(mask_embed\..*|not_a_point_embed\.weight|point_embed\.[01]\.weight)|mask_decoder\.output_hypernetworks_mlps\.[1-9]\d*\..*)$")


def internal_key_from_transformers(key: str) -> Optional[str]:
    """transformers `SamModel` state-dict name -> the executor's name; None for a tensor that is accepted and unused; KeyError for an unknown name"""
    if key in _HF_FIXED:
        return _HF_FIXED[key]
    if _HF_UNUSED.match(key):
        return None
    m = re.match(r"^vision_encoder\.layers\.(\d+)\.(.+)$", key)
    if m:
        rest = m.group(2).replace("layer_norm1.", "norm1.").replace("layer_norm2.", "norm2.")
        if re.match(r"^(norm[12]\.(weight|bias)|attn\.(qkv|proj)\.(weight|bias)|attn\.rel_pos_[hw]|mlp\.lin[12]\.(weight|bias))$", rest):
            return f"blocks.{m.group(1)}.{rest}"
    m = re.match(r"^mask_decoder\.transformer\.layers\.(\d+)\.(self_attn|cross_attn_token_to_image|cross_attn_image_to_token)\.(\w+)\.(weight|bias)$", key)
    if m and m.group(3) in _ATTN:
        a = {"self_attn": "self_attn", "cross_attn_token_to_image": "t2i", "cross_attn_image_to_token": "i2t"}[m.group(2)]
        return f"decoder.layers.{m.group(1)}.{a}.{_ATTN[m.group(3)]}.{m.group(4)}"
    m = re.match(r"^mask_decoder\.transformer\.layers\.(\d+)\.(layer_norm[1-4]|mlp\.lin[12])\.(weight|bias)$", key)
    if m:
        return f"decoder.layers.{m.group(1)}.{m.group(2).replace('layer_norm', 'norm')}.{m.group(3)}"
    m = re.match(r"^mask_decoder\.transformer\.final_attn_token_to_image\.(\w+)\.(weight|bias)$", key)
    if m and m.group(1) in _ATTN:
        return f"decoder.final_attn.{_ATTN[m.group(1)]}.{m.group(2)}"
    m = re.match(r"^mask_decoder\.(output_hypernetworks_mlps\.0|iou_prediction_head)\.(proj_in|layers\.0|proj_out)\.(weight|bias)$", key)
    if m:
        return f"decoder.{'hyper0' if m.group(1).startswith('output') else 'iou_head'}.{_MLP3[m.group(2)]}.{m.group(3)}"
    raise KeyError(f"unknown SAM parameter key '{key}'")


_ORIG_RULES = [      # (pattern on the checkpoint's name, replacement giving transformers' name)
    (r"^image_encoder\.patch_embed\.proj\.", "vision_encoder.patch_embed.projection."),
    (r"^image_encoder\.pos_embed$", "vision_encoder.pos_embed"),
    (r"^image_encoder\.blocks\.(\d+)\.norm([12])\.", r"vision_encoder.layers.\1.layer_norm\2."),
    (r"^image_encoder\.blocks\.(\d+)\.", r"vision_encoder.layers.\1."),
    (r"^image_encoder\.neck\.0\.", "vision_encoder.neck.conv1."), (r"^image_encoder\.neck\.1\.", "vision_encoder.neck.layer_norm1."),
    (r"^image_encoder\.neck\.2\.", "vision_encoder.neck.conv2."), (r"^image_encoder\.neck\.3\.", "vision_encoder.neck.layer_norm2."),
    (r"^prompt_encoder\.pe_layer\.positional_encoding_gaussian_matrix$", "shared_image_embedding.positional_embedding"),
    (r"^prompt_encoder\.point_embeddings\.(\d+)\.", r"prompt_encoder.point_embed.\1."),
    (r"^prompt_encoder\.mask_downscaling\.0\.", "prompt_encoder.mask_embed.conv1."), (r"^prompt_encoder\.mask_downscaling\.1\.", "prompt_encoder.mask_embed.layer_norm1."),
    (r"^prompt_encoder\.mask_downscaling\.3\.", "prompt_encoder.mask_embed.conv2."), (r"^prompt_encoder\.mask_downscaling\.4\.", "prompt_encoder.mask_embed.layer_norm2."),
    (r"^prompt_encoder\.mask_downscaling\.6\.", "prompt_encoder.mask_embed.conv3."),
    (r"^mask_decoder\.transformer\.layers\.(\d+)\.norm([1-4])\.", r"mask_decoder.transformer.layers.\1.layer_norm\2."),
    (r"^mask_decoder\.transformer\.norm_final_attn\.", "mask_decoder.transformer.layer_norm_final_attn."),
    (r"^mask_decoder\.output_upscaling\.0\.", "mask_decoder.upscale_conv1."), (r"^mask_decoder\.output_upscaling\.1\.", "mask_decoder.upscale_layer_norm."),
    (r"^mask_decoder\.output_upscaling\.3\.", "mask_decoder.upscale_conv2."),
    (r"^mask_decoder\.(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.layers\.0\.", r"mask_decoder.\1.proj_in."),
    (r"^mask_decoder\.(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.layers\.1\.", r"mask_decoder.\1.layers.0."),
    (r"^mask_decoder\.(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.layers\.2\.", r"mask_decoder.\1.proj_out."),
]
_HF_TO_ORIG_RULES = [
    (r"^vision_encoder\.patch_embed\.projection\.", "image_encoder.patch_embed.proj."),
    (r"^vision_encoder\.pos_embed$", "image_encoder.pos_embed"),
    (r"^vision_encoder\.layers\.(\d+)\.layer_norm([12])\.", r"image_encoder.blocks.\1.norm\2."),
    (r"^vision_encoder\.layers\.(\d+)\.", r"image_encoder.blocks.\1."),
    (r"^vision_encoder\.neck\.conv1\.", "image_encoder.neck.0."), (r"^vision_encoder\.neck\.layer_norm1\.", "image_encoder.neck.1."),
    (r"^vision_encoder\.neck\.conv2\.", "image_encoder.neck.2."), (r"^vision_encoder\.neck\.layer_norm2\.", "image_encoder.neck.3."),
    (r"^(shared_image_embedding|prompt_encoder\.shared_embedding)\.positional_embedding$", "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"),
    (r"^prompt_encoder\.point_embed\.(\d+)\.", r"prompt_encoder.point_embeddings.\1."),
    (r"^prompt_encoder\.mask_embed\.conv1\.", "prompt_encoder.mask_downscaling.0."), (r"^prompt_encoder\.mask_embed\.layer_norm1\.", "prompt_encoder.mask_downscaling.1."),
    (r"^prompt_encoder\.mask_embed\.conv2\.", "prompt_encoder.mask_downscaling.3."), (r"^prompt_encoder\.mask_embed\.layer_norm2\.", "prompt_encoder.mask_downscaling.4."),
    (r"^prompt_encoder\.mask_embed\.conv3\.", "prompt_encoder.mask_downscaling.6."),
    (r"^mask_decoder\.transformer\.layers\.(\d+)\.layer_norm([1-4])\.", r"mask_decoder.transformer.layers.\1.norm\2."),
    (r"^mask_decoder\.transformer\.layer_norm_final_attn\.", "mask_decoder.transformer.norm_final_attn."),
    (r"^mask_decoder\.upscale_conv1\.", "mask_decoder.output_upscaling.0."), (r"^mask_decoder\.upscale_layer_norm\.", "mask_decoder.output_upscaling.1."),
    (r"^mask_decoder\.upscale_conv2\.", "mask_decoder.output_upscaling.3."),
    (r"^mask_decoder\.(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.proj_in\.", r"mask_decoder.\1.layers.0."),
    (r"^mask_decoder\.(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.layers\.0\.", r"mask_decoder.\1.layers.1."),
    (r"^mask_decoder\.(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.proj_out\.", r"mask_decoder.\1.layers.2."),
]


def _rewrite(key: str, rules) -> str:
    for pat, rep in rules:
        new, n = re.subn(pat, rep, key)
        if n:
            return new
    return key


def transformers_key_from_original(key: str) -> str:
    """a name of the original checkpoint (`image_encoder.*`, `prompt_encoder.pe_layer.*`, `mask_decoder.output_upscaling.*`, ...) -> transformers' name"""
    return _rewrite(key, _ORIG_RULES)


def original_key_from_transformers(key: str) -> str:
    return _rewrite(key, _HF_TO_ORIG_RULES)


def internal_key(key: str, original_names: bool) -> Optional[str]:
    """a name in the stated spelling -> the executor's name (None: accepted and unused; KeyError: unknown). The spelling cannot be told from one key:
    `mask_decoder.iou_prediction_head.layers.0.weight` is the first linear of the original checkpoint and the second of transformers'."""
    return internal_key_from_transformers(transformers_key_from_original(key) if original_names else key)


def internal_tensor(name: str, v: torch.Tensor) -> torch.Tensor:
    """the layout the executor takes: a ConvTranspose2d(k = 2, s = 2) weight [Ci, Co, 2, 2] as GEMM rows (ky, kx, co) of [4 Co, Ci], its bias four times"""
    if name in ("decoder.upscale1.weight", "decoder.upscale2.weight"):
        return v.permute(2, 3, 1, 0).reshape(4 * v.shape[1], v.shape[0])
    if name in ("decoder.upscale1.bias", "decoder.upscale2.bias"):
        return v.repeat(4)
    return v


def internal_state_dict(state_dict, original_names: Optional[bool] = None) -> dict:
    """{executor name: tensor} of a checkpoint in either spelling. `original_names`: None = decide by the presence of `image_encoder.` keys."""
    keys = list(state_dict.keys())
    if original_names is None:
        original_names = any(k.startswith("image_encoder.") for k in keys)
    out = {}
    for k in keys:
        name = internal_key(k, original_names)
        if name is not None:
            out[name] = internal_tensor(name, state_dict[k])
    return out


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
class HipSamModel(_ffi.Executor):
    """SAM behind the C ABI (`ia2p_sam_*`): `encode_image(pixels)` and `predict_boxes(embeddings, boxes)`"""

    def __init__(self, config: SamConfig = None, device="cuda:0"):
        self.config = config or sam_vit_h_config()
        super().__init__("sam", _ffi.make_sam_config(self.config), device)

    def load_state_dict(self, state_dict, strict: bool = True):
        """transformers' `SamModel` names or the original checkpoint's; an unknown key is a KeyError, and so is a tensor the executor misses"""
        for name, v in internal_state_dict(state_dict).items():
            self.load_tensor(name, v)
        self.finalize()
        return self

    def _workspace(self, n_boxes: int):
        return self.workspace(self._lib.ia2p_sam_workspace_bytes(self._h, 1, n_boxes))

    @torch.no_grad()
    @_ffi.on_device
    def encode_image(self, pixels: torch.Tensor) -> torch.Tensor:
        """pixels [1, 3, S, S] (normalised, zero-padded) -> fp16 [1, gh * gw, 256] image embeddings, channels-last rows"""
        cfg = self.config
        if pixels.ndim != 4 or tuple(pixels.shape) != (1, 3, cfg.image_size, cfg.image_size):
            raise ValueError(f"expected [1, 3, {cfg.image_size}, {cfg.image_size}], got {tuple(pixels.shape)}")
        x = pixels.to(device=self.device, dtype=torch.float16).contiguous()
        ws = self._workspace(1)
        emb = torch.empty(1, cfg.grid * cfg.grid, cfg.output_channels, dtype=torch.float16, device=self.device)
        self.check(self._lib.ia2p_sam_encode_image(self._h, _ffi.current_stream(), _ffi.ptr(x), 1, _ffi.ptr(emb), _ffi.ptr(ws), ws.numel()))
        return emb

    @torch.no_grad()
    @_ffi.on_device
    def predict_boxes(self, embeddings: torch.Tensor, boxes) -> Tuple[torch.Tensor, torch.Tensor]:
        """boxes [n, 4] x0 y0 x1 y1 in pixels of the S x S input -> (low-res mask logits fp32 [n, 4 gh, 4 gw], predicted IoU fp32 [n]), on the device"""
        cfg = self.config
        b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 4))
        n = b.shape[0]
        ws = self._workspace(n)
        low = torch.empty(n, 4 * cfg.grid, 4 * cfg.grid, dtype=torch.float32, device=self.device)
        iou = torch.empty(n, dtype=torch.float32, device=self.device)
        self.check(self._lib.ia2p_sam_predict_boxes(self._h, _ffi.current_stream(), _ffi.ptr(embeddings), b.ctypes.data_as(C.POINTER(C.c_float)), n,
                                                    _ffi.ptr(low), _ffi.ptr(iou), _ffi.ptr(ws), ws.numel()))
        return low, iou


def upsample_threshold(logits: torch.Tensor, size: Tuple[int, int], crop: Optional[Tuple[int, int]] = None, threshold: float = 0.0, want_logits: bool = False):
    """`ia2p_mask_upsample_threshold`: fp32 [n, h, w] (its top-left `crop` corner) -> uint8 [n, H, W] mask (255 where the resized logit > threshold)
    [, fp32 [n, H, W] resized logits]"""
    assert logits.dtype == torch.float32 and logits.ndim == 3
    n, h, w = logits.shape
    ch, cw = crop or (h, w)
    H, W = size
    mask = torch.empty(n, H, W, dtype=torch.uint8, device=logits.device)
    out = torch.empty(n, H, W, dtype=torch.float32, device=logits.device) if want_logits else None
    _ffi.check(_ffi.lib().ia2p_mask_upsample_threshold(_ffi.current_stream(), _ffi.ptr(logits), n, ch, cw, w, h * w, H, W, float(threshold), _ffi.ptr(out), _ffi.ptr(mask)))
    return (mask, out) if want_logits else mask


def morph(mask: torch.Tensor, k: int, dilate: bool) -> torch.Tensor:
    """`ia2p_mask_morph`: uint8 [H, W] on the device -> its k x k erosion / dilation (window offsets -(k // 2) .. k - k // 2 - 1, pixels outside the image ignored:
    OpenCV's default anchor for `cv2.erode` / `cv2.dilate` and its default border, restated from its documentation)"""
    assert mask.dtype == torch.uint8 and mask.ndim == 2
    H, W = mask.shape
    dst, tmp = torch.empty_like(mask), torch.empty_like(mask)
    _ffi.check(_ffi.lib().ia2p_mask_morph(_ffi.current_stream(), _ffi.ptr(mask), _ffi.ptr(dst), _ffi.ptr(tmp), H, W, int(k), 1 if dilate else 0))
    return dst


class HipSamPredictor:
    """The two calls the reference makes on `segment_anything.SamPredictor`."""

    def __init__(self, model: HipSamModel):
        self.model = model
        self.is_image_set = False

    @staticmethod
    def preprocess_shape(h: int, w: int, long_side: int) -> Tuple[int, int]:
        scale = long_side * 1.0 / max(h, w)
        return int(h * scale + 0.5), int(w * scale + 0.5)

    def set_image(self, image, image_format: str = "RGB"):
        """np.uint8 [H, W, 3] (or a PIL image): longest side to the model's size (PIL bilinear, on the host, when it is not that size already), mean / std,
        zero padding at the bottom / right, then the image encoder"""
        from PIL import Image
        if isinstance(image, Image.Image):
            image = np.asarray(image.convert("RGB"))
        a = np.asarray(image)
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError(f"set_image takes uint8 [H, W, 3], got {a.dtype} {a.shape}")
        if image_format != "RGB":
            a = a[..., ::-1]
        S = self.model.config.image_size
        H, W = a.shape[:2]
        nh, nw = self.preprocess_shape(H, W, S)
        if (nh, nw) != (H, W):
            a = np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize((nw, nh), Image.BILINEAR))
        x = (a.astype(np.float32) - np.asarray(PIXEL_MEAN, np.float32)) / np.asarray(PIXEL_STD, np.float32)
        px = np.zeros((1, 3, S, S), np.float32)
        px[0, :, :nh, :nw] = x.transpose(2, 0, 1)
        self.pixels = torch.from_numpy(px)
        self.features = self.model.encode_image(self.pixels)
        self.original_size, self.input_size = (H, W), (nh, nw)
        self.is_image_set = True

    def predict_torch(self, box):
        """-> (uint8 mask [1, H, W] on the device, 255 inside; IoU fp32 [1]; low-res logits fp32 [1, 4 gh, 4 gw])"""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        b = np.asarray(box, dtype=np.float32).reshape(-1, 4)
        if b.shape[0] != 1:
            raise ValueError(f"predict takes one box [1, 4], got {b.shape}")
        (H, W), (nh, nw) = self.original_size, self.input_size
        b = b * np.asarray([nw / W, nh / H, nw / W, nh / H], np.float32)
        low, iou = self.model.predict_boxes(self.features, b)
        S, thr = self.model.config.image_size, self.model.config.mask_threshold
        if (nh, nw) == (S, S) == (H, W):
            mask = upsample_threshold(low, (H, W), threshold=thr)
        else:      # `postprocess_masks`: to the padded square, crop the un-padded corner, then to the original size
            _, sq = upsample_threshold(low, (S, S), threshold=thr, want_logits=True)
            mask = upsample_threshold(sq, (H, W), crop=(nh, nw), threshold=thr)
        return mask, iou, low

    def predict(self, point_coords=None, point_labels=None, box=None, mask_input=None, multimask_output: bool = False, return_logits: bool = False):
        """-> (masks bool [1, H, W], iou [1], low_res_logits [1, 4 gh, 4 gw]) as numpy arrays"""
        if point_coords is not None or point_labels is not None or mask_input is not None:
            raise NotImplementedError("point and mask prompts are not built: the reference prompts SAM with one box")
        if multimask_output or return_logits:
            raise NotImplementedError("multimask_output / return_logits are not built: the reference never asks for them")
        if box is None:
            raise ValueError("predict needs box=[1, 4]")
        mask, iou, low = self.predict_torch(box)
        return mask.cpu().numpy() > 0, iou.cpu().numpy(), low.cpu().numpy()


# ---- reference gdino/lib.py:21-51 ------------------------------------------------------------------------------------------------------------------
def select_box(ph: str, boxes, phrases, i: int = 0, size: int = 1024) -> np.ndarray:
    """the box of phrase `ph` as `get_mask` computes it: the i-th box whose phrase contains `ph` or is contained in it, cxcywh in [0, 1] scaled by `size`,
    truncated to integers, corners by integer halving -> int [4] x0 y0 x1 y1"""
    zz = np.array([(ph in x or x in ph) for x in phrases], dtype=bool)
    bx = torch.as_tensor(np.asarray(boxes), dtype=torch.float32).reshape(-1, 4)
    if zz.shape[0] != bx.shape[0]:
        raise ValueError(f"{bx.shape[0]} boxes for {zz.shape[0]} phrases")
    sel = bx[torch.from_numpy(zz)]
    if i >= sel.shape[0]:
        raise IndexError(f"no box {i} for phrase {ph!r} among {list(phrases)}")
    box = (sel[i] * size).int().numpy()
    pt1 = (box[0] - box[2] // 2, box[1] - box[3] // 2)
    pt2 = (box[0] + box[2] // 2, box[1] + box[3] // 2)
    return np.array([*pt1, *pt2])


def get_mask(ph, boxes, phrases, predictor, i=0, d=40, e=10, b=0, size=1024):
    """reference `get_mask`: SAM mask of the phrase's box, eroded with an e x e window, dilated with a d x d window (both on the device, `ia2p_mask_morph`;
    a 1 x 1 window is the identity and launches nothing), then PIL's `GaussianBlur(radius=b)` on the host when b > 0. -> PIL image, mode L.
    `size`: what the boxes are scaled by (the reference's literal 1024, the side of the images it generates)."""
    from PIL import Image, ImageFilter
    box = select_box(ph, boxes, phrases, i, size)
    if hasattr(predictor, "predict_torch") and isinstance(predictor, HipSamPredictor):
        mask = predictor.predict_torch(box.reshape(1, 4))[0][0]
    else:
        masks, _, _ = predictor.predict(point_coords=None, point_labels=None, box=box.reshape(1, 4), multimask_output=False)
        mask = torch.from_numpy(np.ascontiguousarray(masks[0].astype(np.uint8) * 255))
    if e > 1 or d > 1:
        mask = mask.cuda() if not mask.is_cuda else mask
        if e > 1:
            mask = morph(mask, e, dilate=False)
        if d > 1:
            mask = morph(mask, d, dilate=True)
    img = Image.fromarray(mask.cpu().numpy())
    if b > 0:
        img = img.filter(ImageFilter.GaussianBlur(radius=b))
    return img
