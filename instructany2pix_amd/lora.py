"""LoRA adapters for the UNets (the value rule is in include/ia2p.h, "LoRA adapters"; kernel: csrc/lora.hip).

Host side only: `parse_lora_state_dict` maps an adapter file's keys onto the UNet's own module keys (PEFT / diffusers spellings and kohya's
flattened names over the diffusers or the SGM module tree), `LoraManager` keeps the adapters of one `HipUNet2DConditionModel` on the device,
a pristine copy of every weight an adapter touches, and re-merges a touched weight FROM THAT COPY (`ia2p_lora_merge`, then the UNet's own
`_load`) whenever the active set or a weight changes. Nothing is ever subtracted from a merged weight, so disabling gives the loaded bits back.
There is no torch arithmetic on the weights here and no fallback: a missing kernel is an error.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import re
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .config import UNetConfig
from .weights import unet_param_specs

MAX_RANK = 256          # IA2P_LORA_MAX_RANK
MAX_ADAPTERS = 8        # IA2P_LORA_MAX_ADAPTERS: adapters merged into ONE weight by one launch

TEXT_ENCODER_PREFIXES = ("lora_te_", "lora_te1_", "lora_te2_", "text_encoder.", "text_encoder_2.")
_REFUSED_KINDS = (("dora_scale", "DoRA"), ("lora_magnitude_vector", "DoRA"), ("hada_", "LoHa"), ("lokr_", "LoKr"), ("lora_mid", "a Tucker / CP middle factor (lora_mid)"))
_PROC = re.compile(r"^(.*\.attn[12])\.processor\.(to_q|to_k|to_v|to_out)_lora\.(down|up)\.weight$")
_TAILS = (
    (re.compile(r"^(.*)\.lora_A(?:\.[^.]+)?\.weight$"), "down"), (re.compile(r"^(.*)\.lora_B(?:\.[^.]+)?\.weight$"), "up"),
    (re.compile(r"^(.*)\.lora\.down\.weight$"), "down"), (re.compile(r"^(.*)\.lora\.up\.weight$"), "up"),
    (re.compile(r"^(.*)\.lora_down\.weight$"), "down"), (re.compile(r"^(.*)\.lora_up\.weight$"), "up"),
    (re.compile(r"^(.*)\.alpha$"), "alpha"),
)
_BIAS = re.compile(r"(\.bias$|\.diff_b$|\.lora_B(?:\.[^.]+)?\.bias$)")


def unet_lora_modules(cfg: UNetConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """{module key: weight shape} of every linear and convolution of the UNet (its `.weight` key without the suffix), in registration order."""
    return OrderedDict((k[: -len(".weight")], tuple(s)) for k, s, _ in unet_param_specs(cfg) if k.endswith(".weight") and len(s) >= 2)


def sgm_module_names(cfg: UNetConfig) -> "OrderedDict[str, str]":
    """{SGM module path: diffusers module key} for the same modules, derived from the config (layers_per_block, which levels carry transformers):
    input_blocks.0.0 = conv_in, then one index per resnet (.0 resnet, .1 its transformer) and one per downsampler (.0.op); middle_block.0/1/2;
    output_blocks.{i (layers_per_block + 1) + j}.0/.1, the level's upsampler `.conv` behind them (position 2 behind a transformer, else 1).
    Written from knowledge of the two layouts; not checked against a real kohya file."""
    mods = unet_lora_modules(cfg)
    depth, n, lpb = list(cfg.transformer_layers_per_block), len(cfg.block_out_channels), cfg.layers_per_block
    prefix: Dict[str, str] = {"conv_in": "input_blocks.0.0", "conv_out": "out.2",
                              "time_embedding.linear_1": "time_embed.0", "time_embedding.linear_2": "time_embed.2",
                              "add_embedding.linear_1": "label_emb.0.0", "add_embedding.linear_2": "label_emb.0.2"}
    idx = 1
    for i in range(n):
        for j in range(lpb):
            prefix[f"down_blocks.{i}.resnets.{j}"] = f"input_blocks.{idx}.0"
            if depth[i] > 0:
                prefix[f"down_blocks.{i}.attentions.{j}"] = f"input_blocks.{idx}.1"
            idx += 1
        if i != n - 1:
            prefix[f"down_blocks.{i}.downsamplers.0.conv"] = f"input_blocks.{idx}.0.op"
            idx += 1
    prefix.update({"mid_block.resnets.0": "middle_block.0", "mid_block.attentions.0": "middle_block.1", "mid_block.resnets.1": "middle_block.2"})
    rdepth = depth[::-1]
    for i in range(n):
        for j in range(lpb + 1):
            o = i * (lpb + 1) + j
            prefix[f"up_blocks.{i}.resnets.{j}"] = f"output_blocks.{o}.0"
            if rdepth[i] > 0:
                prefix[f"up_blocks.{i}.attentions.{j}"] = f"output_blocks.{o}.1"
        if i != n - 1:
            prefix[f"up_blocks.{i}.upsamplers.0.conv"] = f"output_blocks.{i * (lpb + 1) + lpb}.{2 if rdepth[i] > 0 else 1}.conv"
    resnet = {"conv1": "in_layers.2", "time_emb_proj": "emb_layers.1", "conv2": "out_layers.3", "conv_shortcut": "skip_connection"}
    out: "OrderedDict[str, str]" = OrderedDict()
    for m in mods:
        if m in prefix:
            out[prefix[m]] = m
            continue
        head = next((p for p in prefix if m.startswith(p + ".")), None)
        if head is None:
            raise AssertionError(f"no SGM name for {m}")
        rest = m[len(head) + 1:]
        out[prefix[head] + "." + (resnet[rest] if ".resnets." in head else rest)] = m      # (a transformer's inner names are the same in both trees)
    return out


def kohya_names(cfg: UNetConfig) -> Dict[str, str]:
    """{kohya flattened name (`lora_unet_` + a module path with '.' -> '_'): diffusers module key}, over BOTH trees. The flattened names are looked up
    whole: a path is never split on '_' (module names carry underscores of their own)."""
    table: Dict[str, str] = {}
    for path, m in list((k, k) for k in unet_lora_modules(cfg)) + list(sgm_module_names(cfg).items()):
        flat = "lora_unet_" + path.replace(".", "_")
        if table.setdefault(flat, m) != m:
            raise AssertionError(f"kohya name {flat} is ambiguous: {table[flat]} / {m}")
    return table


def lora_coef(weight: float, alpha: float, rank: int) -> float:
    """coef = weight * alpha / rank, every operation in fp32 (the value `ia2p_lora_merge` is handed)"""
    return float(np.float32(np.float32(weight) * np.float32(alpha)) / np.float32(rank))


def _to_fp16(key: str, t) -> torch.Tensor:
    t = torch.as_tensor(t)
    if not t.is_floating_point():
        raise ValueError(f"LoRA key '{key}': dtype {t.dtype} is not a floating-point type")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"LoRA key '{key}' holds non-finite values")
    h = t.detach().to(torch.float16)            # round to nearest even, once
    if not bool(torch.isfinite(h).all()):
        raise ValueError(f"LoRA key '{key}' overflows fp16")
    return h.contiguous()


def load_lora_file(path_or_dict) -> Dict[str, torch.Tensor]:
    if hasattr(path_or_dict, "items"):
        return dict(path_or_dict.items())
    p = str(path_or_dict)
    if not p.endswith(".safetensors"):
        raise ValueError(f"LoRA adapters are read from a .safetensors file or a dict, got {p}")
    from safetensors.torch import load_file
    return load_file(p)


def parse_lora_state_dict(sd, unet_config: UNetConfig, text_encoder_keys: str = "error"):
    """{diffusers module key: (down fp16 [r, K], up fp16 [N, r], alpha)} from an adapter's state dict (a dict or a `.safetensors` path); with
    `text_encoder_keys="skip"` -> (that dict, the sorted names of the text-encoder keys dropped). Spellings accepted: an optional `unet.` prefix in
    front of `<module>.lora_A[.<name>].weight` / `.lora_B...`, `<module>.lora.down.weight` / `.lora.up.weight`, `<module>.lora_down.weight` /
    `.lora_up.weight`, the old attention-processor form `...attnN.processor.to_q_lora.down.weight` (`to_out_lora` -> `to_out.0`), and kohya's
    `lora_unet_<flattened path>.lora_down.weight` / `.lora_up.weight` / `.alpha` over the diffusers or the SGM tree (`kohya_names`). `alpha` comes
    from `<module>.alpha`, else it is the rank. A convolution's `down` [r, Ci, kh, kw] is flattened to [r, Ci kh kw], its `up` is [Co, r, 1, 1].
    fp32 / bf16 tensors are rounded to fp16 once, here. Every refusal is a ValueError naming the key."""
    if text_encoder_keys not in ("error", "skip"):
        raise ValueError("text_encoder_keys must be 'error' or 'skip'")
    sd = load_lora_file(sd)
    mods = unet_lora_modules(unet_config)
    kohya = None
    halves: "OrderedDict[str, dict]" = OrderedDict()
    skipped: List[str] = []
    for key in sd:
        if key.startswith(TEXT_ENCODER_PREFIXES):
            if text_encoder_keys == "error":
                raise ValueError(f"LoRA key '{key}' belongs to a text encoder; adapters on the CLIP towers are not applied: pass text_encoder_keys='skip' to drop such keys")
            skipped.append(key)
            continue
        for token, what in _REFUSED_KINDS:
            if token in key:
                raise ValueError(f"LoRA key '{key}': {what} adapters are not supported")
        if _BIAS.search(key):
            raise ValueError(f"LoRA key '{key}': bias deltas are not supported")
        m = _PROC.match(key)
        if m:
            stem, role = m.group(1) + "." + ("to_out.0" if m.group(2) == "to_out" else m.group(2)), m.group(3)
        else:
            stem = role = None
            for rx, r in _TAILS:
                mm = rx.match(key)
                if mm:
                    stem, role = mm.group(1), r
                    break
            if stem is None:
                raise ValueError(f"LoRA key '{key}' is in no spelling this reader knows")
        if stem.startswith("lora_unet_"):
            if kohya is None:
                kohya = kohya_names(unet_config)
            if stem not in kohya:
                raise ValueError(f"LoRA key '{key}': the UNet has no module '{stem}'")
            module = kohya[stem]
        else:
            module = stem[len("unet."):] if stem.startswith("unet.") else stem
            if module not in mods:
                raise ValueError(f"LoRA key '{key}': the UNet has no module '{module}'")
        slot = halves.setdefault(module, {})
        if role in slot:
            raise ValueError(f"LoRA key '{key}': a second '{role}' tensor for module '{module}' (first: '{slot[role][0]}')")
        slot[role] = (key, sd[key])
    out: "OrderedDict[str, Tuple[torch.Tensor, torch.Tensor, float]]" = OrderedDict()
    for module in [m for m in mods if m in halves]:      # the UNet's registration order, whatever order the file has (safetensors sorts its keys)
        slot = halves[module]
        if "down" not in slot or "up" not in slot:
            have = next(iter(slot.values()))[0]
            raise ValueError(f"LoRA key '{have}': module '{module}' has no '{'up' if 'up' not in slot else 'down'}' tensor to go with it")
        (kd, down), (ku, up) = slot["down"], slot["up"]
        shape = mods[module]
        N, K = shape[0], int(np.prod(shape[1:]))
        down, up = torch.as_tensor(down), torch.as_tensor(up)
        if up.ndim == 4:
            if tuple(up.shape[2:]) != (1, 1):
                raise ValueError(f"LoRA key '{ku}': an up convolution of {tuple(up.shape[2:])} is not supported (1 x 1 only)")
            up = up.reshape(up.shape[0], up.shape[1])
        if up.ndim != 2 or down.ndim not in (2, 4):
            raise ValueError(f"LoRA key '{ku if up.ndim != 2 else kd}': shape {tuple(up.shape if up.ndim != 2 else down.shape)} is neither a linear nor a convolution factor")
        r = int(down.shape[0])
        if r < 1 or r > MAX_RANK:
            raise ValueError(f"LoRA key '{kd}': rank {r} is outside 1 .. {MAX_RANK}")
        if down.ndim == 4 and tuple(down.shape[1:]) != tuple(shape[1:]):
            raise ValueError(f"LoRA key '{kd}': shape {tuple(down.shape)} does not fit '{module}' {shape}")
        down = down.reshape(r, -1)
        if down.shape[1] != K:
            raise ValueError(f"LoRA key '{kd}': shape {tuple(slot['down'][1].shape)} does not fit '{module}' {shape}")
        if tuple(up.shape) != (N, r):
            raise ValueError(f"LoRA key '{ku}': shape {tuple(slot['up'][1].shape)} does not fit '{module}' {shape} at rank {r}")
        alpha = float(r)
        if "alpha" in slot:
            ka, a = slot["alpha"]
            a = torch.as_tensor(a, dtype=torch.float64).reshape(-1)
            if a.numel() != 1 or not math.isfinite(float(a[0])):
                raise ValueError(f"LoRA key '{ka}': alpha must be one finite number")
            alpha = float(a[0])
        out[module] = (_to_fp16(kd, down), _to_fp16(ku, up), alpha)
    if not out and not skipped:
        raise ValueError("the adapter holds no LoRA tensors")
    return (out, sorted(skipped)) if text_encoder_keys == "skip" else out


# ---- the device side ------------------------------------------------------------------------------------------------------------------------------------------
def lora_merge(base: torch.Tensor, ups: Sequence[torch.Tensor], downs: Sequence[torch.Tensor], coefs: Sequence[float], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`ia2p_lora_merge` on the current stream: base fp16 [N, ...] (K = the rest), ups[a] [N, r_a], downs[a] [r_a, K] -> out (default: a new tensor; `base` itself: in place)."""
    from . import _ffi
    n = len(ups)
    N = int(base.shape[0])
    K = base.numel() // max(N, 1)
    if out is None:
        out = torch.empty_like(base)
    up_p = (C.c_void_p * max(n, 1))(*[u.data_ptr() for u in ups])
    dn_p = (C.c_void_p * max(n, 1))(*[d.data_ptr() for d in downs])
    ranks = (C.c_int * max(n, 1))(*[int(u.shape[1]) for u in ups])
    cf = (C.c_float * max(n, 1))(*[float(c) for c in coefs])
    for t in (base, out, *ups, *downs):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float16, "ia2p_lora_merge takes contiguous fp16 device tensors"
    _ffi.check(_ffi.lib().ia2p_lora_merge(_ffi.current_stream(), _ffi.ptr(base), _ffi.ptr(out), N, K, n, up_p, dn_p, ranks, cf), None)
    return out


class LoraManager:
    """The adapter state of one `HipUNet2DConditionModel`.

    Per module an adapter touches, a pristine device copy of the weight is taken with `ia2p_read_tensor` the first time an adapter is merged into it
    (memory: the touched weights once more, about 1.9 GB for attention-only adapters on SDXL-base) and kept until `unload()`. Every change of the
    active set or of a weight re-merges the touched weights whose contribution changed FROM the pristine copy into one reused scratch tensor and loads
    that through the UNet's own `_load` (so `fold_dirty`, the weight generation that guards the cached context K/V, and every packing are the existing
    ones); a weight whose contribution became empty is reloaded from the pristine copy, bit for bit. A state that is already applied launches nothing.
    A UNet whose base weights are reloaded (`load_state_dict`) while adapters are loaded must `unload()` first: the pristine copies would be stale."""

    def __init__(self, unet):
        self.unet = unet
        self.modules = unet_lora_modules(unet.config)
        self.adapters: "OrderedDict[str, OrderedDict[str, Tuple[torch.Tensor, torch.Tensor, float]]]" = OrderedDict()
        self.active: "OrderedDict[str, float]" = OrderedDict()
        self.enabled = True
        self.pristine: Dict[str, torch.Tensor] = {}
        self.applied: Dict[str, tuple] = {}      # module -> ((adapter name, coef), ...) merged into the arena now
        self._scratch: Optional[torch.Tensor] = None
        self.skipped_keys: Dict[str, List[str]] = {}

    # -- the public verbs (HipUNet2DConditionModel forwards to these)
    def load(self, path_or_dict, adapter_name: str = "default", **parse_kw):
        if adapter_name in self.adapters:
            raise ValueError(f"adapter '{adapter_name}' is already loaded: delete_adapters(['{adapter_name}']) first")
        parsed = parse_lora_state_dict(path_or_dict, self.unet.config, **parse_kw)
        if isinstance(parsed, tuple):
            parsed, self.skipped_keys[adapter_name] = parsed
        dev = self.unet.device
        self.adapters[adapter_name] = OrderedDict((m, (d.to(dev), u.to(dev), a)) for m, (d, u, a) in parsed.items())      # (not active yet: set_adapters)

    def set_adapters(self, names: Union[str, Sequence[str]], weights: Union[float, Sequence[float]] = 1.0):
        names = [names] if isinstance(names, str) else list(names)
        weights = [float(weights)] * len(names) if not isinstance(weights, (list, tuple)) else [float(w) for w in weights]
        if len(weights) != len(names):
            raise ValueError(f"{len(names)} adapter names for {len(weights)} weights")
        if len(set(names)) != len(names):
            raise ValueError("an adapter is named twice")
        for nm, w in zip(names, weights):
            if nm not in self.adapters:
                raise ValueError(f"no adapter '{nm}' is loaded (loaded: {list(self.adapters)})")
            if not math.isfinite(w):
                raise ValueError(f"adapter '{nm}': weight {w} is not finite")
        self.active = OrderedDict(zip(names, weights))
        self.sync()

    def disable(self):
        self.enabled = False
        self.sync()

    def enable(self):
        self.enabled = True
        self.sync()

    def delete(self, names: Union[str, Sequence[str]]):
        names = [names] if isinstance(names, str) else list(names)
        for nm in names:
            if nm not in self.adapters:
                raise ValueError(f"no adapter '{nm}' is loaded (loaded: {list(self.adapters)})")
        for nm in names:
            self.active.pop(nm, None)
        self.sync()                              # while the tensors are still here: the weights they touched go back first
        for nm in names:
            del self.adapters[nm]
            self.skipped_keys.pop(nm, None)
        touched = {m for ad in self.adapters.values() for m in ad}
        for m in [m for m in self.pristine if m not in touched]:
            del self.pristine[m]

    def unload(self):
        self.active = OrderedDict()
        self.sync()
        self.adapters.clear(); self.pristine.clear(); self.skipped_keys.clear()
        self._scratch = None
        self.enabled = True

    def active_adapters(self) -> List[Tuple[str, float]]:
        return [(n, w) for n, w in self.active.items()] if self.enabled else []

    @contextlib.contextmanager
    def scaled(self, scale: Optional[float]):
        """The active weights times `scale` inside the block, the state before it afterwards (also when the block raises). None: nothing happens."""
        if scale is None:
            yield
            return
        scale = float(scale)
        if not math.isfinite(scale):
            raise ValueError(f"lora_scale {scale} is not finite")
        before = OrderedDict(self.active)
        self.active = OrderedDict((n, w * scale) for n, w in before.items())
        try:
            self.sync()
            yield
        finally:
            self.active = before
            self.sync()

    @contextlib.contextmanager
    def using(self, names: Union[str, Sequence[str]], weights: Union[float, Sequence[float]] = 1.0):
        """The adapters `names` at `weights` active (and enabled) inside the block, the state before it afterwards (also when the block raises, and when
        `set_adapters` itself refuses the names: nothing has changed then)."""
        before, enabled = OrderedDict(self.active), self.enabled
        try:
            self.enabled = True
            self.set_adapters(names, weights)
            yield
        finally:
            self.active, self.enabled = before, enabled
            self.sync()

    # -- state -> arena
    def _wanted(self) -> Dict[str, tuple]:
        want: Dict[str, list] = {}
        if self.enabled:
            for nm, w in self.active.items():
                if w == 0.0:
                    continue
                for m, (d, u, alpha) in self.adapters[nm].items():
                    want.setdefault(m, []).append((nm, lora_coef(w, alpha, d.shape[0])))
        return {m: tuple(v) for m, v in want.items()}

    def _pristine_of(self, module: str) -> torch.Tensor:
        t = self.pristine.get(module)
        if t is None:
            t = self.pristine[module] = self.unet.read_tensor(module + ".weight", self.modules[module])
        return t

    def sync(self) -> int:
        """Bring the arena to the wanted state; returns the number of weights it reloaded (0: nothing was launched)."""
        want = self._wanted()
        todo = [m for m in self.modules if want.get(m, ()) != self.applied.get(m, ())]
        if not todo:
            return 0
        for m in todo:
            if len(want.get(m, ())) > MAX_ADAPTERS:
                raise ValueError(f"module '{m}': {len(want[m])} active adapters touch it, at most {MAX_ADAPTERS} are merged into one weight")
        un = self.unet
        with un._on_device():
            for m in todo:
                base = self._pristine_of(m)      # (taken while the arena still holds the weight as loaded: applied[m] is empty then)
                sig = want.get(m, ())
                if not sig:
                    un._load(m + ".weight", base)
                    self.applied.pop(m, None)
                    continue
                if self._scratch is None or self._scratch.numel() < base.numel():      # one tensor, sized for the largest weight any loaded adapter touches
                    need = max(int(np.prod(self.modules[k])) for ad in self.adapters.values() for k in ad)
                    self._scratch = torch.empty(need, dtype=torch.float16, device=un.device)
                out = self._scratch[: base.numel()].view(base.shape)
                ads = [self.adapters[nm][m] for nm, _ in sig]
                lora_merge(base, [u for _, u, _ in ads], [d for d, _, _ in ads], [c for _, c in sig], out=out)
                un._load(m + ".weight", out)     # (waits for the copy into the arena: the scratch tensor is free again)
                self.applied[m] = sig
        return len(todo)
