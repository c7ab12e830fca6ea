"""Times the SAM path on the GPU at ViT-H size with seeded weights: `set_image` (image encoder), `predict` (one box), and the two relative-position
attention launches on their own. Prints one line per figure; the algorithmic FLOPs beside them are in docs/LOG.md.

    python tools/sam_bench.py [--reps 5] [--tiny]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def seeded_state_dict(cfg, seed=0):
    """executor-named tensors straight from a generator (the transformers model at ViT-H size takes minutes to build on a CPU): the init of tests/sam_ref.py"""
    from instructany2pix_amd import _ffi
    import ctypes as C
    g = torch.Generator().manual_seed(seed)
    H, I, D, Cc, gr = cfg.hidden_size, cfg.mlp_dim, cfg.hidden_size // cfg.num_heads, cfg.output_channels, cfg.grid
    n = lambda std, *s: (torch.randn(*s, generator=g) * std).half()
    lin = lambda o, i: n(i ** -0.5, o, i)
    sd = {"patch_embed.weight": lin(H, 3 * cfg.patch_size ** 2), "patch_embed.bias": n(0.1, H), "pos_embed": n(0.5, gr * gr, H)}
    for i in range(cfg.num_layers):
        S = gr if i in cfg.global_attn_indexes else cfg.window_size
        p = f"blocks.{i}."
        sd.update({p + "norm1.weight": 1 + n(0.1, H), p + "norm1.bias": n(0.1, H), p + "norm2.weight": 1 + n(0.1, H), p + "norm2.bias": n(0.1, H),
                   p + "attn.qkv.weight": lin(3 * H, H), p + "attn.qkv.bias": n(0.1, 3 * H), p + "attn.proj.weight": lin(H, H), p + "attn.proj.bias": n(0.1, H),
                   p + "attn.rel_pos_h": n(0.1, 2 * S - 1, D), p + "attn.rel_pos_w": n(0.1, 2 * S - 1, D),
                   p + "mlp.lin1.weight": lin(I, H), p + "mlp.lin1.bias": n(0.1, I), p + "mlp.lin2.weight": lin(H, I), p + "mlp.lin2.bias": n(0.1, H)})
    sd.update({"neck.conv1.weight": lin(Cc, H), "neck.norm1.weight": 1 + n(0.1, Cc), "neck.norm1.bias": n(0.1, Cc),
               "neck.conv2.weight": n((9 * Cc) ** -0.5, Cc, Cc, 3, 3), "neck.norm2.weight": 1 + n(0.1, Cc), "neck.norm2.bias": n(0.1, Cc),
               "prompt.pe_gaussian": n(1.0, 2, Cc // 2), "prompt.point_embed.2": n(1.0, Cc), "prompt.point_embed.3": n(1.0, Cc), "prompt.no_mask_embed": n(1.0, Cc),
               "decoder.iou_token": n(1.0, Cc), "decoder.mask_tokens": n(1.0, 4, Cc), "decoder.norm_final.weight": 1 + n(0.1, Cc), "decoder.norm_final.bias": n(0.1, Cc),
               "decoder.upscale1.weight": lin(Cc, Cc), "decoder.upscale1.bias": n(0.1, Cc // 4).repeat(4), "decoder.upscale_norm.weight": 1 + n(0.1, Cc // 4),
               "decoder.upscale_norm.bias": n(0.1, Cc // 4), "decoder.upscale2.weight": lin(Cc // 2, Cc // 4), "decoder.upscale2.bias": n(0.1, Cc // 8).repeat(4)})

    def attn(p, ds):
        Ci = Cc // ds
        for k, (o, i) in {"q": (Ci, Cc), "k": (Ci, Cc), "v": (Ci, Cc), "out": (Cc, Ci)}.items():
            sd[p + k + ".weight"], sd[p + k + ".bias"] = lin(o, i), n(0.1, o)
    for i in range(cfg.dec_layers):
        p = f"decoder.layers.{i}."
        attn(p + "self_attn.", 1), attn(p + "t2i.", cfg.dec_downsample_rate), attn(p + "i2t.", cfg.dec_downsample_rate)
        for k in range(1, 5):
            sd[p + f"norm{k}.weight"], sd[p + f"norm{k}.bias"] = 1 + n(0.1, Cc), n(0.1, Cc)
        sd.update({p + "mlp.lin1.weight": lin(cfg.dec_mlp_dim, Cc), p + "mlp.lin1.bias": n(0.1, cfg.dec_mlp_dim), p + "mlp.lin2.weight": lin(Cc, cfg.dec_mlp_dim),
                   p + "mlp.lin2.bias": n(0.1, Cc)})
    attn("decoder.final_attn.", cfg.dec_downsample_rate)
    for k in range(3):
        sd[f"decoder.hyper0.{k}.weight"], sd[f"decoder.hyper0.{k}.bias"] = lin(Cc // 8 if k == 2 else Cc, Cc), n(0.1, Cc // 8 if k == 2 else Cc)
        sd[f"decoder.iou_head.{k}.weight"], sd[f"decoder.iou_head.{k}.bias"] = lin(4 if k == 2 else Cc, Cc), n(0.1, 4 if k == 2 else Cc)
    return sd


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    from instructany2pix_amd import _ffi
    from instructany2pix_amd.sam import HipSamModel, HipSamPredictor, sam_tiny_config, sam_vit_h_config
    cfg = sam_tiny_config() if a.tiny else sam_vit_h_config()
    model = HipSamModel(cfg, "cuda:0")
    for k, v in seeded_state_dict(cfg).items():
        model.load_tensor(k, v)
    _ffi.check(model._lib.ia2p_sam_finalize_weights(model._h), model._h, sam=True)
    pred = HipSamPredictor(model)
    S = cfg.image_size
    img = np.random.default_rng(0).integers(0, 256, (S, S, 3), dtype=np.uint8)
    box = np.array([[S * 0.2, S * 0.25, S * 0.7, S * 0.8]], np.float32)
    med, lo = timed(lambda: pred.set_image(img), a.reps)
    print(f"set_image   {S}x{S}  median {med:9.2f} ms  min {lo:9.2f} ms   (host normalise + upload + image encoder)")
    px = pred.pixels.to("cuda:0").half()
    med, lo = timed(lambda: model.encode_image(px), a.reps)
    print(f"encoder     {S}x{S}  median {med:9.2f} ms  min {lo:9.2f} ms")
    med, lo = timed(lambda: pred.predict(box=box), a.reps)
    print(f"predict     1 box    median {med:9.2f} ms  min {lo:9.2f} ms   (prompt on the host, mask decoder, resize + threshold, copy back)")
    L, g, heads, D, H = model._lib, cfg.grid, cfg.num_heads, cfg.hidden_size // cfg.num_heads, cfg.hidden_size
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen).half().to("cuda:0")
    qkv, out, bias = rn(g * g, 3 * H), torch.empty(g * g, H, dtype=torch.half, device="cuda:0"), rn(3 * H)
    w = cfg.window_size
    rh, rw, gh_, gw_ = rn(2 * w - 1, D), rn(2 * w - 1, D), rn(2 * g - 1, D), rn(2 * g - 1, D)
    s = _ffi.current_stream()
    med, lo = timed(lambda: _ffi.check(L.ia2p_attention_window_relpos(s, _ffi.ptr(qkv), _ffi.ptr(out), _ffi.ptr(bias), _ffi.ptr(rh), _ffi.ptr(rw), 1, g, g, heads, D, w)), 20)
    nw = -(-g // w)
    print(f"window attn {g}x{g} grid, {nw * nw} windows x {heads} heads, D={D}: median {med * 1e3:8.1f} us  min {lo * 1e3:8.1f} us   ({4.0 * nw * nw * heads * (w * w) ** 2 * D / 1e9:.2f} GFLOP)")
    med, lo = timed(lambda: _ffi.check(L.ia2p_attention_global_relpos(s, _ffi.ptr(qkv), _ffi.ptr(out), _ffi.ptr(gh_), _ffi.ptr(gw_), 1, g, g, heads, D)), 20)
    print(f"global attn {g * g} keys x {heads} heads, D={D}: median {med * 1e3:8.1f} us  min {lo * 1e3:8.1f} us   ({4.0 * heads * (g * g) ** 2 * D / 1e9:.2f} GFLOP)")


if __name__ == "__main__":
    main()
