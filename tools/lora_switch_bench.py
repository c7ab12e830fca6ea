"""What an adapter switch costs (docs/LOG.md §35): `set_adapters` on a full-size UNet with seeded synthetic weights and two seeded synthetic adapters,
  (a) attention  rank R on every attention projection (attn1 / attn2 to_q, to_k, to_v, to_out.0),
  (b) lcm        rank R on every linear and convolution an LCM-style adapter touches (the attention projections, proj_in / proj_out, ff.net.0.proj / ff.net.2,
                 conv1 / conv2 / conv_shortcut / time_emb_proj of the resnets, the down- and upsampler convolutions),
each as a FIRST activation (the pristine copies are taken) and as a WEIGHT CHANGE (copies held), against three yardsticks in the same process, interleaved rep by rep:
  1. host    the route a caller has without this feature: fp32 merge on the host cores (torch, THREADS threads) + load of every touched tensor,
  2. addmm   the merges alone against torch.addmm in fp32 on the device (the vendor GEMM; a yardstick in the manner of tools/yardstick.py, not used by the product),
  3. copy    the merges alone against a device-to-device copy of the same weights (what an HBM-bound pass should be measured against).
Times are host clocks around work that ends in a device synchronise; median [min .. max] over REPS. The split of a switch into merge launches and reloads comes from a
second, instrumented pass (a synchronise around every merge), the re-fold from the first forward after a switch against the steady forward (it also re-projects the
cached context K/V). `--dry` prints what the tool counts from the shapes (touched parameters, bytes, launches) and needs no GPU.

Usage: python tools/lora_switch_bench.py [--config sdxl|tiny] [--rank 64] [--reps 5] [--threads 16] [--out bench_out/lora_switch.json] [--dry]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instructany2pix_amd import lora as Lm  # noqa: E402
from instructany2pix_amd.config import sdxl_base, tiny  # noqa: E402

ATTN = (".to_q", ".to_k", ".to_v", ".to_out.0")
LCM = ATTN + (".proj_in", ".proj_out", ".ff.net.0.proj", ".ff.net.2", ".conv1", ".conv2", ".conv_shortcut", ".time_emb_proj", ".downsamplers.0.conv", ".upsamplers.0.conv")


def targets(cfg, which):
    return [m for m in Lm.unet_lora_modules(cfg) if m.endswith(ATTN if which == "attention" else LCM)]


def counts(cfg, mods, rank):
    shapes = Lm.unet_lora_modules(cfg)
    n = sum(int(torch.Size(shapes[m]).numel()) for m in mods)
    fac = sum(rank * (shapes[m][0] + int(torch.Size(shapes[m][1:]).numel())) for m in mods)
    return dict(modules=len(mods), params=n, weight_bytes=2 * n, factor_bytes=2 * fac, merge_bytes=4 * n + 2 * fac, flops=2.0 * n * rank,
                largest=max(int(torch.Size(shapes[m]).numel()) for m in mods))


def synthetic_adapter(cfg, mods, rank, seed, device):
    """{PEFT key: tensor}: seeded N(0, 1 / K) / N(0, 1 / r) factors, alpha = r / 2"""
    shapes = Lm.unet_lora_modules(cfg)
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for m in mods:
        s = shapes[m]
        K = int(torch.Size(s[1:]).numel())
        sd[f"unet.{m}.lora_A.weight"] = (torch.randn((rank,) + tuple(s[1:]), generator=g, device=device) * K ** -0.5).half()
        sd[f"unet.{m}.lora_B.weight"] = (torch.randn((s[0], rank) + ((1, 1) if len(s) == 4 else ()), generator=g, device=device) * rank ** -0.5).half()
        sd[f"unet.{m}.alpha"] = torch.tensor(rank / 2.0)
    return sd


def stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def fmt(s, unit="ms", k=1e3):
    return f"{k * s['median']:9.2f} [{k * s['min']:8.2f} .. {k * s['max']:8.2f}] {unit}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sdxl", choices=("sdxl", "tiny"))
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join("bench_out", "lora_switch.json"))
    ap.add_argument("--dry", action="store_true")
    args = ap.parse_args()
    cfg = sdxl_base() if args.config == "sdxl" else tiny()
    plan = {w: counts(cfg, targets(cfg, w), args.rank) for w in ("attention", "lcm")}
    for w, c in plan.items():
        print(f"[{w}] {c['modules']} weights, {c['params'] / 1e9:.3f} G parameters ({c['weight_bytes'] / 1e9:.3f} GB fp16), factors {c['factor_bytes'] / 1e6:.1f} MB, "
              f"per switch: {c['modules']} merge launches + {c['modules']} reloads, {c['merge_bytes'] / 1e9:.3f} GB moved by the merges, {c['flops'] / 1e9:.1f} GFLOP "
              f"({c['flops'] / c['merge_bytes']:.1f} FLOP/B); pristine copies {c['weight_bytes'] / 1e9:.3f} GB + scratch {2 * c['largest'] / 1e6:.1f} MB")
    if args.dry:
        return
    if not torch.cuda.is_available():
        raise SystemExit("lora_switch_bench measures on the GPU and found none (use --dry for the counts)")
    from instructany2pix_amd.unet import HipUNet2DConditionModel
    from instructany2pix_amd.weights import iter_synthetic, unet_param_specs
    dev = "cuda:0"
    torch.set_num_threads(args.threads)
    sync = lambda: torch.cuda.synchronize()
    unet = HipUNet2DConditionModel(cfg, dev)
    unet.load_state_dict(iter_synthetic(unet_param_specs(cfg), 7, dev, torch.float16))
    shapes = Lm.unet_lora_modules(cfg)
    hw = 128 if args.config == "sdxl" else 16
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(2, 4, hw, hw, generator=g, device=dev).half()
    ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g, device=dev).half()
    added = dict(text_embeds=torch.randn(2, cfg.pooled_dim, generator=g, device=dev).half(), time_ids=torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]] * 2, device=dev).half())

    def forward():
        sync()
        t0 = time.perf_counter()
        unet(x, 501, encoder_hidden_states=ctx, added_cond_kwargs=added)
        sync()
        return time.perf_counter() - t0

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0

    for _ in range(3):
        forward()
    result = dict(config=args.config, rank=args.rank, reps=args.reps, threads=args.threads, device=torch.cuda.get_device_name(0), counts=plan, adapters={})
    for which in ("attention", "lcm"):
        mods, c = targets(cfg, which), plan[which]
        asd = synthetic_adapter(cfg, mods, args.rank, 11, dev)
        parsed = Lm.parse_lora_state_dict(asd, cfg)
        facs = {m: (parsed[m][0].to(dev), parsed[m][1].to(dev)) for m in mods}
        coef = Lm.lora_coef(0.8, args.rank / 2.0, args.rank)
        base = {m: unet.read_tensor(m + ".weight", shapes[m]) for m in mods}           # the yardsticks' operands: the weights as loaded
        scratch = torch.empty(c["largest"], dtype=torch.float16, device=dev)
        host = {m: (base[m].cpu(), facs[m][0].cpu().float(), facs[m][1].cpu().float()) for m in mods}
        f32 = {m: (facs[m][0].float(), facs[m][1].float()) for m in mods}
        out_of = lambda m: scratch[: base[m].numel()].view(base[m].shape)

        def merges():
            for m in mods:
                Lm.lora_merge(base[m], [facs[m][1]], [facs[m][0]], [coef], out=out_of(m))

        def addmm():
            for m in mods:
                b = base[m]
                out_of(m).copy_(torch.addmm(b.reshape(b.shape[0], -1).float(), f32[m][1], f32[m][0], alpha=coef).reshape(b.shape))

        def copies():
            for m in mods:
                out_of(m).copy_(base[m])

        def host_route():
            for m in mods:
                b, d, u = host[m]
                unet._load(m + ".weight", torch.addmm(b.reshape(b.shape[0], -1).float(), u, d, alpha=coef).half().reshape(b.shape))

        def restore_host():
            for m in mods:
                unet._load(m + ".weight", base[m])

        split = dict(merge=0.0, reload=0.0)
        real_merge, real_load = Lm.lora_merge, unet._load

        def merge_probe(*a, **k):
            sync()
            t0 = time.perf_counter()
            r = real_merge(*a, **k)
            sync()
            split["merge"] += time.perf_counter() - t0
            return r

        def load_probe(*a, **k):
            t0 = time.perf_counter()
            r = real_load(*a, **k)
            split["reload"] += time.perf_counter() - t0
            return r

        for fn in (merges, addmm, copies):          # warm every shape the timed windows use
            fn()
        sync()
        peak0 = torch.cuda.memory_allocated()
        T = {k: [] for k in ("first", "change", "change_merge", "change_reload", "disable", "refold_forward", "steady_forward", "host", "host_merge_only", "merges", "addmm", "copies")}
        for rep in range(args.reps + 1):            # rep 0 is the warm-up of every column
            unet.unload_lora()
            unet.load_lora_adapter(asd, "bench")
            forward()
            row = dict(first=timed(lambda: unet.set_adapters(["bench"], 0.8)))
            if rep == 0:
                extra = torch.cuda.memory_allocated() - peak0
            row["refold_forward"] = forward()
            row["steady_forward"] = statistics.median(forward() for _ in range(3))
            row["change"] = timed(lambda: unet.set_adapters(["bench"], 0.6))
            forward()
            split["merge"] = split["reload"] = 0.0
            Lm.lora_merge, unet._load = merge_probe, load_probe
            try:
                unet.set_adapters(["bench"], 0.8)
            finally:
                Lm.lora_merge = real_merge
                del unet._load
            row["change_merge"], row["change_reload"] = split["merge"], split["reload"]
            forward()
            row["disable"] = timed(unet.disable_lora)
            unet.enable_lora()
            unet.unload_lora()
            row["merges"], row["addmm"], row["copies"] = timed(merges), timed(addmm), timed(copies)
            t0 = time.perf_counter()
            for m in mods[: max(1, len(mods) // 8)]:                      # the host merge alone, on an eighth of the weights (scaled up below)
                b, d, u = host[m]
                torch.addmm(b.reshape(b.shape[0], -1).float(), u, d, alpha=coef).half()
            row["host_merge_only"] = (time.perf_counter() - t0) * c["params"] / sum(base[m].numel() for m in mods[: max(1, len(mods) // 8)])
            row["host"] = timed(host_route)
            restore_host()
            forward()
            if rep:
                for k, v in row.items():
                    T[k].append(v)
        S = {k: stat(v) for k, v in T.items()}
        refold = [a - b for a, b in zip(T["refold_forward"], T["steady_forward"])]
        S["refold"] = stat(refold)
        gbs = lambda nbytes, s: nbytes / s["median"] / 1e9
        res = dict(times=S, extra_device_bytes=extra, merge_GBps=gbs(c["merge_bytes"], S["merges"]), copy_GBps=gbs(2 * c["weight_bytes"], S["copies"]),
                   merge_TFLOPs=c["flops"] / S["merges"]["median"] / 1e12, refold_share_of_switch=S["refold"]["median"] / (S["change"]["median"] + S["refold"]["median"]))
        result["adapters"][which] = res
        print(f"\n== {which}: {c['modules']} weights, {c['weight_bytes'] / 1e9:.3f} GB, rank {args.rank} ==")
        print(f"set_adapters, first (pristine copies taken)   {fmt(S['first'])}")
        print(f"set_adapters, weight change                   {fmt(S['change'])}")
        print(f"   of it merge launches (instrumented pass)   {fmt(S['change_merge'])}")
        print(f"   of it reloads (load + synchronise each)    {fmt(S['change_reload'])}")
        print(f"disable_lora (reloads from the copies)        {fmt(S['disable'])}")
        print(f"re-fold + context K/V at the next forward     {fmt(S['refold'])}   (first forward {fmt(S['refold_forward'])}, steady {fmt(S['steady_forward'])})")
        print(f"   share of switch + re-fold                  {100 * res['refold_share_of_switch']:.1f} %")
        print(f"yardstick 1: host fp32 merge + loads          {fmt(S['host'])}   (the merge alone, scaled from an eighth: {fmt(S['host_merge_only'])})")
        print(f"merges alone (ia2p_lora_merge)                {fmt(S['merges'])}   {res['merge_GBps']:.0f} GB/s, {res['merge_TFLOPs']:.1f} TFLOP/s")
        print(f"yardstick 2: torch.addmm fp32 on the device   {fmt(S['addmm'])}")
        print(f"yardstick 3: device-to-device copies          {fmt(S['copies'])}   {res['copy_GBps']:.0f} GB/s")
        print(f"extra device memory while active              {extra / 1e9:.3f} GB")
        del base, facs, host, f32, scratch
        unet.unload_lora()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"\nwrote {args.out}")


if __name__ == "__main__":
    main()
