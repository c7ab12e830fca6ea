"""Decode speed of the instruction LLM at full size (Vicuna-7B shape, seeded synthetic weights), and the decode GEMV against the only kernel
the library had for M = 1, `ia2p_linear_small`.

  part 1  prompt of 64 rows, 100 decode tokens (teacher-forced ids: the time of a token does not depend on which one it is), after one
          warm-up request; stream-synchronised wall time. Prints the prefill time, ms per token, weight bytes per token / that time in TB/s
          and its fraction of the 6.29 TB/s copy rate (MI355X_MICROARCH.md). The weight bytes are what one token must read: the 32 layers'
          projections and the lm_head, counted from the shapes (norm weights, the KV cache and the activations are left out).
  part 2  the four layer shapes N x K = 12288 x 4096 (fused QKV), 4096 x 4096, 22016 x 4096 (fused gate/up), 4096 x 11008: `ia2p_llm_gemv`
          and `ia2p_linear_small` (M = 1) in the same process, interleaved, each launch on another copy of the weights out of a pool larger
          than the 256 MiB Infinity Cache so both read from HBM; device events around one pass over the pool; median of REPS repetitions.

  --bits 4 [--quant-type fp4|nf4]: part 1 runs both weight formats one after the other in the one process (fp16, then 4-bit: codes + one
          fp32 absmax per 64 weights, 0.5625 bytes per projection weight), and part 2 gets a third column for `ia2p_llm_gemv_q4` on the same
          shapes, interleaved with the other two, its pool holding the quantised copies of the same matrices (a pool over 256 MiB as well).

  --batch 1,2,4,8: part 1 is followed, per format, by the batched decode (`ia2p_llm_decode_batch`, n sequences per weight pass): for every n the ms per
          decode step at n rows beside n serial `ia2p_llm_decode` steps, measured in the same process one after the other (second request, 64-row
          prompts, the same tokens, stream-synchronised wall time; the serial figure is n x the ms of one serial step over the same number of steps).
          Part 2 gets one more line per shape and M: `ia2p_llm_gemv_rows` (and `ia2p_llm_gemv_q4_rows` with --bits 4) on the same pools, interleaved
          with the single-row launches, us per launch and per row.

  --sampler host,device: whole `generate` (n = 1) and `generate_batch` (n = 8) calls, sampling on (temperature 0.3, top-k 50), 64-row prompts, no stopping
          criterion, per format. The samplers named alternate in the one process (round 0 warms up); a call is timed stream-synchronised, once for --tokens new
          tokens and once for one, and the figure is the difference per further token: ms per generated token with the prefills taken out. Under "host" the
          tool passes no `sampler` keyword when the tree's `generate` has none, so the same command times a tree from before the keyword. Then the sampler
          launch alone (`ia2p_sample_tokens` on 1 and 8 logits rows of the vocabulary, device events around 200 launches, us per launch).
  --top-p P (with --sampler): the calls above pass `top_p=P`, and the `ia2p_sample_tokens_p` launch at that top-p is timed next to the `ia2p_sample_tokens`
          launch, the two alternating in the one process: 1 and 8 rows of 32000, top-k 50 and 0.

    python tools/llm_decode_bench.py [--layers 32] [--tokens 100] [--reps 30] [--bits 4] [--quant-type fp4] [--batch 1,2,4,8] [--sampler host,device] [--top-p P] [--rounds 3]
                                     [--skip-decode] [--skip-gemv]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instructany2pix_amd import _ffi
from instructany2pix_amd.config import BNB_4BIT_CODEBOOKS, vicuna_7b
from instructany2pix_amd.llm import HipInstructAny2PixLM
from instructany2pix_amd.weights import iter_synthetic, llm_param_specs

DEV = "cuda:0"
COPY_RATE = 6.29e12


def decode_part(layers, tokens, bits=16, quant_type="fp4"):
    cfg = vicuna_7b(32000)
    cfg.num_hidden_layers = layers
    t0 = time.perf_counter()
    lm = HipInstructAny2PixLM(cfg, DEV, max_positions=256, load_in_4bit=bits == 4, bnb_4bit_quant_type=quant_type)
    lm.load_state_dict(iter_synthetic(llm_param_specs(cfg), 7, DEV, torch.float16))
    torch.cuda.synchronize()
    fmt = "fp16" if bits == 16 else f"4-bit {quant_type}"
    print(f"[{fmt}] model ready in {time.perf_counter() - t0:.1f} s ({layers} layers, arena {lm.arena.numel() / 1e9:.3f} GB)", flush=True)
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    wbytes = int((2 if bits == 16 else 0.5625) * layers * (4 * H * H + 3 * H * I)) + 2 * V * H
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(3, V, (64,), generator=g)
    nxt = torch.randint(3, V, (tokens,), generator=g).tolist()
    for rnd in range(2):           # request 0 warms up
        lm.reset()
        emb = lm.embed_tokens(prompt)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        lm.prefill(emb)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        for t in nxt:
            lm.decode(t)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        ms = (t2 - t1) * 1e3 / tokens
        print(f"[{fmt}] request {rnd}: prefill(64) {(t1 - t0) * 1e3:.2f} ms; decode {ms:.3f} ms per token over {tokens} tokens; "
              f"{wbytes / 1e9:.2f} GB of weights per token -> {wbytes / (ms * 1e-3) / 1e12:.2f} TB/s = {wbytes / (ms * 1e-3) / COPY_RATE:.3f} of the copy rate",
              flush=True)
    del lm
    torch.cuda.empty_cache()


def batch_part(layers, tokens, rows, bits=16, quant_type="fp4"):
    cfg = vicuna_7b(32000)
    cfg.num_hidden_layers = layers
    lm = HipInstructAny2PixLM(cfg, DEV, max_positions=64 + tokens + 8, load_in_4bit=bits == 4, bnb_4bit_quant_type=quant_type, max_batch=max(rows))
    lm.load_state_dict(iter_synthetic(llm_param_specs(cfg), 7, DEV, torch.float16))
    torch.cuda.synchronize()
    fmt = "fp16" if bits == 16 else f"4-bit {quant_type}"
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(3, cfg.vocab_size, (64,), generator=g)
    nxt = torch.randint(3, cfg.vocab_size, (tokens,), generator=g).tolist()
    emb = lm.embed_tokens(prompt)
    print(f"[{fmt}] batched decode, {layers} layers, {max(rows)} slots of {lm.max_positions} positions ({lm.kv.numel() / 2 ** 20:.0f} MiB of cache); ms per step over {tokens} steps")
    for rnd in range(2):           # request 0 warms up
        for n in rows:
            slots = list(range(n))
            for s in slots:
                lm.reset_slot(s)
                lm.prefill_slot(s, emb)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for t in nxt:
                lm.decode_batch(slots, [t] * n)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            lm.reset()
            lm.prefill(emb)
            torch.cuda.synchronize(); t2 = time.perf_counter()
            for t in nxt:
                lm.decode(t)
            torch.cuda.synchronize(); t3 = time.perf_counter()
            b, s1 = (t1 - t0) * 1e3 / tokens, (t3 - t2) * 1e3 / tokens
            print(f"[{fmt}] request {rnd}: n = {n}: decode_batch {b:.3f} ms per step, {n} serial decode steps {n * s1:.3f} ms ({s1:.3f} each), "
                  f"serial / batched {n * s1 / b:.2f}x, {n / (b * 1e-3):.0f} tokens per second over the {n} requests", flush=True)
    del lm
    torch.cuda.empty_cache()


def sampler_part(layers, tokens, samplers, rounds, bits=16, quant_type="fp4", top_p=None):
    import inspect
    cfg = vicuna_7b(32000)
    cfg.num_hidden_layers = layers
    lm = HipInstructAny2PixLM(cfg, DEV, max_positions=64 + tokens + 8, load_in_4bit=bits == 4, bnb_4bit_quant_type=quant_type, max_batch=8)
    lm.load_state_dict(iter_synthetic(llm_param_specs(cfg), 7, DEV, torch.float16))
    torch.cuda.synchronize()
    fmt = "fp16" if bits == 16 else f"4-bit {quant_type}"
    has_kw = "sampler" in inspect.signature(lm.generate).parameters
    if not has_kw and samplers != ["host"]:
        sys.exit("--sampler: this tree's generate() has the host sampler only")
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(3, cfg.vocab_size, (1, 64), generator=g) for _ in range(8)]
    print(f"[{fmt}] whole generate / generate_batch calls, {layers} layers, sampling at temperature 0.3, top-k 50{'' if top_p is None else f', top-p {top_p}'}; ms per generated token = "
          f"(call with {tokens} new tokens - call with 1) / {tokens - 1}", flush=True)

    def call(n, sampler, new):
        kw = dict(do_sample=True, temperature=0.3, max_new_tokens=new, **({"sampler": sampler} if has_kw else {}), **({} if top_p is None else {"top_p": top_p}))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        if n == 1:
            lm.generate(prompts[0], **kw)
        else:
            lm.generate_batch(prompts[:n], **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for rnd in range(rounds + 1):          # round 0 warms up
        for n in (1, 8):
            for sampler in samplers:
                torch.manual_seed(rnd)
                one, full = call(n, sampler, 1), call(n, sampler, tokens)
                print(f"[{fmt}] round {rnd}{' (warm-up)' if rnd == 0 else ''}: n = {n}, sampler {sampler}: {(full - one) / (tokens - 1):.3f} ms per generated token "
                      f"(call of {tokens} tokens {full:.1f} ms, of one token {one:.1f} ms)", flush=True)
    if "device" in samplers:
        lib, s = _ffi.lib(), _ffi.current_stream()
        V = cfg.vocab_size
        logits = torch.randn(8, V, generator=torch.Generator().manual_seed(2)).to(DEV) * 4
        out = torch.empty(8, dtype=torch.int32, device=DEV)
        for n in (1, 8):
            seeds, steps = (C.c_uint64 * n)(*range(1, n + 1)), (C.c_uint32 * n)(*range(n))
            for do_sample, what in ((1, "temperature 0.3, top-k 50"), (0, "argmax")):
                med = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(200):
                        _ffi.check(lib.ia2p_sample_tokens(s, _ffi.ptr(logits), V, n, V, 0.3, 50, do_sample, seeds, steps, _ffi.ptr(out), None, None), None, llm=True)
                    e1.record(); e1.synchronize()
                    med.append(e0.elapsed_time(e1) * 1e3 / 200)
                print(f"  ia2p_sample_tokens, {n} row{'s' if n > 1 else ''} of {V}, {what}: {statistics.median(med):.2f} us per launch (back to back, median of 5 x 200; min {min(med):.2f})", flush=True)
        if top_p is not None:
            nucleus_launch_part(lib, s, logits, out, top_p)
    del lm
    torch.cuda.empty_cache()


def nucleus_launch_part(lib, s, logits, out, top_p):
    """the `ia2p_sample_tokens_p` launch next to the `ia2p_sample_tokens` launch, interleaved in the one process: V = 32000, 1 and 8 rows, top-k 50 and 0"""
    V = logits.shape[1]

    def launches(n, top_k, p, seeds, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            if p is None:
                st = lib.ia2p_sample_tokens(s, _ffi.ptr(logits), V, n, V, 0.3, top_k, 1, seeds, steps, _ffi.ptr(out), None, None)
            else:
                st = lib.ia2p_sample_tokens_p(s, _ffi.ptr(logits), V, n, V, 0.3, top_k, p, 1, seeds, steps, _ffi.ptr(out), None, None)
            _ffi.check(st, None, llm=True)
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / 200

    for n in (1, 8):
        seeds, steps = (C.c_uint64 * n)(*range(1, n + 1)), (C.c_uint32 * n)(*range(n))
        for top_k in (50, 0):
            med = {None: [], top_p: []}
            for rnd in range(6):               # round 0 warms up; the two launches alternate
                for p in (None, top_p):
                    t = launches(n, top_k, p, seeds, steps)
                    if rnd:
                        med[p].append(t)
            a, b = statistics.median(med[None]), statistics.median(med[top_p])
            print(f"  {n} row{'s' if n > 1 else ''} of {V}, temperature 0.3, top-k {top_k}: ia2p_sample_tokens {a:.2f} us per launch (min {min(med[None]):.2f}), "
                  f"ia2p_sample_tokens_p at top-p {top_p} {b:.2f} us (min {min(med[top_p]):.2f}): + {b - a:.2f} us (back to back, median of 5 x 200, interleaved)", flush=True)


def gemv_part(reps, bits=16, quant_type="fp4", rows=()):
    lib = _ffi.lib()
    cb = (C.c_float * 16)(*BNB_4BIT_CODEBOOKS[quant_type])
    g = torch.Generator(device=DEV).manual_seed(2)
    print("GEMV vs linear_small, M = 1, weights cycled through a pool > 256 MiB, median us per launch:")
    for N, K in ((12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)):
        nbytes = N * K * 2
        copies = max(4, -(-(640 << 20) // nbytes))
        pool = [(torch.randn(N, K, generator=g, device=DEV, dtype=torch.float32) * K ** -0.5).half() for _ in range(copies)]
        x16 = torch.randn(1, K, generator=g, device=DEV).half()
        x32 = x16.float().reshape(-1).contiguous()
        xm = torch.cat([x32[None], torch.randn(7, K, generator=g, device=DEV)]).contiguous()      # [8, K]: row 0 is the single-row input
        om = torch.empty(8, N, dtype=torch.float32, device=DEV)
        o16 = torch.empty(1, N, dtype=torch.float16, device=DEV)
        o32 = torch.empty(N, dtype=torch.float32, device=DEV)
        s = _ffi.current_stream()

        def run_gemv():
            for w in pool:
                _ffi.check(lib.ia2p_llm_gemv(s, _ffi.ptr(w), _ffi.ptr(x32), _ffi.ptr(o32), N, K))

        def run_small():
            for w in pool:
                _ffi.check(lib.ia2p_linear_small(s, _ffi.ptr(x16), _ffi.ptr(w), None, _ffi.ptr(o16), 1, N, K, 0, 0))

        def run_rows(M):
            def fn():
                for w in pool:
                    _ffi.check(lib.ia2p_llm_gemv_rows(s, _ffi.ptr(w), _ffi.ptr(xm), _ffi.ptr(om), N, K, M), None, llm=True)
            return fn

        runs = [("gemv", run_gemv), ("small", run_small)] + [(f"rows{M}", run_rows(M)) for M in rows]
        if bits == 4:
            qbytes = lib.ia2p_llm_q4_packed_bytes(N, K) + 4 * (N * K // 64)
            qcopies = max(4, -(-(640 << 20) // qbytes))
            qpool = []
            for i in range(qcopies):
                w = pool[i] if i < copies else (torch.randn(N, K, generator=g, device=DEV, dtype=torch.float32) * K ** -0.5).half()
                packed = torch.empty(lib.ia2p_llm_q4_packed_bytes(N, K), dtype=torch.uint8, device=DEV)
                absmax = torch.empty(N * K // 64, dtype=torch.float32, device=DEV)
                _ffi.check(lib.ia2p_llm_quantize_q4(s, _ffi.ptr(w), N, K, cb, _ffi.ptr(packed), _ffi.ptr(absmax)), None, llm=True)
                qpool.append((packed, absmax))
            del w
            o4 = torch.empty(N, dtype=torch.float32, device=DEV)

            def run_q4():
                for packed, absmax in qpool:
                    _ffi.check(lib.ia2p_llm_gemv_q4(s, _ffi.ptr(packed), _ffi.ptr(absmax), cb, _ffi.ptr(x32), _ffi.ptr(o4), N, K), None, llm=True)

            def run_q4_rows(M):
                def fn():
                    for packed, absmax in qpool:
                        _ffi.check(lib.ia2p_llm_gemv_q4_rows(s, _ffi.ptr(packed), _ffi.ptr(absmax), cb, _ffi.ptr(xm), _ffi.ptr(om), N, K, M), None, llm=True)
                return fn

            runs.append(("q4", run_q4))
            runs += [(f"q4rows{M}", run_q4_rows(M)) for M in rows]
        for _, fn in runs:
            fn()
        torch.cuda.synchronize()
        err = float((o32 - o16.float().reshape(-1)).abs().max())
        times = {name: [] for name, _ in runs}
        per = {name: (qcopies if name.startswith("q4") else copies) for name, _ in runs}
        for _ in range(reps):
            for name, fn in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / per[name])
        a, b = statistics.median(times["gemv"]), statistics.median(times["small"])
        print(f"  {N:6d} x {K:5d} ({nbytes / 1e6:6.1f} MB, pool of {copies}): llm_gemv {a:7.2f} us ({nbytes / a / 1e6:.2f} TB/s), linear_small {b:7.2f} us "
              f"({nbytes / b / 1e6:.2f} TB/s), ratio {b / a:.2f}x, min {min(times['gemv']):.2f} / {min(times['small']):.2f}, max |difference of the outputs| {err:.2e}", flush=True)
        if bits == 4:
            q = statistics.median(times["q4"])
            print(f"  {'':6s}   {'':5s}  4-bit {quant_type} ({qbytes / 1e6:6.1f} MB, pool of {qcopies}): llm_gemv_q4 {q:7.2f} us ({qbytes / q / 1e6:.2f} TB/s of the bytes it reads), "
                  f"min {min(times['q4']):.2f}, fp16 / 4-bit time {a / q:.2f}x", flush=True)
        for M in rows:
            r = statistics.median(times[f"rows{M}"])
            line = f"  {'':6s}   {'':5s}  M = {M}: llm_gemv_rows {r:7.2f} us ({r / M:6.2f} per row, {M * a / r:.2f}x of {M} single-row launches)"
            if bits == 4:
                rq = statistics.median(times[f"q4rows{M}"])
                line += f"; llm_gemv_q4_rows {rq:7.2f} us ({rq / M:6.2f} per row, {M * q / rq:.2f}x of {M} single-row launches)"
            print(line, flush=True)
        if bits == 4:
            del qpool
        del pool
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--bits", type=int, default=16, choices=(16, 4))
    ap.add_argument("--quant-type", default="fp4", choices=sorted(BNB_4BIT_CODEBOOKS))
    ap.add_argument("--batch", default="", help="comma-separated row counts (1..8) for the batched decode and the multi-row GEMVs, e.g. 1,2,4,8")
    ap.add_argument("--sampler", default="", help="comma-separated samplers (host, device) for the whole-call timing of generate / generate_batch")
    ap.add_argument("--top-p", type=float, default=None, help="with --sampler: pass top_p to generate / generate_batch, and time the ia2p_sample_tokens_p launch next to ia2p_sample_tokens")
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds of the --sampler part (after one warm-up round)")
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--skip-gemv", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("llm_decode_bench needs the GPU: no timing is reported without one")
    rows = tuple(int(x) for x in a.batch.split(",") if x)
    if any(n < 1 or n > 8 for n in rows):
        sys.exit("--batch: row counts of 1..8")
    samplers = [x for x in a.sampler.split(",") if x]
    if any(x not in ("host", "device") for x in samplers):
        sys.exit("--sampler: host, device or both")
    if not a.skip_gemv:
        gemv_part(a.reps, a.bits, a.quant_type, rows)
    if not a.skip_decode:
        decode_part(a.layers, a.tokens)
        if rows:
            batch_part(a.layers, a.tokens, rows)
        if a.bits == 4:
            decode_part(a.layers, a.tokens, 4, a.quant_type)
            if rows:
                batch_part(a.layers, a.tokens, rows, 4, a.quant_type)
    if samplers:
        sampler_part(a.layers, a.tokens, samplers, a.rounds, top_p=a.top_p)
        if a.bits == 4:
            sampler_part(a.layers, a.tokens, samplers, a.rounds, 4, a.quant_type, top_p=a.top_p)
