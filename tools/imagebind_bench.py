"""Warm latency of the ImageBind front end at the full `imagebind_huge` sizes on the MI355X, beside the tests' torch oracle on the host cores:
ms per image (vision tower, 32 x 1280, 257 tokens) and per audio file (audio tower, 12 x 768, 3 clips of 229 tokens + bias row), median of --reps
after warm-up, seeded synthetic weights; also the full-depth agreement with the oracle (the tests stop at 4 / 2 layers).

    python tools/imagebind_bench.py [--reps 10] [--oracle-reps 3] [--batch 1]

Prints one line per tower and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from instructany2pix_amd.imagebind import HipImageBindModel, imagebind_huge_config, imagebind_param_specs      # noqa: E402
from instructany2pix_amd.weights import synthetic_state_dict                                                  # noqa: E402
from tests.imagebind_ref import RefTower, postprocess, rel_l2                                                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--oracle-reps", type=int, default=3)
ap.add_argument("--batch", type=int, default=1, help="files per call")
args = ap.parse_args()
DEV = "cuda:0"
torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
cfg = imagebind_huge_config()
result = {"reps": args.reps, "batch": args.batch, "host_threads": torch.get_num_threads()}
g = torch.Generator().manual_seed(3)
for m, shape, clips in (("vision", (args.batch, 3, 224, 224), 1), ("audio", (args.batch, 3, 1, 128, 204), 3)):
    sd = synthetic_state_dict(imagebind_param_specs(cfg, (m,)), seed=71)
    model = HipImageBindModel(cfg, DEV, modalities=(m,))
    model.load_state_dict(sd)
    x = torch.randn(*shape, generator=g).half()
    xd = x.to(DEV)
    for _ in range(3):
        out = model({m: xd})[m]
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = model({m: xd})[m]
        torch.cuda.synchronize(); times.append((time.perf_counter() - t0) * 1e3)
    ref = RefTower(getattr(cfg, m), m, sd)
    flat = x.reshape(-1, *shape[-3:])
    otimes = []
    for _ in range(args.oracle_reps):
        t0 = time.perf_counter()
        want = postprocess(m, ref(flat)[0], clips)
        otimes.append((time.perf_counter() - t0) * 1e3)
    hip_ms, cpu_ms, err = statistics.median(times) / args.batch, statistics.median(otimes) / args.batch, rel_l2(out, want)
    unit = "image" if m == "vision" else "audio file (3 clips)"
    print(f"{m}: HIP {hip_ms:.2f} ms per {unit} (median of {args.reps}, min {min(times) / args.batch:.2f}); oracle on {torch.get_num_threads()} host threads "
          f"{cpu_ms:.0f} ms; full-depth rel_l2 of the embedding {err:.2e}", flush=True)
    result[m] = {"hip_ms": round(hip_ms, 3), "hip_min_ms": round(min(times) / args.batch, 3), "oracle_cpu_ms": round(cpu_ms, 1), "rel_l2": err}
    del model, ref, sd
print(json.dumps(result))
