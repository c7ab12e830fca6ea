"""The three seeded-noise launches, N times each at B = 1 and B = 8 on 4 x 128 x 128 latents: the target of a kernel-trace pass that reads their device
times (tools/e2e_edit_bench.py --seeded times the calls from the host, where the Python call and the launch itself dominate).

    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python tools/noise_launch_probe.py [reps]

Rows of the kernel stats to read: randn_seeded_kernel<true> (fp16 out), posterior_seeded_kernel, polar_mix_kernel; B = 1 and B = 8 run the same kernels with
one and eight rows in grid.y, so the per-B figures come from the trace (grid size), the stats table gives their mean."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instructany2pix_amd import noise  # noqa: E402

DEV = "cuda:0"
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
H = int(os.environ.get("PX", 1024)) // 8
for B in (1, 8):
    seeds = [0x5EED0000 + 977 * i for i in range(B)]
    z = torch.empty(B, 4, H, H, dtype=torch.float16, device=DEV)
    x = noise.randn_seeded(seeds, 9, (4, H, H), torch.float16, DEV)
    mom = noise.randn_seeded(seeds, 8, (8, H, H), torch.float16, DEV)
    for _ in range(REPS):
        noise.randn_seeded(seeds, noise.DRAW_POLAR, (4, H, H), torch.float16, DEV, out=z)
        noise.posterior_sample(mom, seeds, noise.DRAW_BASE_POSTERIOR, 0.13025)
        noise.polar_mix(x, z, 0.7)
    torch.cuda.synchronize()
print(f"noise_launch_probe: {REPS} x 3 launches at B = 1 and B = 8, 4 x {H} x {H} latents")
