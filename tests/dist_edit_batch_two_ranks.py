"""Two ranks sharing ONE GPU (gloo transport): `InstructAny2PixPipeline.edit_batch` shards the requests of each of its three loops (hot segment, refiner pass,
inpaint passes) contiguously over the ranks, every rank runs its shard in groups, the results are all-gathered in request order -- and equal the
single-process run of the same list bit for bit (same groups, same kernels). Launched by tests/test_edit_batch_gpu.py::test_edit_batch_sharded_over_two_ranks
through torch.distributed.run."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["IA2P_DIST_BACKEND"] = "gloo"
from instructany2pix_amd import dist as D
from tests.test_edit_batch_gpu import KNOBS, Models, _cond, _lists

rank, world, _ = D.init_distributed()
assert world == 2
models = Models()                          # same seeded weights on both ranks
# 8 requests, all refined, all with two subjects: every loop sees 8 rows = 4 per rank = groups of 2 on either side of the shard boundary
knobs = [dict(KNOBS[i % 4], refinement=0.1 + 0.06 * (i % 2), subject_strength=0.1 + 0.06 * (i % 3 == 0)) for i in range(8)]
conds = {f"edit {i}": _cond(models, 120 + i, n_subjects=2) for i in range(8)}
pipe = models.pipeline(conds, refiner_handoff="latent")
insts = list(conds)
got = pipe.edit_batch(insts, [[]] * 8, **_lists(knobs), group=2, shard=True)
assert len(got) == 8
mine = torch.cat([torch.cat([nr, oo]) for nr, oo, _ in got]).cpu()
both = D.gather_batches(mine[None])
assert torch.equal(both[0], both[1]), "ranks disagree on the gathered result"
if rank == 0:
    solo = pipe.edit_batch(insts, [[]] * 8, **_lists(knobs), group=2, shard=False)
    for i, ((nr, oo, msg), (snr, soo, _)) in enumerate(zip(got, solo)):
        assert msg == "SUCCESS!" and torch.equal(nr, snr) and torch.equal(oo, soo), (i, float((oo.float() - soo.float()).abs().max()))
        assert not torch.equal(nr, oo)
    assert not torch.equal(got[0][1], got[1][1])
    print("EDIT_BATCH_DIST_OK")
D.barrier()
torch.distributed.destroy_process_group()
