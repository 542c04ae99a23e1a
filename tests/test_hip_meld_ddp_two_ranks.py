"""engine.MeldEngine data-parallel: two ranks (one process each, sharing this box's single GPU; gloo process group because RCCL
wants one GPU per rank), each owning two of the four dialogues of a (12, 4) batch, against one process on the whole batch.
The replicas stay bit-identical after 2 all-reduced steps, and the mean of the ranks' first-step losses weighted by their mask
sums is the one-process loss (MaskedNLLLoss divides by the LOCAL mask sum: model.py:76) at 2e-5 relative."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, tmp, tag, mode):
    port = _free_port()
    procs, outs = [], []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", GANFFN_DP_MODE=mode)
        out = os.path.join(tmp, "%s_r%d.pt" % (tag, r))
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "meld_ddp_gpu_worker.py"), out], env=env))
    for p in procs:
        assert p.wait(timeout=280) == 0
    return [torch.load(o) for o in outs]


@pytest.mark.parametrize("mode", ["inline", "buckets"])
def test_two_ranks_stay_identical_and_average_to_the_global_loss(tmp_path, mode):
    two = _run(2, str(tmp_path), "w2" + mode, mode)
    one = _run(1, str(tmp_path), "w1" + mode, mode)[0]
    for k in ("slab", "exp_avg", "linear"):
        assert torch.equal(two[0][k], two[1][k]), k
    assert two[0]["step"] == two[1]["step"] == one["step"] == 2
    assert torch.equal(two[0]["linear"], one["linear"])                    # never touched, on any rank
    n0, n1 = two[0]["mask_sum"], two[1]["mask_sum"]
    assert n0 + n1 == one["mask_sum"]
    mean = (two[0]["losses"][0] * n0 + two[1]["losses"][0] * n1) / (n0 + n1)
    print("ranks' weighted first-step loss %.7f, one process %.7f" % (mean, one["losses"][0]))
    assert abs(mean - one["losses"][0]) <= 2e-5 * abs(one["losses"][0])
    # Adam ran on the all-reduced gradient
    assert float(two[0]["exp_avg"].abs().max()) > 0
