"""Worker of tests/test_hip_meld_ddp_two_ranks.py: one data-parallel rank of engine.MeldEngine on the (shared) GPU, gloo
process group (RCCL needs one GPU per rank; the data-parallel logic under test is backend-agnostic)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

N_STEPS = 2


def run(rank, world, out_path):
    from gan_ffn_amd import data as D, dialogue_rnn as DR, engine as E
    pg = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        pg = dist.group.WORLD
    torch.manual_seed(99)                                      # identical replicas on every rank
    net = DR.MELDLSTMModel(600, 300, 600, n_classes=7, dropout=0.0).cuda().train()
    full = D.synthetic_batch(B=4, S_max=12, seed=21, device="cuda", n_classes=7, dims={"text": 600}, lo=3, mean=8)
    batch = D.shard_batch(full, rank, world) if world > 1 else full
    eng = E.MeldEngine(net, process_group=pg)
    losses = []
    for _ in range(N_STEPS):
        loss, _ = eng.step(batch, train=True)
        losses.append(float(loss))
    torch.cuda.synchronize()
    torch.save({"losses": losses, "mask_sum": float(batch["umask"].sum()), "slab": eng.slab.detach().cpu().clone(),
                "exp_avg": eng.exp_avg.detach().cpu().clone(), "step": int(eng.step_count.item()),
                "linear": net.linear.weight.detach().cpu().clone()}, out_path)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    run(int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), sys.argv[1])
