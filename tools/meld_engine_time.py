"""Time the MELD classifier's train step and print one JSON line.  All numbers come from the same process, the same model
weights at the start and the same batch — MELDLSTMModel(600, 300, 600, 7 classes) at (S, B) = (33, 32), ragged prefix masks, the
reference script's dropout 0.6, lr 3e-4, L2 1e-4 (train_MELD.py:111-113,143-157):

  engine_train_ms   engine.MeldEngine.step(train=True): the C-ABI step, no autograd graph, one fused Adam
  module_train_ms   the module path: MELDLSTMModel.forward under autograd (the same LSTM and attention kernels through
                    torch.autograd.Functions), MaskedNLLLoss, loss.backward(), torch.optim.Adam over the 36 trained tensors
  engine_eval_ms / module_eval_ms   forward + loss only (model.eval(), no_grad on the module path)

Each figure: a pre-roll, then `--repeats` blocks of `--steps` steps between two device synchronisations, the paths alternating
block by block; the JSON carries every block, the medians, the spread (max - min over the blocks) and the ratios.

    python tools/meld_engine_time.py [--steps 30] [--warmup 20] [--repeats 3] [--only-engine]

--only-engine runs warm-up + timed engine train steps alone (for a kernel trace: rocprofv3 ... -- python ...).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

S, B, C_ = 33, 32, 7
LR, L2, DROPOUT = 3e-4, 1e-4, 0.6


def block(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def batch():
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    lens[0] = S
    umask = (torch.arange(S).unsqueeze(0) < lens.unsqueeze(1)).float()
    text = ((torch.rand(S, B, 600, generator=g) - 0.5) * umask.t().unsqueeze(2)).cuda().contiguous()
    label = (torch.randint(0, C_, (B, S), generator=g) * umask.long()).cuda()
    return {"text": text, "umask": umask.cuda(), "label": label}


def model():
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(3407)
    return DR.MELDLSTMModel(600, 300, 600, n_classes=C_, dropout=DROPOUT).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-engine", action="store_true")
    args = ap.parse_args()
    from gan_ffn_amd import engine, model as M, ops
    ops.manual_seed(3407)
    b = batch()
    net_e = model().train()
    eng = engine.MeldEngine(net_e, lr=LR, weight_decay=L2)
    eng.reserve(S, B)
    if args.only_engine:
        for _ in range(args.warmup):
            eng.step(b, train=True)
        ms = block(lambda: eng.step(b, train=True), args.steps)
        print(json.dumps({"S": S, "B": B, "engine_train_ms": round(ms, 3), "steps": args.steps, "warmup": args.warmup}), flush=True)
        return
    net_m = model().train()
    opt = torch.optim.Adam(net_m.parameters(), lr=LR, weight_decay=L2)
    loss_fn = M.MaskedNLLLoss()

    def module_train():
        opt.zero_grad()
        lp = net_m(b["text"], None, b["umask"])[0]
        loss = loss_fn(lp.transpose(0, 1).contiguous().view(-1, C_), b["label"].view(-1), b["umask"])
        loss.backward()
        opt.step()

    def module_eval():
        with torch.no_grad():
            lp = net_m(b["text"], None, b["umask"])[0]
            loss_fn(lp.transpose(0, 1).contiguous().view(-1, C_), b["label"].view(-1), b["umask"])

    paths = {"engine_train_ms": lambda: eng.step(b, train=True), "module_train_ms": module_train}
    evals = {"engine_eval_ms": lambda: eng.step(b, train=False), "module_eval_ms": module_eval}
    out = {"S": S, "B": B, "dropout": DROPOUT, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "blocks": {}}
    for group, train in ((paths, True), (evals, False)):
        net_m.train(train)
        for step in group.values():
            for _ in range(args.warmup):
                step()
        runs = {k: [] for k in group}
        for _ in range(args.repeats):
            for k, step in group.items():                       # alternating: engine, module, engine, module, ...
                runs[k].append(round(block(step, args.steps), 3))
        for k, v in runs.items():
            out["blocks"][k] = v
            out[k] = round(statistics.median(v), 3)
            out[k.replace("_ms", "_spread_ms")] = round(max(v) - min(v), 3)
    out["train_module_over_engine"] = round(out["module_train_ms"] / out["engine_train_ms"], 3)
    out["eval_module_over_engine"] = round(out["module_eval_ms"] / out["engine_eval_ms"], 3)
    out["train_gain_ms"] = round(out["module_train_ms"] - out["engine_train_ms"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
