"""Time the two recurrent classifiers against the batch size and print one JSON line (the table of profiles/recurrence_batch_ab.txt).

rows     drnn           BiModel (general attention, D_m = 100, D_g = D_p = 500, D_e = D_h = 100, 6 classes) at (94, B), P = 2
         drnn_listener  the same with listener state
         meld           MELDLSTMModel(600, 300, 600, 7 classes) at (33, B)
columns  parent   the module-path train step (forward + backward under autograd, dropout on) with the dialogues in chunks of 32 one after
                  the other, each through the 32-dialogue entry points: the launches of the commit before the wide dialogue axis.
                  Produced inside this process (so that it alternates with the others) by running this tree's module path with
                  ops.MAX_DIALOGUES = 32; `--only module --root <checkout of that commit>` times the real thing for comparison.
         module   the same step as this tree runs it: one native call per direction pair / per LSTM layer up to ops.MAX_DIALOGUES
         engine   the step runner's train step (DrnnEngine on a GAN_FFN_DialogueRNN: three generators + the head + Adam; MeldEngine)
                  built with max_dialogues = max(32, B)
Per cell: the median of rounds x iters device-synchronised iterations timed with HIP events, after a warm-up, the three columns
alternating round by round; ms per step and utterances (valid steps of the ragged batch) per second.

    python tools/recurrence_batch_time.py [--rows drnn,drnn_listener,meld] [--batches 32,64,128,256] [--rounds 3] [--iters 8] [--warmup 5]
    python tools/recurrence_batch_time.py --only {parent,module,engine} --rows drnn --batches 128 [--root DIR]     # one cell; for a
        kernel trace (rocprofv3 --kernel-trace --stats -- python ... --trace-gap 0.5: the launches between the two idle gaps are
        rounds x (1 + iters) steps), or, with --root, the module path of another checkout of this project
"""
import argparse
import json
import os
import statistics
import sys

W = [1.2, 0.60072, 0.38066, 0.94019, 0.67924, 0.34332]          # train_IEMOCAP_DialogueRNN.py:738


def make_cell(row, B, only):
    """-> dict name -> step function, utterances per step"""
    import torch
    from gan_ffn_amd import data as D, dialogue_rnn as DR, model as M, ops
    torch.manual_seed(3407)
    steps = {}
    if row == "meld":
        S, Cn = 33, 7
        b = D.synthetic_batch(B=B, S_max=S, seed=3407, device="cuda", n_classes=Cn, dims={"text": 600}, lo=3, mean=17)
        net = DR.MELDLSTMModel(600, 300, 600, n_classes=Cn, dropout=0.6).cuda().train()
        loss_fn = M.MaskedNLLLoss()

        def module():
            net.zero_grad(set_to_none=True)
            lp = net(b["text"], None, b["umask"])[0]
            loss_fn(lp.transpose(0, 1).contiguous().view(-1, Cn), b["label"].view(-1), b["umask"]).backward()
    else:
        S, Cn = 94, 6
        b = D.synthetic_batch(B=B, S_max=S, seed=3407, device="cuda")
        net = DR.BiModel(100, 500, 500, 100, 100, n_classes=Cn, context_attention="general", listener_state=row == "drnn_listener",
                         dropout_rec=0.1, dropout=0.6).cuda().train()
        loss_fn = M.MaskedNLLLoss(torch.tensor(W, device="cuda"))
        U = b["text"].contiguous()

        def module():
            net.zero_grad(set_to_none=True)
            lp = net(U, b["qmask"], b["umask"])[0]
            loss_fn(lp.transpose(0, 1).contiguous().view(-1, Cn), b["label"].view(-1), b["umask"]).backward()
    assert tuple(b["text"].shape[:2]) == (S, B), b["text"].shape

    def parent():
        keep = ops.MAX_DIALOGUES
        ops.MAX_DIALOGUES = 32               # chunks of 32 through the 32-dialogue entry points
        try:
            module()
        finally:
            ops.MAX_DIALOGUES = keep
    if only in (None, "module"):
        steps["module"] = module
    if only in (None, "parent"):
        steps["parent"] = parent
    if only in (None, "engine"):
        from gan_ffn_amd import engine as E
        torch.manual_seed(3407)
        if row == "meld":
            eng = E.MeldEngine(DR.MELDLSTMModel(600, 300, 600, n_classes=7, dropout=0.6).cuda().train(), max_dialogues=max(32, B))
        else:
            gnet = M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), 100, 500, 500, 100, 100,
                                         100, n_classes=6, listener_state=row == "drnn_listener", context_attention="general",
                                         dropout_rec=0.1, dropout=0.6).cuda().train()
            eng = E.DrnnEngine(gnet, lr=1e-4, weight_decay=1e-5, max_dialogues=max(32, B))
        steps["engine"] = lambda: eng.step(b, train=True)
    return steps, float(b["umask"].sum())


def time_cell(steps, rounds, iters, warmup, gap=0.0):
    """the columns alternate round by round; every iteration is synchronised and timed with its own pair of events.
    gap > 0: the device idles that many seconds before the first and after the last timed round (then one marker launch), so a
    kernel trace shows which launches belong to the rounds x (1 + iters) steps in between"""
    import time
    import torch
    ms = {k: [] for k in steps}
    for k, f in steps.items():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    if gap:
        time.sleep(gap)
    for _ in range(rounds):
        for k, f in steps.items():
            f()                                  # (re-warm after the other columns ran)
            torch.cuda.synchronize()
            for _ in range(iters):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                f()
                t1.record()
                torch.cuda.synchronize()
                ms[k].append(t0.elapsed_time(t1))
    if gap:
        time.sleep(gap)
        torch.zeros(1, device="cuda").add_(1.0)
        torch.cuda.synchronize()
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="drnn,drnn_listener,meld")
    ap.add_argument("--batches", default="32,64,128,256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["parent", "module", "engine"], default=None)
    ap.add_argument("--trace-gap", type=float, default=0.0, help="seconds of idle device around the timed block (for a kernel trace)")
    ap.add_argument("--root", default=None, help="checkout of this project to import gan_ffn_amd from (default: this one)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from gan_ffn_amd import ops
    if not hasattr(ops, "MAX_DIALOGUES"):
        assert args.only == "module", "a checkout without the wide dialogue axis has the module path only"
        ops.MAX_DIALOGUES = 32               # (never read there: its loops are chunks of 32 as written)
    ops.manual_seed(3407)
    out = {"device": torch.cuda.get_device_name(0), "iterations_per_cell": args.rounds * args.iters, "warmup": args.warmup,
           "root": os.path.abspath(args.root) if args.root else None, "cells": []}
    for row in args.rows.split(","):
        for B in (int(x) for x in args.batches.split(",")):
            steps, utt = make_cell(row, B, args.only)
            r = time_cell(steps, args.rounds, args.iters, args.warmup, args.trace_gap)
            cell = {"row": row, "S": 33 if row == "meld" else 94, "B": B, "utterances": utt}
            for k, (med, lo, hi) in r.items():
                cell[k + "_ms"] = round(med, 3)
                cell[k + "_ms_min_max"] = [round(lo, 3), round(hi, 3)]
                cell[k + "_utt_per_s"] = round(utt / (med * 1e-3))
            if "parent_ms" in cell and "module_ms" in cell:
                cell["parent_over_module"] = round(cell["parent_ms"] / cell["module_ms"], 3)
            out["cells"].append(cell)
            print("# %s" % json.dumps(cell), file=sys.stderr, flush=True)
            del steps
            torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
