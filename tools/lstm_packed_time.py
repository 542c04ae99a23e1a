"""Time engine.MeldEngine's train and eval step with the LSTM on padded (the default) and on packed sequences
(MeldEngine(packed=True): ganffn_lstm_stack_packed_*) and print one JSON line: MELDLSTMModel(600, 300, 600, 7 classes) at
(S, B) = (33, 32), dialogue lengths drawn as bench.py's MELD configuration draws them (data.synthetic_batch, lo = 2, mean = 10,
the longest dialogue stretched to 33 so that S is MELD's longest), dropout 0.6, lr 3e-4, L2 1e-4 (train_MELD.py:111-113,143-157).

One process, the same weights at the start and the same batch for both; a warm-up, then `--repeats` rounds in which the two
alternate, each a block of `--steps` steps between two device synchronisations.  The JSON carries every block, the medians and
the spread (max - min over the blocks), and `padded_3_steps_sha16`: a hash of the parameters and log-probabilities after three
seeded train steps of the padded engine (equal on two trees that compute the same).

    python tools/lstm_packed_time.py [--steps 50] [--warmup 20] [--repeats 5] [--root DIR]

--root DIR imports the package from another checkout (with its own built library), e.g. the parent commit's: a tree without the
`packed` argument is timed on its padded step alone.
"""
import argparse
import hashlib
import inspect
import json
import os
import statistics
import sys
import time

S, B, C_ = 33, 32, 7
LR, L2, DROPOUT = 3e-4, 1e-4, 0.6


def block(torch, step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from gan_ffn_amd import data as D, dialogue_rnn as DR, engine, ops
    b = D.synthetic_batch(B=B, S_max=S, seed=3407, device="cpu", n_classes=C_, dims={"text": 600}, lo=2, mean=10)
    lengths = torch.from_numpy(b["lengths"]).long()
    pad = S - int(lengths.max())                       # stretch the batch to MELD's longest dialogue: S = 33 whatever was drawn
    if pad:
        b["text"] = torch.cat((b["text"], torch.zeros(pad, B, 600)), 0)
        b["umask"] = torch.cat((b["umask"], torch.zeros(B, pad)), 1)
        b["label"] = torch.cat((b["label"], torch.zeros(B, pad, dtype=torch.long)), 1)
    b = {k: b[k].cuda().contiguous() for k in ("text", "umask", "label")}
    has_packed = "packed" in inspect.signature(engine.MeldEngine.__init__).parameters
    # what the padded step computes, as a hash (two trees compute the same when it agrees): 3 seeded train steps of a fresh engine
    ops.manual_seed(3407)
    torch.manual_seed(3407)
    e0 = engine.MeldEngine(DR.MELDLSTMModel(600, 300, 600, n_classes=C_, dropout=DROPOUT).cuda().train(), lr=LR, weight_decay=L2)
    for _ in range(3):
        lp = e0.step(b, train=True)[1]
    torch.cuda.synchronize()
    padded_sha = hashlib.sha256(e0.slab.cpu().numpy().tobytes() + lp.cpu().numpy().tobytes()).hexdigest()[:16]
    del e0
    engines = {}
    for name in ("padded", "packed") if has_packed else ("padded",):
        torch.manual_seed(3407)
        net = DR.MELDLSTMModel(600, 300, 600, n_classes=C_, dropout=DROPOUT).cuda().train()
        kw = {"packed": True} if name == "packed" else {}
        engines[name] = engine.MeldEngine(net, lr=LR, weight_decay=L2, **kw)
        engines[name].reserve(S, B)
    ops.manual_seed(3407)
    out = {"root": os.path.abspath(args.root), "S": S, "B": B, "padded_3_steps_sha16": padded_sha, "real_utterances": int(lengths.sum()), "lengths_min_max": [int(lengths.min()), int(lengths.max())],
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "blocks": {}}
    for train in (True, False):
        steps = {"%s_%s_ms" % (k, "train" if train else "eval"): (lambda e=e: e.step(b, train=train)) for k, e in engines.items()}
        for step in steps.values():
            for _ in range(args.warmup):
                step()
        runs = {k: [] for k in steps}
        for _ in range(args.repeats):
            for k, step in steps.items():
                runs[k].append(round(block(torch, step, args.steps), 4))
        for k, v in runs.items():
            out["blocks"][k] = v
            out[k] = round(statistics.median(v), 4)
            out[k.replace("_ms", "_spread_ms")] = round(max(v) - min(v), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
