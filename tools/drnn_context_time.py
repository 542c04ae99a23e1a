"""Time the DialogueRNN context attention types (train_IEMOCAP_DialogueRNN.py --attention, :586) at configuration 5's size
(94 utterances, 30 dialogues) and print one JSON line.  All numbers come from the same process and the same batch:

  engine_ms[att]       engine.DrnnEngine train step of a GAN_FFN_DialogueRNN with context attention `att` (general, simple,
                       dot, general2, concat; dot at D_g = D_p = D_m = 100 — the reference asserts D_m == D_g — the others at
                       D_g = D_p = 500, D_a = 100)
  module_hip_ms[att]   the module path (autograd + torch.optim.Adam) with the recurrence on HIP, for concat and general2
  module_torch_ms[att] the same with the recurrence forced onto the per-step torch ops (ops.dialogue_rnn_supported is
                       monkeypatched to refuse, here only)

    python tools/drnn_context_time.py [--steps 20] [--warmup 60] [--torch-steps 3] [--only concat]

--only ATT times that engine step alone (for a kernel trace of it: rocprofv3 ... -- python ...).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

W = [1.2, 0.60072, 0.38066, 0.94019, 0.67924, 0.34332]          # train_IEMOCAP_DialogueRNN.py:738
TYPES = ["general", "simple", "dot", "general2", "concat"]


def make_net(att):
    from gan_ffn_amd import model as M
    torch.manual_seed(3407)
    H = 100 if att == "dot" else 500
    return M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), 100, H, H, 100, 100,
                                 100, n_classes=6, listener_state=False, context_attention=att, dropout_rec=0.1,
                                 dropout=0.6).cuda().train()


def timed(step, warmup, steps):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def engine_ms(att, batch, warmup, steps):
    from gan_ffn_amd import engine
    eng = engine.DrnnEngine(make_net(att), lr=1e-4, weight_decay=1e-5)
    return timed(lambda: eng.step(batch, train=True), warmup, steps)


def module_ms(att, batch, warmup, steps, torch_ops):
    from gan_ffn_amd import model as M, ops
    net = make_net(att)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=1e-5)
    loss_fn = M.MaskedNLLLoss(torch.tensor(W, device="cuda"))

    def step():
        opt.zero_grad()
        lp = net(batch["acoustic"], batch["visual"], batch["text"], batch["qmask"], batch["umask"])[0]
        loss = loss_fn(lp.transpose(0, 1).contiguous().view(-1, 6), batch["label"].view(-1), batch["umask"])
        loss.backward()
        opt.step()
    keep = ops.dialogue_rnn_supported
    if torch_ops:
        ops.dialogue_rnn_supported = lambda *a, **k: False
    try:
        return timed(step, warmup, steps)
    finally:
        ops.dialogue_rnn_supported = keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--only", choices=TYPES)
    args = ap.parse_args()
    from gan_ffn_amd import data as D, ops
    ops.manual_seed(3407)
    batch = D.synthetic_batch(B=30, S_max=94, seed=3407, device="cuda")
    S, B = batch["text"].shape[:2]
    if args.only:
        ms = engine_ms(args.only, batch, args.warmup, args.steps)
        print(json.dumps({"S": S, "B": B, "att": args.only, "engine_ms": round(ms, 3), "steps": args.steps}), flush=True)
        return
    eng = {att: round(engine_ms(att, batch, args.warmup, args.steps), 3) for att in TYPES}
    hip, tor = {}, {}
    for att in ("concat", "general2"):
        hip[att] = round(module_ms(att, batch, 10, args.steps, False), 3)
        tor[att] = round(module_ms(att, batch, 1, args.torch_steps, True), 2)
    print(json.dumps({"S": S, "B": B, "engine_ms": eng,
                      "engine_over_general": {a: round(eng[a] / eng["general"], 3) for a in TYPES},
                      "module_hip_ms": hip, "module_torch_ms": tor,
                      "torch_over_hip": {a: round(tor[a] / hip[a], 1) for a in hip},
                      "steps": args.steps, "torch_steps": args.torch_steps}), flush=True)


if __name__ == "__main__":
    main()
