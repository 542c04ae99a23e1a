"""Time the listener-state DialogueRNN (listener_state = True; train_IEMOCAP_DialogueRNN.py --active-listener) at configuration
5's size (94 utterances, 30 dialogues) and print one JSON line.  All numbers come from the same process and the same batch:

  engine_listener_ms   engine.DrnnEngine train step of a listener GAN_FFN_DialogueRNN (the HIP listener recurrence)
  engine_ms            the same step without the listener (the configuration bench.py --config drnn measures)
  module_torch_ms      the module path (autograd + torch.optim.Adam) of the listener network with the recurrence forced onto the
                       per-step torch ops: ops.dialogue_rnn_listener_supported is monkeypatched to refuse, here only

    python tools/drnn_listener_time.py [--steps 20] [--warmup 60] [--torch-steps 3] [--listener-only]

--listener-only times the listener engine step alone (for a kernel trace of that step: rocprofv3 ... -- python ...).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

W = [1.2, 0.60072, 0.38066, 0.94019, 0.67924, 0.34332]          # train_IEMOCAP_DialogueRNN.py:738


def make_net(listener):
    from gan_ffn_amd import model as M
    torch.manual_seed(3407)
    return M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), 100, 500, 500, 100, 100,
                                 100, n_classes=6, listener_state=listener, context_attention="general", dropout_rec=0.1,
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


def engine_ms(listener, batch, warmup, steps):
    from gan_ffn_amd import engine
    eng = engine.DrnnEngine(make_net(listener), lr=1e-4, weight_decay=1e-5)
    return timed(lambda: eng.step(batch, train=True), warmup, steps)


def module_torch_ms(batch, warmup, steps):
    from gan_ffn_amd import model as M, ops
    net = make_net(True)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=1e-5)
    loss_fn = M.MaskedNLLLoss(torch.tensor(W, device="cuda"))

    def step():
        opt.zero_grad()
        lp = net(batch["acoustic"], batch["visual"], batch["text"], batch["qmask"], batch["umask"])[0]
        loss = loss_fn(lp.transpose(0, 1).contiguous().view(-1, 6), batch["label"].view(-1), batch["umask"])
        loss.backward()
        opt.step()
    keep = ops.dialogue_rnn_listener_supported
    ops.dialogue_rnn_listener_supported = lambda *a, **k: False
    try:
        return timed(step, warmup, steps)
    finally:
        ops.dialogue_rnn_listener_supported = keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--listener-only", action="store_true")
    args = ap.parse_args()
    from gan_ffn_amd import data as D, ops
    ops.manual_seed(3407)
    batch = D.synthetic_batch(B=30, S_max=94, seed=3407, device="cuda")
    S, B = batch["text"].shape[:2]
    ms_l = engine_ms(True, batch, args.warmup, args.steps)
    if args.listener_only:
        print(json.dumps({"S": S, "B": B, "engine_listener_ms": round(ms_l, 3), "steps": args.steps}), flush=True)
        return
    ms_0 = engine_ms(False, batch, args.warmup, args.steps)
    ms_t = module_torch_ms(batch, 1, args.torch_steps)
    print(json.dumps({"S": S, "B": B, "engine_listener_ms": round(ms_l, 3), "engine_ms": round(ms_0, 3),
                      "module_torch_ms": round(ms_t, 2), "listener_over_plain": round(ms_l / ms_0, 3),
                      "torch_over_listener": round(ms_t / ms_l, 1), "steps": args.steps, "torch_steps": args.torch_steps}),
          flush=True)


if __name__ == "__main__":
    main()
