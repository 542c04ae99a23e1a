"""Time the multi-party DialogueRNN and print one JSON line.  All numbers come from the same process:

  module_hip_ms / module_torch_ms  the module path — BiModel (general attention, no listener state) forward + backward +
                                   torch.optim.Adam under autograd — at (S, B, P) = (33, 32, 9) with MELD's text width
                                   (D_m = 600, D_g = D_p = 500, D_e = D_h = 100, 7 classes), the recurrence on HIP, then
                                   forced onto the per-step torch ops (ops.dialogue_rnn_supported monkeypatched to refuse,
                                   here only)
  engine_ms[P][listener]           engine.DrnnEngine train step of a GAN_FFN_DialogueRNN at (94, 30) on the same batch with
                                   P = 2 and P = 9 one-hot speakers, listener state off and on

    python tools/drnn_parties_time.py [--steps 20] [--warmup 60] [--torch-steps 3] [--only-engine P]

--only-engine P times the listener-free engine step at P parties alone (for a kernel trace: rocprofv3 ... -- python ...).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

W = [1.2, 0.60072, 0.38066, 0.94019, 0.67924, 0.34332]          # train_IEMOCAP_DialogueRNN.py:738


def timed(step, warmup, steps):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def party_batch(P, seed=3407):
    from gan_ffn_amd import data as D
    b = D.synthetic_batch(B=30, S_max=94, seed=seed, device="cuda")
    S, B = b["text"].shape[:2]
    spk = torch.randint(0, P, (S, B), generator=torch.Generator().manual_seed(seed))
    b["qmask"] = torch.nn.functional.one_hot(spk, P).float().cuda() * b["umask"].t().unsqueeze(2)
    return b


def engine_ms(P, listener, warmup, steps):
    from gan_ffn_amd import engine, model as M
    torch.manual_seed(3407)
    net = M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), 100, 500, 500, 100, 100,
                                100, n_classes=6, listener_state=listener, context_attention="general", dropout_rec=0.1,
                                dropout=0.6).cuda().train()
    eng = engine.DrnnEngine(net, lr=1e-4, weight_decay=1e-5)
    batch = party_batch(P)
    return timed(lambda: eng.step(batch, train=True), warmup, steps)


def module_ms(warmup, steps, torch_ops):
    from gan_ffn_amd import dialogue_rnn as DR, model as M, ops
    torch.manual_seed(3407)
    S, B, P = 33, 32, 9
    net = DR.BiModel(600, 500, 500, 100, 100, n_classes=7, context_attention="general", listener_state=False, dropout_rec=0.1,
                     dropout=0.5).cuda().train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=1e-5)
    loss_fn = M.MaskedNLLLoss()
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(5, S + 1, (B,), generator=g)
    lens[0] = S
    umask = (torch.arange(S).unsqueeze(0) < lens.unsqueeze(1)).float()
    U = (torch.rand(S, B, 600, generator=g) * umask.t().unsqueeze(2)).cuda()
    qmask = (torch.nn.functional.one_hot(torch.randint(0, P, (S, B), generator=g), P).float() * umask.t().unsqueeze(2)).cuda()
    label = (torch.randint(0, 7, (B, S), generator=g) * umask.long()).cuda()
    umask = umask.cuda()

    def step():
        opt.zero_grad()
        lp = net(U, qmask, umask)[0]
        loss = loss_fn(lp.transpose(0, 1).contiguous().view(-1, 7), label.view(-1), umask)
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
    ap.add_argument("--only-engine", type=int, default=None)
    args = ap.parse_args()
    from gan_ffn_amd import ops
    ops.manual_seed(3407)
    if args.only_engine:
        ms = engine_ms(args.only_engine, False, args.warmup, args.steps)
        print(json.dumps({"S": 94, "B": 30, "P": args.only_engine, "engine_ms": round(ms, 3), "steps": args.steps}), flush=True)
        return
    eng = {str(P): {("listener" if lis else "no_listener"): round(engine_ms(P, lis, args.warmup, args.steps), 3)
                    for lis in (False, True)} for P in (2, 9)}
    hip = round(module_ms(10, args.steps, False), 3)
    tor = round(module_ms(1, args.torch_steps, True), 2)
    print(json.dumps({"engine_S_B": [94, 30], "engine_ms": eng,
                      "engine_p9_over_p2": {k: round(eng["9"][k] / eng["2"][k], 3) for k in eng["2"]},
                      "module_S_B_P": [33, 32, 9], "module_hip_ms": hip, "module_torch_ms": tor,
                      "torch_over_hip": round(tor / hip, 1), "steps": args.steps, "torch_steps": args.torch_steps}), flush=True)


if __name__ == "__main__":
    main()
