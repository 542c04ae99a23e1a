"""What does the causal DialogueRNN classifier cost?  Prints one JSON line with two measurements, both in ONE process.

general2   the general2 matching attention alone at (94, 30, D) for D = 100 (UniModel's width) and D = 200 (BiModel's), forward
           (ganffn_general2_attention_fwd_mask) and backward (_bwd_mask), flags = 0 against GANFFN_ATTN_CAUSAL on the same
           inputs: blocks of `--calls` calls between two device events, the two variants alternating, `--repeats` blocks each.
step       DrnnEngine at (94, 30) with the lengths of data.synthetic_batch, one stream, eager launches (what `bench.py --config
           drnn` times): an engine on the default net and one on GAN_FFN_DialogueRNN(causal=True), same seed, same batch,
           `--warmup` steps each, then `--repeats` rounds in which the two alternate, each a block of `--steps` steps between two
           device events.  The JSON carries every block, the medians and the ranges.

    python tools/drnn_causal_time.py [--steps 20] [--warmup 60] [--repeats 5] [--calls 200]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    import torch
    from gan_ffn_amd import _lib, data as D, engine, model as M, ops
    S, B = 94, 30
    out = {"shape": [S, B], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "calls": args.calls}

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def summary(dst, key, v):
        dst[key] = {"blocks": v, "median": round(statistics.median(v), 4), "range": [min(v), max(v)]}

    # ---- general2 alone
    P, g = ops._ptr, torch.Generator().manual_seed(3407)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S).unsqueeze(0) < lens.unsqueeze(1)).float().cuda()
    out["general2_us"] = {}
    for Dw in (100, 200):
        mem = (torch.rand(S, B, Dw, generator=g) - 0.5).cuda()
        x = ((torch.rand(S, B, Dw, generator=g) - 0.5) * 0.7).cuda()
        gy = (torch.rand(S, B, Dw, generator=g) - 0.5).cuda()
        att, dx, dm = (torch.empty_like(mem) for _ in range(3))
        alpha, ts, du = (torch.empty(B, S, S, device="cuda") for _ in range(3))

        def fwd(flags):
            _lib.call("ganffn_general2_attention_fwd_mask", P(x), P(mem), P(mask), C.c_uint32(flags), P(att), P(alpha), P(ts), S, B,
                      Dw, ops._stream())

        def bwd(flags):
            _lib.call("ganffn_general2_attention_bwd_mask", P(gy), P(x), P(mem), P(mask), C.c_uint32(flags), P(alpha), P(ts), P(du),
                      P(dx), P(dm), S, B, Dw, ops._stream())
        res = out["general2_us"]["D%d" % Dw] = {}
        for what, fn in (("fwd", fwd), ("bwd", bwd)):
            runs = {0: [], ops.ATTN_CAUSAL: []}
            for flags in runs:
                fwd(flags)                                # the backward reads the forward's alpha and tanh_s of the same flags
                timed(lambda: fn(flags), args.calls)
            for _ in range(args.repeats):
                for flags in runs:
                    fwd(flags)
                    runs[flags].append(round(1e3 * timed(lambda: fn(flags), args.calls), 3))
            summary(res, what + "_default", runs[0])
            summary(res, what + "_causal", runs[ops.ATTN_CAUSAL])

    # ---- the DrnnEngine step
    batch = D.synthetic_batch(B=B, S_max=S, seed=3407, device="cuda")
    out["step_shape"] = [int(batch["text"].shape[0]), int(batch["text"].shape[1])]
    engs = {}
    for name, kw in (("default", {}), ("causal", dict(causal=True))):
        torch.manual_seed(3407)
        net = M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), 100, 500, 500, 100, 100,
                                    100, n_classes=6, listener_state=False, context_attention="general", dropout_rec=0.1,
                                    dropout=0.6, **kw).cuda().train()
        engs[name] = engine.DrnnEngine(net, lr=1e-4, weight_decay=1e-5)
    ops.manual_seed(3407)
    for eng in engs.values():
        timed(lambda: eng.step(batch, train=True), args.warmup)
    runs = {k: [] for k in engs}
    for _ in range(args.repeats):
        for k, eng in engs.items():
            runs[k].append(round(timed(lambda: eng.step(batch, train=True), args.steps), 4))
    out["step_ms"] = {}
    for k, v in runs.items():
        summary(out["step_ms"], k, v)
        out["step_ms"][k]["loss_finite"] = bool(torch.isfinite(engs[k].loss).all())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
