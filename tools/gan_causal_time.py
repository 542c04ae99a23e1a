"""What does GanEngine(causal=True) cost, and does the pairing rule hold under it?  Prints one JSON line.

(94, 32) with the lengths of data.synthetic_batch, three streams, eager launches (the product's mode).  Engines in ONE process, each
over its own copy of the same seeded networks and all on the same batch:
    default            GanEngine(gens, discs, n_streams=3)
    causal             ... causal=True, the default pairing rule (the 512-wide generator's forwards paired)
    causal_unpaired    ... causal=True under GANFFN_GEN_PAIR=0
    causal_all_paired  ... causal=True under GANFFN_GEN_PAIR=all
`--warmup` iterations each, then `--repeats` rounds in which the engines alternate, each a block of `--steps` iterations between two
device events on the current stream (the engine's side streams joined before the second).  The JSON carries every block, the medians
and the ranges.

    python tools/gan_causal_time.py [--steps 20] [--warmup 10] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    from gan_ffn_amd import data as D, engine, ops
    S, B = 94, 32
    batch = D.synthetic_batch(B=B, S_max=S, seed=3407, device="cuda")
    batch = {k: batch[k] for k in ("acoustic", "visual", "text", "umask")}
    out = {"shape": [int(batch["text"].shape[0]), B], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "blocks": {}}
    engs = {}
    for name, kw, pair in (("default", {}, None), ("causal", dict(causal=True), None), ("causal_unpaired", dict(causal=True), "0"),
                           ("causal_all_paired", dict(causal=True), "all")):
        os.environ.pop("GANFFN_GEN_PAIR", None)
        if pair is not None:
            os.environ["GANFFN_GEN_PAIR"] = pair           # read when the engine is built
        gens, discs = engine.build_networks(device="cuda", seed=3407)
        engs[name] = engine.GanEngine(gens, discs, n_streams=3, **kw)
        out.setdefault("gen_pair_mode", {})[name] = engs[name].gen_pair_mode
    os.environ.pop("GANFFN_GEN_PAIR", None)
    ops.manual_seed(3407)

    def block(eng, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            eng.iteration(batch)
        eng.synchronize()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    for eng in engs.values():
        block(eng, args.warmup)
    runs = {k: [] for k in engs}
    for _ in range(args.repeats):
        for k, eng in engs.items():
            runs[k].append(round(block(eng, args.steps), 4))
    for k, v in runs.items():
        out["blocks"][k + "_ms"] = v
        out[k + "_ms"] = round(statistics.median(v), 4)
        out[k + "_range_ms"] = [min(v), max(v)]
        out[k + "_losses_finite"] = bool(torch.isfinite(engs[k].losses).all())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
