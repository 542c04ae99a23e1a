"""Time the two IEMOCAP classifier step runners with and without mask_padding (key lengths in the generators' self-attention:
ganffn_encoder_fwd_len / _bwd_len) and print one JSON line: engine.Phase2Engine on GAN_FFN at (S, B) = (94, 32) and
engine.DrnnEngine on GAN_FFN_DialogueRNN at (94, 30), the batches bench.py times (data.synthetic_batch lengths), the reference
scripts' lr / L2 / dropout.

One process, the same weights at the start and the same batch for both; a warm-up, then `--repeats` rounds in which unmasked and
masked alternate, each a block of `--steps` steps between two device synchronisations.  The JSON carries every block, the medians
and the spread (max - min over the blocks), and `unmasked_3_steps_sha16` per engine: a hash of the generators' parameters and the
log-probabilities after three seeded train steps of the unmasked engine (equal on two trees that compute the same).

    python tools/key_len_time.py [--steps 30] [--warmup 10] [--repeats 5] [--root DIR]

--root DIR imports the package from another checkout (with its own built library), e.g. the parent commit's: a tree without the
`mask_padding` argument is timed on its unmasked step alone.
"""
import argparse
import hashlib
import inspect
import json
import os
import statistics
import sys
import time

S = 94
DIMS = dict(D_m=100, D_g=500, D_p=500, D_e=100, D_h=100, D_a=100)


def block(torch, step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from gan_ffn_amd import data as D, engine, model as M, ops

    def phase2(**kw):
        gens, _ = engine.build_networks(device="cuda", seed=3407)
        net = M.GAN_FFN(gens["acoustic"], gens["visual"], gens["text"], n_classes=6, **kw).cuda().train()
        return engine.Phase2Engine(net, **kw)

    def drnn(**kw):
        torch.manual_seed(3407)
        net = M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), n_classes=6,
                                    listener_state=False, context_attention="general", dropout_rec=0.1, dropout=0.6, **DIMS, **kw)
        return engine.DrnnEngine(net.cuda().train(), **kw)

    out = {"root": os.path.abspath(args.root), "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "blocks": {}}
    for name, make, B in (("phase2", phase2, 32), ("drnn", drnn, 30)):
        b = D.synthetic_batch(B=B, S_max=S, seed=3407, device="cuda")
        lengths = b.pop("lengths")
        if name == "phase2":
            b.pop("qmask")
        out[name + "_shape"] = [int(b["text"].shape[0]), B]
        out[name + "_real_utterances"] = int(lengths.sum())
        has = "mask_padding" in inspect.signature(getattr(engine, "Phase2Engine" if name == "phase2" else "DrnnEngine").__init__).parameters
        ops.manual_seed(3407)
        e0 = make()
        for _ in range(3):
            lp = e0.step(b, train=True)[1]
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for st in e0.G.values():
            h.update(st.slab.cpu().numpy().tobytes())
        h.update(lp.cpu().numpy().tobytes())
        out[name + "_unmasked_3_steps_sha16"] = h.hexdigest()[:16]
        del e0
        engines = {"unmasked": make()}
        if has:
            engines["masked"] = make(mask_padding=True)
        for e in engines.values():
            e.reserve(b["text"].shape[0], B)
        ops.manual_seed(3407)
        for train in (True, False):
            steps = {"%s_%s_%s_ms" % (name, k, "train" if train else "eval"): (lambda e=e: e.step(b, train=train))
                     for k, e in engines.items()}
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
        del engines
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
