"""Time causal self-attention (GANFFN_ATTN_CAUSAL) and print one JSON line.

Default: engine.Phase2Engine on GAN_FFN at (S, B) = (94, 32), the batch bench.py times (data.synthetic_batch lengths), the reference
script's lr / L2 / dropout, with `causal` off and on.  One process, the same weights at the start and the same batch for both; a
warm-up, then `--repeats` rounds in which the variants alternate, each a block of `--steps` steps between two device
synchronisations.  The JSON carries every block, the medians and the spread (max - min over the blocks), and
`causal_off_3_steps_sha16`: a hash of the generators' parameters and the log-probabilities after three seeded train steps of the
engine with causal off (equal on two trees that compute the same).

--kernels: the attention pair alone at S = 94, B = 32, train mode with p = 0.1, head_dim 10 (E = 100, 10 heads: 320 problems, the
16-row kernels) and head_dim 64 (E = 512, 8 heads: 256 problems, the 32-row kernels), through ganffn_attention_fwd_len / _bwd_len
with lengths S and through ganffn_attention_fwd_mask / _bwd_mask with GANFFN_ATTN_CAUSAL; device events around blocks of
`--launches` launches, forms alternating, microseconds per launch.  Run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel times, and with GANFFN_LIB=<a library built with -DGANFFN_CAUSAL_MASK_ONLY> for the causal kernels without tile
skipping.

    python tools/causal_time.py [--steps 30] [--warmup 10] [--repeats 5] [--root DIR]
    python tools/causal_time.py --kernels [--launches 200] [--repeats 5]

--root DIR imports the package from another checkout (with its own built library), e.g. the parent commit's: a tree without the
`causal` argument is timed on its bidirectional step alone.
"""
import argparse
import ctypes as C
import hashlib
import inspect
import json
import os
import statistics
import sys
import time

S = 94


def block(torch, step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def engines(args, torch):
    from gan_ffn_amd import data as D, engine, model as M, ops

    def phase2(**kw):
        gens, _ = engine.build_networks(device="cuda", seed=3407)
        net = M.GAN_FFN(gens["acoustic"], gens["visual"], gens["text"], n_classes=6, **kw).cuda().train()
        return engine.Phase2Engine(net, **kw)

    B = 32
    out = {"root": os.path.abspath(args.root), "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "blocks": {}}
    b = D.synthetic_batch(B=B, S_max=S, seed=3407, device="cuda")
    b.pop("lengths")
    b.pop("qmask")
    out["shape"] = [int(b["text"].shape[0]), B]
    has = "causal" in inspect.signature(engine.Phase2Engine.__init__).parameters
    ops.manual_seed(3407)
    e0 = phase2()
    for _ in range(3):
        lp = e0.step(b, train=True)[1]
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for st in e0.G.values():
        h.update(st.slab.cpu().numpy().tobytes())
    h.update(lp.cpu().numpy().tobytes())
    out["causal_off_3_steps_sha16"] = h.hexdigest()[:16]
    del e0
    engs = {"off": phase2()}
    if has:
        engs["on"] = phase2(causal=True)
    for e in engs.values():
        e.reserve(b["text"].shape[0], B)
    ops.manual_seed(3407)
    for train in (True, False):
        steps = {"phase2_causal_%s_%s_ms" % (k, "train" if train else "eval"): (lambda e=e: e.step(b, train=train))
                 for k, e in engs.items()}
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
    return out


def kernels(args, torch):
    from gan_ffn_amd import _lib
    lib = _lib.load()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"lib": _lib.LIB_PATH, "launches": args.launches, "repeats": args.repeats, "S": S, "B": 32, "blocks": {}}
    for name, E, H in (("hd10", 100, 10), ("hd64", 512, 8)):
        B = 32
        g = torch.Generator().manual_seed(5)
        qkv = (torch.randn(S, B, 3 * E, generator=g) * 1.5).cuda()
        do = torch.randn(S, B, E, generator=g).cuda()
        o, lse, dq = torch.empty(S, B, E, device="cuda"), torch.empty(B * H, S, device="cuda"), torch.empty(S, B, 3 * E, device="cuda")
        keep = torch.zeros(int(lib.ganffn_attention_keep_words(B, H)), dtype=torch.int32, device="cuda")
        kl = torch.full((B,), S, dtype=torch.int32, device="cuda")
        rng = torch.tensor([777, 11], dtype=torch.int64, device="cuda")
        tail = (S, B, E, H, C.c_float(0.1), C.c_uint32(3), p(rng), C.c_uint64(4), None)

        def fwd(flags):
            fl = () if flags is None else (C.c_uint32(flags),)
            args_ = (p(qkv), p(o), p(lse), p(keep), p(kl)) + fl + tail[:-1] + (st(),)
            _lib.call("ganffn_attention_fwd_" + ("len" if flags is None else "mask"), *args_)

        def bwd(flags):
            fl = () if flags is None else (C.c_uint32(flags),)
            args_ = (p(qkv), p(o), p(lse), p(do), p(keep), p(kl)) + fl + (p(dq),) + tail[:-1] + (st(),)
            _lib.call("ganffn_attention_bwd_" + ("len" if flags is None else "mask"), *args_)

        forms = {"len": None, "causal": 1}
        runs = {}
        for _ in range(args.repeats + 1):             # the first round is the warm-up
            for form, flags in forms.items():
                fwd(flags)                              # the backward's o, lse and keep words are this form's
                for which, fn in (("fwd", fwd), ("bwd", bwd)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.launches):
                        fn(flags)
                    e1.record()
                    torch.cuda.synchronize()
                    runs.setdefault("%s_%s_%s_us" % (name, which, form), []).append(round(e0.elapsed_time(e1) * 1e3 / args.launches, 3))
        for k, v in runs.items():
            v = v[1:]
            out["blocks"][k] = v
            out[k] = round(statistics.median(v), 3)
            out[k.replace("_us", "_spread_us")] = round(max(v) - min(v), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    print(json.dumps((kernels if args.kernels else engines)(args, torch)), flush=True)


if __name__ == "__main__":
    main()
