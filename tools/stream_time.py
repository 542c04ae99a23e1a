"""Time the streaming causal classifier (GAN_FFN.stream) against the full-prefix forward and print one JSON line.

Labels 94-utterance dialogues utterance by utterance at B = 1, 8 and 32 concurrent dialogues, all in one process, the same weights
and inputs for every variant:
  (a) prefix : what a tree without the stream offers — GAN_FFN(causal=True).eval() under no_grad on the prefix 0 .. t for every t;
  (b) stream : sess.step, eager;
  (c) graph  : sess.step with use_graph=True.
One block = one whole pass over the 94 utterances between two device synchronisations; two warm-up rounds, then `--repeats`
rounds in which the variants alternate block by block.  The JSON carries every block, the median and [min, max] of the totals (ms per 94
utterances), the same for single calls at t = 0, 31, 63, 93 (a device synchronisation before and after the call), and the
condition "the total of (b) or (c) at B = 32 is lower than (a) by more than the larger of the two min-max spreads".

--kernels: the stream attention kernel alone (ganffn_stream_attention) at position 93 with 32 rows, head_dim 10 (E = 100, 10
heads: 320 problems) and head_dim 64 (E = 512, 8 heads: 256 problems); device events around `--launches` launches captured into one
graph, microseconds per launch.

--extend: reaching utterance 94 of a dialogue that is already under way (a session that joins late, or whose caches are stale
after the weights changed), at B = 1, 8 and 32 concurrent dialogues, the same protocol (one process, the same generators and
inputs, two warm-up rounds, the variants alternating block by block):
  (a) steps  : sess.reset(), then 94 x sess.step — all a tree without StreamSession.extend offers;
  (b) extend : sess.reset(), then sess.extend over the first 93 utterances and sess.step on the 94th.
One block = reset to the label of utterance 94 between two device synchronisations.  The JSON carries every block, median and
[min, max], the largest difference between the two variants' log_prob of utterance 94, and the condition "(b) at B = 32 is lower
than (a) by more than the larger of the two min-max spreads".  With --kernels the chunk attention kernel alone
(ganffn_stream_attention_chunk) is timed too: 32 chunks of 94 rows at position 0 and of 47 rows at position 47.

    python tools/stream_time.py [--repeats 5] [--root DIR]
    python tools/stream_time.py --extend [--repeats 5]
    python tools/stream_time.py --kernels [--launches 200] [--repeats 5]

--root DIR imports the package from another checkout (with its own built library), e.g. the parent commit's: a tree without
`GAN_FFN.stream` is timed on (a) alone.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

S = 94
PROBE_T = (0, 31, 63, 93)
WARMUP_ROUNDS = 2


def summary(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "spread": round(max(v) - min(v), nd)}


def sessions(args, torch):
    from gan_ffn_amd import engine, model as M
    gens, _ = engine.build_networks(device="cuda", seed=3407)
    net = M.GAN_FFN(gens["acoustic"], gens["visual"], gens["text"], n_classes=6, causal=True).cuda().eval()
    has = hasattr(net, "stream")
    out = {"root": os.path.abspath(args.root), "S": S, "repeats": args.repeats, "has_stream": has, "totals_ms": {}, "blocks": {},
           "warmup_blocks": {}, "per_t_ms": {}}
    for B in (1, 8, 32):
        g = torch.Generator().manual_seed(B)
        a, v, t = (torch.rand(S, B, w, generator=g).cuda() for w in (100, 512, 100))

        def prefix_call(u):
            return net(a[:u + 1], v[:u + 1], t[:u + 1])[0]

        variants = {"prefix": prefix_call}
        sess = {}
        if has:
            for name, graph in (("stream", False), ("graph", True)):
                sess[name] = net.stream(capacity=B, use_graph=graph)
                variants[name] = (lambda u, s=sess[name]: s.step(a[u], v[u], t[u]))

        def whole(name):
            if name in sess:
                sess[name].reset()
            fn = variants[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for u in range(S):
                fn(u)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def probed(name, acc):
            if name in sess:
                sess[name].reset()
            fn = variants[name]
            for u in range(S):
                if u in PROBE_T:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(u)
                    torch.cuda.synchronize()
                    acc.setdefault(u, []).append((time.perf_counter() - t0) * 1e3)
                else:
                    fn(u)

        with torch.no_grad():
            runs = {k: [] for k in variants}
            # two warm-up rounds: the first allocates and captures the graphs; with one, the first measured (a) block at B = 32
            # took 1 s in two runs (supposed: a capture empties torch's caching allocator and the module path of (a) refills it)
            for r in range(args.repeats + WARMUP_ROUNDS):
                for k in variants:
                    runs[k].append(whole(k))
            per_t = {k: {} for k in variants}
            for r in range(args.repeats):
                for k in variants:
                    probed(k, per_t[k])
        for k, vals in runs.items():
            key = "B%d_%s" % (B, k)
            out["blocks"][key] = [round(x, 3) for x in vals[WARMUP_ROUNDS:]]
            out["warmup_blocks"][key] = [round(x, 3) for x in vals[:WARMUP_ROUNDS]]
            out["totals_ms"][key] = summary(vals[WARMUP_ROUNDS:])
            out["per_t_ms"][key] = {str(u): summary(x, 4) for u, x in per_t[k].items()}
        del sess
    if has:
        tm = out["totals_ms"]
        a_ = tm["B32_prefix"]
        best = min(("stream", "graph"), key=lambda k: tm["B32_" + k]["median"])
        b_ = tm["B32_" + best]
        margin = max(a_["spread"], b_["spread"])
        out["condition_B32"] = {"prefix_median_ms": a_["median"], "best": best, "best_median_ms": b_["median"],
                                "larger_spread_ms": margin, "holds": bool(a_["median"] - b_["median"] > margin)}
    return out


def extend(args, torch):
    from gan_ffn_amd import engine, model as M
    gens, _ = engine.build_networks(device="cuda", seed=3407)
    net = M.GAN_FFN(gens["acoustic"], gens["visual"], gens["text"], n_classes=6, causal=True).cuda().eval()
    out = {"root": os.path.abspath(args.root), "S": S, "repeats": args.repeats, "totals_ms": {}, "blocks": {}, "warmup_blocks": {},
           "last_label_max_abs_diff": {}}
    for B in (1, 8, 32):
        g = torch.Generator().manual_seed(B)
        a, v, t = (torch.rand(S, B, w, generator=g).cuda() for w in (100, 512, 100))
        sess = net.stream(capacity=B)
        lengths = [S - 1] * B

        def steps():
            for u in range(S):
                lp = sess.step(a[u], v[u], t[u])
            return lp

        def chunk():
            sess.extend(a[:S - 1], v[:S - 1], t[:S - 1], lengths)
            return sess.step(a[S - 1], v[S - 1], t[S - 1])

        variants = {"steps": steps, "extend": chunk}

        def whole(name):
            sess.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lp = variants[name]()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, lp.clone()

        runs = {k: [] for k in variants}
        last = {}
        for r in range(args.repeats + WARMUP_ROUNDS):
            for k in variants:
                ms, last[k] = whole(k)
                runs[k].append(ms)
        out["last_label_max_abs_diff"]["B%d" % B] = float((last["steps"] - last["extend"]).abs().max())
        for k, vals in runs.items():
            key = "B%d_%s" % (B, k)
            out["blocks"][key] = [round(x, 3) for x in vals[WARMUP_ROUNDS:]]
            out["warmup_blocks"][key] = [round(x, 3) for x in vals[:WARMUP_ROUNDS]]
            out["totals_ms"][key] = summary(vals[WARMUP_ROUNDS:])
        del sess
    a_, b_ = out["totals_ms"]["B32_steps"], out["totals_ms"]["B32_extend"]
    margin = max(a_["spread"], b_["spread"])
    out["condition_B32"] = {"steps_median_ms": a_["median"], "extend_median_ms": b_["median"], "larger_spread_ms": margin,
                            "holds": bool(a_["median"] - b_["median"] > margin)}
    return out


def chunk_kernels(args, torch, out):
    """the chunk attention kernel alone: 32 chunks, (count, pos) = (94, 0) and (47, 47), head_dim 10 and 64"""
    from gan_ffn_amd import _lib
    p = lambda x: C.c_void_p(x.data_ptr())
    n = cap = 32
    max_len = 110
    for name, E, H in (("hd10", 100, 10), ("hd64", 512, 8)):
        for count, at in ((S, 0), (S // 2, S // 2)):
            g = torch.Generator().manual_seed(5)
            qkv = (torch.randn(count, n, 3 * E, generator=g) * 1.5).cuda()
            cache = torch.randn(cap * 2 * max_len * E, generator=g).cuda()
            slot = torch.arange(n, dtype=torch.int32, device="cuda")
            cnt = torch.full((n,), count, dtype=torch.int32, device="cuda")
            pos = torch.full((cap,), at, dtype=torch.int32, device="cuda")
            o = torch.empty(count, n, E, device="cuda")

            def launch():
                _lib.call("ganffn_stream_attention_chunk", p(qkv), p(cache), p(slot), p(cnt), p(pos), p(o), n, count, cap, max_len, E,
                          H, C.c_void_p(torch.cuda.current_stream().cuda_stream))

            launch()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(args.launches):
                    launch()
            runs = []
            for _ in range(args.repeats + 1):             # the first round is the warm-up
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph.replay()
                e1.record()
                torch.cuda.synchronize()
                runs.append(round(e0.elapsed_time(e1) * 1e3 / args.launches, 3))
            key = "chunk_%s_count%d_pos%d_us" % (name, count, at)
            out["blocks"][key] = runs[1:]
            out[key] = summary(runs[1:])


def kernels(args, torch):
    from gan_ffn_amd import _lib
    _lib.load()
    p = lambda x: C.c_void_p(x.data_ptr())
    out = {"lib": _lib.LIB_PATH, "launches": args.launches, "repeats": args.repeats, "position": S - 1, "rows": 32, "blocks": {}}
    n = cap = 32
    max_len = 110
    for name, E, H in (("hd10", 100, 10), ("hd64", 512, 8)):
        g = torch.Generator().manual_seed(5)
        qkv = (torch.randn(n, 3 * E, generator=g) * 1.5).cuda()
        cache = torch.randn(cap * 2 * max_len * E, generator=g).cuda()
        slot = torch.arange(n, dtype=torch.int32, device="cuda")
        pos = torch.full((cap,), S - 1, dtype=torch.int32, device="cuda")
        o = torch.empty(n, E, device="cuda")

        def launch():
            _lib.call("ganffn_stream_attention", p(qkv), p(cache), p(slot), p(pos), p(o), n, cap, max_len, E, H,
                      C.c_void_p(torch.cuda.current_stream().cuda_stream))

        # the launches of a block are one captured graph (a chain on one stream), so that the host's launch rate is not what the
        # events see; every launch rewrites the same cache position with the same values
        launch()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.launches):
                launch()
        runs = []
        for _ in range(args.repeats + 1):             # the first round is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            runs.append(round(e0.elapsed_time(e1) * 1e3 / args.launches, 3))
        out["blocks"][name + "_us"] = runs[1:]
        out[name + "_us"] = summary(runs[1:])
        out[name + "_problems"] = n * H
    if hasattr(_lib.load(), "ganffn_stream_attention_chunk"):
        chunk_kernels(args, torch, out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--extend", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    print(json.dumps((kernels if args.kernels else extend if args.extend else sessions)(args, torch)), flush=True)


if __name__ == "__main__":
    main()
