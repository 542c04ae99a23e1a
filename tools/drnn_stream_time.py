"""Time the streaming causal DialogueRNN classifier (GAN_FFN_DialogueRNN(causal=True).stream) against the full-prefix forward and
print one JSON line.

Labels 94-utterance dialogues utterance by utterance at B = 1, 8 and 32 concurrent dialogues, all in one process, the same net and
inputs for every variant:
  (a) prefix   : what a tree without the stream offers — net.eval() under no_grad on the prefix 0 .. t for every t;
  (b) stream   : sess.step;
  (c) no_head  : sess.step without the head's launches (generators, their heads and the sum only): (b) - (c) is the head's share.
One block = one whole pass over the 94 utterances between two device synchronisations; two warm-up rounds, then `--repeats`
rounds in which the variants alternate block by block.  The JSON carries every block, the median and [min, max] of the totals (ms
per 94 utterances), the same for single calls at t = 0, 31, 63, 93 (a device synchronisation before and after the call), and the
condition "the total of (b) at B = 32 is lower than (a) by more than the larger of the two min-max spreads".

--extend: reaching utterance 94 of a dialogue that is already under way, same protocol:
  (a) steps  : sess.reset(), then 94 x sess.step;
  (b) extend : sess.reset(), then sess.extend over the first 93 utterances and sess.step on the 94th.
One block = reset to the label of utterance 94 between two device synchronisations; the condition is the same, at B = 32.

--kernels: the head's recurrence step alone (ganffn_drnn_stream_step: its 7 launches) and the single-query general2 kernel alone
(ganffn_general2_stream_attention) at position 93 with 32 rows, trained widths; device events around `--launches` calls captured
into one graph, microseconds per call.  Run it under a kernel trace for the per-kernel durations of the step's launches.

    python tools/drnn_stream_time.py [--repeats 5] [--root DIR]
    python tools/drnn_stream_time.py --extend [--repeats 5]
    python tools/drnn_stream_time.py --kernels [--launches 200] [--repeats 5]

--root DIR imports the package from another checkout (with its own built library), e.g. the parent commit's: a tree without
`GAN_FFN_DialogueRNN.stream` is timed on (a) alone.
"""
import argparse
import json
import os
import statistics
import sys
import time

S = 94
PROBE_T = (0, 31, 63, 93)
WARMUP_ROUNDS = 2
DIMS = dict(D_m=100, D_g=500, D_p=500, D_e=100, D_h=100, D_a=100)       # the trained widths


def summary(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "spread": round(max(v) - min(v), nd)}


def build_net(torch):
    from gan_ffn_amd import model as M
    torch.manual_seed(3407)
    net = M.GAN_FFN_DialogueRNN(M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100), n_classes=6,
                                listener_state=False, context_attention="general", dropout_rec=0.1, dropout=0.5, causal=True, **DIMS)
    return net.cuda().eval()


def inputs(torch, B):
    g = torch.Generator().manual_seed(B)
    a, v, t = (torch.rand(S, B, w, generator=g).cuda() for w in (100, 512, 100))
    spk = torch.randint(0, 2, (S, B), generator=g)
    qmask = torch.nn.functional.one_hot(spk, 2).float().cuda()
    umask = torch.ones(B, S).cuda()
    return a, v, t, spk.tolist(), qmask, umask


def sessions(args, torch):
    net = build_net(torch)
    has = hasattr(net, "stream")
    out = {"root": os.path.abspath(args.root), "S": S, "repeats": args.repeats, "has_stream": has, "totals_ms": {}, "blocks": {},
           "warmup_blocks": {}, "per_t_ms": {}}
    for B in (1, 8, 32):
        a, v, t, spk, qmask, umask = inputs(torch, B)

        def prefix_call(u):
            return net(a[:u + 1], v[:u + 1], t[:u + 1], qmask[:u + 1], umask[:, :u + 1])[0]

        variants = {"prefix": prefix_call}
        sess = {}
        if has:
            sess["stream"] = net.stream(capacity=B)
            sess["no_head"] = net.stream(capacity=B)
            sess["no_head"]._head_tail = lambda *x, **k: None
            for name in sess:
                variants[name] = (lambda u, s=sess[name]: s.step(a[u], v[u], t[u], spk[u]))

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
        a_, b_ = tm["B32_prefix"], tm["B32_stream"]
        margin = max(a_["spread"], b_["spread"])
        out["condition_B32"] = {"prefix_median_ms": a_["median"], "stream_median_ms": b_["median"], "larger_spread_ms": margin,
                                "holds": bool(a_["median"] - b_["median"] > margin)}
        out["head_share_ms_per_step"] = {"B%d" % B: round((tm["B%d_stream" % B]["median"] - tm["B%d_no_head" % B]["median"]) / S, 4)
                                         for B in (1, 8, 32)}
    return out


def extend(args, torch):
    net = build_net(torch)
    out = {"root": os.path.abspath(args.root), "S": S, "repeats": args.repeats, "totals_ms": {}, "blocks": {}, "warmup_blocks": {},
           "last_label_max_abs_diff": {}}
    for B in (1, 8, 32):
        a, v, t, spk, _, _ = inputs(torch, B)
        sess = net.stream(capacity=B)
        lengths = [S - 1] * B

        def steps():
            for u in range(S):
                lp = sess.step(a[u], v[u], t[u], spk[u])
            return lp

        def chunk():
            sess.extend(a[:S - 1], v[:S - 1], t[:S - 1], spk[:S - 1], lengths)
            return sess.step(a[S - 1], v[S - 1], t[S - 1], spk[S - 1])

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


def kernels(args, torch):
    from gan_ffn_amd import _lib, dialogue_rnn as DR, ops
    out = {"lib": _lib.LIB_PATH, "launches": args.launches, "repeats": args.repeats, "position": S - 1, "rows": 32, "blocks": {}}
    n = cap = 32
    max_len, parties = 110, 2
    Dm, H, He = DIMS["D_m"], DIMS["D_g"], DIMS["D_e"]
    torch.manual_seed(5)
    cell = DR.DialogueRNNCell(Dm, H, H, He, listener_state=False, context_attention="general", D_a=100, dropout=0.1).cuda().eval()
    cfg = ops.drnn_stream_cfg(cap, max_len, parties, Dm, H, He, False, "general")
    n_state, n_ws = ops.drnn_stream_sizes(cfg, n)
    g = torch.Generator().manual_seed(5)
    state = ((torch.rand(n_state, generator=g) - 0.5) * 0.6).cuda()
    ws = torch.empty(n_ws, device="cuda")
    U = (torch.rand(n, Dm, generator=g) - 0.3).cuda()
    slot = torch.arange(n, dtype=torch.int32, device="cuda")
    spk = torch.randint(0, parties, (n,), generator=g).to(torch.int32).cuda()
    pos = torch.full((cap,), S - 1, dtype=torch.int32, device="cuda")
    e_out = torch.empty(n, He, device="cuda")
    ptrs = ops.drnn_stream_cell_ptrs(cell)
    x = (torch.rand(n, He, generator=g) - 0.5).cuda()
    att = torch.empty(n, He, device="cuda")
    e_hist = state[cap * max_len * H + cap * parties * H:]

    def step():       # every call rewrites the same state words (position 93 of every slot) with the same values
        ops.drnn_stream_step_raw(cfg, n, slot, pos, spk, U, ptrs, state, e_out, ws)

    def general2():
        ops.general2_stream_attention_raw(x, e_hist, slot, None, pos, att, None, n, 1, cap, max_len, He)

    for name, launch in (("head_step_7_launches_us", step), ("general2_stream_us", general2)):
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
        out["blocks"][name] = runs[1:]
        out[name] = summary(runs[1:])
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
