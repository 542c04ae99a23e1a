"""What does the causal MELD classifier cost, and did anything else move?  Every measurement is a process of its own, started from
here with a time limit of its own; the first one that fails (a non-zero exit status or its time limit) ends the run — nothing is
started after it.  The report goes to standard output (profiles/meld_causal_ab.txt is one run's).

(a) step    engine.MeldEngine train steps at (33, 32) on a seeded batch (600-wide uniform text, ragged prefix masks, 7 classes),
            dropout 0.6, lr 3e-4, L2 1e-4: MELDLSTMModel(600, 300, 300, causal=True) against the default MELDLSTMModel(600, 300, 600) — and, with
            --parent DIR, the default model on the parent commit's tree (its own library and Python).  `--rounds` rounds; in a round
            every side runs once, a fresh process each: `--warmup` steps, then `--blocks` blocks of `--steps` steps between two device
            events; the order of the sides is reversed every round.  Median, min and max over all blocks of a side.
(b) bench   with --parent DIR: `python bench.py --gpus 1 --steps 20 --warmup 5 --config meld` and `--config drnn` on the parent's
            tree and on this one, the same alternation, `--rounds` runs a side; then the default GAN step once a side with
            --dump-outputs, the files compared byte for byte.  The rule (profiles/drnn_stream_ab.txt): a config's median on this
            tree lies within the parent's min - max range, or the two medians differ by less than the larger min - max spread.

    python tools/meld_causal_time.py [--parent DIR] [--rounds 4] [--steps 20] [--warmup 10] [--blocks 3] [--skip-bench]
    python tools/meld_causal_time.py --side causal|default [--root DIR]        (what (a) starts: prints one JSON line)
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, B = 33, 32


def side(args):
    """one side of (a), in this process"""
    sys.path.insert(0, os.path.abspath(args.root) if args.root else HERE)
    import torch
    from gan_ffn_amd import dialogue_rnn as DR, engine as E, ops
    torch.manual_seed(3407)
    if args.side == "causal":
        net = DR.MELDLSTMModel(600, 300, 300, n_classes=7, dropout=0.6, causal=True).cuda().train()
    else:
        net = DR.MELDLSTMModel(600, 300, 600, n_classes=7, dropout=0.6).cuda().train()
    g = torch.Generator().manual_seed(3407)
    lens = torch.randint(2, S + 1, (B,), generator=g)
    lens[0] = S
    umask = (torch.arange(S).unsqueeze(0) < lens.unsqueeze(1)).float()
    b = {"text": (torch.rand(S, B, 600, generator=g) * umask.t().unsqueeze(-1)).contiguous().cuda(), "umask": umask.cuda(),
         "label": torch.randint(0, 7, (B, S), generator=g).cuda()}
    ops.manual_seed(3407)
    eng = E.MeldEngine(net, lr=3e-4, weight_decay=1e-4)

    def timed(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            eng.step(b, train=True)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    timed(args.warmup)
    blocks = [round(timed(args.steps), 4) for _ in range(args.blocks)]
    print(json.dumps({"side": args.side, "shape": [int(b["text"].shape[0]), int(b["text"].shape[1])], "ms_per_step": blocks,
                      "loss_finite": bool(torch.isfinite(eng.loss).all())}), flush=True)


def run(cmd, cwd, limit):
    """one process under its own time limit -> its standard output; anything but a clean exit ends the whole run"""
    try:
        r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit("STOP: %s (in %s) ran into its %d s limit; nothing more is started" % (" ".join(cmd), cwd, limit))
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-3000:])
        sys.exit("STOP: %s (in %s) ended with status %d; nothing more is started" % (" ".join(cmd), cwd, r.returncode))
    return r.stdout


def json_line(text):
    return json.loads([l for l in text.splitlines() if l.startswith("{")][-1])


def row(name, v):
    print("  %-15s %s   median %.3f   range %.3f - %.3f" % (name, " ".join("%.3f" % x for x in v), statistics.median(v), min(v), max(v)),
          flush=True)


def rule(name, parent, new):
    mp, mn = statistics.median(parent), statistics.median(new)
    inside = min(parent) <= mn <= max(parent)
    spread = max(max(parent) - min(parent), max(new) - min(new))
    ok = inside or abs(mn - mp) < spread
    print("  CONDITION %s: this tree's median %.3f %s the parent's range %.3f - %.3f; the medians differ by %.3f ms, the larger spread "
          "is %.3f ms.  %s" % (name, mn, "inside" if inside else "OUTSIDE", min(parent), max(parent), abs(mn - mp), spread,
                               "HOLDS" if ok else "FAILS"), flush=True)
    return ok


def sha_dir(d):
    return {n: hashlib.sha256(open(os.path.join(d, n), "rb").read()).hexdigest() for n in sorted(os.listdir(d))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=["causal", "default"])
    ap.add_argument("--root")
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds every started process may take")
    ap.add_argument("--skip-bench", action="store_true")
    args = ap.parse_args()
    if args.side:
        return side(args)
    parent = os.path.abspath(args.parent) if args.parent else None
    me = os.path.abspath(__file__)
    ok = True

    # ---- (a)
    sides = [("causal", ["--side", "causal"]), ("default", ["--side", "default"])]
    if parent:
        sides.append(("parent default", ["--side", "default", "--root", parent]))
    print("(a) MeldEngine train step at (%d, %d), ms per step: %d rounds, a fresh process per side and round (%d warm-up steps, %d blocks "
          "of %d steps), the order reversed every round" % (S, B, args.rounds, args.warmup, args.blocks, args.steps), flush=True)
    got = {k: [] for k, _ in sides}
    for r in range(args.rounds):
        for k, extra in (sides if r % 2 == 0 else sides[::-1]):
            line = json_line(run([sys.executable, me] + extra + ["--steps", str(args.steps), "--warmup", str(args.warmup), "--blocks",
                                                                 str(args.blocks)], HERE, args.limit))
            assert line["loss_finite"], line
            got[k] += line["ms_per_step"]
    for k, _ in sides:
        row(k, got[k])
    print("  causal / default = %.3f" % (statistics.median(got["causal"]) / statistics.median(got["default"])), flush=True)
    if parent:
        ok = rule("default MeldEngine step", got["parent default"], got["default"]) and ok

    # ---- (b)
    if parent and not args.skip_bench:
        print("(b) python bench.py --gpus 1 --steps 20 --warmup 5 --config C: the parent's tree and this one alternating, %d runs a side, "
              "the order reversed every round (ms_per_step)" % args.rounds, flush=True)
        trees = [("parent", parent), ("this", HERE)]
        for config in ("meld", "drnn"):
            got = {k: [] for k, _ in trees}
            for r in range(args.rounds):
                for k, root in (trees if r % 2 == 0 else trees[::-1]):
                    out = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--config", config], root,
                              args.limit)
                    got[k].append(float(json_line(out)["ms_per_step"]))
            print("  %s" % config)
            for k, _ in trees:
                row("  " + k, got[k])
            ok = rule(config, got["parent"], got["this"]) and ok
        with tempfile.TemporaryDirectory() as tmp:
            dumps = {}
            for k, root in trees:
                d = os.path.join(tmp, k)
                run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", d],
                    root, args.limit)
                dumps[k] = sha_dir(d)
            differ = [n for n in dumps["parent"] if dumps["this"].get(n) != dumps["parent"][n]]
            same_names = sorted(dumps["parent"]) == sorted(dumps["this"])
            print("  --dump-outputs of the default GAN step: %d files a side, %d differ%s" % (len(dumps["parent"]), len(differ),
                  "" if same_names else " (the file lists differ)"), flush=True)
            ok = ok and same_names and not differ
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
