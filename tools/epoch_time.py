"""Time whole training epochs with the host loader against the device-resident corpus (the table of
profiles/device_corpus_epoch_ab.txt).

rows     meld     MeldEngine on MELDLSTMModel(600, 300, 600, 7 classes): about 1 000 train dialogues of 1..33 utterances, batch 32
         phase2   Phase2Engine on GAN_FFN: 120 train dialogues of 8..110 utterances, batch 32
         drnn     DrnnEngine on GAN_FFN_DialogueRNN (configuration 5): the same corpus, batch 30
         gan      engine.train_GAN (one epoch per call, no log): the same corpus, batch 32
columns  host     the loaders of data.get_*_loaders: collate on the host, six copies to the device and four reads back per batch
                  (artifacts.train_or_eval_model's host path, artifacts._DeviceBatches for train_GAN) — the code as it was before
                  the device path existed
         device   data.DeviceLoader over data.DeviceCorpus: one gather launch and one record launch per batch, one read per epoch
Both columns run in this process on seeded synthetic pickles of the corpora's real sizes, each on its own identically seeded
model; they alternate epoch by epoch: `--warmup` epochs each, then `--epochs` timed ones.  An epoch is timed with the host
clock, from before the loader is asked for its first batch to after a device synchronise behind the last step.  Per cell: the
median and the min - max spread.  "faster" is only said where the device median lies below the host median by more than the
host column's own spread.

    python tools/epoch_time.py [--rows meld,phase2,drnn,gan] [--epochs 7] [--warmup 2] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_row(row, pickles):
    """-> {"host": epoch function, "device": epoch function}, batches per epoch, utterances per epoch"""
    import torch
    from gan_ffn_amd import artifacts as A, data as D, dialogue_rnn as DR, engine as E, model as M, ops
    fns = {}
    for side in ("host", "device"):
        torch.manual_seed(3407)
        ops.manual_seed(3407)
        if row == "meld":
            bs, sets = 32, (D.MELDDataset(pickles["meld"], "emotion", True), D.MELDDataset(pickles["meld"], "emotion", False))
            host_loaders, to_batch = lambda: D.get_MELD_loaders(pickles["meld"], batch_size=bs, valid=0.0), D.to_meld_batch
            eng = E.MeldEngine(DR.MELDLSTMModel(600, 300, 600, n_classes=7, dropout=0.6).cuda())
            eng.reserve(33, bs)
        else:
            bs = 30 if row == "drnn" else 32
            sets = (D.IEMOCAPDataset(pickles["iemocap"], True), D.IEMOCAPDataset(pickles["iemocap"], False))
            host_loaders, to_batch = lambda: D.get_IEMOCAP_loaders(pickles["iemocap"], batch_size=bs, valid=0.0), D.to_batch
            gens = [M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100)]
            if row == "phase2":
                eng = E.Phase2Engine(M.GAN_FFN(*gens, n_classes=6).cuda(), lr=1e-4, weight_decay=0.008)
                eng.reserve(110, bs)
            elif row == "drnn":
                eng = E.DrnnEngine(M.GAN_FFN_DialogueRNN(*gens, 100, 500, 500, 100, 100, 100, n_classes=6, listener_state=False,
                                                         context_attention="general", dropout_rec=0.1, dropout=0.6).cuda(),
                                   lr=1e-4, weight_decay=1e-5)
                eng.reserve(110, bs)
            else:
                gens, discs = E.build_networks(100, 0.2, "cuda", 3407)
        loader = D.get_device_loaders(sets[0], sets[1], bs, 0.0, "cuda")[0] if side == "device" else host_loaders()[0]
        if row == "gan":
            batches = loader if side == "device" else A._DeviceBatches(loader, "cuda")
            fns[side] = lambda gens=gens, discs=discs, batches=batches: E.train_GAN(gens, discs, batches, epochs=1, reserve_S=110)
        else:
            fns[side] = lambda eng=eng, loader=loader, to_batch=to_batch: A.train_or_eval_model(eng, loader, True, "cuda", to_batch)
    n_utt = sum(len(sets[0].videoLabels[k]) for k in sets[0].keys)
    return fns, (len(sets[0]) + bs - 1) // bs, n_utt


def time_row(fns, epochs, warmup):
    import torch
    s = {k: [] for k in fns}
    for i in range(warmup + epochs):
        for k, f in fns.items():                 # host, device, host, device, ...
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if i >= warmup:
                s[k].append(time.perf_counter() - t0)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in s.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="meld,phase2,drnn,gan")
    ap.add_argument("--epochs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert args.epochs >= 5 and args.warmup >= 2, "the median of at least 5 epochs after at least 2 warm-up epochs"
    import torch
    from gan_ffn_amd import data as D
    lines = ["whole training epochs, host loader against device-resident corpus (tools/epoch_time.py): %s, %d timed epochs per cell "
             "after %d warm-up epochs, the two columns alternating; seconds per epoch, host clock around an epoch ending in a "
             "device synchronise" % (torch.cuda.get_device_name(0), args.epochs, args.warmup),
             "%-7s %7s %10s | %9s %19s | %9s %19s | %11s  %s" % ("row", "batches", "utterances", "host med", "host min - max",
                                                                "dev med", "dev min - max", "host / dev", "verdict")]
    with tempfile.TemporaryDirectory() as tmp:
        pickles = {"meld": os.path.join(tmp, "meld.pkl"), "iemocap": os.path.join(tmp, "iemocap.pkl")}
        D.write_synthetic_meld_pickle(pickles["meld"], n_train=1000, n_test=4, seed=3407, lo=1, hi=33)
        D.write_synthetic_iemocap_pickle(pickles["iemocap"], n_train=120, n_test=4, seed=3407, lo=8, hi=110)
        for row in args.rows.split(","):
            fns, n_batches, n_utt = make_row(row, pickles)
            r = time_row(fns, args.epochs, args.warmup)
            (hm, hlo, hhi), (dm, dlo, dhi) = r["host"], r["device"]
            verdict = "device faster" if dm < hm - (hhi - hlo) else "host faster" if hm < dm - (dhi - dlo) else "no difference beyond the spread"
            lines.append("%-7s %7d %10d | %9.4f %8.4f - %8.4f | %9.4f %8.4f - %8.4f | %11.3f  %s"
                         % (row, n_batches, n_utt, hm, hlo, hhi, dm, dlo, dhi, hm / dm, verdict))
            print(lines[-1], file=sys.stderr, flush=True)
            del fns
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
