"""The corpus on the GPU (data.DeviceCorpus / data.DeviceLoader, csrc/batch.hip): gathered batches equal the host collate bit
for bit, the record kernel equals engine.predictions, and whole epochs through artifacts.train_or_eval_model / engine.train_GAN
give the host loaders' results exactly — with a number of device-to-host reads that does not grow with the batches."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ------------------------------------------------------------------------------------------------
# corpora
# ------------------------------------------------------------------------------------------------
class Tiny(torch.utils.data.Dataset):
    """IEMOCAP's item layout with widths (6, 10, 3) and 3 speakers: no width is a multiple of 4 — the scalar path alone"""
    LENGTHS = [1, 4, 2, 7, 3, 1, 5, 2]

    def __init__(self):
        g = torch.Generator().manual_seed(5)
        self.keys = ["t%d" % i for i in range(len(self.LENGTHS))]
        self.items = []
        for k, L in zip(self.keys, self.LENGTHS):
            spk = torch.nn.functional.one_hot(torch.randint(0, 3, (L,), generator=g), 3).float()
            self.items.append((torch.randn(L, 6, generator=g), torch.randn(L, 10, generator=g), torch.randn(L, 3, generator=g), spk,
                               torch.ones(L), torch.randint(0, 6, (L,), generator=g), k))

    def __getitem__(self, i):
        return self.items[i]

    def __len__(self):
        return len(self.items)

    @staticmethod
    def collate_fn(data):
        from gan_ffn_amd.data import IEMOCAPDataset
        return IEMOCAPDataset.collate_fn(data)


@pytest.fixture(scope="module")
def corpora(tmp_path_factory):
    """kind -> (dataset, to_batch, DeviceCorpus on the GPU)"""
    from gan_ffn_amd import data as D
    d = tmp_path_factory.mktemp("device_corpus_gpu")
    ie, me = str(d / "ie.pkl"), str(d / "me.pkl")
    D.write_synthetic_iemocap_pickle(ie, n_train=9, n_test=3, seed=2, lo=1, hi=6)
    D.write_synthetic_meld_pickle(me, n_train=23, n_test=3, seed=1, lo=1, hi=6)
    sets = {"iemocap": (D.IEMOCAPDataset(ie, True), D.to_batch), "meld": (D.MELDDataset(me, "emotion", True), D.to_meld_batch),
            "tiny": (Tiny(), D.to_batch)}
    out = {k: (ds, tb, D.DeviceCorpus(ds, DEV)) for k, (ds, tb) in sets.items()}
    assert len(out["iemocap"][0]) == 9 and len(out["meld"][0]) == 23
    assert out["iemocap"][2].widths == {"text": 100, "visual": 512, "acoustic": 100} and out["iemocap"][2].n_parties == 2
    assert out["meld"][2].widths == {"text": 600, "acoustic": 300} and out["meld"][2].n_parties == 9
    assert out["tiny"][2].widths == {"text": 6, "visual": 10, "acoustic": 3} and out["tiny"][2].n_parties == 3
    return out


def assert_same_batch(got, want):
    assert list(got) == list(want)
    for k in want:
        if torch.is_tensor(want[k]):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].device == want[k].device, k
            assert got[k].is_contiguous(), k
            assert torch.equal(got[k], want[k]), k
        else:
            assert got[k] == want[k], k


def index_batches(lengths):
    n = len(lengths)
    one = lengths.index(1)
    return {"length1": [one], "repeat": [3, 1, 3, 3, 2], "last_first": [n - 1, 0], "whole": list(range(n)),
            "last_first_repeat": [n - 1, 0, 0, 4]}


@pytest.mark.parametrize("kind", ["iemocap", "meld", "tiny"])
@pytest.mark.parametrize("case", ["length1", "repeat", "last_first", "whole", "last_first_repeat"])
def test_gather_equals_host_collate(corpora, kind, case):
    ds, to_batch, corpus = corpora[kind]
    idx = index_batches(corpus.lengths)[case]
    want = to_batch(ds.collate_fn([ds[i] for i in idx]), DEV)
    S = max(corpus.lengths[i] for i in idx)
    got = corpus.gather(torch.tensor(idx, dtype=torch.int32, device=DEV), S)
    got["vids"] = [corpus.keys[i] for i in idx]
    if case == "length1":
        assert S == 1
    assert_same_batch(got, want)


@pytest.mark.parametrize("kind", ["iemocap", "meld", "tiny"])
def test_loader_epoch_equals_host_loader_with_a_short_last_batch(corpora, kind):
    from torch.utils.data import DataLoader
    from gan_ffn_amd import data as D
    ds, to_batch, corpus = corpora[kind]
    bs = 4 if kind != "tiny" else 3
    assert len(ds) % bs                                           # the last batch is short
    host = [to_batch(c, DEV) for c in DataLoader(ds, batch_size=bs, collate_fn=ds.collate_fn)]
    dev = list(D.DeviceLoader(corpus, None, bs))
    assert len(dev) == len(host) and dev[-1]["umask"].shape[0] == len(ds) % bs
    for g, w in zip(dev, host):
        assert_same_batch(g, w)


def test_shards_equal_shard_batch(corpora):
    from gan_ffn_amd import data as D
    _, _, corpus = corpora["tiny"]
    sampler = torch.utils.data.SubsetRandomSampler(list(range(8)))
    torch.manual_seed(3)
    full = list(D.DeviceLoader(corpus, sampler, 4))
    assert len(full) == 2
    for rank in (0, 1):
        torch.manual_seed(3)
        part = list(D.DeviceLoader(corpus, sampler, 4, rank, 2))
        for p, f in zip(part, full):
            assert_same_batch(p, D.shard_batch(f, rank, 2))


# ------------------------------------------------------------------------------------------------
# the raw calls
# ------------------------------------------------------------------------------------------------
def test_raw_gather_writes_its_destinations_and_nothing_else():
    """destinations inside NaN-filled buffers; an index outside the corpus, a row range outside n_rows and S below the longest
    dialogue (5 rows, S = 4) behave as include/ganffn.h says: empty dialogues, and the first S rows"""
    from gan_ffn_amd import _lib, ops
    lengths = [3, 1, 5, 2]
    row0 = [0, 3, 4, 9, 11]
    n_rows = 9                                                   # dialogue 3 (rows 9, 10) lies outside: an empty dialogue
    g = torch.Generator().manual_seed(1)
    src8, src3 = torch.randn(11, 8, generator=g), torch.randn(11, 3, generator=g)
    lab = torch.randint(1, 6, (11,), generator=g)
    idx = [2, 7, -1, 0, 3, 2, 1]
    S, B, PAD = 4, len(idx), 64
    eff = {0: 3, 1: 1, 2: 4}                                     # rows copied per valid index
    want8, want3 = torch.zeros(S, B, 8), torch.zeros(S, B, 3)
    want_m, want_l = torch.zeros(B, S), torch.zeros(B, S, dtype=torch.int64)
    for b, d in enumerate(idx):
        n = eff.get(d, 0)
        if n:
            want8[:n, b], want3[:n, b] = src8[row0[d]:row0[d] + n], src3[row0[d]:row0[d] + n]
            want_m[b, :n], want_l[b, :n] = 1, lab[row0[d]:row0[d] + n]
    nan = float("nan")
    buf8 = torch.full((PAD + S * B * 8 + PAD,), nan, device=DEV)
    buf3 = torch.full((PAD + S * B * 3 + PAD,), nan, device=DEV)
    bufm = torch.full((PAD + B * S + PAD,), nan, device=DEV)
    bufl = torch.full((PAD + B * S + PAD,), -7777, dtype=torch.int64, device=DEV)
    d8, d3 = buf8[PAD:PAD + S * B * 8].view(S, B, 8), buf3[PAD:PAD + S * B * 3].view(S, B, 3)
    dm, dl = bufm[PAD:PAD + B * S].view(B, S), bufl[PAD:PAD + B * S].view(B, S)
    ops.batch_gather_raw([(src8.to(DEV), d8, 8), (src3.to(DEV), d3, 3)], lab.to(DEV), torch.tensor(row0, device=DEV), n_rows,
                         torch.tensor(idx, dtype=torch.int32, device=DEV), dm, dl, S, B, 4)
    torch.cuda.synchronize()
    assert torch.equal(d8.cpu(), want8) and torch.equal(d3.cpu(), want3) and torch.equal(dm.cpu(), want_m) and torch.equal(dl.cpu(), want_l)
    for buf, n in ((buf8, S * B * 8), (buf3, S * B * 3), (bufm, B * S)):
        assert bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + n:]).all())
    assert bool((bufl[:PAD] == -7777).all()) and bool((bufl[PAD + B * S:] == -7777).all())
    # a misaligned 16-byte column is an argument error, not a launch
    with pytest.raises(_lib.GanffnError, match="16-byte aligned"):
        ops.batch_gather_raw([(src8.to(DEV), buf8[1:1 + S * B * 8], 8)], lab.to(DEV), torch.tensor(row0, device=DEV), n_rows,
                             torch.tensor(idx, dtype=torch.int32, device=DEV), dm, dl, S, B, 4)


def test_record_ties_go_to_the_lowest_class():
    from gan_ffn_amd import ops
    S, B, Cn = 5, 3, 7
    g = torch.Generator().manual_seed(2)
    lp = torch.randint(-3, 1, (S, B, Cn), generator=g).float()            # few distinct values: most rows have tied maxima
    lp[0, 0] = 0.0                                                       # all seven tied
    lp[1, 2] = torch.tensor([-1.0, -2.0, -1.0, -3.0, -1.0, -2.0, -1.0])
    ref = np.argmax(lp.numpy().transpose(1, 0, 2).reshape(-1, Cn), axis=1)
    assert sum(int((row == row.max()).sum() > 1) for row in lp.numpy().reshape(-1, Cn)) >= 5
    label = torch.randint(0, Cn, (B, S), generator=g)
    umask = (torch.rand(B, S, generator=g) < 0.6).float()
    loss = torch.tensor([1.625])
    off, cap = 11, 11 + S * B + 6
    rec = ops.EpochRecord(cap, 3, DEV)
    rec.preds.fill_(-5); rec.labels.fill_(-5); rec.masks.fill_(-5.0); rec.loss.fill_(-5.0); rec.count.fill_(-5.0)
    rec.record(1, off, lp.to(DEV), label.to(DEV), umask.to(DEV), loss.to(DEV))
    preds, labels, masks, loss_h, count_h = rec.host()
    assert preds.dtype == np.int64 and labels.dtype == np.int64 and masks.dtype == np.float32
    assert np.array_equal(preds[off:off + S * B], ref)
    assert np.array_equal(labels[off:off + S * B], label.reshape(-1).numpy()) and np.array_equal(masks[off:off + S * B], umask.reshape(-1).numpy())
    for a in (preds, labels, masks):
        assert (a[:off] == -5).all() and (a[off + S * B:] == -5).all()
    assert list(loss_h) == [-5.0, 1.625, -5.0] and list(count_h) == [-5.0, float(umask.sum()), -5.0]


def meld_engine(seed=11):
    from gan_ffn_amd import dialogue_rnn as DR, engine as E, ops
    torch.manual_seed(seed)
    # (D_h = 2 D_e, as in the script's MELDLSTMModel(600, 300, 600): the att2 branch feeds the 2 D_e wide state to smax_fc)
    net = DR.MELDLSTMModel(600, 8, 16, n_classes=7, dropout=0.6).to(DEV)
    ops.manual_seed(4242)
    return E.MeldEngine(net)


def test_record_equals_engine_predictions_on_real_outputs(corpora):
    from gan_ffn_amd import ops
    ds, to_batch, corpus = corpora["meld"]
    eng = meld_engine()
    idx = list(range(5, 12))
    batch = corpus.gather(torch.tensor(idx, dtype=torch.int32, device=DEV), max(corpus.lengths[i] for i in idx))
    loss, log_prob = eng.step(batch, train=False)
    B, S = batch["umask"].shape
    rec = ops.EpochRecord(B * S, 1, DEV)
    rec.record(0, 0, log_prob, batch["label"], batch["umask"], loss)
    preds, labels, masks, loss_h, count_h = rec.host()
    assert np.array_equal(preds, eng.predictions(log_prob).cpu().numpy())
    assert np.array_equal(labels, batch["label"].reshape(-1).cpu().numpy())
    assert np.array_equal(masks, batch["umask"].reshape(-1).cpu().numpy())
    assert loss_h[0] == float(loss) and count_h[0] == float(batch["umask"].sum()) == sum(corpus.lengths[i] for i in idx)


# ------------------------------------------------------------------------------------------------
# whole epochs: host loaders against device loaders, two identically seeded copies
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def epoch_pickles(tmp_path_factory):
    from gan_ffn_amd import data as D
    d = tmp_path_factory.mktemp("device_corpus_epochs")
    ie, me = str(d / "ie.pkl"), str(d / "me.pkl")
    D.write_synthetic_iemocap_pickle(ie, n_train=12, n_test=5, seed=21, lo=2, hi=12, dtype=np.float32)
    D.write_synthetic_meld_pickle(me, n_train=12, n_test=5, seed=22, lo=1, hi=12)
    return ie, me


def loaders_of(kind, path, device_side):
    from gan_ffn_amd import data as D
    if kind == "meld":
        if device_side:
            return D.get_device_loaders(D.MELDDataset(path, "emotion", True), D.MELDDataset(path, "emotion", False), 4, 0.25, DEV)
        return D.get_MELD_loaders(path, batch_size=4, valid=0.25)
    if device_side:
        return D.get_device_loaders(D.IEMOCAPDataset(path, True), D.IEMOCAPDataset(path, False), 4, 0.25, DEV)
    return D.get_IEMOCAP_loaders(path, batch_size=4, valid=0.25)


def build_engine(kind):
    from gan_ffn_amd import engine as E, model as M, ops
    if kind == "meld":
        return meld_engine()
    torch.manual_seed(13)
    gens = [M.AcousticGenerator(100), M.VisualGenerator(100), M.TextGenerator(100)]
    if kind == "phase2":
        net = M.GAN_FFN(*gens, n_classes=6).to(DEV)
        ops.manual_seed(4242)
        return E.Phase2Engine(net)
    net = M.GAN_FFN_DialogueRNN(*gens, n_classes=6, listener_state=False, context_attention="general", dropout_rec=0.1, dropout=0.6,
                                D_m=100, D_g=500, D_p=500, D_e=100, D_h=100, D_a=100).to(DEV)
    ops.manual_seed(4242)
    return E.DrnnEngine(net)


def run_epochs(kind, path, device_side):
    """one train epoch, then the valid and test epochs in eval mode -> ([result tuples], parameters)"""
    from gan_ffn_amd import artifacts as A, data as D
    eng = build_engine(kind)
    train, valid, test = loaders_of(kind, path, device_side)
    to_batch = D.to_meld_batch if kind == "meld" else D.to_batch
    torch.manual_seed(99)
    out = [A.train_or_eval_model(eng, train, True, DEV, to_batch), A.train_or_eval_model(eng, valid, False, DEV, to_batch),
           A.train_or_eval_model(eng, test, False, DEV, to_batch)]
    torch.cuda.synchronize()
    return out, [p.detach().clone() for p in eng.module.parameters()]


@pytest.mark.parametrize("kind", ["meld", "phase2", "drnn"])
def test_epochs_equal_the_host_loaders(epoch_pickles, kind):
    path = epoch_pickles[1] if kind == "meld" else epoch_pickles[0]
    host, p_host = run_epochs(kind, path, False)
    dev, p_dev = run_epochs(kind, path, True)
    for i, (h, d) in enumerate(zip(host, dev)):
        assert len(h) == len(d) == 7
        assert (h[0], h[1], h[5]) == (d[0], d[1], d[5]), (i, h[0], d[0], h[1], d[1], h[5], d[5])
        assert type(h[0]) is type(d[0]) and np.isfinite(h[0]) and h[4].sum() > 0
        for j in (2, 3, 4):
            assert h[j].dtype == d[j].dtype and np.array_equal(h[j], d[j]), (i, j)
        assert h[6][3] == d[6][3] and h[6][1:3] == d[6][1:3] == [[], []]
        if i:
            assert len(h[6][3]) > 0                                       # eval epochs carry the vids
        assert len(h[6][0]) == len(d[6][0])
        if kind == "meld" and i:
            assert len(h[6][0]) > 0
        for a, b in zip(h[6][0], d[6][0]):
            assert torch.equal(a, b)
    assert len(p_host) == len(p_dev) > 0
    for a, b in zip(p_host, p_dev):
        assert torch.equal(a, b)


def test_train_GAN_rows_and_parameters_equal_the_host_loader(epoch_pickles):
    from gan_ffn_amd import artifacts as A, data as D, engine as E, ops

    def run(device_side):
        gens, discs = E.build_networks(100, 0.2, DEV, seed=17)
        ops.manual_seed(4242)
        train = loaders_of("iemocap", epoch_pickles[0], device_side)[0]
        batches = train if device_side else A._DeviceBatches(train, DEV)
        torch.manual_seed(99)
        rows = E.train_GAN(gens, discs, batches, epochs=2, reserve_S=12)
        torch.cuda.synchronize()
        return rows, [p.detach().clone() for m in list(gens.values()) + list(discs.values()) for p in m.parameters()]

    rows_h, p_h = run(False)
    rows_d, p_d = run(True)
    assert len(rows_h) == 2 and rows_h == rows_d and all(np.isfinite(v) for r in rows_h for v in r.values())
    assert len(p_h) == len(p_d) > 0
    for a, b in zip(p_h, p_d):
        assert torch.equal(a, b)


def test_train_GAN_with_a_log_reads_every_batch(epoch_pickles):
    """the per-batch host read stays where somebody asks for it, and gives the row the silent run gives"""
    from gan_ffn_amd import engine as E, ops

    def run(log):
        gens, discs = E.build_networks(100, 0.2, DEV, seed=17)
        ops.manual_seed(4242)
        torch.manual_seed(99)
        return E.train_GAN(gens, discs, loaders_of("iemocap", epoch_pickles[0], True)[0], epochs=1, reserve_S=12, log=log)

    seen = []
    rows = run(lambda e, d: seen.append(dict(d)))
    assert len(seen) == 3 and {c: seen[-1][c] for c in E.LOSS_COLUMNS} == {c: rows[0][c] for c in E.LOSS_COLUMNS}
    assert rows == run(None)


# ------------------------------------------------------------------------------------------------
# device-to-host reads
# ------------------------------------------------------------------------------------------------
def test_device_epoch_reads_the_device_a_fixed_number_of_times(tmp_path, monkeypatch):
    """Tensor.cpu / item / tolist / __float__ / numpy on GPU tensors during one eval epoch of MeldEngine: the device loader's
    count is the same for 2 batches as for 5, the host loader's grows"""
    from gan_ffn_amd import artifacts as A, data as D
    pk = str(tmp_path / "me.pkl")
    D.write_synthetic_meld_pickle(pk, n_train=2, n_test=10, seed=5, lo=2, hi=9)
    eng = meld_engine()
    testset = D.MELDDataset(pk, "emotion", False)
    corpus = D.DeviceCorpus(testset, DEV)
    from torch.utils.data import DataLoader
    host = {bs: DataLoader(testset, batch_size=bs, collate_fn=testset.collate_fn) for bs in (5, 2)}
    dev = {bs: D.DeviceLoader(corpus, None, bs) for bs in (5, 2)}
    assert [len(dev[5]), len(dev[2])] == [2, 5]
    for l in (host[5], dev[5]):                                              # warm-up: allocations, lazy initialisation
        A.train_or_eval_model(eng, l, False, DEV, D.to_meld_batch)
    calls = []
    for name in ("cpu", "item", "tolist", "__float__", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                calls.append(_name)
            return _orig(self, *a, **k)

        monkeypatch.setattr(torch.Tensor, name, counted)
    counts = {}
    for side, loaders in (("host", host), ("dev", dev)):
        for bs in (5, 2):
            calls.clear()
            A.train_or_eval_model(eng, loaders[bs], False, DEV, D.to_meld_batch)
            counts[side, bs] = len(calls)
    assert counts["dev", 5] == counts["dev", 2] > 0, counts
    assert counts["host", 2] >= counts["host", 5] + 3, counts             # at least one read per batch: 5 batches against 2
