"""The host-side logic of the device-resident corpus (data.DeviceCorpus / data.DeviceLoader) and the argument checks of the
two exports behind it (csrc/batch.hip).  No GPU: the corpus is packed on "cpu", the exports are called with arguments they
must refuse before any device call."""
import ctypes as C

import numpy as np
import pytest
import torch

from gan_ffn_amd import _lib
from gan_ffn_amd import data as D


@pytest.fixture(scope="module")
def pickles(tmp_path_factory):
    d = tmp_path_factory.mktemp("device_corpus")
    ie, me = str(d / "iemocap.pkl"), str(d / "meld.pkl")
    D.write_synthetic_iemocap_pickle(ie, n_train=12, n_test=5)
    D.write_synthetic_meld_pickle(me, n_train=12, n_test=5)
    return ie, me


def host_and_device_loaders(kind, path, batch_size, valid):
    if kind == "iemocap":
        host = D.get_IEMOCAP_loaders(path, batch_size=batch_size, valid=valid)
        sets = D.IEMOCAPDataset(path, True), D.IEMOCAPDataset(path, False)
    else:
        host = D.get_MELD_loaders(path, batch_size=batch_size, valid=valid)
        sets = D.MELDDataset(path, "emotion", True), D.MELDDataset(path, "emotion", False)
    return host, D.get_device_loaders(sets[0], sets[1], batch_size, valid, "cpu")


@pytest.mark.parametrize("kind,valid", [("iemocap", 0.25), ("meld", 0.25), ("meld", 0.0)])
def test_index_stream_is_the_host_loaders(pickles, kind, valid):
    """same vids in the same order and the same global RNG state afterwards: train, valid and test loaders, two epochs"""
    host, dev = host_and_device_loaders(kind, pickles[0] if kind == "iemocap" else pickles[1], 4, valid)
    torch.manual_seed(77)
    want = []
    for _ in range(2):
        for loader in host:
            want.append([list(collated[-1]) for collated in loader])
    state_host = torch.get_rng_state()
    torch.manual_seed(77)
    got = []
    for _ in range(2):
        for loader in dev:
            keys = loader.corpus.keys
            got.append([[keys[i] for i in idx] for idx in loader.index_batches()])
    assert got == want
    assert torch.equal(torch.get_rng_state(), state_host)
    assert want[0] != want[3]                                  # (the train order is reshuffled per epoch: the test is not vacuous)
    assert [len(l) for l in dev] == [len(l) for l in host]


def test_epoch_plan_pads_to_the_longest_dialogue_and_shards_by_rank(pickles):
    ds = D.IEMOCAPDataset(pickles[0], True)
    corpus = D.DeviceCorpus(ds, "cpu")
    full = D.DeviceLoader(corpus, None, 4).epoch()
    L = corpus.lengths
    assert [b[0] for b in full.batches] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]
    at = 0
    for idx, S, off in full.batches:
        assert S == max(L[i] for i in idx) and off == at
        at += S * len(idx)
    assert full.total == at
    for rank in (0, 1):
        part = D.DeviceLoader(corpus, None, 4, rank, 2).epoch()
        assert [b[0] for b in part.batches] == [b[0][2 * rank:2 * rank + 2] for b in full.batches]
        assert [b[1] for b in part.batches] == [b[1] for b in full.batches]        # S of the FULL batch, as shard_batch keeps it
        assert part.total == full.total // 2
    with pytest.raises(_lib.GanffnError, match="no CPU"):
        next(iter(D.DeviceLoader(corpus, None, 4)))


@pytest.mark.parametrize("kind", ["iemocap", "meld", "meld_lo1"])
def test_packing(pickles, tmp_path, kind):
    if kind == "iemocap":
        ds, widths, P = D.IEMOCAPDataset(pickles[0], True), {"text": 100, "visual": 512, "acoustic": 100}, 2
    elif kind == "meld":
        ds, widths, P = D.MELDDataset(pickles[1], "emotion", False), {"text": 600, "acoustic": 300}, 9
    else:
        p = str(tmp_path / "lo1.pkl")
        D.write_synthetic_meld_pickle(p, n_train=40, n_test=2, lo=1, hi=3)
        ds, widths, P = D.MELDDataset(p, "emotion", True), {"text": 600, "acoustic": 300}, 9
    c = D.DeviceCorpus(ds, "cpu")
    items = [ds[i] for i in range(len(ds))]
    lengths = [int(it[-2].shape[0]) for it in items]
    if kind == "meld_lo1":
        assert 1 in lengths
    assert c.keys == list(ds.keys) and c.lengths == lengths and len(c) == len(ds)
    assert c.n_dialogues == len(ds) and c.n_rows == sum(lengths)
    assert c.row0.dtype == torch.int64 and c.row0.tolist() == [0] + list(np.cumsum(lengths))
    assert list(c.features) == list(widths) and c.widths == widths and c.n_parties == P
    for j, (k, w) in enumerate(widths.items()):
        assert c.features[k].dtype == torch.float32 and tuple(c.features[k].shape) == (c.n_rows, w) and c.features[k].is_contiguous()
        assert torch.equal(c.features[k], torch.cat([it[j] for it in items]))
    assert c.qmask.dtype == torch.float32 and tuple(c.qmask.shape) == (c.n_rows, P)
    assert torch.equal(c.qmask, torch.cat([it[len(widths)] for it in items]))
    assert c.labels.dtype == torch.int64 and torch.equal(c.labels, torch.cat([it[-2] for it in items]))


def test_packing_refuses_other_item_layouts():
    class Odd(torch.utils.data.Dataset):
        keys = ["a"]

        def __len__(self):
            return 1

        def __getitem__(self, i):
            return (torch.zeros(2, 4), torch.ones(2), torch.zeros(2, dtype=torch.long), "a")

    with pytest.raises(ValueError, match="fields"):
        D.DeviceCorpus(Odd(), "cpu")


# ------------------------------------------------------------------------------------------------
# the exports: present, bound, and refusing bad arguments before any device call (there is no device here)
# ------------------------------------------------------------------------------------------------
def gather_args(n_cols=2, S=5, B=3, n_dialogues=7, null=None):
    """arguments whose pointers are non-null but never dereferenced: every case below must be refused on the host"""
    cols = (_lib.BatchCol * 6)()
    for c in cols:
        c.src, c.dst, c.width = 4096, 8192, 100
    p = lambda name: None if null == name else C.c_void_p(4096)
    return [None if null == "cols" else C.cast(cols, C.c_void_p), n_cols, p("labels"), p("row0"), C.c_int64(50), p("idx"), p("umask"),
            p("label"), S, B, n_dialogues, None]


def record_args(S=5, B=3, Cn=7, offset=0, capacity=100, step=0, n_steps=2, null=None):
    p = lambda name: None if null == name else C.c_void_p(4096)
    return [p("log_prob"), p("label"), p("umask"), p("loss"), S, B, Cn, p("preds"), p("labels_out"), p("masks"), C.c_int64(offset),
            C.c_int64(capacity), p("loss_out"), p("count"), step, n_steps, None]


def refused(name, args, match):
    lib = _lib.load()
    assert getattr(lib, name)(*args) != 0
    assert match.encode() in lib.ganffn_last_error(), lib.ganffn_last_error()
    with pytest.raises(_lib.GanffnError, match=match):
        _lib.call(name, *args)


def test_exports_exist_with_header_text_and_bindings():
    import os
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ganffn.h")).read()
    for s in ("ganffn_batch_gather", "ganffn_epoch_record"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES and "int %s(" % s in header
    assert "#define GANFFN_BATCH_MAX_COLS %d" % _lib.BATCH_MAX_COLS in header
    assert C.sizeof(_lib.BatchCol) == 24


@pytest.mark.parametrize("kw,match", [(dict(S=0), "S=0"), (dict(S=-3), "S=-3"), (dict(B=0), "B=0"), (dict(B=257), "B=257"),
                                      (dict(n_cols=5), "n_cols=5"), (dict(n_cols=0), "n_cols=0"), (dict(n_dialogues=0), "n_dialogues=0")]
                         + [(dict(null=n), "null pointer") for n in ("cols", "labels", "row0", "idx", "umask", "label")])
def test_batch_gather_refuses_bad_arguments(kw, match):
    refused("ganffn_batch_gather", gather_args(**kw), match)


def test_batch_gather_refuses_bad_columns():
    for field, value, match in (("src", None, "column 1: null"), ("dst", None, "column 1: null"), ("width", 0, "width=0"),
                                ("src", 4100, "16-byte aligned"), ("dst", 8196, "16-byte aligned")):
        args = gather_args()
        cols = (_lib.BatchCol * 2)()
        for c in cols:
            c.src, c.dst, c.width = 4096, 8192, 100
        setattr(cols[1], field, value)
        args[0] = C.cast(cols, C.c_void_p)
        refused("ganffn_batch_gather", args, match)


@pytest.mark.parametrize("kw,match", [(dict(S=0), "S=0"), (dict(B=0), "B=0"), (dict(B=257), "B=257"), (dict(Cn=17), "C=17"), (dict(Cn=0), "C=0"),
                                      (dict(offset=-1), "offset=-1"), (dict(offset=86), "offset=86"), (dict(capacity=14), "epoch buffers of 14"),
                                      (dict(step=2), "step=2"), (dict(step=-1), "step=-1")]
                         + [(dict(null=n), "null pointer") for n in ("log_prob", "label", "umask", "loss", "preds", "labels_out", "masks",
                                                                      "loss_out", "count")])
def test_epoch_record_refuses_bad_arguments(kw, match):
    refused("ganffn_epoch_record", record_args(**kw), match)


def test_wrappers_refuse_cpu_tensors():
    from gan_ffn_amd import ops
    f, l = torch.zeros(4, 4), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(_lib.GanffnError, match="no CPU fallback"):
        ops.batch_gather_raw([(f, torch.zeros(2, 1, 4), 4)], l, torch.tensor([0, 4]), 4, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2),
                             torch.zeros(1, 2, dtype=torch.int64), 2, 1, 1)
    with pytest.raises(_lib.GanffnError, match="no CPU fallback"):
        ops.EpochRecord(8, 1, "cpu")


def test_training_flows_take_device_corpus_and_default_to_the_host_loaders():
    import inspect
    from gan_ffn_amd import artifacts as A
    for fn in (A.run_training, A.run_meld_training):
        assert inspect.signature(fn).parameters["device_corpus"].default is False
