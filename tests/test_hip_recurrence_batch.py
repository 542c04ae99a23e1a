"""Batches above 32 dialogues on the HIP recurrences (the dialogue-tile axis of the skinny products: csrc/dialogue_rnn.hip,
csrc/lstm.hip; ganffn_drnn_batch_*, ganffn_lstm_batch_*, ganffn_lstm_stack_batch_*), on the device:
  1. the module path against the REFERENCE-made fixture tests/golden/recurrence_batch.npz (tests/test_recurrence_batch_cpu.py pins
     it to the CPU restatement), with the bounds tests/test_hip_drnn_parties.py and tests/test_hip_meld_engine.py hold the same
     quantities to;
  2. each recurrence alone against the fp64 torch restatement, eval mode and train mode with the same Philox masks (rows t*B + b
     of the WHOLE batch), B in {33, 64, 100, 256}, with and without listener state, 2 and 9 parties, every attention type; the
     skinny products alone, and the tile property: a row's bits do not depend on which other dialogues share the launch;
  3. the proof that one native call runs per forward (two above ops.MAX_DIALOGUES dialogues), none of the 32-dialogue ones;
  4. B <= 32 through the _batch_ entry points bit for bit against the existing ones;
  5. DrnnEngine(max_dialogues=64) and MeldEngine(max_dialogues=128) against the fp64 step oracles with the engines' own masks,
     Adam included; eval steps against the module path; the refusals; determinism.
Every case compares every element or every stored sample; the distances are printed before they are asserted.
Not here: a two-rank gloo run at 40 dialogues per rank — the worker scripts (tests/ddp_gpu_worker.py, tests/meld_ddp_gpu_worker.py)
build their engines without max_dialogues and on 4-dialogue batches, and existing test files are not edited."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import make_golden_batch as MB
from gan_ffn_amd.ops import MAX_DIALOGUES        # (a tree without the wide dialogue axis fails here, before any launch)
from oracle import ganffn_oracle as O
from oracle import lstm_oracle as LO
from test_hip_drnn_kernel import _MaskSeq, compare
from test_hip_drnn_parties import build, make_inputs, party_masks
from util import golden

pytestmark = pytest.mark.gpu

SEED = 20261016


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


class _Calls:
    """counts _lib.call per entry point"""

    def __init__(self, monkeypatch):
        from gan_ffn_amd import _lib
        self.n = {}
        real = _lib.call

        def counted(name, *a):
            self.n[name] = self.n.get(name, 0) + 1
            return real(name, *a)
        monkeypatch.setattr(_lib, "call", counted)

    def of(self, prefix):
        return {k: v for k, v in self.n.items() if k.startswith(prefix)}


# ------------------------------------------------------------------------------------------------------------------
# 1. the module path against the reference-made fixture
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(MB.DRNN_CASES))
def test_bimodel_matches_reference_fixture(tag, monkeypatch):
    """the tighter of tests/test_hip_drnn_parties.py:110-115's bounds: log-probabilities 5e-5, dU 2e-4, the parameter gradients
    5e-4 of the tensor's scale, every stored sample, no outliers (the l2 of every gradient tensor 2e-3); one native call each way"""
    import test_recurrence_batch_cpu as X
    calls = _Calls(monkeypatch)
    X.check_drnn_case(X.batch_model(MB.DRNN_CASES[tag][0]).cuda(), tag, "cuda", rtol=5e-5, grtol=5e-4, du_rtol=2e-4)
    rec = {k: v for k, v in calls.of("ganffn_drnn_").items() if "join" not in k}
    assert rec == {"ganffn_drnn_batch_fwd": 1, "ganffn_drnn_batch_bwd": 1}, rec


@pytest.mark.parametrize("tag", list(MB.MELD_CASES))
def test_meld_module_path_and_engine_reproduce_the_reference_fixture(tag):
    """tests/test_hip_meld_engine.test_engine_reproduces_the_reference_fixture's bounds: step 0 log_prob 5e-5 of scale (the loss
    likewise), later steps at most twice the module path's own distance or the step-0 bound, final parameters within 2 lr
    N_STEPS; here for the module path (autograd + torch.optim.Adam, one ganffn_lstm_batch_layer_* call per layer) and the engine"""
    import test_recurrence_batch_cpu as X
    from gan_ffn_amd import engine as E
    from test_hip_meld_engine import dist, mirror, module_step
    g = golden("recurrence_batch")
    S, B, Cn = MB.MELD_CASES[tag]
    U, umask, label = MB.meld_inputs(tag)
    b = {"text": torch.from_numpy(U).cuda(), "umask": torch.from_numpy(umask).cuda(), "label": torch.from_numpy(label).cuda()}
    m_e, m_m = mirror(Cn), mirror(Cn)
    eng = E.MeldEngine(m_e, lr=MB.LR, weight_decay=MB.L2, max_dialogues=128)
    opt = torch.optim.Adam(m_m.parameters(), lr=MB.LR, weight_decay=MB.L2)
    pre = "meld/%s/" % tag
    res_e, res_m = [], []
    for i in range(MB.N_STEPS):
        loss_e, lp_e = eng.step(b, train=True)
        res_e.append((float(loss_e), lp_e.cpu().numpy().copy()))
        loss_m, lp_m, _ = module_step(m_m, b, opt)
        res_m.append((float(loss_m), lp_m.cpu().numpy().copy()))
    idx = MB.F_.sample_indices(S * B * Cn)
    lp_scale = float(g[pre + "log_prob0/maxabs"])
    full = pre + "log_prob0/full" in g.files                 # (formula.summarize stores small tensors whole)
    pick = (lambda a: a) if full else (lambda a: a.reshape(-1)[idx])
    for i in range(MB.N_STEPS):
        ref_lp, ref_loss = g[pre + "log_prob%d/%s" % (i, "full" if full else "sample")], float(g[pre + "loss"][i])
        d_e, d_m = dist(pick(res_e[i][1]), ref_lp), dist(pick(res_m[i][1]), ref_lp)
        dl_e, dl_m = abs(res_e[i][0] - ref_loss), abs(res_m[i][0] - ref_loss)
        print("%s step %d: log_prob engine %.2e module %.2e | loss engine %.2e module %.2e" % (tag, i, d_e, d_m, dl_e, dl_m))
        assert d_m <= 5e-5 and dl_m <= 5e-5 * lp_scale, (tag, i, d_m, dl_m)
        assert d_e <= (5e-5 if i == 0 else max(2 * d_m, 5e-5)), (tag, i, d_e, d_m)
        assert dl_e <= (5e-5 * lp_scale if i == 0 else max(2 * dl_m, 5e-5 * lp_scale)), (tag, i, dl_e, dl_m)
    worst = (0.0, 0.0, "")
    pm = dict(m_m.named_parameters())
    for k, p in m_e.named_parameters():
        ref = g[pre + "param/" + k].astype(np.float64)
        de = float(np.abs(MB.sample(p.detach().cpu().numpy()) - ref).max())
        dm = float(np.abs(MB.sample(pm[k].detach().cpu().numpy()) - ref).max())
        worst = max(worst, (de, dm, k))
        assert dm <= 2 * MB.LR * MB.N_STEPS and de <= max(2 * dm, 2 * MB.LR * MB.N_STEPS), (tag, k, de, dm)
    print("%s final parameters: worst engine %.2e (module %.2e) %s" % (tag, *worst))
    assert int(eng.step_count.item()) == MB.N_STEPS


# ------------------------------------------------------------------------------------------------------------------
# 2. the recurrences alone against the fp64 restatement
# ------------------------------------------------------------------------------------------------------------------
# (S, B, P, listener, attention): every attention type above 32 dialogues, both party counts with and without listener state (P = 9 with
# listener state: the wide skinny group, 20 problems per launch); one case at (94, 64); B = 256 at S <= 33
EVAL_CASES = [(20, 33, 2, False, "general"), (94, 64, 2, False, "general"), (33, 100, 9, True, "concat"), (20, 256, 9, False, "general2"),
              (12, 256, 9, True, "general"), (15, 100, 2, True, "simple"), (15, 64, 2, False, "dot"), (33, 33, 9, False, "concat")]


@pytest.mark.parametrize("S,B,P,listener,att", EVAL_CASES)
def test_drnn_eval_mode_matches_torch_restatement(S, B, P, listener, att):
    from gan_ffn_amd import ops
    U, qmask = make_inputs(S, B, P, seed=S * 100 + B + P, Dm=100)
    m_cpu = build(listener, att).double().eval()
    m_gpu = copy.deepcopy(m_cpu).float().cuda().eval()
    pred = ops.dialogue_rnn_listener_supported if listener else ops.dialogue_rnn_supported
    assert pred(m_gpu.dialogue_cell, U.cuda(), qmask.cuda())
    compare(m_gpu, m_cpu, U, qmask)          # emotions, alpha, dU, every parameter gradient


@pytest.mark.parametrize("S,B,P,listener", [(9, 33, 2, False), (13, 100, 9, True), (9, 256, 2, True), (11, 64, 9, False)])
def test_drnn_train_mode_matches_torch_restatement_with_the_same_philox_masks(S, B, P, listener):
    """the masks are Philox rows t*B + b of the whole batch (oracle.philox.keep_mask with S*B rows)"""
    from gan_ffn_amd import ops
    U, qmask = make_inputs(S, B, P, seed=S + B + P)
    p = 0.1
    m_cpu = build(listener, dropout=p).double().train()
    m_gpu = copy.deepcopy(m_cpu).float().cuda().train()
    m_cpu.dialogue_cell.dropout = _MaskSeq(party_masks(S, B, 500, 100, p, SEED, 0, P, listener))
    ops.manual_seed(SEED)                       # the call below takes rng offset 0
    compare(m_gpu, m_cpu, U, qmask)


@pytest.mark.parametrize("S,B,In,H", [(12, 33, 600, 300), (33, 64, 600, 300), (7, 100, 600, 300), (5, 256, 600, 300), (6, 40, 64, 20)])
def test_lstm_layer_matches_fp64_oracle(S, B, In, H, monkeypatch):
    """tests/test_hip_lstm.test_one_bidirectional_layer_forward_and_backward's comparison and bounds, one native call each way"""
    from gan_ffn_amd import ops
    from test_hip_lstm import make_lstm
    calls = _Calls(monkeypatch)
    lstm = make_lstm(In, H, 1, seed=S * 7 + B)
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    params = [getattr(lstm, n) for n in names] + [getattr(lstm, n + "_reverse") for n in names]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(S, B, In, generator=g)
    gy = torch.randn(S, B, 2 * H, generator=g)
    P = {k: p.detach().double().requires_grad_(True) for k, p in lstm.named_parameters()}
    xo = x.double().requires_grad_(True)
    yo = LO.lstm_forward(xo, P, 1)
    (yo * gy.double()).sum().backward()
    pc = [p.detach().cuda().requires_grad_(True) for p in params]
    xc = x.cuda().requires_grad_(True)
    y = ops.LstmLayerFn.apply(xc, *pc)
    (y * gy.cuda()).sum().backward()
    assert calls.of("ganffn_lstm") == {"ganffn_lstm_batch_layer_fwd": 1, "ganffn_lstm_batch_layer_bwd": 1}
    keys = names + [n + "_reverse" for n in names]
    r = [rel(y, yo), rel(xc.grad, xo.grad)] + [rel(t.grad, P[k].grad) for k, t in zip(keys, pc)]
    print("lstm layer (%d, %d, %d, %d): out %.1e dx %.1e worst parameter gradient %.1e" % (S, B, In, H, r[0], r[1], max(r[2:])))
    assert r[0] < 2e-6 and r[1] < 2e-5 and max(r[2:]) < 3e-5
    xc2 = x.cuda().requires_grad_(True)                # deterministic: the same call again gives the same bits
    pc2 = [p.detach().cuda().requires_grad_(True) for p in params]
    y2 = ops.LstmLayerFn.apply(xc2, *pc2)
    (y2 * gy.cuda()).sum().backward()
    assert torch.equal(y2, y) and torch.equal(xc2.grad, xc.grad)
    for a, b in zip(pc, pc2):
        assert torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("S,B,train", [(33, 64, True), (12, 100, False), (12, 100, True), (8, 256, True)])
def test_four_layer_stack_matches_oracle_with_the_same_dropout_masks(S, B, train):
    """tests/test_hip_lstm.test_four_layer_stack_matches_oracle_with_the_same_dropout_masks above 32 dialogues: the inter-layer
    masks are rows t*B + b of the whole batch"""
    from gan_ffn_amd import ops
    from test_hip_lstm import make_lstm
    In, H, L, p = 600, 300, 4, 0.5
    lstm = make_lstm(In, H, L, seed=11, dropout=p)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(S, B, In, generator=g) * 0.5
    gy = torch.randn(S, B, 2 * H, generator=g)
    seed = 424242
    P = {k: v.detach().double().requires_grad_(True) for k, v in lstm.named_parameters()}
    xo = x.double().requires_grad_(True)
    yo = LO.lstm_forward(xo, P, L, p, rng=O.Rng(seed, 0, train))
    (yo * gy.double()).sum().backward()
    m = lstm.cuda()
    m.train(train)
    ops.manual_seed(seed)
    xc = x.cuda().requires_grad_(True)
    y = ops.lstm_forward(xc, m, train)
    (y * gy.cuda()).sum().backward()
    r = [rel(y, yo), rel(xc.grad, xo.grad), max(rel(v.grad, P[k].grad) for k, v in m.named_parameters())]
    print("lstm stack (%d, %d) train %d: out %.1e dx %.1e worst parameter gradient %.1e" % (S, B, train, *r))
    assert r[0] < 1e-5 and r[1] < 1e-4 and r[2] < 2e-4


@pytest.mark.parametrize("nn", [0, 1])
@pytest.mark.parametrize("M,N,K", [(33, 1500, 500), (64, 500, 1500), (100, 300, 100), (256, 1500, 500), (256, 500, 1500), (97, 52, 36)])
def test_skinny_products_with_dialogue_tiles(nn, M, N, K):
    """the tiled skinny products against fp64 matmul (tests/test_hip_drnn_kernel.test_skinny_products' bound), and the tile
    property: every row has the bits the one-tile launch gives for the 32-row slice it lies in"""
    from gan_ffn_amd import _lib, ops
    g = torch.Generator().manual_seed(M * 7 + N + K + nn)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(8, K, N, generator=g) if nn else torch.randn(8, N, K, generator=g)
    Ad, Wd = A.cuda(), W.cuda().contiguous()
    Cd = torch.full((8, M, N), float("nan"), device="cuda")
    _lib.call("ganffn_drnn_skinny_batch", nn, 8, ops._ptr(Ad), ops._ptr(Wd), ops._ptr(Cd), M, N, K, ops._stream())
    for i in range(8):
        ref = A.double() @ (W[i].double() if nn else W[i].double().T)
        assert float((Cd[i].cpu().double() - ref).abs().max() / ref.abs().max()) < 3e-6 * max(1.0, K ** 0.5)
    for m0 in range(0, M, 32):
        m1 = min(M, m0 + 32)
        As = Ad[m0:m1].contiguous()
        Cs = torch.full((8, m1 - m0, N), float("nan"), device="cuda")
        _lib.call("ganffn_drnn_skinny", nn, 8, ops._ptr(As), ops._ptr(Wd), ops._ptr(Cs), m1 - m0, N, K, ops._stream())
        assert torch.equal(Cs, Cd[:, m0:m1]), (m0, m1)


@pytest.mark.parametrize("listener", [False, True])
def test_eval_rows_do_not_depend_on_the_other_dialogues_of_the_call(listener):
    """eval mode: dialogue b of a 64-dialogue call has the bits of the same dialogue in a 32-dialogue call (either half), emotions
    and attention maps — every per-dialogue sum is formed in the order of the 32-dialogue launch"""
    S, B, P = 17, 64, 9
    U, qmask = make_inputs(S, B, P, seed=5)
    m = build(listener).cuda().eval()
    with torch.no_grad():
        e, alpha = m(U.cuda(), qmask.cuda())
        for b0 in (0, 32):
            e_h, alpha_h = m(U[:, b0:b0 + 32].contiguous().cuda(), qmask[:, b0:b0 + 32].contiguous().cuda())
            assert torch.equal(e[:, b0:b0 + 32], e_h), b0
            for a, ah in zip(alpha, alpha_h):
                assert torch.equal(a[b0:b0 + 32], ah), b0
    assert float(e.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------
# 3. one native call per forward
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n", [(100, 1), (MAX_DIALOGUES, 1), (300, 2), (20, 0)])
def test_one_batch_call_per_bimodel_forward(B, n, monkeypatch):
    from gan_ffn_amd import dialogue_rnn as DR
    calls = _Calls(monkeypatch)
    torch.manual_seed(4)
    m = DR.BiModel(D_m=100, D_g=500, D_p=500, D_e=100, D_h=100, n_classes=6, context_attention="general", listener_state=False,
                   dropout_rec=0.1, dropout=0.6).cuda().train()

    def refuse(*a, **k):
        raise AssertionError("DialogueRNNCell.forward called: the recurrence ran on torch ops")
    monkeypatch.setattr(DR.DialogueRNNCell, "forward", refuse)
    U, qmask = make_inputs(7, B, 2, seed=9)
    umask = (qmask.sum(2) > 0).float().t().contiguous()
    Ug = U.cuda().requires_grad_(True)
    lp = m(Ug, qmask.cuda(), umask.cuda())[0]
    rec = {k: v for k, v in calls.of("ganffn_drnn_").items() if "join" not in k}
    assert rec == ({"ganffn_drnn_batch_fwd": n} if n else {"ganffn_drnn_fwd": 1}), rec
    lp.sum().backward()
    rec = {k: v for k, v in calls.of("ganffn_drnn_").items() if "join" not in k}
    assert rec == ({"ganffn_drnn_batch_fwd": n, "ganffn_drnn_batch_bwd": n} if n else {"ganffn_drnn_fwd": 1, "ganffn_drnn_bwd": 1}), rec
    assert torch.isfinite(Ug.grad).all() and float(Ug.grad.abs().max()) > 0


@pytest.mark.parametrize("B,n", [(100, 1), (300, 2), (32, 0)])
def test_one_batch_call_per_lstm_layer(B, n, monkeypatch):
    from gan_ffn_amd import dialogue_rnn as DR
    calls = _Calls(monkeypatch)
    torch.manual_seed(5)
    m = DR.MELDLSTMModel(600, 300, 600, n_classes=7, dropout=0.0).cuda().eval()
    with torch.no_grad():
        lp = m(torch.rand(5, B, 600, device="cuda"), None, torch.ones(B, 5, device="cuda"))[0]
    assert calls.of("ganffn_lstm") == ({"ganffn_lstm_batch_layer_fwd": 4 * n} if n else {"ganffn_lstm_layer_fwd": 4})
    assert lp.shape == (5, B, 7) and bool(torch.isfinite(lp).all())


# ------------------------------------------------------------------------------------------------------------------
# 4. B <= 32 through the _batch_ entry points is the existing entry points, bit for bit
# ------------------------------------------------------------------------------------------------------------------
def _run_drnn(cell, U, qmask, gy, fam, train):
    """one direction through ganffn_drnn_<fam>_fwd / _bwd (fam: party | batch), forward and backward -> every output, the saved
    block included"""
    from gan_ffn_amd import _lib, ops
    att, listener = ops.drnn_att_type(cell), bool(cell.listener_state)
    Ux, params = ops._drnn_cell_args(cell, U)
    Ux, params = Ux.contiguous(), [p.detach().contiguous() for p in params]
    S, B, Dm = Ux.shape
    P = qmask.size(2)
    n_att = len(ops.DRNN_ATT_KEYS[att])
    assert att != "simple"
    prm = params[:12] + [None]                   # (general: transform.weight goes in as the attention's own parameter)
    aprm, att_c = params[12:12 + n_att], att
    lprm = params[12 + n_att:] if listener else None
    spk64 = torch.argmax(qmask, 2)
    mval = qmask.gather(2, spk64.unsqueeze(2)).squeeze(2).contiguous()
    spk = spk64.to(torch.int32).contiguous()
    cfg = _lib.DrnnCfg(S, B, Dm, cell.D_g, cell.D_e, float(cell.dropout.p) if train else 0.0, 1 if train else 0)
    acfg = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att_c], int(cell.attention.transform.weight.shape[0]) if att == "concat" else 0)
    lib = _lib.load()
    ns = getattr(lib, "ganffn_drnn_%s_saved_floats" % fam)(C.byref(cfg), C.byref(acfg), int(listener), P)
    nw = getattr(lib, "ganffn_drnn_%s_workspace_floats" % fam)(C.byref(cfg), C.byref(acfg), int(listener), P)
    assert ns > 0 and nw > 0
    dev = U.device
    sv, ws = torch.zeros(ns, device=dev), torch.zeros(nw, device=dev)
    e, al = torch.empty(S, B, cell.D_e, device=dev), torch.empty(B, S, S, device=dev)
    A = ops._ptr_array
    P1 = (_lib.DrnnPtrs * 1)(ops._drnn_ptrs(prm))
    LP = (_lib.DrnnListenerPtrs * 1)(ops._drnn_ptrs(lprm, _lib.DrnnListenerPtrs)) if listener else None
    AP = (_lib.DrnnAttPtrs * 1)(ops._att_ptrs(att_c, aprm))
    rng = ops.DeviceRng.get(dev).state
    ops.manual_seed(SEED)
    _lib.call("ganffn_drnn_%s_fwd" % fam, C.byref(cfg), C.byref(acfg), P, 1, A([Ux]), A([spk]), A([mval]), P1, LP, AP, A([e]), A([al]),
              A([sv]), A([ws]), ops._ptr(rng), C.c_uint64(0), ops._stream())
    saved_fwd = sv.clone()
    dU = torch.empty_like(Ux)
    grads = [torch.zeros_like(t) if t is not None else None for t in prm]
    agr = [torch.zeros_like(t) for t in aprm]
    lgr = [torch.zeros_like(t) for t in lprm] if listener else []
    G1 = (_lib.DrnnPtrs * 1)(ops._drnn_ptrs(grads))
    AG = (_lib.DrnnAttPtrs * 1)(ops._att_ptrs(att_c, agr))
    LG = (_lib.DrnnListenerPtrs * 1)(ops._drnn_ptrs(lgr, _lib.DrnnListenerPtrs)) if listener else None
    _lib.call("ganffn_drnn_%s_bwd" % fam, C.byref(cfg), C.byref(acfg), P, 1, A([gy.contiguous()]), A([Ux]), A([spk]), A([mval]), P1, LP, AP,
              G1, LG, AG, A([dU]), A([al]), A([sv]), A([ws]), ops._ptr(rng), C.c_uint64(0), ops._stream())
    torch.cuda.synchronize()
    return [e, al, saved_fwd, dU] + [g for g in grads if g is not None] + agr + lgr


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("att,listener,P,B", [("general", False, 2, 32), ("general", True, 9, 30), ("concat", True, 2, 6), ("general2", False, 9, 17)])
def test_batch_entry_points_up_to_32_dialogues_equal_the_party_ones(att, listener, P, B, train):
    m = build(listener, att).cuda()
    S = 23
    U, qmask = make_inputs(S, B, P, seed=5)
    U, qmask = U.cuda(), qmask.cuda()
    gy = (torch.rand(S, B, 100, generator=torch.Generator().manual_seed(2)) - 0.5).cuda()
    with torch.no_grad():
        old = _run_drnn(m.dialogue_cell, U, qmask, gy, "party", train)
        new = _run_drnn(m.dialogue_cell, U, qmask, gy, "batch", train)
    assert len(old) == len(new) >= 16
    for i, (a, b) in enumerate(zip(old, new)):
        assert torch.equal(a, b), i
    assert float(old[3].abs().max()) > 0


@pytest.mark.parametrize("train", [False, True])
def test_lstm_batch_entry_points_up_to_32_dialogues_equal_the_existing_ones(train):
    """the per-layer pair and the stack pair: outputs, saved blocks, dx and all 32 parameter gradients, torch.equal"""
    from gan_ffn_amd import _lib, ops
    S, B, In, H, L, p = 21, 32, 600, 300, 4, 0.6
    torch.manual_seed(4)
    lstm = torch.nn.LSTM(In, H, num_layers=L, bidirectional=True, dropout=p).cuda()
    names = [k for k, _ in lstm.named_parameters()]
    Pd = {k: v.detach() for k, v in lstm.named_parameters()}
    x = torch.rand(S, B, In, device="cuda") - 0.5
    dy = torch.randn(S, B, 2 * H, device="cuda")
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    col = lambda j, src: [src[names[4 * i + j]] for i in range(2 * L)]
    lib = _lib.load()
    rng = ops.DeviceRng.get(x.device)
    ops.manual_seed(SEED)
    res = {}
    for fam in ("ganffn_lstm_stack_", "ganffn_lstm_stack_batch_"):
        cfg = _lib.LstmStackCfg(S, B, In, H, L, p, 1 if train else 0)
        n_saved, n_ws = int(getattr(lib, fam + "saved_floats")(C.byref(cfg))), int(getattr(lib, fam + "workspace_floats")(C.byref(cfg)))
        saved, ws = torch.zeros(n_saved, device="cuda"), torch.zeros(n_ws, device="cuda")
        out, dx = torch.empty(S, B, 2 * H, device="cuda"), torch.empty(S, B, In, device="cuda")
        G = {k: torch.zeros_like(v) for k, v in Pd.items()}
        _lib.call(fam + "fwd", C.byref(cfg), ops._ptr(x), arr(col(0, Pd)), arr(col(1, Pd)), arr(col(2, Pd)), arr(col(3, Pd)), ops._ptr(out),
                  ops._ptr(saved), ops._ptr(ws), ops._ptr(rng.state), C.c_uint64(7), ops._stream())
        _lib.call(fam + "bwd", C.byref(cfg), ops._ptr(dy), ops._ptr(x), ops._ptr(out), arr(col(0, Pd)), arr(col(1, Pd)), ops._ptr(dx),
                  arr(col(0, G)), arr(col(1, G)), arr(col(2, G)), arr(col(3, G)), ops._ptr(saved), ops._ptr(ws), ops._ptr(rng.state),
                  C.c_uint64(7), ops._stream())
        torch.cuda.synchronize()
        res[fam] = [out, saved, dx] + [G[k] for k in names]
    for i, (a, b) in enumerate(zip(*res.values())):
        assert torch.equal(a, b), i
    assert float(res["ganffn_lstm_stack_"][2].abs().max()) > 0
    # one layer
    res = {}
    for fam in ("ganffn_lstm_", "ganffn_lstm_batch_"):
        cfg = _lib.LstmCfg(S, B, In, H)
        n_saved, n_ws = int(getattr(lib, fam + "saved_floats")(C.byref(cfg))), int(getattr(lib, fam + "workspace_floats")(C.byref(cfg)))
        saved, ws = torch.zeros(n_saved, device="cuda"), torch.zeros(n_ws, device="cuda")
        out, dx = torch.empty(S, B, 2 * H, device="cuda"), torch.empty(S, B, In, device="cuda")
        G = {k: torch.zeros_like(Pd[k]) for k in names[:8]}
        w = lambda j, src: [src[names[j]], src[names[4 + j]]]
        _lib.call(fam + "layer_fwd", C.byref(cfg), ops._ptr(x), arr(w(0, Pd)), arr(w(1, Pd)), arr(w(2, Pd)), arr(w(3, Pd)), ops._ptr(out),
                  ops._ptr(saved), ops._ptr(ws), ops._stream())
        _lib.call(fam + "layer_bwd", C.byref(cfg), ops._ptr(dy), ops._ptr(x), ops._ptr(out), arr(w(0, Pd)), arr(w(1, Pd)), ops._ptr(dx),
                  arr(w(0, G)), arr(w(1, G)), arr(w(2, G)), arr(w(3, G)), ops._ptr(saved), ops._ptr(ws), ops._stream())
        torch.cuda.synchronize()
        res[fam] = [out, saved, dx] + [G[k] for k in names[:8]]
    for i, (a, b) in enumerate(zip(*res.values())):
        assert torch.equal(a, b), i


# ------------------------------------------------------------------------------------------------------------------
# 5. the step runners
# ------------------------------------------------------------------------------------------------------------------
def test_drnn_engine_train_steps_at_64_dialogues_match_fp64_oracle():
    """DrnnEngine(max_dialogues=64) at (94, 64), dropout at the reference script's values, two consecutive steps from the captured
    pre-step state: tests/engine_oracle.drnn_step with the engine's Philox masks on the engine's ReLU patterns — loss 2e-5, log_prob
    1e-4, every head gradient tensor 1e-3 of its scale, no outliers — and Adam elementwise on every slab
    (tests/test_hip_classifier_engines_train_oracle's bounds and _check_adam)"""
    import engine_oracle as EO
    import test_hip_classifier_engines_train_oracle as TO
    from gan_ffn_amd import engine as E, ops
    from util import relu_masks
    S, B = 94, 64
    net = TO._drnn_net(False)
    eng = E.DrnnEngine(net, lr=TO.DRNN_LR, weight_decay=TO.DRNN_L2, class_weights=TO.W, max_dialogues=64)
    names = {id(p): n for n, p in net.named_parameters()}
    hnames = [names[id(p)][len("bi_model."):] for p in eng._hparams]
    bm = copy.deepcopy(net.bi_model).cpu().double()
    slabs = TO._gen_slabs(eng, TO.DRNN_LR, TO.DRNN_L2) + [
        TO._Slab("head", eng.h_slab, eng.h_grad, eng.h_m, eng.h_v, eng.h_step, TO.DRNN_LR, TO.DRNN_L2,
                 [(o, p.numel()) for o, p in zip(eng._hoffs, eng._hparams)])]
    ops.manual_seed(TO.SEED)
    for i in range(2):
        batch = TO._batch(S, B, 100 * S + B + i)
        torch.cuda.synchronize()
        pre = [sl.host() for sl in slabs]
        loss, _ = eng.step(batch, train=True)
        torch.cuda.synchronize()
        post = [sl.host(grad=True) for sl in slabs]
        assert eng._shape == (S, B, 2)
        b = eng._base_add
        T, f = S * B, eng._f
        hb = TO._host_batch(batch)
        with torch.no_grad():
            params = dict(bm.named_parameters())
            for n, o, p in zip(hnames, eng._hoffs, eng._hparams):
                params[n].copy_(pre[3]["slab"][o:o + p.numel()].view(p.shape).double())
        gens = {k: EO.Net.from_state(eng.G[k], pre[j]["slab"]) for j, k in enumerate(EO.GEN_KEYS)}
        masks_g = {k: relu_masks(eng.pass_G[k], eng.pass_G[k].cfg_train, S, B) for k in EO.GEN_KEYS}
        pattern = f["hidden"][:T * eng.Dh2].view(S, B, eng.Dh2).cpu().double() > 0
        ch = EO.drnn_step(gens, bm, hb, TO.SEED, b, True, relu_masks=masks_g, hidden_pattern=pattern, class_w=TO.W)
        tag = "max_dialogues 64, step %d (%d, %d)" % (i, S, B)
        print("%s: loss %.7f oracle %.7f" % (tag, float(loss), ch["loss"]))
        assert abs(float(loss) - ch["loss"]) < 2e-5 * abs(ch["loss"]), (float(loss), ch["loss"])
        TO._close("log_prob", f["log_prob"][:T * 6].view(S, B, 6).cpu().double(), ch["log_prob"], 1e-4, 0.0, tag + " log_prob")
        hg = post[3]["grad"]
        for n, o, p in zip(hnames, eng._hoffs, eng._hparams):
            TO._close("head gradient", hg[o:o + p.numel()].view(p.shape).double(), ch["grads"][n], 1e-3, 1e-12, "%s grad %s" % (tag, n))
        TO._close("d_fusion", f["dU_f"][:T * eng.Dm].view(S, B, eng.Dm).cpu().double(), ch["d_fusion"], 1e-3, 1e-12, tag + " d_fusion")
        for sl, a, z in zip(slabs, pre, post):
            TO._check_adam(sl, a, z, tag)
    print("largest error / tolerance per check: " + ", ".join("%s %.3g" % kv for kv in sorted(TO.WORST.items())))


def test_meld_engine_train_steps_at_100_dialogues_match_fp64_oracle():
    """MeldEngine(max_dialogues=128) at (33, 100), dropout 0.6, three consecutive steps:
    tests/test_hip_meld_engine.test_train_mode_step_matches_fp64_oracle_with_the_engines_masks' comparison and bounds (log_prob, the
    loss and every gradient element 1e-3 of scale; Adam elementwise)"""
    import meld_step_oracle as MO
    import test_hip_classifier_engines_train_oracle as TO
    from gan_ffn_amd import engine as E, ops
    from test_hip_meld_engine import L2, LR, dist, engine_grads, engine_named, mirror, random_batch
    S, B, Cn = 33, 100, 7
    net = mirror(Cn, dropout=0.6, formula=False, seed=7)
    b = random_batch(S, B, Cn, seed=9)
    ops.manual_seed(SEED)
    eng = E.MeldEngine(net, lr=LR, weight_decay=L2, max_dialogues=128)
    names = engine_named(eng)
    assert names == MO.trained_names()
    sl = TO._Slab("meld", eng.slab, eng.grad, eng.exp_avg, eng.exp_avg_sq, eng.step_count, LR, L2,
                  [(o, p.numel()) for o, p in zip(eng._offs, eng._params)])
    text, umask, label = b["text"].cpu().numpy(), b["umask"].cpu().numpy(), b["label"].cpu().numpy()
    for i in range(3):
        pre = sl.host()
        P = {k: eng._p(j).view_as(eng._params[j]).detach().cpu().numpy().copy() for j, k in enumerate(names)}
        loss, lp = eng.step(b, train=True)
        torch.cuda.synchronize()
        post = sl.host(grad=True)
        base = eng._base_add
        offsets = [base + l for l in range(eng.L - 1)]
        seed = int(ops.DeviceRng.get(eng.dev).state.cpu()[0])
        o = MO.step(P, text, umask, label, 0.6, seed=seed, offsets=offsets, train=True)
        d_lp, d_loss = dist(lp.cpu().numpy(), o["log_prob"]), abs(float(loss) - o["loss"]) / abs(o["loss"])
        g_e = engine_grads(eng)
        worst = max((dist(g_e[k], o["grads"][k]), k) for k in names)
        print("meld max_dialogues 128, step %d: log_prob %.2e loss %.2e worst gradient %.2e (%s)" % (i, d_lp, d_loss, *worst))
        assert d_lp <= 1e-3 and d_loss <= 1e-3 and worst[0] <= 1e-3
        TO._check_adam(sl, pre, post, "meld step %d" % i)


def test_engine_eval_steps_equal_the_module_paths_eval_forward():
    """eval: the engines run the launches of the module path above 32 dialogues too — the same bits"""
    from gan_ffn_amd import engine as E
    from test_hip_classifier_engines_train_oracle import W, _batch, _drnn_net
    from test_hip_meld_engine import mirror, module_step, random_batch
    net = mirror(7, dropout=0.6, formula=False, seed=11)
    eng = E.MeldEngine(net, max_dialogues=128)
    b = random_batch(33, 100, 7)
    loss, lp = eng.step(b, train=False)
    net.eval()
    with torch.no_grad():
        loss_m, lp_m, alpha_m = module_step(net, b)
    print("meld eval (33, 100): loss %.2e log_prob %.2e alpha %.2e" % (abs(float(loss) - float(loss_m)), rel(lp, lp_m), rel(eng.alpha, alpha_m)))
    assert abs(float(loss) - float(loss_m)) < 2e-5 * abs(float(loss_m)) and rel(lp, lp_m) < 1e-4 and rel(eng.alpha, alpha_m) < 1e-4
    assert int(eng.step_count.item()) == 0
    dnet = _drnn_net(False)
    deng = E.DrnnEngine(dnet, class_weights=W, max_dialogues=64)
    db = _batch(40, 64, 7)
    dloss, dlp = deng.step(db, train=False)
    dnet.eval()
    with torch.no_grad():
        lp_ref = dnet(db["acoustic"], db["visual"], db["text"], db["qmask"], db["umask"])[0]
    print("drnn eval (40, 64): log_prob %.2e" % rel(dlp, lp_ref))
    assert rel(dlp, lp_ref) < 1e-4 and bool(torch.isfinite(dloss).all())


def test_capacity_limits():
    from gan_ffn_amd import engine as E
    from test_hip_classifier_engines_train_oracle import _batch, _drnn_net
    from test_hip_meld_engine import mirror, random_batch
    net = mirror(7, formula=False)
    for n in (MAX_DIALOGUES + 1, 31):
        with pytest.raises(ValueError, match="max_dialogues"):
            E.MeldEngine(mirror(7, formula=False), max_dialogues=n)
    eng = E.MeldEngine(net)                                           # the default capacity still refuses 33 dialogues
    before = eng.slab.clone()
    with pytest.raises(ValueError, match="module path"):
        eng.step(random_batch(5, 33, 7), train=True)
    with pytest.raises(ValueError, match="module path"):
        eng.reserve(33, 33)
    assert int(eng.step_count.item()) == 0 and torch.equal(eng.slab, before) and eng._shape is None
    eng64 = E.MeldEngine(mirror(7, formula=False), max_dialogues=64)
    with pytest.raises(ValueError, match="module path"):
        eng64.step(random_batch(5, 65, 7), train=True)
    eng64.reserve(33, 64)
    eng64.step(random_batch(5, 64, 7), train=True)
    ptrs = {k: v.data_ptr() for k, v in eng64._f.items()}
    eng64.step(random_batch(9, 20, 7), train=True)                    # at most 32 dialogues: the existing entry points, same buffers
    eng64.step(random_batch(33, 33, 7), train=True)
    torch.cuda.synchronize()
    assert {k: v.data_ptr() for k, v in eng64._f.items()} == ptrs and int(eng64.step_count.item()) == 3
    dnet = _drnn_net(False)
    with pytest.raises(ValueError, match="max_dialogues"):
        E.DrnnEngine(dnet, max_dialogues=MAX_DIALOGUES + 1)
    deng = E.DrnnEngine(dnet)
    with pytest.raises(ValueError, match="module path"):
        deng.step(_batch(13, 33, 1), train=True)
    assert deng._shape is None


def test_the_capacity_is_not_a_switch(monkeypatch):
    """a batch of at most 32 dialogues takes the existing entry points whatever the capacity is, and gives the bits of a default engine"""
    from gan_ffn_amd import engine as E, ops
    from test_hip_meld_engine import mirror, random_batch
    calls = _Calls(monkeypatch)
    b = random_batch(20, 32, 7)
    slabs = []
    for cap in (32, 256):
        ops.manual_seed(SEED)
        eng = E.MeldEngine(mirror(7, dropout=0.6, formula=False, seed=13), max_dialogues=cap)
        for _ in range(2):
            eng.step(b, train=True)
        torch.cuda.synchronize()
        slabs.append([t.clone() for t in (eng.slab, eng.grad, eng.exp_avg, eng.loss)])
    for t0, t1 in zip(*slabs):
        assert torch.equal(t0, t1)
    assert calls.of("ganffn_lstm") == {"ganffn_lstm_stack_fwd": 4, "ganffn_lstm_stack_bwd": 4}
    eng.step(random_batch(20, 40, 7), train=True)
    assert calls.of("ganffn_lstm_stack_batch") == {"ganffn_lstm_stack_batch_fwd": 1, "ganffn_lstm_stack_batch_bwd": 1}


def test_two_engines_same_seed_are_bit_identical_at_100_dialogues():
    from gan_ffn_amd import engine as E, ops
    from test_hip_classifier_engines_train_oracle import W, _batch, _drnn_net
    from test_hip_meld_engine import mirror, random_batch
    b = random_batch(33, 100, 7)
    slabs = []
    for _ in range(2):
        ops.manual_seed(SEED)
        eng = E.MeldEngine(mirror(7, dropout=0.6, formula=False, seed=13), max_dialogues=128)
        for _ in range(3):
            eng.step(b, train=True)
        torch.cuda.synchronize()
        slabs.append([t.clone() for t in (eng.slab, eng.grad, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.loss)])
    for t0, t1 in zip(*slabs):
        assert torch.equal(t0, t1)
    db = _batch(30, 100, 3)
    slabs = []
    for _ in range(2):
        ops.manual_seed(SEED)
        deng = E.DrnnEngine(_drnn_net(True), class_weights=W, max_dialogues=128)
        for _ in range(3):
            deng.step(db, train=True)
        torch.cuda.synchronize()
        slabs.append([t.clone() for t in (deng.h_slab, deng.h_grad, deng.h_m, deng.h_v, deng.loss)] + [deng.G[k].slab.clone() for k in deng.G])
    for t0, t1 in zip(*slabs):
        assert torch.equal(t0, t1)


def test_run_meld_training_takes_a_batch_size_above_32(tmp_path, monkeypatch):
    """artifacts.run_meld_training(batch_size=64) builds its engine with the capacity and trains on it"""
    from gan_ffn_amd import artifacts as A, data as D
    calls = _Calls(monkeypatch)
    path = str(tmp_path / "meld.pkl")
    D.write_synthetic_meld_pickle(path, n_train=70, n_test=40, seed=5)
    A.run_meld_training(path, n_epochs=1, batch_size=64)
    n = calls.of("ganffn_lstm_stack")
    assert n.get("ganffn_lstm_stack_batch_fwd", 0) >= 2 and n.get("ganffn_lstm_stack_batch_bwd", 0) >= 1, n
