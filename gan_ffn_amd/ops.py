"""Tensor-level wrappers over libganffn.so: raw calls on torch CUDA(ROCm) tensors plus the
torch.autograd.Functions the nn.Modules in model.py are built from.

torch is plumbing here (device memory, streams, autograd bookkeeping); all arithmetic of the
hot path runs in the HIP library.  Every wrapper raises if the tensors are not on a GPU.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import EncCfg, HeadCfg, GanffnError

FF = 2048            # nn.TransformerEncoderLayer default dim_feedforward (reference passes none, model.py:1210)
ENC_DROPOUT = 0.1    # nn.TransformerEncoderLayer default dropout
PE_DROPOUT = 0.2     # PositionalEncoding default (model.py:1179)
LN_EPS = 1e-5
N_LAYERS = 8         # model.py:1212


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise GanffnError("GAN-FFN ops run only on an MI355X (HIP) device; got a %s tensor. "
                              "There is no CPU fallback." % t.device)


def _f32c(t):
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------------------------------------------
# RNG state (device-resident {seed, offset}; kernels read it at run time -> graph-replay safe)
# ----------------------------------------------------------------------------------------------
class DeviceRng:
    """Per-device Philox state.  `next_add()` hands out one unique offset per dropout-bearing call."""
    _states = {}

    def __init__(self, device, seed=3407):  # 3407: the reference's seed, train_IEMOCAP.py:46
        self.state = torch.tensor([seed, 0], dtype=torch.int64, device=device)
        self.counter = 0

    @classmethod
    def get(cls, device):
        key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
        if key not in cls._states:
            cls._states[key] = DeviceRng(torch.device("cuda", key))
        return cls._states[key]

    def manual_seed(self, seed, offset=0):
        self.state.copy_(torch.tensor([seed, offset], dtype=torch.int64))
        self.counter = 0

    def next_add(self, n=1):
        """reserve n consecutive dropout offsets: the allocator of this device's EAGER paths — the autograd/module path
        takes one per call, eager GanEngine / Phase2Engine iterations take one block each, so no two dropout-bearing
        eager launches of a process share a (seed, offset) pair.  A hipGraph-replayed engine (`use_graph=True`) cannot
        take host-side blocks (its launch arguments are frozen at capture): it advances the DEVICE-side offset instead,
        which every eager launch adds its host offset to — so masks of a graph-replayed engine and of eager calls issued
        on the same device in between may coincide (correlated masks, never wrong arithmetic).  Do not mix the two modes
        on one device where independent masks matter."""
        v = self.counter
        self.counter += n
        return v

    def state_dict(self):
        """{seed, offset, counter} — saved beside the checkpoints (artifacts.save_GAN_models) so that a resumed run
        continues the Philox stream instead of replaying the masks of the run it resumes"""
        seed, offset = [int(v) for v in self.state.cpu()]
        return {"seed": seed, "offset": offset, "counter": int(self.counter)}

    def load_state_dict(self, d):
        self.state.copy_(torch.tensor([int(d["seed"]), int(d["offset"])], dtype=torch.int64))
        self.counter = int(d["counter"])


def manual_seed(seed, device=None):
    DeviceRng.get(device if device is not None else torch.cuda.current_device()).manual_seed(seed)


# ----------------------------------------------------------------------------------------------
# layout helpers
# ----------------------------------------------------------------------------------------------
LAYER_KEYS = ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
              "self_attn.out_proj.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
              "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"]


def layer_shapes(E, F=FF):
    return [(3 * E, E), (3 * E,), (E, E), (E,), (F, E), (F,), (E, F), (E,), (E,), (E,), (E,), (E,)]


def layer_layout(E, F=FF):
    """-> (floats per layer, [12 offsets]) from the library (single source of truth)."""
    lib = _lib.load()
    offs = (C.c_int64 * 12)()
    _lib.check(lib.ganffn_layer_param_offsets(E, F, offs), "ganffn_layer_param_offsets")
    return int(lib.ganffn_layer_param_count(E, F)), [int(o) for o in offs]


def enc_cfg(S, B, E, H, L=N_LAYERS, F=FF, train=False, p_pe=PE_DROPOUT, p_enc=ENC_DROPOUT):
    return EncCfg(S, B, E, H, F, L, p_pe, p_enc, LN_EPS, 1 if train else 0)


def enc_sizes(cfg):
    lib = _lib.load()
    s = int(lib.ganffn_encoder_saved_floats(C.byref(cfg)))
    w = int(lib.ganffn_encoder_workspace_floats(C.byref(cfg)))
    if s < 0 or w < 0:
        _lib.check(-1, "ganffn_encoder_*_floats")
    return s, w


def head_cfg(T, E, D1, D2, kind, p=0.2, train=False):
    """kind 0: generator head, 1: discriminator head (include/ganffn.h ganffn_head_cfg)"""
    return HeadCfg(T, E, D1, D2, kind, p, 1 if train else 0)


def head_sizes(cfg):
    lib = _lib.load()
    s = int(lib.ganffn_head_saved_floats(C.byref(cfg)))
    w = int(lib.ganffn_head_workspace_floats(C.byref(cfg)))
    if s < 0 or w < 0:
        _lib.check(-1, "ganffn_head_*_floats")
    return s, w


# ----------------------------------------------------------------------------------------------
# raw calls (no autograd) — used by the autograd Functions below and by engine.py
# ----------------------------------------------------------------------------------------------
def key_lengths_from_umask(umask):
    """int32 [batch] utterance counts of a prefix mask [batch, seq_len], computed where umask lives (no host read): the key
    lengths of a mask_padding forward"""
    if umask is None:
        raise ValueError("mask_padding=True needs umask (batch, seq_len) to know every dialogue's length")
    return umask.sum(1).to(torch.int32)


def check_prefix_mask(umask, who):
    """GANFFN_CHECK_QMASK=1 (one host sync per batch): lengths are umask.sum(1) — a mask with holes would silently mask the
    wrong keys / steps"""
    S = umask.shape[1]
    L_ = umask.sum(1).long()
    if not bool((umask == (torch.arange(S, device=umask.device).unsqueeze(0) < L_.unsqueeze(1)).to(umask.dtype)).all()):
        raise ValueError("%s: umask rows must be prefixes (1 .. 1 0 .. 0)" % who)


def _check_key_len(key_len, cfg):
    if key_len.dtype != torch.int32 or not key_len.is_cuda or not key_len.is_contiguous() or key_len.numel() != cfg.B:
        raise ValueError("key_len must be a contiguous int32 device tensor with one entry per dialogue (%d)" % cfg.B)


ATTN_CAUSAL = 1                    # GANFFN_ATTN_CAUSAL


def encoder_fwd_raw(cfg, x, pe, slab, out, saved, ws, rng, add, key_len=None, causal=False):
    """ganffn_encoder_fwd_mask.  key_len (int32 device tensor [B], or None): the attention of every layer sees keys
    j < key_len[b] of dialogue b only; None (a null pointer) is the plain call.  causal=True (the GANFFN_ATTN_CAUSAL flag): query i
    sees keys j <= i as well, with or without lengths — row t of the output then depends on rows 0 .. t of x alone."""
    if key_len is not None:
        _check_key_len(key_len, cfg)
    _lib.call("ganffn_encoder_fwd_mask", C.byref(cfg), _ptr(key_len), C.c_uint32(ATTN_CAUSAL if causal else 0), _ptr(x), _ptr(pe),
              _ptr(slab), _ptr(out), _ptr(saved), _ptr(ws), _ptr(rng), C.c_uint64(add), _stream())


def stream_sizes(cfg, n_max):
    """(K/V cache floats, workspace floats for steps of up to n_max rows) of a streamed stack; cfg describes the cache:
    cfg.S = positions per slot, cfg.B = slots, eval (ganffn_stream_cache_floats / ganffn_stream_workspace_floats)"""
    lib = _lib.load()
    c = int(lib.ganffn_stream_cache_floats(C.byref(cfg)))
    w = int(lib.ganffn_stream_workspace_floats(C.byref(cfg), n_max)) if c >= 0 else -1
    if c < 0 or w < 0:
        _lib.check(-1, "ganffn_stream_*_floats")
    return c, w


def encoder_stream_step_raw(cfg, n, slot, pos, x, pe, slab, cache, out, ws):
    """one streaming step of an encoder stack (ganffn_encoder_stream_step; no autograd, eval math): row i of x [n x E] is the
    next utterance of the dialogue in cache slot slot[i] (int32 device tensor [n], distinct), at position pos[slot[i]] (int32
    device tensor [cfg.B], read only: the caller advances it).  Appends the row's K / V to every layer's cache and writes the
    stack's output for the row to out [n x E]."""
    for t, k in ((slot, n), (pos, cfg.B)):
        if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.numel() < k:
            raise ValueError("slot / pos must be contiguous int32 device tensors with %d / %d entries" % (n, cfg.B))
    _need_gpu(x, pe, slab, cache, out, ws)
    _lib.call("ganffn_encoder_stream_step", C.byref(cfg), n, _ptr(slot), _ptr(pos), _ptr(x), _ptr(pe), _ptr(slab), _ptr(cache),
              _ptr(out), _ptr(ws), _stream())


STREAM_EXTEND_MAX_ROWS = 110 * 32      # rows of one ganffn_encoder_stream_extend call from StreamSession.extend: the flagship
                                       # training shape's row count, for which the row-wise kernels are exercised


def stream_extend_sizes(cfg, rows_max):
    """workspace floats of ganffn_encoder_stream_extend calls of up to rows_max = m * n rows (cfg describes the cache, as for
    stream_sizes; ganffn_stream_extend_workspace_floats)"""
    w = int(_lib.load().ganffn_stream_extend_workspace_floats(C.byref(cfg), int(rows_max)))
    if w < 0:
        _lib.check(-1, "ganffn_stream_extend_workspace_floats")
    return w


def encoder_stream_extend_raw(cfg, n, m, slot, count, pos, x, pe, slab, cache, out, ws):
    """several new utterances per dialogue through an encoder stack (ganffn_encoder_stream_extend; no autograd, eval math):
    x [m x n x E], time-major — chunk i holds count[i] <= m new rows of the dialogue in cache slot slot[i] (int32 device tensors
    [n]; slots distinct), at positions pos[slot[i]] .. + count[i] - 1 (pos: int32 device tensor [cfg.B], read only: the caller
    advances it by count).  Appends the rows' K / V to every layer's cache and writes the stack's output to out [m x n x E]; rows
    j >= count[i] of x must be finite and their out rows are meaningless.  ws: stream_extend_sizes(cfg, rows_max >= m * n)."""
    for t, k in ((slot, n), (count, n), (pos, cfg.B)):
        if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.numel() < k:
            raise ValueError("slot / count / pos must be contiguous int32 device tensors with %d / %d / %d entries" % (n, n, cfg.B))
    _need_gpu(x, pe, slab, cache, out, ws)
    _lib.call("ganffn_encoder_stream_extend", C.byref(cfg), n, m, _ptr(slot), _ptr(count), _ptr(pos), _ptr(x), _ptr(pe), _ptr(slab),
              _ptr(cache), _ptr(out), _ptr(ws), C.c_int64(ws.numel()), _stream())


def encoder_fwd_pair_supported(cfg):
    """can the eval-mode and the train-mode forward of this configuration share their launches (ganffn_encoder_fwd_pair)?"""
    return int(_lib.load().ganffn_encoder_fwd_pair_supported(C.byref(cfg))) == 1


def encoder_fwd_pair_workspace_floats(cfg):
    w = int(_lib.load().ganffn_encoder_fwd_pair_workspace_floats(C.byref(cfg)))
    if w < 0:
        _lib.check(-1, "ganffn_encoder_fwd_pair_workspace_floats")
    return w


def encoder_fwd_pair_raw(cfg, x, pe, slab, out_eval, out_train, saved_train, ws, rng, add_train, key_len=None, causal=False):
    """cfg: the train-mode cfg.  out_eval = the eval-mode forward of x (nothing kept), out_train / saved_train = the
    train-mode forward with its saved set — one pass, the bits of the two encoder_fwd_raw calls (ganffn_encoder_fwd_pair_mask).
    key_len (int32 device tensor [B], or None for a null pointer): the lengths of the B dialogues, for both segments.
    causal=True (the GANFFN_ATTN_CAUSAL flag): both segments under the causal mask, as encoder_fwd_raw(causal=True) twice."""
    if key_len is not None:
        _check_key_len(key_len, cfg)
    _lib.call("ganffn_encoder_fwd_pair_mask", C.byref(cfg), _ptr(key_len), C.c_uint32(ATTN_CAUSAL if causal else 0), _ptr(x), _ptr(pe),
              _ptr(slab), _ptr(out_eval), _ptr(out_train), _ptr(saved_train), _ptr(ws), _ptr(rng), C.c_uint64(add_train), _stream())


def encoder_bwd_raw(cfg, lo, hi, dx, slab, gslab, saved, ws, rng, add, need_dx_in=True, key_len=None, causal=False):
    """need_dx_in=False: the stack's input needs no gradient — with lo == 0 the bottom in-proj dgrad and the PE dropout
    backward are skipped (as autograd skips them) and dx is undefined afterwards.  key_len, causal: what the forward was given
    (ganffn_encoder_bwd_mask: a null pointer for None, the GANFFN_ATTN_CAUSAL flag for causal)."""
    if key_len is not None:
        _check_key_len(key_len, cfg)
    _lib.call("ganffn_encoder_bwd_mask", C.byref(cfg), _ptr(key_len), C.c_uint32(ATTN_CAUSAL if causal else 0), lo, hi, _ptr(dx),
              _ptr(slab), _ptr(gslab), _ptr(saved), _ptr(ws), _ptr(rng), C.c_uint64(add), 1 if need_dx_in else 0, _stream())


def encoder_bwd_parts_supported(cfg):
    """does the whole-stack backward of this configuration leave its weight gradients unreduced (ganffn_encoder_bwd_parts)?"""
    return int(_lib.load().ganffn_encoder_bwd_parts_supported(C.byref(cfg))) == 1


def encoder_bwd_parts_raw(cfg, dx, slab, gslab, saved, ws, rng, add, need_dx_in=True, key_len=None, causal=False):
    """whole-stack backward with unreduced weight gradients -> (parts tensor view into ws or None, part_stride, n_parts, offset
    of the parts in ws): hand them to adam_step_parts_raw before anything else touches ws[offset:].  key_len, causal: what the
    forward was given (ganffn_encoder_bwd_parts_mask: a null pointer for None, the GANFFN_ATTN_CAUSAL flag for causal)."""
    off, stride, n = C.c_int64(0), C.c_int64(0), C.c_int(0)
    if key_len is not None:
        _check_key_len(key_len, cfg)
    _lib.call("ganffn_encoder_bwd_parts_mask", C.byref(cfg), _ptr(key_len), C.c_uint32(ATTN_CAUSAL if causal else 0), _ptr(dx), _ptr(slab),
              _ptr(gslab), _ptr(saved), _ptr(ws), _ptr(rng), C.c_uint64(add), 1 if need_dx_in else 0, C.byref(off), C.byref(stride),
              C.byref(n), _stream())
    return (ws[off.value:] if n.value > 1 else None), stride.value, n.value, off.value


def adam_step_parts_raw(p, g, m, v, step, n, lr, b1, b2, parts, part_stride, n_parts, enc_floats, layer_floats, covered, eps=1e-8,
                        wd=0.0, gscale=1.0):
    _lib.call("ganffn_adam_step_parts", _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(step), C.c_int64(n), C.c_float(lr), C.c_float(b1),
              C.c_float(b2), C.c_float(eps), C.c_float(wd), C.c_float(gscale), _ptr(parts), C.c_int64(part_stride), n_parts,
              C.c_int64(enc_floats), C.c_int64(layer_floats), C.c_int64(covered), _stream())


def head_fwd_raw(cfg, x, w1, b1, w2, b2, w3, b3, out, saved, ws, rng, add):
    _lib.call("ganffn_head_fwd", C.byref(cfg), _ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3),
              _ptr(out), _ptr(saved), _ptr(ws), _ptr(rng), C.c_uint64(add), _stream())


def head_bwd_raw(cfg, d_out, x, w1, w2, w3, gw1, gb1, gw2, gb2, gw3, gb3, dx, saved, ws, rng, add):
    _lib.call("ganffn_head_bwd", C.byref(cfg), _ptr(d_out), _ptr(x), _ptr(w1), _ptr(w2), _ptr(w3), _ptr(gw1), _ptr(gb1),
              _ptr(gw2), _ptr(gb2), _ptr(gw3), _ptr(gb3), _ptr(dx), _ptr(saved), _ptr(ws), _ptr(rng), C.c_uint64(add),
              _stream())


def linear_fwd_raw(x, w, b, y, T, K, N):
    _lib.call("ganffn_linear_fwd", _ptr(x), _ptr(w), _ptr(b), _ptr(y), T, K, N, _stream())


def linear_bwd_raw(dy, x, w, dx, gw, gb, T, K, N, ws=None):
    """ws: optional scratch tensor (any size; used for the split weight-gradient GEMM when large enough)"""
    _lib.call("ganffn_linear_bwd", _ptr(dy), _ptr(x), _ptr(w), _ptr(dx), _ptr(gw), _ptr(gb), T, K, N, _ptr(ws),
              C.c_int64(ws.numel() if ws is not None else 0), _stream())


def bce_fwd_raw(prob, target, n, scale, loss, accumulate):
    _lib.call("ganffn_bce_fwd", _ptr(prob), C.c_float(target), n, C.c_float(scale), _ptr(loss), 1 if accumulate else 0,
              _stream())


def bce_bwd_raw(prob, target, n, scale, dprob):
    _lib.call("ganffn_bce_bwd", _ptr(prob), C.c_float(target), n, C.c_float(scale), _ptr(dprob), _stream())


def _check_bce_len(key_len, n_len):
    if key_len is not None and (key_len.dtype != torch.int32 or not key_len.is_cuda or not key_len.is_contiguous()
                                or key_len.numel() != n_len):
        raise ValueError("key_len must be a contiguous int32 device tensor with n_len (%d) entries" % n_len)


def bce_len_fwd_raw(prob, key_len, n_len, target_a, target_b, S, Bt, split, scale, loss, accumulate):
    """BCELoss(mean) over the real utterances of prob [S x Bt]: column c has target_a if c < split else target_b and
    clamp(key_len[c % n_len], 1, S) real rows (ganffn_bce_len_fwd); key_len None = ganffn_bce2_fwd with period Bt"""
    _check_bce_len(key_len, n_len)
    _lib.call("ganffn_bce_len_fwd", _ptr(prob), _ptr(key_len), n_len, C.c_float(target_a), C.c_float(target_b), S, Bt, split,
              C.c_float(scale), _ptr(loss), 1 if accumulate else 0, _stream())


def bce_len_bwd_raw(prob, key_len, n_len, target_a, target_b, S, Bt, split, scale, dprob):
    """d loss / d prob of bce_len_fwd_raw; padded entries are written as exact zeros"""
    _check_bce_len(key_len, n_len)
    _lib.call("ganffn_bce_len_bwd", _ptr(prob), _ptr(key_len), n_len, C.c_float(target_a), C.c_float(target_b), S, Bt, split,
              C.c_float(scale), _ptr(dprob), _stream())


def adam_step_raw(p, g, m, v, step, n, lr, b1, b2, eps=1e-8, wd=0.0, gscale=1.0):
    _lib.call("ganffn_adam_step", _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(step), C.c_int64(n), C.c_float(lr),
              C.c_float(b1), C.c_float(b2), C.c_float(eps), C.c_float(wd), C.c_float(gscale), _stream())


def adam_update_raw(p, g, m, v, step, n, lr, b1, b2, eps=1e-8, wd=0.0, gscale=1.0):
    """Adam on a slice, step counter untouched (see ganffn_adam_update)"""
    _lib.call("ganffn_adam_update", _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(step), C.c_int64(n), C.c_float(lr),
              C.c_float(b1), C.c_float(b2), C.c_float(eps), C.c_float(wd), C.c_float(gscale), _stream())


def adam_bump_raw(step):
    _lib.call("ganffn_adam_bump", _ptr(step), _stream())


def rng_advance_raw(rng, delta):
    _lib.call("ganffn_rng_advance", _ptr(rng), C.c_uint64(delta), _stream())


def add3_raw(a, b, c, out, n):
    _lib.call("ganffn_add3", _ptr(a), _ptr(b), _ptr(c), _ptr(out), C.c_int64(n), _stream())


def dropout_raw(x, out, R, C_, p, site, rng_state, add):
    """out = dropout(x [R x C_]) with the mask of (site, rng_state + add); the same call on dy is its backward"""
    _lib.call("ganffn_dropout", _ptr(x), _ptr(out), R, C_, C.c_float(p), C.c_uint32(site), _ptr(rng_state), C.c_uint64(add), _stream())


def linear1_fwd_raw(x, w, b, out, T, K, N, p, site, rng_state, add, train):
    """out [T x N] = dropout(relu(x [T x K] W^T + b)); train false (or p 0): no dropout, rng_state may be None"""
    _lib.call("ganffn_ffn_linear1_fwd", _ptr(x), _ptr(w), _ptr(b), _ptr(out), T, K, N, C.c_float(p), C.c_uint32(site), _ptr(rng_state),
              C.c_uint64(add), 1 if train else 0, _stream())


def general2_attention_fwd_raw(x, mem, mask, att, alpha, tanh_s, S, B, D, flags=None):
    """masked general2 attention, every step the query: flags None: ganffn_general2_attention_fwd; an int (ATTN_CAUSAL or 0):
    ganffn_general2_attention_fwd_mask with the flags behind the mask"""
    if flags is None:
        _lib.call("ganffn_general2_attention_fwd", _ptr(x), _ptr(mem), _ptr(mask), _ptr(att), _ptr(alpha), _ptr(tanh_s), S, B, D, _stream())
    else:
        _lib.call("ganffn_general2_attention_fwd_mask", _ptr(x), _ptr(mem), _ptr(mask), C.c_uint32(flags), _ptr(att), _ptr(alpha),
                  _ptr(tanh_s), S, B, D, _stream())


def general2_attention_bwd_raw(d_att, x, mem, mask, alpha, tanh_s, du, dx, dmem, S, B, D, flags=None):
    """general2_attention_fwd_raw's backward, flags as the forward was given"""
    if flags is None:
        _lib.call("ganffn_general2_attention_bwd", _ptr(d_att), _ptr(x), _ptr(mem), _ptr(mask), _ptr(alpha), _ptr(tanh_s), _ptr(du),
                  _ptr(dx), _ptr(dmem), S, B, D, _stream())
    else:
        _lib.call("ganffn_general2_attention_bwd_mask", _ptr(d_att), _ptr(x), _ptr(mem), _ptr(mask), C.c_uint32(flags), _ptr(alpha),
                  _ptr(tanh_s), _ptr(du), _ptr(dx), _ptr(dmem), S, B, D, _stream())


# ----------------------------------------------------------------------------------------------
# autograd Functions
# ----------------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    """y = x W^T + b over the last dim (VisualDiscriminator.object, GAN_FFN.fc)."""

    @staticmethod
    def forward(ctx, x, w, b):
        _need_gpu(x, w, b)
        xc, wc, bc = _f32c(x), _f32c(w), _f32c(b)
        K, N = wc.shape[1], wc.shape[0]
        T = xc.numel() // K
        y = torch.empty(*xc.shape[:-1], N, device=x.device, dtype=torch.float32)
        linear_fwd_raw(xc, wc, bc, y, T, K, N)
        ctx.save_for_backward(xc, wc)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, wc = ctx.saved_tensors
        dy = _f32c(dy)
        K, N = wc.shape[1], wc.shape[0]
        T = xc.numel() // K
        dx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        gw = torch.zeros_like(wc) if ctx.needs_input_grad[1] else None
        gb = torch.zeros(N, device=dy.device, dtype=torch.float32) if gw is not None else None
        linear_bwd_raw(dy, xc, wc, dx, gw, gb, T, K, N)
        return dx, gw, (gb if ctx.needs_input_grad[2] else None)


class EncoderFn(torch.autograd.Function):
    """PositionalEncoding + L encoder layers.  `slab` is the packed parameter block the library reads;
    `*params` are the nn.Parameter views into it (only there so autograd tracks them)."""

    @staticmethod
    def forward(ctx, x, pe, slab, meta, *params):
        _need_gpu(x, slab)
        E, H, L, train = meta["E"], meta["H"], meta["L"], meta["train"]
        S, B = x.shape[0], x.shape[1]
        xc = _f32c(x)
        cfg = enc_cfg(S, B, E, H, L, train=train, p_pe=meta.get("p_pe", PE_DROPOUT), p_enc=meta.get("p_enc", ENC_DROPOUT))
        n_saved, n_ws = enc_sizes(cfg)
        need_grad = any(ctx.needs_input_grad)
        saved = torch.empty(n_saved, device=x.device, dtype=torch.float32) if need_grad else None
        ws = torch.empty(n_ws, device=x.device, dtype=torch.float32)
        out = torch.empty(S, B, E, device=x.device, dtype=torch.float32)
        rng = DeviceRng.get(x.device)
        add = rng.next_add() if train else 0
        key_len = meta.get("key_len")
        causal = bool(meta.get("causal", False))
        encoder_fwd_raw(cfg, xc, pe, slab, out, saved, ws, rng.state, add, key_len=key_len, causal=causal)
        ctx.key_len = key_len          # (kept alive for the backward)
        ctx.causal = causal
        ctx.cfg, ctx.add, ctx.rng_state = cfg, add, rng.state
        ctx.slab, ctx.saved = slab, saved
        ctx.param_meta = meta
        return out

    @staticmethod
    def backward(ctx, dout):
        cfg, meta = ctx.cfg, ctx.param_meta
        dx = _f32c(dout).clone()
        n_saved, n_ws = enc_sizes(cfg)
        ws = torch.empty(n_ws, device=dx.device, dtype=torch.float32)
        want_w = any(ctx.needs_input_grad[4:])
        gslab = torch.zeros_like(ctx.slab) if want_w else None
        encoder_bwd_raw(cfg, 0, cfg.L, dx, ctx.slab, gslab, ctx.saved, ws, ctx.rng_state, ctx.add,
                        need_dx_in=ctx.needs_input_grad[0], key_len=ctx.key_len, causal=ctx.causal)
        grads = [None] * len(meta["views"])
        if want_w:
            for i, (off, shape) in enumerate(meta["views"]):
                n = 1
                for d in shape:
                    n *= d
                grads[i] = gslab[off:off + n].view(shape)
        return (dx if ctx.needs_input_grad[0] else None, None, None, None, *grads)


class HeadFn(torch.autograd.Function):
    """generator / discriminator head after the encoder stack."""

    @staticmethod
    def forward(ctx, x, kind, p, train, w1, b1, w2, b2, w3, b3):
        _need_gpu(x, w1)
        xc = _f32c(x)
        S, B, E = xc.shape
        T = S * B
        D1, D2 = w1.shape[0], w2.shape[0]
        cfg = HeadCfg(T, E, D1, D2, kind, p, 1 if train else 0)
        n_saved, n_ws = head_sizes(cfg)
        saved = torch.empty(n_saved, device=x.device, dtype=torch.float32)
        ws = torch.empty(n_ws, device=x.device, dtype=torch.float32)
        out = torch.empty(S, B, D2 if kind == 0 else 1, device=x.device, dtype=torch.float32)
        rng = DeviceRng.get(x.device)
        add = rng.next_add() if train else 0
        head_fwd_raw(cfg, xc, w1, b1, w2, b2, w3, b3, out, saved, ws, rng.state, add)
        ctx.cfg, ctx.add, ctx.rng_state, ctx.saved = cfg, add, rng.state, saved
        ctx.save_for_backward(xc, w1, w2, w3)
        return out

    @staticmethod
    def backward(ctx, dout):
        xc, w1, w2, w3 = ctx.saved_tensors
        cfg = ctx.cfg
        dout = _f32c(dout)
        n_saved, n_ws = head_sizes(cfg)
        ws = torch.empty(n_ws, device=dout.device, dtype=torch.float32)
        dx = torch.empty_like(xc)
        z = lambda t: torch.zeros_like(t) if t is not None else None
        gw1, gw2, gw3 = z(w1), z(w2), z(w3)
        gb1 = torch.zeros(w1.shape[0], device=dout.device)
        gb2 = torch.zeros(w2.shape[0], device=dout.device)
        gb3 = torch.zeros(1, device=dout.device) if w3 is not None else None
        head_bwd_raw(cfg, dout, xc, w1, w2, w3, gw1, gb1, gw2, gb2, gw3, gb3, dx, ctx.saved, ws, ctx.rng_state, ctx.add)
        return dx, None, None, None, gw1, gb1, gw2, gb2, gw3, gb3


class BCEMeanFn(torch.autograd.Function):
    """nn.BCELoss() against a constant target (the reference only ever uses all-ones / all-zeros labels,
    train_IEMOCAP.py:341-346)."""

    @staticmethod
    def forward(ctx, prob, target):
        _need_gpu(prob)
        pc = _f32c(prob)
        loss = torch.empty(1, device=prob.device, dtype=torch.float32)
        bce_fwd_raw(pc, float(target), pc.numel(), 1.0, loss, False)
        ctx.save_for_backward(pc)
        ctx.target = float(target)
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        (pc,) = ctx.saved_tensors
        d = torch.empty_like(pc)
        bce_bwd_raw(pc, ctx.target, pc.numel(), 1.0, d)
        return d * dloss, None


def bce_mean(prob, target):
    return BCEMeanFn.apply(prob, target)


class DropoutFn(torch.autograd.Function):
    """nn.Dropout(p) on a (.., C) tensor with the Philox contract (standalone PositionalEncoding use)."""

    @staticmethod
    def forward(ctx, x, p, train, site):
        ctx.active = bool(train) and p > 0.0
        if not ctx.active:
            return x
        _need_gpu(x)
        xc = _f32c(x)
        C_ = xc.shape[-1]
        R = xc.numel() // C_
        rng = DeviceRng.get(x.device)
        add = rng.next_add()
        out = torch.empty_like(xc)
        dropout_raw(xc, out, R, C_, p, site, rng.state, add)
        ctx.args = (R, C_, p, site, rng.state, add)
        return out

    @staticmethod
    def backward(ctx, dy):
        if not ctx.active:
            return dy, None, None, None
        dy = _f32c(dy)
        dx = torch.empty_like(dy)
        dropout_raw(dy, dx, *ctx.args)
        return dx, None, None, None


class Add3Fn(torch.autograd.Function):
    """fusion = a + b + c   (model.py:1445)"""

    @staticmethod
    def forward(ctx, a, b, c):
        _need_gpu(a, b, c)
        a, b, c = _f32c(a), _f32c(b), _f32c(c)
        out = torch.empty_like(a)
        add3_raw(a, b, c, out, a.numel())
        return out

    @staticmethod
    def backward(ctx, d):
        return d, d, d


def logsoftmax_nll_raw(logits, labels, umask, class_w, log_prob, loss, dlogits, ws2, S, B, Cn):
    _lib.call("ganffn_logsoftmax_nll", _ptr(logits), _ptr(labels), _ptr(umask), _ptr(class_w), _ptr(log_prob),
              _ptr(loss), _ptr(dlogits), _ptr(ws2), S, B, Cn, _stream())


class LogSoftmaxFn(torch.autograd.Function):
    """F.log_softmax(x, 2) on (S, B, C)   (model.py:1449)"""

    @staticmethod
    def forward(ctx, logits):
        _need_gpu(logits)
        x = _f32c(logits)
        S, B, Cn = x.shape
        lp = torch.empty_like(x)
        logsoftmax_nll_raw(x, None, None, None, lp, None, None, None, S, B, Cn)
        ctx.save_for_backward(lp)
        return lp

    @staticmethod
    def backward(ctx, d):
        (lp,) = ctx.saved_tensors
        return d - torch.exp(lp) * d.sum(-1, keepdim=True)


class General2AttnFn(torch.autograd.Function):
    """masked general2 matching attention with every time step as the query (include/ganffn.h, N2):
    (x = transform(mem) (S,B,D), mem (S,B,D), mask (B,S)) -> (att (S,B,D), alpha (B,S,S)); alpha is an inspection
    output (the reference returns it to the caller, nothing differentiates through it).  causal=True (the GANFFN_ATTN_CAUSAL
    flag of ganffn_general2_attention_*_mask): query step t attends to memory steps j <= t only, alpha is exactly 0 above the
    diagonal."""

    @staticmethod
    def forward(ctx, x, mem, mask, causal=False):
        _need_gpu(x, mem)
        xc, mc, kc = _f32c(x), _f32c(mem), _f32c(mask)
        S, B, D = mc.shape
        att = torch.empty_like(mc)
        alpha = torch.empty(B, S, S, device=mc.device, dtype=torch.float32)
        ts = torch.empty(B, S, S, device=mc.device, dtype=torch.float32)
        ctx.flags = ATTN_CAUSAL if causal else 0
        general2_attention_fwd_raw(xc, mc, kc, att, alpha, ts, S, B, D, ctx.flags)
        ctx.save_for_backward(xc, mc, kc, alpha, ts)
        ctx.mark_non_differentiable(alpha)
        return att, alpha

    @staticmethod
    def backward(ctx, d_att, _d_alpha):
        xc, mc, kc, alpha, ts = ctx.saved_tensors
        S, B, D = mc.shape
        g = _f32c(d_att)
        du = torch.empty_like(alpha)
        dx, dm = torch.empty_like(mc), torch.empty_like(mc)
        general2_attention_bwd_raw(g, xc, mc, kc, alpha, ts, du, dx, dm, S, B, D, ctx.flags)
        return dx, dm, None, None


# ----------------------------------------------------------------------------------------------
# N2: DialogueRNN recurrence (include/ganffn.h "N2 (config 5)")
# ----------------------------------------------------------------------------------------------
DRNN_KEYS = ["g_cell.weight_ih", "g_cell.weight_hh", "g_cell.bias_ih", "g_cell.bias_hh",
             "p_cell.weight_ih", "p_cell.weight_hh", "p_cell.bias_ih", "p_cell.bias_hh",
             "e_cell.weight_ih", "e_cell.weight_hh", "e_cell.bias_ih", "e_cell.bias_hh", "attention.transform.weight"]
DRNN_LISTENER_KEYS = ["l_cell.weight_ih", "l_cell.weight_hh", "l_cell.bias_ih", "l_cell.bias_hh"]
DRNN_MAX_PARTIES = 16      # GANFFN_DRNN_MAX_PARTIES: qmask's party axis on the HIP recurrence is 1 .. 16 wide
MAX_DIALOGUES = 256        # GANFFN_MAX_DIALOGUES: dialogues per native call of either recurrence (ganffn_drnn_batch_* / ganffn_lstm_batch_*)


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def _drnn_ptrs(tensors, cls=_lib.DrnnPtrs):
    s = cls()
    for (name, _), t in zip(cls._fields_, tensors):
        setattr(s, name, t.data_ptr() if t is not None else None)
    return s


# context attention parameters per type (named_parameters order under attention.), besides general's transform.weight
DRNN_ATT_KEYS = {"general": ["attention.transform.weight"], "dot": [],
                 "general2": ["attention.transform.weight", "attention.transform.bias"],
                 "concat": ["attention.transform.weight", "attention.vector_prod.weight"],
                 "simple": ["attention.scalar.weight"]}


def _att_ptrs(att, tensors):
    """ganffn_drnn_att_params / _grads of one direction from the type's tensors (DRNN_ATT_KEYS order)"""
    s = _lib.DrnnAttPtrs()
    names = {"general": ["w"], "simple": ["w"], "dot": [], "general2": ["w", "b"], "concat": ["w", "v"]}[att]
    for n, t in zip(names, tensors):
        setattr(s, n, t.data_ptr() if t is not None else None)
    return s


def _ptr_structs(cls, rows, fill=_drnn_ptrs):
    """one ctypes array of `cls` pointer structs, one per direction (None when there are no rows)"""
    return (cls * len(rows))(*[fill(r, cls) for r in rows]) if rows is not None else None


def drnn_family(B, parties, att_type, listener):
    """THE rule for which entry-point family of the recurrence a call takes (every family is a thin wrapper over the one
    drnn_fwd / drnn_bwd driver in csrc/dialogue_rnn.hip):
      "batch"     B > 32 dialogues (up to MAX_DIALOGUES), whatever the rest      ganffn_drnn_batch_*
      "party"     otherwise a party axis other than 2 wide                       ganffn_drnn_party_*
      "att"       otherwise a context attention type other than general          ganffn_drnn_att_*
      "listener"  otherwise listener state                                       ganffn_drnn_listener_*
      ""          otherwise                                                      ganffn_drnn_*
    att_type: the _lib.DrnnAtt.type value or its name, as the caller has it.  The rule only sees what it is given: the module
    path runs simple attention as general (_drnn_cell_args), DrnnEngine passes simple as its own type."""
    if B > 32:
        return "batch"
    if parties != 2:
        return "party"
    if att_type not in ("general", _lib.DRNN_ATT_TYPES["general"]):
        return "att"
    return "listener" if listener else ""


def _drnn_entry(family, what):
    return "ganffn_drnn_%s%s" % (family + "_" if family else "", what)


def drnn_floats(cfg, acfg, listener, parties):
    """(n_saved, n_ws) floats per direction, from the size functions of the family cfg.B and the rest select (drnn_family)"""
    lib = _lib.load()
    fam = drnn_family(cfg.B, parties, acfg.type, listener)
    args = {"": (cfg,), "listener": (cfg,), "att": (cfg, acfg, int(listener))}.get(fam, (cfg, acfg, int(listener), parties))
    n_saved, n_ws = (int(getattr(lib, _drnn_entry(fam, w))(*args)) for w in ("saved_floats", "workspace_floats"))
    if n_saved < 0 or n_ws < 0:
        _lib.check(-1, "ganffn_drnn_*_floats")
    return n_saved, n_ws


# what each family's argument list leaves out of the party family's (the full) one
_DRNN_OMIT = {"": ("acfg", "parties", "LP", "AP", "LG", "AG"), "listener": ("acfg", "parties", "AP", "AG"), "att": ("parties",),
              "party": (), "batch": ()}


def _drnn_call(what, named, rng, add):
    a = dict(named)
    fam = drnn_family(a["cfg"].B, a["parties"], a["acfg"].type, a["LP"] is not None)
    _lib.call(_drnn_entry(fam, what), *[v for k, v in named if k not in _DRNN_OMIT[fam]], rng, C.c_uint64(add), _stream())


def drnn_fwd_raw(cfg, acfg, parties, ndir, U, spk, mval, P, LP, AP, e, alpha, saved, ws, rng, add):
    """the recurrence forward of ndir directions: ONE call of ganffn_drnn_<family>_fwd (drnn_family; listener = LP is given)
    with that family's argument list — the full one here, in this order, less what the family does not take.  cfg / acfg:
    _lib.DrnnCfg / _lib.DrnnAtt; P / LP / AP: arrays of ndir pointer structs (AP always given: general's is the 13th cell
    tensor); the rest: arrays of ndir device pointers, rng the Philox state's pointer, add the offset."""
    _drnn_call("fwd", [("cfg", cfg), ("acfg", acfg), ("parties", parties), ("ndir", ndir), ("U", U), ("spk", spk), ("mval", mval),
                       ("P", P), ("LP", LP), ("AP", AP), ("e", e), ("alpha", alpha), ("saved", saved), ("ws", ws)], rng, add)


def drnn_bwd_raw(cfg, acfg, parties, ndir, d_e, U, spk, mval, P, LP, AP, G, LG, AG, dU, alpha, saved, ws, rng, add):
    """drnn_fwd_raw's backward: ONE call of ganffn_drnn_<family>_bwd; G / LG / AG: the gradients' pointer structs (weight
    gradients accumulate), d_e / dU: arrays of ndir device pointers."""
    _drnn_call("bwd", [("cfg", cfg), ("acfg", acfg), ("parties", parties), ("ndir", ndir), ("d_e", d_e), ("U", U), ("spk", spk),
                       ("mval", mval), ("P", P), ("LP", LP), ("AP", AP), ("G", G), ("LG", LG), ("AG", AG), ("dU", dU),
                       ("alpha", alpha), ("saved", saved), ("ws", ws)], rng, add)


# ---- the streamed head (csrc/drnn_stream.hip): one recurrence step per new utterance against per-slot state -----------------
def drnn_stream_cfg(capacity, max_len, parties, Dm, H, He, listener, att, Da=0):
    """_lib.DrnnStreamCfg: the state's shape (capacity slots of max_len positions, `parties` party rows) and the cell's widths,
    listener state and context attention type (a DRNN_ATT_TYPES name; Da: concat's D_a)"""
    return _lib.DrnnStreamCfg(int(capacity), int(max_len), int(parties), int(Dm), int(H), int(He), 1 if listener else 0,
                              _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], int(Da)))


def drnn_stream_sizes(cfg, n_max):
    """(state floats, workspace floats for calls of up to n_max rows) of a streamed head (ganffn_drnn_stream_*_floats)"""
    lib = _lib.load()
    s = int(lib.ganffn_drnn_stream_state_floats(C.byref(cfg)))
    w = int(lib.ganffn_drnn_stream_workspace_floats(C.byref(cfg), int(n_max))) if s >= 0 else -1
    if s < 0 or w < 0:
        _lib.check(-1, "ganffn_drnn_stream_*_floats")
    return s, w


def drnn_stream_cell_ptrs(cell):
    """(ganffn_drnn_params, ganffn_drnn_listener_params or None, ganffn_drnn_att_params or None) of a DialogueRNNCell, read from
    its parameter tensors now: pointer structs for ganffn_drnn_stream_step / _extend.  The attention's parameters go in their own
    struct for every type (general's transform.weight too); att_w of the first stays null."""
    sd = dict(cell.named_parameters())
    att = drnn_att_type(cell)
    tensors = [sd[k] for k in DRNN_KEYS[:12] + DRNN_ATT_KEYS[att] + (DRNN_LISTENER_KEYS if cell.listener_state else [])]
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise GanffnError("the streamed DialogueRNN step reads the cell's parameters in place: float32 and contiguous")
    _need_gpu(*tensors)
    prm = _drnn_ptrs(tensors[:12] + [None])
    n_att = len(DRNN_ATT_KEYS[att])
    aprm = _att_ptrs(att, tensors[12:12 + n_att]) if att != "dot" else None
    lprm = _drnn_ptrs(tensors[12 + n_att:], _lib.DrnnListenerPtrs) if cell.listener_state else None
    return prm, lprm, aprm


def _byref(s):
    return C.byref(s) if s is not None else None


def drnn_stream_step_raw(cfg, n, slot, pos, spk, U, ptrs, state, e_out, ws, off=0, count=None):
    """one recurrence step of n rows (ganffn_drnn_stream_step; eval math): row i of U [n x Dm], speaker spk[i], is utterance
    pos[slot[i]] + off of the dialogue in slot slot[i]; writes the state and e_out [n x He].  pos is not advanced.
    ptrs: drnn_stream_cell_ptrs(cell)."""
    _need_gpu(slot, pos, spk, U, state, e_out, ws)
    prm, lprm, aprm = ptrs
    _lib.call("ganffn_drnn_stream_step", C.byref(cfg), n, _ptr(slot), _ptr(pos), int(off), _ptr(count), _ptr(spk), _ptr(U),
              C.byref(prm), _byref(lprm), _byref(aprm), _ptr(state), _ptr(e_out), _ptr(ws), _stream())


def drnn_stream_extend_raw(cfg, n, m, slot, count, pos, spk, U, ptrs, state, e_out, ws):
    """count[i] consecutive recurrence steps of n dialogues in one native call (ganffn_drnn_stream_extend): spk [m][n],
    U [m][n][Dm] and e_out [m][n][He] time-major.  pos is not advanced."""
    _need_gpu(slot, count, pos, spk, U, state, e_out, ws)
    prm, lprm, aprm = ptrs
    _lib.call("ganffn_drnn_stream_extend", C.byref(cfg), n, m, _ptr(slot), _ptr(count), _ptr(pos), _ptr(spk), _ptr(U),
              C.byref(prm), _byref(lprm), _byref(aprm), _ptr(state), _ptr(e_out), _ptr(ws), _stream())


def general2_stream_attention_raw(x, e_hist, slot, count, pos, att, alpha, n, m, capacity, max_len, D):
    """the second attention of new rows (ganffn_general2_stream_attention): x, att [m][n][D]; e_hist: the state's E region, which
    already holds the new rows; count None = one row each; alpha [m][n][max_len] or None"""
    _need_gpu(x, e_hist, slot, pos, att)
    _lib.call("ganffn_general2_stream_attention", _ptr(x), _ptr(e_hist), _ptr(slot), _ptr(count), _ptr(pos), _ptr(att), _ptr(alpha),
              n, m, capacity, max_len, D, _stream())


# ---- the streamed LSTM (csrc/lstm_stream.hip): one step of the L layers per new utterance against per-slot state ---------------
LSTM_STREAM_MAX_H = 1024       # the emotion history is the memory of ganffn_general2_stream_attention (D <= 1024)
LSTM_STREAM_MAX_LAYERS = 16
MELD_HEAD_MAX_CLASSES = 16     # ganffn_meld_head_*: smax_fc's rows are held per thread


def lstm_stream_cfg(capacity, max_len, In, H, L):
    """_lib.LstmStreamCfg: the state's shape (capacity slots of max_len positions, L layers) and the LSTM's widths"""
    return _lib.LstmStreamCfg(int(capacity), int(max_len), int(In), int(H), int(L))


def lstm_stream_sizes(cfg, n_max):
    """(state floats, workspace floats for calls of up to n_max rows) of a streamed LSTM (ganffn_stream_lstm_*_floats)"""
    lib = _lib.load()
    s = int(lib.ganffn_stream_lstm_state_floats(C.byref(cfg)))
    w = int(lib.ganffn_stream_lstm_workspace_floats(C.byref(cfg), int(n_max))) if s >= 0 else -1
    if s < 0 or w < 0:
        _lib.check(-1, "ganffn_stream_lstm_*_floats")
    return s, w


def lstm_stream_ptrs(lstm):
    """(w_ih, w_hh, b_ih, b_hh): arrays of num_layers device pointers of a forward-only nn.LSTM, read from lstm.weight_ih_l{k}, ...
    now — the streamed step reads the parameters in place, wherever they live at call time (a step runner's slab included)"""
    names = ("weight_ih_l%d", "weight_hh_l%d", "bias_ih_l%d", "bias_hh_l%d")
    tensors = [[getattr(lstm, n % l) for l in range(lstm.num_layers)] for n in names]
    for t in (t for row in tensors for t in row):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise GanffnError("the streamed LSTM step reads the LSTM's parameters in place: float32 and contiguous")
    _need_gpu(*[t for row in tensors for t in row])
    return tuple(_ptr_array(row) for row in tensors)


def lstm_stream_step_raw(cfg, n, slot, pos, x, ptrs, state, e_out, ws, off=0, count=None):
    """one step of the L layers over n rows (ganffn_stream_lstm_step; eval math): row i of x [n x In] is utterance
    pos[slot[i]] + off of the dialogue in slot slot[i]; writes the state and e_out [n x H].  pos is not advanced.
    ptrs: lstm_stream_ptrs(lstm)."""
    _need_gpu(slot, pos, count, x, state, e_out, ws)
    _lib.call("ganffn_stream_lstm_step", C.byref(cfg), n, _ptr(slot), _ptr(pos), int(off), _ptr(count), _ptr(x), *ptrs, _ptr(state),
              _ptr(e_out), _ptr(ws), _stream())


def lstm_stream_extend_raw(cfg, n, m, slot, count, pos, x, ptrs, state, e_out, ws):
    """count[i] consecutive steps of n dialogues in one native call (ganffn_stream_lstm_extend): x [m][n][In] and e_out [m][n][H]
    time-major.  pos is not advanced."""
    _need_gpu(slot, count, pos, x, state, e_out, ws)
    _lib.call("ganffn_stream_lstm_extend", C.byref(cfg), n, m, _ptr(slot), _ptr(count), _ptr(pos), _ptr(x), *ptrs, _ptr(state),
              _ptr(e_out), _ptr(ws), _stream())


def meld_head_fwd_raw(emotions, att, w_fc, b_fc, hidden, logits, T, D, Cn):
    """hidden = hardswish(emotions + hardswish(att)), logits = hidden w_fc^T + b_fc over T rows (ganffn_meld_head_fwd)"""
    _need_gpu(emotions, att, w_fc, b_fc, hidden, logits)
    _lib.call("ganffn_meld_head_fwd", _ptr(emotions), _ptr(att), _ptr(w_fc), _ptr(b_fc), _ptr(hidden), _ptr(logits), T, D, Cn, _stream())


class DialogueRNNFn(torch.autograd.Function):
    """ndir (1 or 2) DialogueRNNs through one chain of launches (drnn_fwd_raw / drnn_bwd_raw; which entry points they reach:
    drnn_family).
    apply(cfg_dict, U_0, spk_0, mval_0, *13 params_0 [, U_1, spk_1, mval_1, *13 params_1]) ->
    (e_0 (S,B,D_e), alpha_0 (B,S,S) [, e_1, alpha_1]).  alpha is an inspection output (non-differentiable).
    cfg_dict["listener"] true: listener_state = True; every direction then takes 17 parameter tensors, the 13 above followed
    by l_cell's weight_ih, weight_hh, bias_ih, bias_hh (DRNN_LISTENER_KEYS).
    cfg_dict["att"] (default "general"): the context attention type.  Other than general, the 13th tensor (general's
    transform.weight) is replaced by the type's own DRNN_ATT_KEYS tensors (none for dot, two for general2 and concat;
    cfg_dict["Da"]: concat's D_a).
    cfg_dict["parties"] (default 2): the width P of qmask's party axis, 1 .. DRNN_MAX_PARTIES.
    At most MAX_DIALOGUES dialogues.  Arguments and gradients are the same whichever family runs."""

    @staticmethod
    def forward(ctx, meta, *args):
        listener = bool(meta.get("listener", False))
        att = meta.get("att", "general")
        n_att = len(DRNN_ATT_KEYS[att])
        na = 15 + n_att + (4 if listener else 0)
        ndir = len(args) // na
        assert len(args) == na * ndir and ndir in (1, 2)
        U = [_f32c(args[na * z]) for z in range(ndir)]
        spk = [args[na * z + 1].to(torch.int32).contiguous() for z in range(ndir)]
        mval = [_f32c(args[na * z + 2]) for z in range(ndir)]
        if att == "general":
            prm = [[_f32c(p) for p in args[na * z + 3:na * z + 16]] for z in range(ndir)]
            aprm = None
        else:
            prm = [[_f32c(p) for p in args[na * z + 3:na * z + 15]] + [None] for z in range(ndir)]
            aprm = [[_f32c(p) for p in args[na * z + 15:na * z + 15 + n_att]] for z in range(ndir)]
        l0 = 15 + n_att
        lprm = [[_f32c(p) for p in args[na * z + l0:na * z + l0 + 4]] for z in range(ndir)] if listener else None
        _need_gpu(*U)
        S, B, Dm = U[0].shape
        H, He = prm[0][1].shape[1], prm[0][9].shape[1]
        train = bool(meta["train"]) and meta["p"] > 0.0
        cfg = _lib.DrnnCfg(S, B, Dm, H, He, float(meta["p"]), 1 if train else 0)
        acfg = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], int(meta.get("Da", 0)))
        parties = int(meta.get("parties", 2))
        n_saved, n_ws = drnn_floats(cfg, acfg, listener, parties)
        dev = U[0].device
        saved = [torch.empty(n_saved, device=dev) for _ in range(ndir)]
        ws = [torch.empty(n_ws, device=dev) for _ in range(ndir)]
        e = [torch.empty(S, B, He, device=dev) for _ in range(ndir)]
        alpha = [torch.empty(B, S, S, device=dev) for _ in range(ndir)]
        rng = DeviceRng.get(dev)
        add = rng.next_add() if train else 0
        # (general: transform.weight, the 13th cell tensor, is the attention's own parameter)
        AP = _ptr_structs(_lib.DrnnAttPtrs, aprm or [[p[12]] for p in prm], lambda a, _: _att_ptrs(att, a))
        drnn_fwd_raw(cfg, acfg, parties, ndir, _ptr_array(U), _ptr_array(spk), _ptr_array(mval), _ptr_structs(_lib.DrnnPtrs, prm),
                     _ptr_structs(_lib.DrnnListenerPtrs, lprm), AP, _ptr_array(e), _ptr_array(alpha), _ptr_array(saved),
                     _ptr_array(ws), _ptr(rng.state), add)
        ctx.cfg, ctx.ndir, ctx.add, ctx.rng_state = cfg, ndir, add, rng.state
        ctx.att, ctx.acfg, ctx.aprm, ctx.parties = att, acfg, aprm, parties
        ctx.keep = (U, spk, mval, prm, lprm, alpha, saved, ws)
        out = []
        for z in range(ndir):
            out += [e[z], alpha[z]]
            ctx.mark_non_differentiable(alpha[z])
        return tuple(out)

    @staticmethod
    def backward(ctx, *douts):
        U, spk, mval, prm, lprm, alpha, saved, ws = ctx.keep
        ndir, cfg = ctx.ndir, ctx.cfg
        d_e = [_f32c(douts[2 * z]) if douts[2 * z] is not None else torch.zeros_like(U[z][..., :cfg.He]) for z in range(ndir)]
        dU = [torch.empty_like(U[z]) for z in range(ndir)]
        grads = [[torch.zeros_like(p) if p is not None else None for p in prm[z]] for z in range(ndir)]
        general = ctx.aprm is None        # (general: transform.weight and its gradient are the attention's own parameter)
        aprm = [[p[12]] for p in prm] if general else ctx.aprm
        agrads = [[g[12]] for g in grads] if general else [[torch.zeros_like(p) for p in aprm[z]] for z in range(ndir)]
        lgrads = [[torch.zeros_like(p) for p in lprm[z]] for z in range(ndir)] if lprm is not None else None
        att_ptrs = lambda a, _: _att_ptrs(ctx.att, a)
        drnn_bwd_raw(cfg, ctx.acfg, ctx.parties, ndir, _ptr_array(d_e), _ptr_array(U), _ptr_array(spk), _ptr_array(mval),
                     _ptr_structs(_lib.DrnnPtrs, prm), _ptr_structs(_lib.DrnnListenerPtrs, lprm),
                     _ptr_structs(_lib.DrnnAttPtrs, aprm, att_ptrs), _ptr_structs(_lib.DrnnPtrs, grads),
                     _ptr_structs(_lib.DrnnListenerPtrs, lgrads), _ptr_structs(_lib.DrnnAttPtrs, agrads, att_ptrs),
                     _ptr_array(dU), _ptr_array(alpha), _ptr_array(saved), _ptr_array(ws), _ptr(ctx.rng_state), ctx.add)
        out = [None]
        for z in range(ndir):
            # the 13th slot is general's transform.weight; any other type's own tensors follow the 12 cell gradients
            out += [dU[z], None, None] + (grads[z] if general else grads[z][:12] + agrads[z]) + (lgrads[z] if lgrads else [])
        return tuple(out)


_CHECK_QMASK = __import__("os").environ.get("GANFFN_CHECK_QMASK", "0") == "1"


def dialogue_rnn_supported(cell, U, qmask):
    """the configurations the HIP recurrence implements: every context attention type — general (the trained
    configuration), simple (DialogueRNNCell's constructor default; run as general attention with a constant query:
    _drnn_cell_args), dot (D_m = D_g), general2, concat (D_a % 4 == 0, D_a <= 512) — no listener, 1 to DRNN_MAX_PARTIES
    parties (qmask.size(2)), dims % 4, D_g = D_p <= 512 (the attention kernels keep one state column per thread), at most
    112 steps, on a GPU.
    PRECONDITION (not tested here: the test would be a device->host sync in front of ~760 latency-sized launches): every
    qmask row is one-hot or all zero, as the reference's loaders produce (dataloader.py:41-50) — the gate kernels use
    (argmax, value at argmax) only.  GANFFN_CHECK_QMASK=1 verifies it on every call."""
    return not cell.listener_state and _drnn_limits_hold(cell, U, qmask)


def dialogue_rnn_listener_supported(cell, U, qmask):
    """dialogue_rnn_supported's limits for a cell WITH listener state (listener_state = True, model.py:899-921): the HIP
    recurrence's listener path (ganffn_drnn_listener_fwd / _bwd).  Same qmask precondition."""
    return bool(cell.listener_state) and _drnn_limits_hold(cell, U, qmask)


def drnn_att_type(cell):
    """the cell's context attention type: simple / general / dot / general2 / concat"""
    if type(cell.attention).__name__ == "SimpleAttention":            # softmax over time of a learned scalar score (model.py:117-131)
        return "simple"
    return cell.attention.att_type


def drnn_att_limits_hold(cell):
    """the attention type's own limits on the HIP recurrence: dot needs D_m = D_g, concat D_a % 4 == 0 and D_a <= 512"""
    att = drnn_att_type(cell)
    if att == "dot":
        return cell.D_m == cell.D_g
    if att == "concat":
        Da = cell.attention.transform.weight.shape[0]
        return Da % 4 == 0 and 4 <= Da <= 512
    return att in ("general", "general2", "simple")


def _drnn_limits_hold(cell, U, qmask):
    ok = (U.is_cuda and drnn_att_limits_hold(cell)
          and 1 <= qmask.size(2) <= DRNN_MAX_PARTIES and cell.D_g == cell.D_p and cell.D_g <= 512 and cell.D_m % 4 == 0 and cell.D_g % 4 == 0
          and cell.D_e % 4 == 0 and U.size(0) <= 112)
    if ok and _CHECK_QMASK:
        ok = bool((((qmask == 0) | (qmask == 1)).all() & (qmask.sum(2) <= 1).all()).item())
    return ok


def _drnn_cell_args(cell, U):
    """(U, the 13 parameter tensors — 17 with the listener's, DRNN_LISTENER_KEYS) the recurrence kernels take for one
    DialogueRNNCell.
    general attention (model.py:160-166): as they are.
    dot / general2 / concat: the 12 cell tensors, then the type's own (DRNN_ATT_KEYS: none / transform weight and bias /
    transform.weight and vector_prod.weight), then the listener's; DialogueRNNFn passes them on as the attention's own.
    simple attention (model.py:117-131): alpha = softmax_s(w . g_s) is general attention with the CONSTANT query w (general:
    alpha = softmax_s(q_t . g_s), q_t = W_att U_t).  A constant cannot come out of W_att U_t, so the utterance features get one
    more column that is always 1 (and three zero columns: the kernels want widths in multiples of 4), the input-side weights of
    the global and party cells get matching zero columns, and the attention weight becomes [0 | w^T | 0]: q_t = w for every t.
    All of it is torch.cat on the way in, so autograd carries dU and d(w) back out; the recurrence itself is the same HIP launch
    chain.  (The scalar score has no bias in the reference; a bias would cancel in the softmax anyway.)"""
    sd = dict(cell.named_parameters())
    att = drnn_att_type(cell)
    if att not in ("general", "simple"):     # dot / general2 / concat: the 12 cell tensors, the type's own, the listener's
        return U, [sd[k] for k in DRNN_KEYS[:12] + DRNN_ATT_KEYS[att] + (DRNN_LISTENER_KEYS if cell.listener_state else [])]
    keys = DRNN_KEYS + (DRNN_LISTENER_KEYS if cell.listener_state else [])
    if att == "general":
        return U, [sd[k] for k in keys]
    S, B, Dm = U.shape
    H = cell.D_g
    Ux = torch.cat([U, U.new_ones(S, B, 1), U.new_zeros(S, B, 3)], 2)

    def pad_ih(W):
        return torch.cat([W[:, :Dm], W.new_zeros(W.size(0), 4), W[:, Dm:]], 1)
    w = sd["attention.scalar.weight"]                                   # [1 x D_g]
    att = torch.cat([w.new_zeros(H, Dm), w.t(), w.new_zeros(H, 3)], 1)  # [D_g x (D_m + 4)]
    params = []
    for k in DRNN_KEYS[:-1]:
        params.append(pad_ih(sd[k]) if k in ("g_cell.weight_ih", "p_cell.weight_ih") else sd[k])
    params.append(att)
    if cell.listener_state:            # the listener's input side takes U too: the same zero columns
        params += [pad_ih(sd[k]) if k == "l_cell.weight_ih" else sd[k] for k in DRNN_LISTENER_KEYS]
    return Ux, params


def dialogue_rnn_run(cells, Us, qmasks, training):
    """cells / Us / qmasks: one entry per direction.  -> [(emotions (S,B,D_e), [alpha_t (B,t)] for t >= 1)] per direction.
    One native call for B <= MAX_DIALOGUES (which entry points: drnn_family; more than 32 dialogues run in tiles of 32 inside
    every launch); beyond that, chunks of MAX_DIALOGUES (chunks are independent)."""
    ndir = len(cells)
    S, B = Us[0].shape[:2]
    e_parts, a_parts = [[] for _ in range(ndir)], [[] for _ in range(ndir)]
    for b0 in range(0, B, MAX_DIALOGUES):
        b1 = min(B, b0 + MAX_DIALOGUES)
        args = []
        for z in range(ndir):
            qm = qmasks[z][:, b0:b1]
            spk = torch.argmax(qm, 2)
            mval = qm.gather(2, spk.unsqueeze(2)).squeeze(2)
            Ux, params = _drnn_cell_args(cells[z], Us[z][:, b0:b1])
            args += [Ux.contiguous(), spk, mval] + params
        meta = {"p": float(cells[0].dropout.p), "train": bool(training), "listener": bool(cells[0].listener_state),
                "parties": int(qmasks[0].size(2))}
        att = drnn_att_type(cells[0])
        if att not in ("general", "simple"):
            meta["att"] = att
            meta["Da"] = int(cells[0].attention.transform.weight.shape[0]) if att == "concat" else 0
        out = DialogueRNNFn.apply(meta, *args)
        for z in range(ndir):
            e_parts[z].append(out[2 * z])
            a_parts[z].append(out[2 * z + 1])
    res = []
    for z in range(ndir):
        e = torch.cat(e_parts[z], 1) if len(e_parts[z]) > 1 else e_parts[z][0]
        al = torch.cat(a_parts[z], 0) if len(a_parts[z]) > 1 else a_parts[z][0]
        res.append((e, [al[:, t, :t] for t in range(1, S)]))
    return res


# ----------------------------------------------------------------------------------------------
# N4: bidirectional LSTM (include/ganffn.h "N4"; csrc/lstm.hip) — the recurrence of nn.LSTM inside MELDLSTMModel
# (/root/reference/model.py:520-562, train_MELD.py:147-151)
# ----------------------------------------------------------------------------------------------
SITE_LSTM = 64          # + layer: the dropout nn.LSTM(dropout=p) applies to the output of every layer but the last

# The entry points of each family (lstm_family).  The naming is irregular — "batch" / "packed" stand before "layer" and behind
# "stack" — so the heads are written out; the packed family has no size functions of its own and takes the _batch_ ones.  "uni" is
# the one-direction family (include/ganffn.h "the LSTM recurrence with ONE direction"; an extension the reference does not have).
_LSTM_ENTRY = {
    "": {"layer": "ganffn_lstm_layer_", "stack": "ganffn_lstm_stack_",
         "layer_sizes": "ganffn_lstm_", "stack_sizes": "ganffn_lstm_stack_"},
    "batch": {"layer": "ganffn_lstm_batch_layer_", "stack": "ganffn_lstm_stack_batch_",
              "layer_sizes": "ganffn_lstm_batch_", "stack_sizes": "ganffn_lstm_stack_batch_"},
    "packed": {"layer": "ganffn_lstm_packed_layer_", "stack": "ganffn_lstm_stack_packed_",
               "layer_sizes": "ganffn_lstm_batch_", "stack_sizes": "ganffn_lstm_stack_batch_"},
    "uni": {"layer": "ganffn_unilstm_layer_", "stack": "ganffn_unilstm_stack_",
            "layer_sizes": "ganffn_unilstm_", "stack_sizes": "ganffn_unilstm_stack_"},
}


def lstm_family(B, packed, ndir=2):
    """THE rule for which entry-point family of the LSTM a call takes (every family is a thin wrapper over the one set of
    drivers in csrc/lstm.hip, which take a direction count; the names: _LSTM_ENTRY):
      "uni"     one direction, whatever B (up to MAX_DIALOGUES) and packed   ganffn_unilstm_layer_* / ganffn_unilstm_stack_*
      "packed"  otherwise lengths are given, whatever B                      ganffn_lstm_packed_layer_* / ganffn_lstm_stack_packed_*
      "batch"   otherwise B > 32 dialogues (up to MAX_DIALOGUES)             ganffn_lstm_batch_layer_* / ganffn_lstm_stack_batch_*
      ""        otherwise                                                    ganffn_lstm_layer_* / ganffn_lstm_stack_*
    lengths stand behind cfg in "packed" and in "uni" (there always: NULL for the padded run)."""
    if ndir == 1:
        return "uni"
    if packed:
        return "packed"
    return "batch" if B > 32 else ""


def lstm_sizes(cfg, packed=False, ndir=2):
    """(n_saved, n_ws) floats of a layer call (_lib.LstmCfg) or a stack call (_lib.LstmStackCfg), from the size functions of
    the family cfg.B, `packed` and ndir select"""
    head = _LSTM_ENTRY[lstm_family(cfg.B, packed, ndir)]["stack_sizes" if isinstance(cfg, _lib.LstmStackCfg) else "layer_sizes"]
    n_saved, n_ws = (int(getattr(_lib.load(), head + w)(C.byref(cfg))) for w in ("saved_floats", "workspace_floats"))
    if n_saved < 0 or n_ws < 0:
        _lib.check(-1, head + "*_floats")
    return n_saved, n_ws


def _lstm_call(kind, what, cfg, lengths, ndir, *args):
    fam = lstm_family(cfg.B, lengths is not None, ndir)
    head = (C.byref(cfg),) if lengths is None and ndir == 2 else (C.byref(cfg), _ptr(lengths))
    _lib.call(_LSTM_ENTRY[fam][kind] + what, *head, *args, _stream())


def lstm_layer_fwd_raw(cfg, x, w_ih, w_hh, b_ih, b_hh, out, saved, ws, lengths=None, ndir=2):
    """one layer forward: ONE call of the family's layer_fwd (lstm_family; lengths behind cfg where the family takes them).
    cfg: _lib.LstmCfg; w_* / b_*: arrays of ndir device pointers (forward, reverse), passed as they are; the rest: tensors."""
    _lstm_call("layer", "fwd", cfg, lengths, ndir, _ptr(x), w_ih, w_hh, b_ih, b_hh, _ptr(out), _ptr(saved), _ptr(ws))


def lstm_layer_bwd_raw(cfg, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, ws, lengths=None, ndir=2):
    """lstm_layer_fwd_raw's backward: ONE call of the family's layer_bwd; g*: arrays of ndir gradient pointers (accumulated into;
    None or a null entry: not wanted), dx may be None"""
    _lstm_call("layer", "bwd", cfg, lengths, ndir, _ptr(d_out), _ptr(x), _ptr(out), w_ih, w_hh, _ptr(dx), gw_ih, gw_hh, gb_ih, gb_hh,
               _ptr(saved), _ptr(ws))


def lstm_stack_fwd_raw(cfg, x, w_ih, w_hh, b_ih, b_hh, out, saved, ws, rng, add, lengths=None, ndir=2):
    """L layers with the inter-layer dropout forward: ONE call of the family's stack fwd.  cfg: _lib.LstmStackCfg; w_* / b_*:
    arrays of [L][ndir] device pointers, passed as they are; rng: the Philox state tensor, add: the offset."""
    _lstm_call("stack", "fwd", cfg, lengths, ndir, _ptr(x), w_ih, w_hh, b_ih, b_hh, _ptr(out), _ptr(saved), _ptr(ws), _ptr(rng),
               C.c_uint64(add))


def lstm_stack_bwd_raw(cfg, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, ws, rng, add, lengths=None, ndir=2):
    """lstm_stack_fwd_raw's backward: ONE call of the family's stack bwd; g*: arrays of [L][ndir] gradient pointers"""
    _lstm_call("stack", "bwd", cfg, lengths, ndir, _ptr(d_out), _ptr(x), _ptr(out), w_ih, w_hh, _ptr(dx), gw_ih, gw_hh, gb_ih, gb_hh,
               _ptr(saved), _ptr(ws), _ptr(rng), C.c_uint64(add))


# the one-direction forms under their own names (ndir=1 of the above: same arguments, arrays of 1 / [L][1] pointers)
def unilstm_sizes(cfg):
    return lstm_sizes(cfg, False, 1)


def unilstm_layer_fwd_raw(cfg, x, w_ih, w_hh, b_ih, b_hh, out, saved, ws, lengths=None):
    lstm_layer_fwd_raw(cfg, x, w_ih, w_hh, b_ih, b_hh, out, saved, ws, lengths, 1)


def unilstm_layer_bwd_raw(cfg, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, ws, lengths=None):
    lstm_layer_bwd_raw(cfg, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, ws, lengths, 1)


def unilstm_stack_fwd_raw(cfg, x, w_ih, w_hh, b_ih, b_hh, out, saved, ws, rng, add, lengths=None):
    lstm_stack_fwd_raw(cfg, x, w_ih, w_hh, b_ih, b_hh, out, saved, ws, rng, add, lengths, 1)


def unilstm_stack_bwd_raw(cfg, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, ws, rng, add, lengths=None):
    lstm_stack_bwd_raw(cfg, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, ws, rng, add, lengths, 1)


def _lstm_layer_fwd(ctx, x, lengths, params):
    """the forward of LstmLayerFn (lengths None), LstmPackedLayerFn and UniLstmLayerFn (4 parameter tensors: one direction):
    chunks of MAX_DIALOGUES, lengths sliced with the batch"""
    _need_gpu(x, *params)
    x = _f32c(x)
    p = [_f32c(t.detach()) for t in params]          # w_ih, w_hh, b_ih, b_hh of the forward direction, then of the reverse one
    ndir = len(p) // 4
    S, B, In = x.shape
    H = p[1].shape[1]
    if lengths is not None:
        _need_gpu(lengths)
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,):
            raise ValueError("lstm: lengths must be an int32 tensor of shape (%d,) on the device; got %s %s"
                             % (B, lengths.dtype, tuple(lengths.shape)))
        lengths = lengths.contiguous()
    out = torch.empty(S, B, ndir * H, device=x.device, dtype=torch.float32)
    chunks = []
    for b0 in range(0, B, MAX_DIALOGUES):
        b1 = min(B, b0 + MAX_DIALOGUES)
        cfg = _lib.LstmCfg(S, b1 - b0, In, H)
        n_saved, n_ws = lstm_sizes(cfg, lengths is not None, ndir)
        xc = x if (b0, b1) == (0, B) else x[:, b0:b1].contiguous()
        oc = out if (b0, b1) == (0, B) else torch.empty(S, b1 - b0, ndir * H, device=x.device, dtype=torch.float32)
        saved = torch.empty(n_saved, device=x.device, dtype=torch.float32)
        ws = torch.empty(n_ws, device=x.device, dtype=torch.float32)
        lc = None if lengths is None else lengths[b0:b1]          # (a slice of a contiguous vector: contiguous, 4-byte aligned)
        lstm_layer_fwd_raw(cfg, xc, *[_ptr_array(p[j::4]) for j in range(4)], oc, saved, ws, lengths=lc, ndir=ndir)
        if oc is not out:
            out[:, b0:b1] = oc
        chunks.append((b0, b1, xc, oc, saved, lc))
    ctx.chunks, ctx.p, ctx.shape = chunks, p, (S, B, In, H)
    return out


def _lstm_layer_bwd(ctx, d_out, i_x, i_p):
    """-> (dx, parameter gradients); i_x / i_p: where x / the first parameter sit among the Function's inputs"""
    S, B, In, H = ctx.shape
    p = ctx.p
    ndir = len(p) // 4
    d_out = _f32c(d_out)
    need_dx = ctx.needs_input_grad[i_x]
    dx = torch.empty(S, B, In, device=d_out.device, dtype=torch.float32) if need_dx else None
    grads = [torch.zeros_like(t) if ctx.needs_input_grad[i_p + i] else None for i, t in enumerate(p)]
    for (b0, b1, xc, oc, saved, lc) in ctx.chunks:
        cfg = _lib.LstmCfg(S, b1 - b0, In, H)
        ws = torch.empty(lstm_sizes(cfg, lc is not None, ndir)[1], device=d_out.device, dtype=torch.float32)
        dc = d_out if (b0, b1) == (0, B) else d_out[:, b0:b1].contiguous()
        dxc = None
        if need_dx:
            dxc = dx if (b0, b1) == (0, B) else torch.empty(S, b1 - b0, In, device=d_out.device, dtype=torch.float32)
        lstm_layer_bwd_raw(cfg, dc, xc, oc, _ptr_array(p[0::4]), _ptr_array(p[1::4]), dxc,
                           *[_ptr_array(grads[j::4]) for j in range(4)], saved, ws, lengths=lc, ndir=ndir)
        if need_dx and dxc is not dx:
            dx[:, b0:b1] = dxc
    return dx, grads


class LstmLayerFn(torch.autograd.Function):
    """one bidirectional LSTM layer: x (S, B, In) -> (S, B, 2H) = [h forward | h reverse]; torch's parameters
    weight_ih [4H x In], weight_hh [4H x H], bias_ih, bias_hh [4H] per direction (gate order i, f, g, o).  One native call for
    B <= MAX_DIALOGUES (at most 32 dialogues: ganffn_lstm_layer_*; more: ganffn_lstm_batch_layer_*); bigger batches run in chunks of
    MAX_DIALOGUES (dialogues are independent)."""

    @staticmethod
    def forward(ctx, x, *params):
        return _lstm_layer_fwd(ctx, x, None, params)

    @staticmethod
    def backward(ctx, d_out):
        dx, grads = _lstm_layer_bwd(ctx, d_out, 0, 1)
        return (dx, *grads)


class LstmPackedLayerFn(torch.autograd.Function):
    """LstmLayerFn on packed sequences (ganffn_lstm_packed_layer_*; an extension the reference does not have): lengths int32 (B,)
    on the device, lengths[b] real steps of dialogue b — what pack_padded_sequence -> one nn.LSTM layer ->
    pad_packed_sequence(total_length = S) gives: zero output past a dialogue's end, the reverse direction starting at its last
    real step, zero dx at padded positions, upstream gradients at padded positions ignored.  x must be finite at padded
    positions; its values there change nothing.  The same chunking at MAX_DIALOGUES, lengths sliced alongside the batch."""

    @staticmethod
    def forward(ctx, x, lengths, *params):
        return _lstm_layer_fwd(ctx, x, lengths, params)

    @staticmethod
    def backward(ctx, d_out):
        dx, grads = _lstm_layer_bwd(ctx, d_out, 0, 2)
        return (dx, None, *grads)


class UniLstmLayerFn(torch.autograd.Function):
    """one forward-only LSTM layer (nn.LSTM(bidirectional=False); the "uni" family): x (S, B, In) -> (S, B, H), out[t] a
    function of x[0 .. t] alone; torch's parameters weight_ih [4H x In], weight_hh [4H x H], bias_ih, bias_hh [4H].  lengths: None
    (the padded run) or int32 (B,) on the device with LstmPackedLayerFn's rule (zero output and zero dx past a dialogue's end;
    x finite there).  The same call path as the two above: the direction count is the number of parameter tensors / 4."""

    @staticmethod
    def forward(ctx, x, lengths, *params):
        return _lstm_layer_fwd(ctx, x, lengths, params)

    @staticmethod
    def backward(ctx, d_out):
        dx, grads = _lstm_layer_bwd(ctx, d_out, 0, 2)
        return (dx, None, *grads)


def lstm_supported(lstm):
    """whether lstm_forward runs this nn.LSTM on the HIP kernels: any input_size and hidden_size that are multiples of 4, any
    num_layers, any dropout, bidirectional OR NOT — with the default (seq, batch, feature) layout, biases and no projection.
    batch_first=True, bias=False and proj_size > 0 are not supported."""
    return (not lstm.batch_first and lstm.proj_size == 0 and bool(lstm.bias)
            and lstm.input_size % 4 == 0 and lstm.hidden_size % 4 == 0)


def lstm_forward(x, lstm, training, lengths=None):
    """nn.LSTM(..., dropout=p).forward(x)[0] for a padded (S, B, In) CUDA batch, on the HIP kernels, with the module's own
    parameters (state_dict keys unchanged: lstm.weight_ih_l{k}[_reverse], ...).  Inter-layer dropout (every layer but the last,
    train mode only) follows the Philox contract (site SITE_LSTM + layer).
    Supported configurations (lstm_supported): bidirectional=True — the MELDLSTMModel configuration, LstmLayerFn /
    LstmPackedLayerFn — and bidirectional=False — the forward direction alone, parameters weight_ih_l{k}, ... with no _reverse,
    UniLstmLayerFn, an extension the reference does not have; input and hidden sizes multiples of 4, any num_layers and dropout;
    not batch_first, bias=False or proj_size > 0.
    lengths (int32 (B,) on the device; default None: the padded run above, as the reference): the packed run —
    pack_padded_sequence(x, lengths, enforce_sorted=False) -> lstm -> pad_packed_sequence(total_length=S)[0]."""
    assert not lstm.batch_first and lstm.proj_size == 0 and lstm.bias, "lstm_forward: (seq, batch, feature) layout, biases, no projection"
    h = x
    for l in range(lstm.num_layers):
        names = ["weight_ih_l%d", "weight_hh_l%d", "bias_ih_l%d", "bias_hh_l%d"]
        if lstm.bidirectional:
            params = [getattr(lstm, n % l) for n in names] + [getattr(lstm, (n % l) + "_reverse") for n in names]
            h = LstmLayerFn.apply(h, *params) if lengths is None else LstmPackedLayerFn.apply(h, lengths, *params)
        else:
            h = UniLstmLayerFn.apply(h, lengths, *[getattr(lstm, n % l) for n in names])
        if l + 1 < lstm.num_layers and lstm.dropout > 0.0:
            h = DropoutFn.apply(h, float(lstm.dropout), training, SITE_LSTM + l)
    return h


# ----------------------------------------------------------------------------------------------
# the epoch loop with the corpus on the device (csrc/batch.hip; data.DeviceLoader, artifacts.train_or_eval_model)
# ----------------------------------------------------------------------------------------------
def batch_gather_raw(cols, labels_src, row0, n_rows, idx, umask, label, S, B, n_dialogues):
    """cols: [(src [n_rows x width], dst [S x B x width], width)], at most _lib.BATCH_MAX_COLS; idx int32 [B] on the device.
    One launch writes every dst, umask (B, S) and label (B, S)."""
    _need_gpu(labels_src, row0, idx, umask, label, *[t for c in cols for t in c[:2]])
    arr = (_lib.BatchCol * max(1, len(cols)))()
    for a, (src, dst, width) in zip(arr, cols):
        a.src, a.dst, a.width = src.data_ptr(), dst.data_ptr(), int(width)
    _lib.call("ganffn_batch_gather", C.cast(arr, C.c_void_p), len(cols), _ptr(labels_src), _ptr(row0), C.c_int64(n_rows), _ptr(idx),
              _ptr(umask), _ptr(label), S, B, n_dialogues, _stream())


class EpochRecord:
    """An epoch's results on the device — predictions, labels and masks of `capacity` (step, dialogue) cells and the loss and
    real-utterance count of `n_steps` steps — written by one ganffn_epoch_record launch per step and read once by `host()`."""

    def __init__(self, capacity, n_steps, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise GanffnError("EpochRecord keeps an epoch's results on an MI355X (HIP) device; got %s. There is no CPU fallback." % dev)
        self.capacity, self.n_steps = int(capacity), int(n_steps)
        n, k = max(1, self.capacity), max(1, self.n_steps)
        self.preds = torch.empty(n, dtype=torch.int64, device=dev)
        self.labels = torch.empty(n, dtype=torch.int64, device=dev)
        self.masks = torch.empty(n, dtype=torch.float32, device=dev)
        self.loss = torch.empty(k, dtype=torch.float32, device=dev)
        self.count = torch.empty(k, dtype=torch.float32, device=dev)

    def record(self, step, offset, log_prob, label, umask, loss):
        """log_prob (S, B, C), label (B, S) int64, umask (B, S) float32, loss: the step's scalar — as the step runners return them"""
        _need_gpu(log_prob, label, umask, loss)
        S, B, Cn = log_prob.shape
        if (log_prob.dtype != torch.float32 or umask.dtype != torch.float32 or label.dtype != torch.int64 or loss.dtype != torch.float32
                or not (log_prob.is_contiguous() and label.is_contiguous() and umask.is_contiguous())
                or label.numel() != S * B or umask.numel() != S * B or loss.numel() < 1):
            raise GanffnError("EpochRecord.record: contiguous float32 log_prob (S, B, C), float32 umask (B, S), int64 label (B, S) and "
                              "a float32 loss; got %s %s, %s %s, %s %s, %s" % (tuple(log_prob.shape), log_prob.dtype, tuple(umask.shape),
                                                                             umask.dtype, tuple(label.shape), label.dtype, loss.dtype))
        _lib.call("ganffn_epoch_record", _ptr(log_prob), _ptr(label), _ptr(umask), _ptr(loss), S, B, Cn, _ptr(self.preds),
                  _ptr(self.labels), _ptr(self.masks), C.c_int64(offset), C.c_int64(self.capacity), _ptr(self.loss), _ptr(self.count),
                  int(step), self.n_steps, _stream())

    def host(self):
        """-> numpy (preds, labels, masks, loss, count): one synchronise, one copy each"""
        torch.cuda.current_stream().synchronize()
        return tuple(t.cpu().numpy() for t in (self.preds[:self.capacity], self.labels[:self.capacity], self.masks[:self.capacity],
                                               self.loss[:self.n_steps], self.count[:self.n_steps]))
