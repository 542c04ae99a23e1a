"""The heads alone: the lines of oracle.ganffn_oracle.generator_forward / discriminator_forward behind the encoder stack, on a
2-D [T x E] input, so that the Philox rows of the dropout masks are the token rows (what ganffn_head_fwd / _bwd see).  Built
from the oracle's own gelu, _drop2d and SITE_HEAD0..3; gradients come from autograd.  tests/test_head_oracle_cpu.py pins it
to stock torch."""
import torch

from oracle import ganffn_oracle as O

GEN, DISC = 0, 1          # ganffn_head_cfg.kind
GRAD_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")


def head_forward(kind, x, w1, b1, w2, b2, w3=None, b3=None, p=0.2, rng=None, dtype=torch.float64, logits=False):
    """generator:      gelu(drop(fc2(gelu(drop(fc1(drop(gelu(x))))))))             -> [T x D2]
    discriminator:  sigmoid(drop(fc3(gelu(drop(fc2(gelu(drop(fc1(gelu(x))))))))))  -> [T x 1]
    rng: O.Rng with the offset of THIS call (rng[1] + rng_offset_add); None or train = False: no dropout.
    logits: a discriminator returns drop(fc3(..)), the argument of its sigmoid."""
    x, w1, b1, w2, b2 = (t.to(dtype) for t in (x, w1, b1, w2, b2))
    t = O.gelu(x)
    if kind == GEN:
        t = O._drop2d(t, p, O.SITE_HEAD0, rng)
    t = O.gelu(O._drop2d(t @ w1.T + b1, p, O.SITE_HEAD1, rng))
    t = O.gelu(O._drop2d(t @ w2.T + b2, p, O.SITE_HEAD2, rng))
    if kind == GEN:
        return t
    u3 = O._drop2d(t @ w3.to(dtype).T + b3.to(dtype), p, O.SITE_HEAD3, rng)
    return u3 if logits else torch.sigmoid(u3)


def head_leaves(kind, x, w1, b1, w2, b2, w3=None, b3=None, dtype=torch.float64):
    """detached copies in `dtype` that require grad: {"x", "w1", "b1", "w2", "b2"[, "w3", "b3"]}"""
    named = dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2)
    if kind == DISC:
        named.update(w3=w3, b3=b3)
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in named.items()}


def head_run(kind, tensors, d_out, p, rng, dtype=torch.float64, loss=None, logits=False):
    """forward + backward of sum(out * d_out) — or of loss(out) when given — -> (out, {"x": dx, "w1": ..}), detached"""
    L = head_leaves(kind, *tensors, dtype=dtype)
    out = head_forward(kind, L["x"], L["w1"], L["b1"], L["w2"], L["b2"], L.get("w3"), L.get("b3"), p, rng, dtype, logits)
    (loss(out) if loss is not None else (out * d_out.to(dtype)).sum()).backward()
    return out.detach(), {k: v.grad for k, v in L.items()}
