"""The fp64 oracle's encoder layer against stock torch.nn.TransformerEncoderLayer at the widths where no reference fixture
exists (tests/test_hip_dispatch_range.py checks the HIP encoder against the oracle there): post-LN, ReLU, sequence-first,
dropout 0, the same weights in double — forward and input gradient to 1e-12 relative."""
import pytest
import torch

from oracle import ganffn_oracle as O

KEYS = ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
        "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
        "norm2.bias"]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("E,H,F", [(64, 4, 128), (128, 4, 256), (136, 4, 64), (248, 4, 132)])
def test_oracle_encoder_layer_is_stock_torch_at_off_workload_widths(E, H, F):
    S, B = 7, 2
    torch.manual_seed(E + F)
    layer = torch.nn.TransformerEncoderLayer(d_model=E, nhead=H, dim_feedforward=F, dropout=0.0, activation="relu",
                                             norm_first=False, batch_first=False).double()
    sd = layer.state_dict()
    assert sorted(sd) == sorted(KEYS)
    with torch.no_grad():                      # LayerNorm parameters off their 1 / 0 initial values, biases off 0
        for k in KEYS:
            if k.startswith("norm") or k.endswith("bias"):
                sd[k].add_(0.1 * torch.randn(sd[k].shape, dtype=torch.float64))
    layer.load_state_dict(sd)
    P = {"l." + k: v.detach().clone() for k, v in sd.items()}
    x = torch.randn(S, B, E, dtype=torch.float64)
    gy = torch.randn(S, B, E, dtype=torch.float64)
    xt, xo = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yt = layer(xt)                             # train mode, dropout 0: torch's plain (unfused) path
    yo = O.encoder_layer(xo, P, "l.", 0, H, None)
    (yt * gy).sum().backward()
    (yo * gy).sum().backward()
    assert rel(yo.detach(), yt.detach()) < 1e-12
    assert rel(xo.grad, xt.grad) < 1e-12
