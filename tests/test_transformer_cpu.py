"""TransformerConv (conv="Transformer", reference configs/transformer_msigmae*.py): construction through get_conv /
create_model, PyG state-dict names, interchangeability with the fp64 reference model, and the test restatement itself
pinned by gradcheck and a hand-computed known answer.  No GPU needed."""
import copy

import pytest
import torch

from tests.transformer_ref import TransformerConv as RefConv, reference_model, softmax

KEYS = {"lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight", "lin_value.bias",
        "lin_edge.weight", "lin_skip.weight", "lin_skip.bias"}


def _cfg(**kw):
    from gnnepcsaft_amd.data import default_config
    cfg = default_config(2)
    cfg.update(dict(conv="Transformer"), **kw)
    return cfg


def test_get_conv_and_create_model_build_the_layer():
    from gnnepcsaft_amd import nn as gnn
    from gnnepcsaft_amd.train import models as M
    cfg = _cfg(dropout=0.25)
    conv = M.get_conv(cfg)
    assert isinstance(conv, gnn.TransformerConv)
    assert (conv.in_channels, conv.out_channels, conv.heads, conv.dropout) == (128, 64, 2, 0.25)
    assert conv.concat and not conv.beta and conv.root_weight and conv.edge_dim == 128
    m = M.create_model(_cfg(hidden_dim=32, heads=4, propagation_depth=3), [0, 4, 2])
    assert len(m.model.convs) == 3 and all(isinstance(c, gnn.TransformerConv) for c in m.model.convs)
    assert len({c.seed for c in m.model.convs}) == 3  # every layer draws its own attention-dropout stream


def test_state_dict_keys_and_assert_message():
    from gnnepcsaft_amd.train import models as M
    conv = M.get_conv(_cfg())
    assert set(conv.state_dict()) == KEYS
    assert conv.lin_edge.bias is None
    assert tuple(conv.lin_edge.weight.shape) == (128, 128) and tuple(conv.lin_key.weight.shape) == (128, 128)
    with pytest.raises(AssertionError, match="hidden_dim must be divisible by heads"):
        M.get_conv(_cfg(hidden_dim=30, heads=4))


def test_state_dict_is_interchangeable_with_the_fp64_reference_model():
    from gnnepcsaft_amd.train.models import GNNePCSAFT
    cfg = _cfg(hidden_dim=32, heads=2, propagation_depth=2, deg=[0, 3, 2])
    native = GNNePCSAFT(cfg)
    ref = reference_model(cfg).double()
    ref.load_state_dict(native.state_dict(), strict=True)
    native.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    assert set(ref.state_dict()) == set(native.state_dict())
    sub = {k for k in native.state_dict() if k.startswith("convs.1.")}
    assert sub == {"convs.1." + k for k in KEYS}


def test_get_conv_gatv2_still_raises():
    from gnnepcsaft_amd.train import models as M
    with pytest.raises(NotImplementedError):
        M.get_conv(_cfg(conv="GATv2"))


def test_restatement_gradcheck():
    torch.manual_seed(0)
    conv = RefConv(8, 4, heads=2, edge_dim=8).double()
    x = torch.randn(5, 8, dtype=torch.float64, requires_grad=True)
    ei = torch.tensor([[1, 2, 3, 0, 4, 4], [0, 0, 0, 1, 1, 2]])  # node 3 has no in-edges
    ea = torch.randn(6, 8, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b: conv(a, ei, b), (x, ea))
    keep = torch.tensor([[1, 0], [1, 1], [0, 1], [1, 1], [0, 0], [1, 0]])
    conv.dropout, conv.keep = 0.25, keep
    assert torch.autograd.gradcheck(lambda a, b: conv(a, ei, b), (x, ea))


def test_restatement_known_answer():
    """3 nodes, 1 head, C = H = 2, every projection the identity with zero bias.  Node 0 receives from 1 and 2 with EQUAL
    scores (q_0 = (1,0) is orthogonal to both keys): alpha = 1/2 each.  Node 1 receives from 0 through a bond whose edge
    term (1,1) is added to the key AND the value: alpha = 1.  Node 2 has no in-edge: out = skip = x_2."""
    conv = RefConv(2, 2, heads=1, edge_dim=2).double()
    with torch.no_grad():
        for lin in (conv.lin_key, conv.lin_query, conv.lin_value, conv.lin_skip):
            lin.weight.copy_(torch.eye(2))
            lin.bias.zero_()
        conv.lin_edge.weight.copy_(torch.eye(2))
    x = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.0, 3.0]], dtype=torch.float64)
    ei = torch.tensor([[1, 2, 0], [0, 0, 1]])
    ea = torch.tensor([[0.0, 0.0], [0.0, 0.0], [1.0, 1.0]], dtype=torch.float64)
    out = conv(x, ei, ea)
    want = torch.tensor([[1.0, 2.0], [2.0, 2.0], [0.0, 3.0]], dtype=torch.float64)
    assert torch.allclose(out, want, rtol=0, atol=1e-14), out
    a = softmax(torch.tensor([[0.5], [0.5], [7.0]], dtype=torch.float64), torch.tensor([0, 0, 1]), 3)
    assert torch.allclose(a, torch.tensor([[0.5], [0.5], [1.0]], dtype=torch.float64), rtol=0, atol=1e-14)
    # the replayed mask at p = 0.5: node 0 keeps 2 x 1/2 of its first message only, node 1 twice its message
    conv.dropout, conv.keep = 0.5, torch.tensor([[1], [0], [1]])
    out = conv(x, ei, ea)
    want = torch.tensor([[1.0, 1.0], [4.0, 3.0], [0.0, 3.0]], dtype=torch.float64)
    assert torch.allclose(out, want, rtol=0, atol=1e-14), out


def test_model_config_copy_keeps_dispatch():
    """The reference model swap leaves a config untouched (the oracle's own get_conv knows no Transformer)."""
    cfg = _cfg(hidden_dim=16, propagation_depth=1, deg=[0, 1])
    before = copy.deepcopy(cfg)
    reference_model(cfg)
    assert cfg == before
