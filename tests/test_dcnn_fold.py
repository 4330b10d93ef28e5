"""nets.fold_dcnn + nets.dcnn_fullframe_forward: DCNNet.eval() as the device path computes it (BN
folded into the convolutions and Linears, every convolution a pad-1 convolution on the full frame,
the interior of the fourth output in (r, col, c) order into the column-permuted fc1) is
DCNNet.eval() itself. Checked in fp64, where the two differ by rounding only (~2e-15 measured;
the bar is 1e-12)."""
import pytest
import torch


def _dcnn(N, P, A=97, channels=128, seed=0):
    from blokus_rl_amd.nets import DCNNet

    torch.manual_seed(seed)
    m = DCNNet(N, P, A, num_channels=channels).eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.1, 0.1)
    return m


@pytest.mark.parametrize("N,P", [(7, 2), (14, 2), (20, 4)])
def test_fullframe_forward_is_the_eval_model(N, P):
    from blokus_rl_amd.nets import dcnn_fullframe_forward, fold_dcnn

    m = _dcnn(N, P, seed=N + P).double()
    g = torch.Generator().manual_seed(3 * N + P)
    obs = (torch.rand((3, 2 * P, N, N), generator=g) < 0.3).double()
    with torch.no_grad():
        lp_ref, v_ref = m(obs)
        f = fold_dcnn(m)
        lp, v = dcnn_fullframe_forward(f, obs)
        feat, v2 = dcnn_fullframe_forward(f, obs, features=True)
        logits, _ = dcnn_fullframe_forward(f, obs, normalize=False)
    e_lp, e_v = float((lp - lp_ref).abs().max()), float((v - v_ref).abs().max())
    print(f"N={N} P={P}: log-probs {e_lp:.3e}  v {e_v:.3e}")
    assert lp.dtype == torch.float64 and lp.shape == lp_ref.shape and v.shape == v_ref.shape
    assert e_lp <= 1e-12 and e_v <= 1e-12
    # the features are fc3's / fc4's input: the sparse head's operands give the same logits
    assert feat.shape == (3, 64) and torch.equal(v2, v)
    assert torch.equal(torch.nn.functional.linear(feat, m.fc3.weight, m.fc3.bias), logits)
    assert float((torch.log_softmax(logits, dim=1) - lp_ref).abs().max()) <= 1e-12


def test_fold_leaves_the_model_alone():
    from blokus_rl_amd.nets import fold_dcnn

    m = _dcnn(7, 2)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    f = fold_dcnn(m)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert f.N == 7 and [tuple(w.shape) for w in f.conv_w] == [(128, 4, 3, 3)] + [(128, 128, 3, 3)] * 3
    assert tuple(f.fc1_w.shape) == (128, 128 * 9) and tuple(f.fc2_w.shape) == (64, 128)
    assert f.fc3_w.data_ptr() != m.fc3.weight.data_ptr()


def test_leaf_dcnnet_reports_why_it_does_not_qualify():
    from blokus_rl_amd.nets import LeafDCNNet

    m = _dcnn(7, 2, channels=32)
    leaf = LeafDCNNet(m)
    assert not leaf.native and "32 channels" in leaf.reason
    assert leaf.sparse_head() is None and not leaf.planar_input and not leaf.takes_states()
    obs = (torch.rand((2, 4, 7, 7)) < 0.3).float()
    with torch.no_grad():
        lp_ref, v_ref = m(obs)
    lp, v = leaf(obs)
    assert torch.equal(lp, lp_ref) and torch.equal(v, v_ref)
    # a 128-channel net off the device says so too
    assert "HIP device" in LeafDCNNet(_dcnn(7, 2)).reason
    assert "board" in LeafDCNNet(_dcnn(9, 2)).reason and "input planes" in LeafDCNNet(_dcnn(7, 1)).reason


def test_knob(monkeypatch):
    from blokus_rl_amd.nets import DCNNet, LeafDCNNet, dcnn_leaf_mode, inference_model

    monkeypatch.delenv("BK_DCNN_LEAF", raising=False)
    m = _dcnn(7, 2, channels=32)
    assert dcnn_leaf_mode() == "torch" and inference_model(m) is m
    assert isinstance(inference_model(m, dcnn_leaf="x3"), LeafDCNNet)
    assert type(inference_model(m, dcnn_leaf="x3", dtype=torch.bfloat16)) is DCNNet
    monkeypatch.setenv("BK_DCNN_LEAF", "x3")
    assert isinstance(inference_model(m), LeafDCNNet) and inference_model(m, dcnn_leaf="torch") is m
    monkeypatch.setenv("BK_DCNN_LEAF", "fast")
    with pytest.raises(ValueError):
        inference_model(m)
