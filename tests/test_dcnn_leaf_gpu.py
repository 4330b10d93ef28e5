"""nets.LeafDCNNet (dcnn_leaf / BK_DCNN_LEAF "x3"): DCNNet's leaf evaluation with the convolutions
on bk_conv128_first / bk_conv128_x3, the 64 features after fc2 into the search's sparse policy
head, and self-play's captured simulation graph.

Accuracy: the project's fp32-class bar (tests/test_leafnet_gpu.py): against the fp64 model on the
CPU, the device path's error is within 4x that of PyTorch's fp32 model.eval() on the same device,
or 2e-6 of the output scale (features and log-probs relative to the largest reference magnitude,
v absolute: |v| <= 1)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _dcnn(N, P, A, channels=128, seed=0):
    from blokus_rl_amd.nets import DCNNet

    torch.manual_seed(seed)
    m = DCNNet(N, P, A, num_channels=channels).cuda().eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.1, 0.1)
    return m


def _parts(m, obs):
    """DCNNet.eval()'s forward from the model's own layers: (features after fc2, log-probs, v)."""
    with torch.no_grad():
        x = obs
        for conv, bn in ((m.conv1, m.bn1), (m.conv2, m.bn2), (m.conv3, m.bn3), (m.conv4, m.bn4)):
            x = torch.relu(bn(conv(x)))
        x = x.reshape(x.shape[0], -1)
        x = torch.relu(m.fc_bn1(m.fc1(x)))
        x = torch.relu(m.fc_bn2(m.fc2(x)))
        return x, torch.log_softmax(m.fc3(x), dim=1), torch.tanh(m.fc4(x))


def _rel(a, ref):
    return float((a.double().cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


@pytest.mark.parametrize("N,P,B,kind", [(7, 2, 5, "binary"), (14, 2, 3, "binary"), (20, 4, 2, "binary"),
                                        (14, 2, 3, "dense")])
def test_leaf_dcnnet_is_fp32_class(N, P, B, kind):
    from blokus_rl_amd.nets import LeafDCNNet

    m = _dcnn(N, P, A=257, seed=N + P)
    g = torch.Generator(device="cuda").manual_seed(3 * N + B)
    if kind == "binary":
        obs = (torch.rand((B, 2 * P, N, N), device="cuda", generator=g) < 0.3).float()
    else:
        obs = torch.randn((B, 2 * P, N, N), device="cuda", generator=g)
    feats, dense = LeafDCNNet(m, features=True), LeafDCNNet(m)
    assert feats.native and feats.reason is None and not feats.takes_states() and feats.sparse_head() is m.fc3
    f, v = feats(obs)
    lp, v2 = dense(obs)
    raw, _ = LeafDCNNet(m, normalize=False)(obs)
    f32, _, _ = _parts(m, obs)  # PyTorch's fp32 on the device: the features, and the model's own outputs
    with torch.no_grad():
        lp32, v32 = m(obs)
    torch.cuda.synchronize()
    f_ref, lp_ref, v_ref = _parts(copy.deepcopy(m).double().cpu(), obs.double().cpu())
    assert tuple(f.shape) == (B, 64) and tuple(lp.shape) == (B, 257) and tuple(v.shape) == (B, P)
    assert torch.isfinite(f).all() and torch.isfinite(lp).all() and torch.equal(v, v2)
    assert torch.equal(torch.log_softmax(raw, dim=1), lp)
    for what, e_x3, e_32 in (("features", _rel(f, f_ref), _rel(f32, f_ref)),
                             ("log-probs", _rel(lp, lp_ref), _rel(lp32, lp_ref)),
                             ("v", float((v.double().cpu() - v_ref).abs().max()),
                              float((v32.double().cpu() - v_ref).abs().max()))):
        print(f"N={N} P={P} B={B} {kind} {what}: x3 {e_x3:.3g}  fp32 {e_32:.3g}")
        assert e_x3 <= max(4 * e_32, 2e-6), (what, e_x3, e_32)
    # the same batch again (the activation buffers are reused)
    f_again, _ = feats(obs)
    assert torch.equal(f_again, f)


@pytest.mark.parametrize("preset,max_plies", [((7, 2, 5), 6), ((20, 4, 5), 30)])
def test_sparse_policy_head_matches_dense_priors_at_64_features(preset, max_plies):
    """tests/test_selfplay_gpu.py::test_sparse_policy_head_matches_dense_priors's procedure with
    LeafDCNNet: bk_mcts_leaf_logits over the 64 features and fc3's rows of the legal ids gives the
    priors of the dense head, to f32 rounding."""
    from blokus_rl_amd.alphazero.batched_mcts import BatchedMCTS
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import LeafDCNNet

    eng = Engine(*preset)
    net = _dcnn(eng.N, eng.P, eng.A, seed=1)
    dense = LeafDCNNet(net, normalize=False).eval()
    feats = LeafDCNNet(net, normalize=False, features=True).eval()
    T = 8
    roots = random_boards(eng, T, seed0=5, max_plies=max_plies)
    m1 = BatchedMCTS(eng, T, node_cap=64, child_cap=T * 64 * 700)
    m2 = BatchedMCTS(eng, T, node_cap=64, child_cap=T * 64 * 700)
    for _ in range(3):
        _, obs, _ = m1.select(roots, None, 1.0)
        _, obs2, _ = m2.select(roots, None, 1.0)
        assert torch.equal(obs, obs2)
        lg, v = dense(obs)
        pf, v2 = feats(obs)
        assert pf.shape[1] == 64
        m1.expand_backup(lg.contiguous(), v.contiguous(), 0)
        m2.leaf_logits(pf.contiguous(), net.fc3.weight.detach().contiguous(), net.fc3.bias.detach().contiguous())
        m2.expand_backup(None, v2.contiguous(), 2)
    c1, c2 = m1.check(), m2.check()
    assert c1["expanded"] == c2["expanded"] == 3 * T
    i1, n1, q1, p1, k1 = m1.root_stats(roots)
    i2, n2, q2, p2, k2 = m2.root_stats(roots)
    assert torch.equal(k1, k2) and torch.equal(i1, i2)
    assert (p1 - p2).abs().max().item() < 1e-6


def test_selfplay_with_and_without_the_graph(monkeypatch):
    from blokus_rl_amd.alphazero.selfplay import SelfPlay
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import DCNNet, LeafDCNNet

    monkeypatch.delenv("BK_DCNN_LEAF", raising=False)
    eng = Engine(7, 2, 5)
    net = _dcnn(7, 2, eng.A, seed=2)
    runs = []
    for use_graph in (True, False):
        sp = SelfPlay(eng, net, 8, num_sims=8, seed=3, use_graph=use_graph, dcnn_leaf="x3")
        ev = sp.evaluator
        assert ev.sparse and ev.planar and isinstance(ev.model, LeafDCNNet) and ev.model.native
        assert not ev.takes_states and sp.sim_groups == 1 and sp.leaf_input == "planes"
        assert tuple(ev.policy_w.shape) == (eng.A, 64)
        actions = []
        for _ in range(4):
            sp.play_ply()
            actions.append(sp.last_action.clone())
        c = sp.check()
        assert c["expanded"] > 0 and (sp._graph is not None) == use_graph
        runs.append((sp, c, torch.stack(actions)))
    (a, ca, aa), (b, cb, ab) = runs
    assert bool((aa >= 0).all()) and torch.equal(aa, ab) and ca == cb
    assert torch.equal(a.roots, b.roots)
    for x, y in zip(a.mcts.root_stats(a.roots), b.mcts.root_stats(b.roots)):
        assert torch.equal(x, y)
    # the knob: off by default (the plain DCNNet on PyTorch, dense priors), BK_DCNN_LEAF reads it
    off = SelfPlay(eng, net, 8, num_sims=8, seed=3, use_graph=False)
    assert type(off.evaluator.model) is DCNNet and not off.evaluator.sparse and not off.evaluator.planar
    monkeypatch.setenv("BK_DCNN_LEAF", "x3")
    env = SelfPlay(eng, net, 8, num_sims=8, seed=3, use_graph=False)
    assert isinstance(env.evaluator.model, LeafDCNNet) and env.evaluator.sparse
    monkeypatch.setenv("BK_DCNN_LEAF", "mfma")
    with pytest.raises(ValueError):
        SelfPlay(eng, net, 8, num_sims=8, use_graph=False)


def test_diverged_fc3_is_refused():
    from blokus_rl_amd.alphazero.selfplay import LeafEvaluator
    from blokus_rl_amd.engine import Engine, EngineError

    eng = Engine(7, 2, 5)
    net = _dcnn(7, 2, eng.A, seed=4)
    with torch.no_grad():
        net.fc3.weight[5, 7] = float("nan")
    with pytest.raises(EngineError):
        LeafEvaluator(net, eng, 4, use_graph=False, dcnn_leaf="x3")


def test_a_net_that_does_not_qualify_runs_the_model():
    from blokus_rl_amd.alphazero.selfplay import LeafEvaluator
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import LeafDCNNet, inference_model

    eng = Engine(7, 2, 5)
    net = _dcnn(7, 2, eng.A, channels=32, seed=5)
    leaf = inference_model(net, normalize=False, features=True, dcnn_leaf="x3")
    assert isinstance(leaf, LeafDCNNet) and not leaf.native and "32 channels" in leaf.reason
    g = torch.Generator(device="cuda").manual_seed(6)
    obs = (torch.rand((4, 4, 7, 7), device="cuda", generator=g) < 0.3).float()
    with torch.no_grad():
        lp_ref, v_ref = net(obs)
    lp, v = leaf(obs)
    assert torch.equal(lp, lp_ref) and torch.equal(v, v_ref)
    # the evaluator under the knob is the evaluator without it (dense priors, channels_last input)
    ev = LeafEvaluator(net, eng, 4, use_graph=False, dcnn_leaf="x3")
    assert not ev.sparse and not ev.planar and not ev.takes_states
    lp_off, v_off = LeafEvaluator(net, eng, 4, use_graph=False, dcnn_leaf="torch")(obs)
    lp2, v2 = ev(obs)
    assert torch.equal(lp2, lp_off) and torch.equal(v2, v_off)
