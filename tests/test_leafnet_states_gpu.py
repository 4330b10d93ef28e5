"""bk_leafnet_x3_states (k_leafnet_x3's packed-state input form) against the planar entry on
bk_observe of the same states: every output equal as a float value (torch.equal: +-0 compare
equal). The states form builds the binary stem input from the state's row words and drops the
product with its all-zero lo half, which adds exactly +-0, so nothing else may differ. Boards come
from seeded random playouts: the empty board, every mover, mid-games, finished games."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 37


@functools.lru_cache(maxsize=None)
def _engine(N):
    from blokus_rl_amd.engine import Engine

    return Engine(N, 4, 5)


@functools.lru_cache(maxsize=None)
def _states(N):
    """B states of seeded uniform random playouts, board b taken after target[b] plies: 0 (the
    empty board), 1..4 (each mover), to the end of the game (rows 5..7), the rest mid-game."""
    eng = _engine(N)
    dev = eng.device
    g = torch.Generator(device="cpu").manual_seed(1000 + N)
    last = 4 * eng.num_pieces  # no game has more plies
    target = torch.randint(5, 3 * last // 4, (B,), generator=g)
    target[:5] = torch.arange(5)
    target[5:8] = last
    target = target.to(dev)
    states = eng.init_states(B)
    snap = states.clone()
    for ply in range(1, last + 1):
        ids, counts = eng.legal_ids(states, cap=4096)
        assert int(counts.min()) >= 0
        u = torch.rand(B, generator=g, dtype=torch.float64).to(dev)
        pick = (u * counts).long().clamp(max=(counts - 1).clamp(min=0).long())
        act = torch.where(counts > 0, ids.gather(1, pick.view(-1, 1)).view(-1), torch.full_like(counts, -1))
        states, _, status = eng.next_state(states, act.to(torch.int32).contiguous())
        assert int(status.max()) == 0
        snap = torch.where((target == ply).view(-1, 1), states, snap)
    ended, _ = eng.game_ended(snap)
    assert torch.equal(snap[0], eng.init_states(1)[0])
    assert set(eng.to_move(snap[:5]).tolist()) == {0, 1, 2, 3}
    assert bool(ended[5:8].all()) and not bool(ended[:5].any())
    return snap.contiguous()


@functools.lru_cache(maxsize=None)
def _leaf(N, nblocks):
    from blokus_rl_amd.nets import LeafResNet, ResNet

    torch.manual_seed(7 * N + nblocks)
    net = ResNet(N, 4, 100, nblocks).cuda().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.1, 0.1)
    leaf = LeafResNet(net, normalize=False, features=True).eval()
    assert leaf.x3 and leaf.f.stem.out_channels == 64
    return leaf


@functools.lru_cache(maxsize=None)
def _planar(N, nblocks):
    """The planar entry's outputs on the observed states, computed once."""
    from blokus_rl_amd.nets import leafnet_x3

    pf, v, out = leafnet_x3(_engine(N).observe(_states(N)), _leaf(N, nblocks), want_out=True)
    assert torch.isfinite(pf).all() and torch.isfinite(v).all()
    return pf, v, out


@pytest.mark.parametrize("N,nblocks", [(20, 1), (20, 5), (14, 1), (14, 5)])
def test_states_entry_equals_planar_entry(N, nblocks):
    from blokus_rl_amd.nets import leafnet_x3_states

    pf, v, out = _planar(N, nblocks)
    pfs, vs, outs = leafnet_x3_states(_states(N), None, _leaf(N, nblocks), want_out=True)
    assert torch.equal(pfs, pf) and torch.equal(vs, v) and torch.equal(outs, out)
    # one board alone (B = 1): a mid-game board and the empty board
    for b in (B - 1, 0):
        pf1, v1 = leafnet_x3_states(_states(N)[b:b + 1].contiguous(), None, _leaf(N, nblocks))
        assert torch.equal(pf1, pf[b:b + 1]) and torch.equal(v1, v[b:b + 1])


@pytest.mark.parametrize("N,nblocks", [(20, 5), (14, 1)])
def test_status_rows_are_the_zero_observation(N, nblocks):
    """Rows whose status is not 1 (0, 2, -1 on a third of the batch) are evaluated as the all-zero
    observation and their state bytes (0xFF here) are not interpreted."""
    from blokus_rl_amd.nets import leafnet_x3, leafnet_x3_states

    eng, leaf = _engine(N), _leaf(N, nblocks)
    status = torch.ones(B, dtype=torch.int32, device=eng.device)
    third = torch.arange(0, B, 3, device=eng.device)
    status[third] = torch.tensor([0, 2, -1], dtype=torch.int32, device=eng.device).repeat(B)[: len(third)]
    assert set(status.tolist()) == {1, 0, 2, -1}
    dead = status != 1
    states = _states(N).clone()
    states[dead] = 0xFF
    obs = eng.observe(_states(N))
    obs[dead] = 0.0
    pf, v = leafnet_x3(obs, leaf)
    pfs, vs = leafnet_x3_states(states, status, leaf)
    torch.cuda.synchronize()
    assert torch.equal(pfs, pf) and torch.equal(vs, v)
    # the live rows are the unmasked batch's
    assert torch.equal(pfs[~dead], _planar(N, nblocks)[0][~dead])
    # a raw device address in place of the tensor (what the search hands the net)
    pfp, vp = leafnet_x3_states(states.data_ptr(), status, leaf)
    assert torch.equal(pfp, pf) and torch.equal(vp, v)


def test_forward_states_and_fallback(monkeypatch):
    """LeafResNet.forward_states equals forward on the observed planes: through the states kernel
    by default, and through bk_observe + the f32 kernels with BK_NET_MATH=f32."""
    N = 20
    eng, leaf, states = _engine(N), _leaf(N, 1), _states(N)
    obs = eng.observe(states)
    status = torch.ones(B, dtype=torch.int32, device=eng.device)
    status[3::4] = 0
    assert leaf.takes_states()
    for st in (None, status):
        o = obs if st is None else obs * (st == 1).view(-1, 1, 1, 1)
        pf, v = leaf(o)
        pfs, vs = leaf.forward_states(states, st)
        assert torch.equal(pfs, pf) and torch.equal(vs, v)
    x3 = leaf(obs)
    monkeypatch.setenv("BK_NET_MATH", "f32")
    assert not leaf.takes_states()
    for st in (None, status):
        o = obs if st is None else obs * (st == 1).view(-1, 1, 1, 1)
        pf, v = leaf(o)
        pfs, vs = leaf.forward_states(states, st)
        assert torch.equal(pfs, pf) and torch.equal(vs, v)
    assert not torch.equal(leaf(obs)[0], x3[0])  # the f32 path it is, not x3


@pytest.mark.parametrize("model_type", ["resnet", "dumbnet"])
def test_predict_states_equals_predict_batch(model_type):
    from blokus_rl_amd.colossumrl import ColosseumBlokusGameWrapper
    from blokus_rl_amd.hparams import AlphaZeroHparams
    from blokus_rl_amd.neural_network import BlokusNNetWrapper

    hp = AlphaZeroHparams(board_size=20, number_of_players=4, num_res_blocks=2, model_type=model_type)
    game = ColosseumBlokusGameWrapper(hp)
    torch.manual_seed(3)
    nn = BlokusNNetWrapper(game, hp, device=game.device)
    states = _states(20)[:9].contiguous()
    lp, v = nn.predict_batch(_engine(20).observe(states))
    lps, vs = nn.predict_states(states)
    assert lps.shape == (9, game.get_action_size()) and torch.isfinite(lps).all()
    assert torch.equal(lps, lp) and torch.equal(vs, v)
