"""PPO remainder against the reference's own outputs
(tests/golden/ppo_golden.npz from tests/golden/make_ppo_golden.py): GAE, FilterLegalMoves, the
agent's log-prob/entropy/value, and whole _optimize_agent passes; plus the device kernels at the
config-5 scale against the CPU restatement (oracle/ppo_oracle.py)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_net_golden import det_state_dict  # noqa: E402
from make_ppo_golden import AGENT_HP, PPO_DEFAULTS  # noqa: E402

from oracle.ppo_oracle import filter_legal, gae_f32  # noqa: E402

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "ppo_golden.npz"))
N, A = 7, 919


def _hp(**kw):
    from blokus_rl_amd.ppo.trainer import PPOHparams

    d = dict(PPO_DEFAULTS, **AGENT_HP, num_steps=7, num_envs=6, agent_type="cnn", board_size=7, max_piece_cells=4)
    d.update(kw)
    return PPOHparams(**d)


def _agent(device="cpu"):
    from blokus_rl_amd.ppo.agent import CnnAgent

    agent = CnnAgent((N, N), A, types.SimpleNamespace(**AGENT_HP))
    agent.load_state_dict(det_state_dict({k: t.shape for k, t in agent.state_dict().items()}))
    return agent.to(device)


def _batch(device="cpu"):
    return {
        "obs": torch.from_numpy(G["agent_obs"]).to(device),
        "actions": torch.from_numpy(G["agent_actions"].astype(np.float32)).to(device),
        "logprobs": torch.from_numpy(G["update_in_logprobs"]).to(device),
        "advantages": torch.from_numpy(G["update_in_advantages"]).to(device),
        "returns": torch.from_numpy(G["update_in_returns"]).to(device),
        "values": torch.from_numpy(G["update_in_values"]).to(device),
    }


# ---------------------------------------------------------------- CPU: oracle + torch parts
def test_oracle_gae_matches_reference_bit_exact():
    adv, ret = gae_f32(G["gae_r"], G["gae_v"], G["gae_d"], G["gae_nv"], G["gae_nd"], 0.99, 0.95)
    assert np.array_equal(adv, G["gae_adv"])
    assert np.array_equal(ret, G["gae_adv"] + G["gae_v"])


def test_oracle_filter_matches_reference():
    assert np.array_equal(filter_legal(G["filter_x"], G["filter_mask"]), G["filter_out"])


def test_agent_layout_and_unmasked_outputs_match_reference():
    agent = _agent()
    ref_keys = sorted(k[len("update_param_"):] for k in G.files if k.startswith("update_param_"))
    assert sorted(agent.state_dict()) == ref_keys
    for k, t in agent.state_dict().items():
        assert tuple(t.shape) == G[f"update_param_{k}"].shape
    with torch.no_grad():
        _, lp, ent, _ = agent.get_action_and_value(torch.from_numpy(G["agent_obs"]),
                                                   torch.from_numpy(G["agent_actions"]))
    np.testing.assert_allclose(lp.numpy(), G["agent_logprob_unmasked"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ent.numpy(), G["agent_entropy_unmasked"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("case,seed,kl", [("update", 123, 0.01), ("update2", 321, None)])
def test_optimize_agent_matches_reference_cpu(case, seed, kl):
    from blokus_rl_amd.ppo.trainer import optimize_agent

    hp = _hp(target_kl=kl)
    agent = _agent()
    opt = torch.optim.Adam(agent.parameters(), lr=hp.learning_rate, eps=hp.eps)
    batch = _batch()
    if case == "update2":
        batch["logprobs"] = torch.from_numpy(G["agent_logprob_unmasked"])
    np.random.seed(seed)
    log = optimize_agent(agent, opt, batch, hp)
    for k, t in agent.state_dict().items():
        np.testing.assert_allclose(t.numpy(), G[f"{case}_param_{k}"], rtol=1e-4, atol=1e-6, err_msg=k)
    for k in ("loss", "value_loss", "policy_loss", "entropy", "approx_kl", "clipfrac"):
        np.testing.assert_allclose(log[k], G[f"{case}_log_{k}"][0], rtol=1e-4, atol=1e-6, err_msg=k)


def test_mask_words_from_id_lists():
    from blokus_rl_amd.ppo.agent import ids_to_mask_words

    m = G["filter_mask"]
    words = ids_to_mask_words([np.flatnonzero(r) for r in m], A, "cpu").numpy().view(np.uint64)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(m.shape[0], -1)[:, :A]
    assert np.array_equal(bits.astype(np.uint8), m)


# ---------------------------------------------------------------- GPU kernels
@pytest.mark.gpu
def test_gae_kernel_matches_reference_and_oracle():
    from blokus_rl_amd.ppo.trainer import compute_gae

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    adv, ret = compute_gae(t(G["gae_r"]), t(G["gae_v"]), t(G["gae_d"]), t(G["gae_nv"]), t(G["gae_nd"]), 0.99, 0.95)
    assert np.array_equal(adv.cpu().numpy(), G["gae_adv"])
    assert np.array_equal(ret.cpu().numpy(), G["gae_adv"] + G["gae_v"])
    # config-5 scale: 32 steps x 8192 envs
    rng = np.random.default_rng(0)
    T, E = 32, 8192
    r = (rng.integers(-1, 2, (T, E)) * (rng.random((T, E)) < 0.1)).astype(np.float32)
    v = rng.standard_normal((T, E)).astype(np.float32)
    d = (rng.random((T, E)) < 0.1).astype(np.float32)
    nv = rng.standard_normal(E).astype(np.float32)
    nd = (rng.random(E) < 0.1).astype(np.float32)
    adv, ret = compute_gae(t(r), t(v), t(d), t(nv), t(nd), 0.99, 0.95)
    ra, rr = gae_f32(r, v, d, nv, nd, 0.99, 0.95)
    assert np.array_equal(adv.cpu().numpy(), ra) and np.array_equal(ret.cpu().numpy(), rr)


@pytest.mark.gpu
def test_filter_kernel_matches_reference():
    from blokus_rl_amd.ppo.agent import FilterLegalMoves, ids_to_mask_words

    m = G["filter_mask"]
    x = torch.from_numpy(G["filter_x"]).cuda()
    out = FilterLegalMoves()(x, [np.flatnonzero(r) for r in m])
    assert np.array_equal(out.cpu().numpy(), G["filter_out"])
    out2 = FilterLegalMoves()(x, ids_to_mask_words([np.flatnonzero(r) for r in m], A, "cuda"))
    assert torch.equal(out, out2)


def _filter_case(E, A, seed):
    """Masks of density ~0.02 with, from three rows up, an all-zero first and an all-ones last row;
    logits normal x 3 with exact +0.0 and -0.0 planted on legal and on illegal ids of every row
    that has both kinds (the reference masks a legal exact zero, and -0.0 == 0)."""
    rng = np.random.default_rng(seed)
    m = (rng.random((E, A)) < 0.02).astype(np.uint8)
    m[:, (0, 1, A - 2, A - 1)] = 1  # the first ids and the last (the last mask word's top used bits)
    if E >= 3:
        m[0], m[-1] = 0, 1
    x = (rng.standard_normal((E, A)) * 3.0).astype(np.float32)
    z = rng.random((E, A))
    x[z < 0.03] = 0.0
    x[(z >= 0.03) & (z < 0.06)] = -0.0
    for e in range(E):
        for ids in (np.flatnonzero(m[e]), np.flatnonzero(m[e] == 0)):
            if ids.size >= 4:
                x[e, ids[[0, -1]]] = (1.5, -2.5)
                x[e, ids[[1, -2]]] = (0.0, -0.0)
    return x, m


@pytest.mark.gpu
@pytest.mark.parametrize("E,A", [(5, 387), (3, 13729), (1, 49), (140, 30433)])
def test_filter_kernel_other_shapes_match_oracle(E, A):
    """bk_filter_legal against oracle.ppo_oracle.filter_legal (a copy or a constant: exact) at
    the 2-player presets' action counts: masks of 7, 215, 1 and 476 words, each with a partly
    used last word, and 140 x 30433 = 4.26 M elements, past the 16384 x 256 grid, so the
    grid-stride loop takes a second trip. Mask bits at positions >= A must change nothing."""
    from blokus_rl_amd.ppo.agent import FilterLegalMoves, ids_to_mask_words

    assert (E * A > 16384 * 256) == (E == 140)
    x_h, m = _filter_case(E, A, seed=A)
    zero = x_h == 0
    neg = np.signbit(x_h)
    for legal in (m == 1, m == 0):  # the planted cases are there
        assert (zero & neg & legal).any() and (zero & ~neg & legal).any() and (~zero & legal).any()
    want = filter_legal(x_h, m)
    x = torch.from_numpy(x_h).cuda()
    ids = [np.flatnonzero(r) for r in m]
    out = FilterLegalMoves()(x, ids)
    assert np.array_equal(out.cpu().numpy(), want)
    words = ids_to_mask_words(ids, A, "cuda")
    assert tuple(words.shape) == (E, (A + 63) // 64) and A % 64 != 0
    assert torch.equal(FilterLegalMoves()(x, words), out)
    stray = words.clone()
    stray[:, -1] |= -1 << (A % 64)  # every bit of the last word from position A up
    assert not torch.equal(stray, words)
    assert torch.equal(FilterLegalMoves()(x, stray), out)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), x_h.view(np.uint32))  # the input is left alone


@pytest.mark.gpu
def test_filter_autograd_routes_gradient_through_kept_logits():
    """FilterLegalMoves with a logits tensor that wants a gradient: the forward values are the
    kernel's, and the gradient is the reference op's (y = x * mask; y[y == 0] = -1e9, restated in
    float64 torch): g where the output kept x, exactly 0 elsewhere (illegal ids and legal zeros)."""
    from blokus_rl_amd.ppo.agent import FilterLegalMoves, ids_to_mask_words

    E, A = 5, 387
    x_h, m = _filter_case(E, A, seed=1)
    words = ids_to_mask_words([np.flatnonzero(r) for r in m], A, "cuda")
    x = torch.from_numpy(x_h).cuda().requires_grad_()
    y = FilterLegalMoves()(x, words)
    assert y.requires_grad and np.array_equal(y.detach().cpu().numpy(), filter_legal(x_h, m))
    g = torch.from_numpy(np.random.default_rng(2).standard_normal((E, A)).astype(np.float32)).cuda()
    y.backward(g)
    x64 = torch.from_numpy(x_h).double().requires_grad_()
    y64 = x64 * torch.from_numpy(m).double()
    y64 = y64.masked_fill(y64 == 0, -1e9)
    y64.backward(g.cpu().double())
    assert torch.equal(x.grad.cpu().double(), x64.grad)
    keep = y.detach() != -1e9
    assert 0 < int(keep.sum()) < int(torch.from_numpy(m).sum())  # some legal logits were zeros
    assert torch.equal(x.grad, torch.where(keep, g, torch.zeros_like(g)))
    with torch.no_grad():  # and without a graph the kernel's output comes back as it is
        assert not FilterLegalMoves()(x, words).requires_grad


@pytest.mark.gpu
def test_agent_masked_outputs_match_reference_gpu():
    agent = _agent("cuda")
    with torch.no_grad():
        _, lp, ent, val = agent.get_action_and_value(torch.from_numpy(G["agent_obs"]).cuda(),
                                                     torch.from_numpy(G["agent_actions"]).cuda(),
                                                     possible_moves=[np.flatnonzero(r) for r in G["agent_mask"]])
    np.testing.assert_allclose(lp.cpu().numpy(), G["agent_logprob"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(ent.cpu().numpy(), G["agent_entropy"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(val.cpu().numpy(), G["agent_value"], rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
def test_optimize_agent_matches_reference_gpu():
    from blokus_rl_amd.ppo.trainer import optimize_agent

    hp = _hp(target_kl=None)
    agent = _agent("cuda")
    opt = torch.optim.Adam(agent.parameters(), lr=hp.learning_rate, eps=hp.eps)
    batch = _batch("cuda")
    batch["logprobs"] = torch.from_numpy(G["agent_logprob_unmasked"]).cuda()
    np.random.seed(321)
    optimize_agent(agent, opt, batch, hp)
    for k, t in agent.state_dict().items():
        np.testing.assert_allclose(t.cpu().numpy(), G[f"update2_param_{k}"], rtol=1e-3, atol=1e-5, err_msg=k)


@pytest.mark.gpu
def test_ppo_trainer_updates_on_device_env(tmp_path):
    from blokus_rl_amd.ppo.trainer import PPOTrainer

    hp = _hp(num_envs=64, num_steps=16, total_timesteps=64 * 16 * 3, agent_type="cnn", save_interval=2,
             checkpoint_dir=tmp_path)
    tr = PPOTrainer(hp)
    logs = tr.train()
    assert len(logs) == 3 and all(np.isfinite(l["loss"]) for l in logs)
    assert tr.global_step == 64 * 16 * 3 and tr.total_episodes > 0
    assert (tmp_path / "checkpoint_2.pt").exists()
    tr2 = PPOTrainer(hp)
    tr2._load_checkpoint(2)
    assert tr2.update == 3


@pytest.mark.gpu
@pytest.mark.parametrize("board_size,max_cells,device_sampling", [
    pytest.param(7, 4, True, id="True"), pytest.param(7, 4, False, id="False"),
    pytest.param(5, 5, None, id="5x5-5-default"), pytest.param(7, 3, None, id="7x7-3-default")])
def test_ppo_rollout_draws(board_size, max_cells, device_sampling):
    """The rollout's draw on the device (bk_vec_policy over the actor's raw logits) or through torch's
    Categorical over FilterLegalMoves (the trainer's own default on the presets without the draw
    kernels): the stored actions are the drawn ones and their log-probs are finite and <= 0; a
    draw is a legal id unless every legal logit of its row is exactly 0 — the reference filter's
    all -1e9 row (ppo/agent.py:40-41), uniform over every id, which the freshly initialised agent
    produces for a few envs whose last hidden layer is all zero. That holds for torch's draw over
    the filter as well: a masked id has probability exp(-1e9 - max) = 0 in float32."""
    from blokus_rl_amd.ppo.trainer import PPOTrainer

    hp = _hp(num_envs=64, num_steps=16, total_timesteps=64 * 16, agent_type="cnn", save_interval=10**6,
             board_size=board_size, max_piece_cells=max_cells)
    tr = PPOTrainer(hp) if device_sampling is None else PPOTrainer(hp, device_sampling=device_sampling)
    assert tr.device_sampling is (tr.envs.policy_kernels if device_sampling is None else device_sampling)
    assert tr.envs.policy_kernels is ((board_size, max_cells) == (7, 4))
    device_sampling = tr.device_sampling
    obs, _ = tr.envs.reset(seed=0)
    masks, acts, rows = [], [], []
    orig_step, orig_sample = tr.envs.step, tr.envs.sample_policy

    def rec_step(action):
        masks.append(tr.envs.valid_mask().clone())
        acts.append(action.long().clone())
        return orig_step(action)

    def rec_sample(logits, zero_masked=True):
        rows.append(logits.clone())
        return orig_sample(logits, zero_masked)

    orig_sp = tr.envs.step_policy

    def rec_step_policy(logits, zero_masked=True):
        masks.append(tr.envs.valid_mask().clone())
        rows.append(logits.clone())
        a, lp = orig_sp(logits, zero_masked)
        acts.append(a.long().clone())
        return a, lp

    tr.envs.step, tr.envs.sample_policy, tr.envs.step_policy = rec_step, rec_sample, rec_step_policy
    if not device_sampling:  # the torch path: the actor's raw logits are the filter's input
        tr.agent.actor.filter_legal_moves.register_forward_hook(lambda mod, args, out: rows.append(args[0].clone()))
    tr._play_env(obs.float(), torch.zeros(64, device=tr.device))
    assert len(acts) == hp.num_steps and len(rows) == hp.num_steps
    illegal = 0
    for t, (m, a) in enumerate(zip(masks, acts)):
        assert torch.equal(tr.memory.actions[t].long(), a)
        bad = ~m.gather(1, a.view(-1, 1)).view(-1)
        no_candidate = ~(m & (rows[t] != 0)).any(dim=1)
        assert bool((no_candidate | ~bad).all()), (t, torch.nonzero(bad & ~no_candidate).view(-1).tolist())
        illegal += int(bad.sum())
    lp = tr.memory.logprobs
    assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())
    if (board_size, max_cells) == (7, 4):
        assert device_sampling or illegal <= 64  # torch's draw over the same filter (same quirk)
