"""PPOTrainer(policy_draw="all"): the rollout's draw inside the env step (bk_vec_step_policy through
the one-wave-per-env kernel) on presets other than 7x7/4|5, with the invariants of
tests/test_ppo.py test_ppo_rollout_draws, and one update."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_ppo_golden import AGENT_HP, PPO_DEFAULTS  # noqa: E402

pytestmark = pytest.mark.gpu


def _hp(**kw):
    from blokus_rl_amd.ppo.trainer import PPOHparams

    d = dict(PPO_DEFAULTS, **AGENT_HP, agent_type="cnn", save_interval=10**6)
    d.update(kw)
    return PPOHparams(**d)


@pytest.mark.parametrize("board_size,num_envs,num_steps", [(5, 64, 16), (14, 16, 8)])
def test_ppo_rollout_draws_on_the_device_under_policy_draw_all(board_size, num_envs, num_steps):
    """The stored actions are the drawn ones, their log-probs finite and <= 0, and a draw is a legal
    id unless no legal logit of its row is non-zero (the all -1e9 row: uniform over every id)."""
    from blokus_rl_amd.ppo.trainer import PPOTrainer

    hp = _hp(num_envs=num_envs, num_steps=num_steps, total_timesteps=num_envs * num_steps, board_size=board_size,
             max_piece_cells=5)
    assert PPOTrainer(hp).device_sampling is False  # the default stays torch's Categorical here
    with pytest.raises(ValueError, match=f"board_size={board_size}, max_piece_cells=5"):
        PPOTrainer(hp, device_sampling=True)
    tr = PPOTrainer(hp, policy_draw="all")
    assert tr.envs.policy_kernels is True and tr.device_sampling is True
    obs, _ = tr.envs.reset(seed=0)
    masks, acts, rows = [], [], []
    orig_sp = tr.envs.step_policy

    def rec_step_policy(logits, zero_masked=True):
        masks.append(tr.envs.valid_mask().clone())
        rows.append(logits.clone())
        a, lp = orig_sp(logits, zero_masked)
        acts.append(a.long().clone())
        return a, lp

    def no_step(action):
        raise AssertionError("the torch path ran")

    tr.envs.step_policy, tr.envs.step = rec_step_policy, no_step
    tr._play_env(obs.float(), torch.zeros(num_envs, device=tr.device))
    assert len(acts) == num_steps and len(rows) == num_steps
    legal_draws = 0
    for t, (m, a) in enumerate(zip(masks, acts)):
        assert torch.equal(tr.memory.actions[t].long(), a)
        bad = ~m.gather(1, a.view(-1, 1)).view(-1)
        no_candidate = ~(m & (rows[t] != 0)).any(dim=1)
        assert bool((no_candidate | ~bad).all()), (t, torch.nonzero(bad & ~no_candidate).view(-1).tolist())
        legal_draws += int((~bad).sum())
    lp = tr.memory.logprobs
    assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())
    assert legal_draws > 0


def test_ppo_update_under_policy_draw_all():
    from blokus_rl_amd.ppo.trainer import PPOTrainer

    hp = _hp(num_envs=64, num_steps=16, total_timesteps=64 * 16, board_size=5, max_piece_cells=5)
    tr = PPOTrainer(hp, policy_draw="all")
    assert tr.device_sampling is True
    logs = tr.train(num_updates=1)
    assert len(logs) == 1 and np.isfinite(logs[0]["loss"])
    assert tr.global_step == 64 * 16
