"""The masked-policy draw on every 2-player preset (BlokusVectorEnv(policy_draw="all"): the
one-wave-per-env k_vec_policy_wave and k_vec_step with the draw in front) against its CPU
restatement, oracle/vecenv_oracle.py policy_sample: actions, log-prob bits and the random streams
bit for bit, the env stepped with the drawn ids beside the oracle; the fused step against the two
launches; the staged and the unstaged path of the kernel (BK_VEC_PCAP); the 7x7 kernels against the
wave kernels (BK_VEC_WAVE); a captured graph; log-probs against torch.

The oracle's walk of a preset does not depend on the kernel (it steps with its own draws), so it is
computed once per preset and shared by the tests that use the same schedule."""
import functools

import numpy as np
import pytest
import torch

from oracle.vecenv_oracle import VecEnvOracle

pytestmark = pytest.mark.gpu


def _policy_logits(E, A, t, rng):
    """The recipe of tests/test_vecenv_gpu.py: a spread that changes with t, exact zeros (+0 on 1/8
    of the ids, -0 on 2%), every 5th env all zero (under zero_masked: no candidate -> the all -1e9
    row, uniform over every id)."""
    x = (rng.standard_normal((E, A)) * (0.5 + 4.0 * (t % 3))).astype(np.float32)
    x[rng.random((E, A)) < 0.125] = 0.0
    x[rng.random((E, A)) < 0.02] = -0.0
    x[::5] = 0.0
    return x


def _obs_of(states: np.ndarray, N: int) -> np.ndarray:
    occ = np.ascontiguousarray(states[:, :320]).view(np.uint32).reshape(-1, 4, 20)[:, :2, :N]
    bits = (occ[..., None] >> np.arange(N, dtype=np.uint32)) & 1
    return np.where(bits[:, 0] == 1, 1, np.where(bits[:, 1] == 1, 2, 0)).astype(np.uint8)


def _snapshot(ref):
    return {"states": np.stack(ref.states).copy(), "masks": np.stack([ref.mask(e) for e in range(ref.E)]),
            "rng": np.array(ref.rng, dtype=np.uint64)}


@functools.lru_cache(maxsize=None)
def _oracle_walk(N, cells, E, T):
    """T steps of the schedule on the oracle alone: reset(seed=2), default_rng(11), zero_masked off
    every 4th step. Per step: the logits, the env before the draw, the draw (ids, log-probs, streams
    after it), reward / done and the env after the step. Read-only for its users."""
    ref = VecEnvOracle(E, N, cells)
    ref.reset(seed=2)
    rng = np.random.default_rng(11)
    A = ref.o.A
    steps = []
    for t in range(T):
        zm = t % 4 != 3
        x = _policy_logits(E, A, t, rng)
        before = _snapshot(ref)
        ra, rlp = ref.sample_policy(x, zero_masked=zm)
        drawn_rng = np.array(ref.rng, dtype=np.uint64)
        out = [ref.step(e, int(ra[e])) for e in range(E)]
        steps.append({"zm": zm, "x": x, "before": before, "a": ra, "lp": rlp, "drawn_rng": drawn_rng,
                      "rew": np.array([r for r, _ in out], dtype=np.float32),
                      "done": np.array([d for _, d in out], dtype=np.int32), "after": _snapshot(ref)})
    return {"A": A, "W": ref.o.W, "steps": steps}


def _assert_env_is(env, snap, N, tag):
    st = env.states.cpu().numpy()
    bad = np.nonzero((st != snap["states"]).any(axis=1))[0]
    assert bad.size == 0, (tag, "state", bad[:8])
    assert (env.obs.cpu().numpy() == _obs_of(snap["states"], N)).all(), (tag, "obs")
    m = env.mask_words.cpu().numpy().view(np.uint64)
    assert m.shape == snap["masks"].shape and (m == snap["masks"]).all(), (tag, "mask")
    assert (env.rng.cpu().numpy().view(np.uint64) == snap["rng"]).all(), (tag, "rng")


def _assert_draw_is(a, lp, step, tag):
    got = a.cpu().numpy()
    assert (got == step["a"]).all(), (tag, "action", np.nonzero(got != step["a"])[0][:8])
    assert (lp.cpu().numpy().view(np.uint32) == step["lp"].view(np.uint32)).all(), (tag, "logp")


def _walk_stats(walk):
    """Uniform (all -1e9) rows drawn, the largest legal count, the most legal bits in one mask word:
    from the oracle's masks and log-probs."""
    uniform = maxk = maxw = 0
    for s in walk["steps"]:
        if s["zm"]:
            uniform += int((s["lp"][::5] == 0.0).sum())
        bits = np.unpackbits(s["before"]["masks"].view(np.uint8), axis=1, bitorder="little")
        maxk = max(maxk, int(bits.sum(axis=1).max()))
        maxw = max(maxw, int(bits.reshape(bits.shape[0], -1, 64).sum(axis=2).max()))
    return uniform, maxk, maxw


def _draw_then_step(N, cells, E, T):
    from blokus_rl_amd.vector_env import BlokusVectorEnv

    walk = _oracle_walk(N, cells, E, T)
    env = BlokusVectorEnv(E, N, cells, policy_draw="all")
    assert env.policy_kernels is True and env.eng.A == walk["A"] and env.eng.W == walk["W"]
    env.reset(seed=2)
    for t, s in enumerate(walk["steps"]):
        _assert_env_is(env, s["before"], N, (t, "before"))
        a, lp = env.sample_policy(torch.from_numpy(s["x"]).to(env.device), zero_masked=s["zm"])
        _assert_draw_is(a, lp, s, t)
        assert (env.rng.cpu().numpy().view(np.uint64) == s["drawn_rng"]).all(), (t, "rng after the draw")
        env.step_raw(a)
        assert (env.reward.cpu().numpy() == s["rew"]).all() and (env.done.cpu().numpy() == s["done"]).all(), t
        _assert_env_is(env, s["after"], N, (t, "after"))
    return _walk_stats(walk)


# (N, cells, E, T): W64 = 1 (7x7/1: only owner 0 has a word), 7 / 15 / 6 (5x5/4, 5x5/5, 7x7/3: fewer
# words than owners, an odd count), 56 / 215 / 476 (8x8, 14x14, 20x20: 4 / 14 / 30 words an owner, a
# ragged last round), a partial last word everywhere.
PRESETS = [(5, 4, 5, 40), (5, 5, 5, 40), (7, 1, 5, 12), (7, 3, 5, 40), (8, 5, 5, 40), (14, 5, 4, 16), (20, 5, 4, 14)]
WALK_T = {(N, cells): T for N, cells, _, T in PRESETS}


@pytest.mark.parametrize("N,cells,E,T", PRESETS)
def test_policy_draw_matches_oracle_on_every_preset(N, cells, E, T):
    """sample_policy vs VecEnvOracle.sample_policy at every step (ids, log-prob bits, streams), then
    step_raw with the drawn ids vs the oracle's step (states, obs, masks, streams, reward, done).
    Not vacuous, by the oracle's own masks and log-probs: all -1e9 rows are drawn on every preset,
    rows with >= 400 legal ids on 14x14 and 20x20, a word with >= 8 legal bits on all but 7x7/1."""
    uniform, maxk, maxw = _draw_then_step(N, cells, E, T)
    assert uniform > 0, uniform
    if N >= 14:
        assert maxk >= 400, maxk
    if (N, cells) != (7, 1):
        assert maxw >= 8, maxw


@pytest.mark.parametrize("N,cells,E", [(5, 5, 5), (8, 5, 5), (14, 5, 4), (20, 5, 4)])
def test_fused_policy_step_matches_two_launches_and_oracle(N, cells, E):
    """step_policy(fused=True) (k_vec_step<policy>: the mask built in the kernel) on one env,
    step_policy(fused=False) (k_vec_policy_wave + k_vec_step) on its twin, 12 steps of the schedule:
    everything bit for bit after every step, and the first env against the oracle."""
    from blokus_rl_amd.vector_env import BlokusVectorEnv

    walk = _oracle_walk(N, cells, E, WALK_T[(N, cells)])
    env1, env2 = (BlokusVectorEnv(E, N, cells, policy_draw="all") for _ in range(2))
    env1.reset(seed=2)
    env2.reset(seed=2)
    for t, s in enumerate(walk["steps"][:12]):
        x = torch.from_numpy(s["x"]).to(env1.device)
        a1, l1 = env1.step_policy(x, zero_masked=s["zm"])
        a2, l2 = env2.step_policy(x, zero_masked=s["zm"], fused=False)
        assert torch.equal(a1, a2) and torch.equal(l1.view(torch.int32), l2.view(torch.int32)), t
        for n in ("states", "rng", "obs", "mask_words", "reward", "done"):
            assert torch.equal(getattr(env1, n), getattr(env2, n)), (t, n)
        _assert_draw_is(a1, l1, s, t)
        assert (env1.reward.cpu().numpy() == s["rew"]).all() and (env1.done.cpu().numpy() == s["done"]).all(), t
        _assert_env_is(env1, s["after"], N, t)


def test_policy_draw_unstaged_path_matches_oracle(monkeypatch):
    """The 14x14 walk again with BK_VEC_PCAP=64: rows with more than 64 legal ids (the oracle sees up
    to several hundred) take the kernel's unstaged path, the opening rows still the staged one; the
    same bits either way."""
    monkeypatch.setenv("BK_VEC_PCAP", "64")
    _, maxk, _ = _draw_then_step(14, 5, 4, 16)
    assert 64 < maxk, maxk
    mink = min(int(np.unpackbits(s["before"]["masks"].view(np.uint8), axis=1).sum(axis=1).min())
               for s in _oracle_walk(14, 5, 4, 16)["steps"])
    assert mink <= 64, mink  # and the staged path ran as well


def test_fused_policy_step_unstaged_path_matches_oracle(monkeypatch):
    """k_vec_step<policy> with the staging switched off (BK_VEC_PCAP=0) on 14x14 against the oracle."""
    from blokus_rl_amd.vector_env import BlokusVectorEnv

    monkeypatch.setenv("BK_VEC_PCAP", "0")
    walk = _oracle_walk(14, 5, 4, 16)
    env = BlokusVectorEnv(4, 14, 5, policy_draw="all")
    env.reset(seed=2)
    for t, s in enumerate(walk["steps"][:12]):
        a, lp = env.step_policy(torch.from_numpy(s["x"]).to(env.device), zero_masked=s["zm"])
        _assert_draw_is(a, lp, s, t)
        _assert_env_is(env, s["after"], 14, t)


@pytest.mark.parametrize("cells,E", [(4, 37), (5, 21)])
def test_wave_draw_matches_the_7x7_kernels(cells, E, monkeypatch):
    """BK_VEC_WAVE=1 sends the 7x7 presets through the wave kernels from both entries: sample_policy
    + step_raw and step_policy, 20 steps each, bit for bit what k_vec_policy / k_vec_step7 give with
    the variable unset, from the same seeds."""
    from blokus_rl_amd.vector_env import BlokusVectorEnv

    def run(fused):
        env = BlokusVectorEnv(E, 7, cells)
        env.reset(seed=7)
        rng = np.random.default_rng(3)
        out = []
        for t in range(20):
            zm = t % 4 != 3
            x = torch.from_numpy(_policy_logits(E, env.eng.A, t, rng)).to(env.device)
            if fused:
                a, lp = env.step_policy(x, zero_masked=zm)
            else:
                a, lp = env.sample_policy(x, zero_masked=zm)
                drawn = env.rng.clone()
                env.step_raw(a)
            rec = [a.clone(), lp.view(torch.int32).clone()] + ([] if fused else [drawn])
            out.append(rec + [getattr(env, n).clone() for n in ("states", "rng", "obs", "mask_words", "reward", "done")])
        return out

    for fused in (False, True):
        monkeypatch.delenv("BK_VEC_WAVE", raising=False)
        classic = run(fused)
        monkeypatch.setenv("BK_VEC_WAVE", "1")
        wave = run(fused)
        for t, (c, w) in enumerate(zip(classic, wave)):
            for i, (ct, wt) in enumerate(zip(c, w)):
                assert torch.equal(ct, wt), (fused, t, i)
        assert sum(int(c[-1].sum()) for c in classic) > 0  # episodes ended and reset on the way


def test_policy_step_graph_matches_oracle():
    """14x14, 64 envs, one static logits tensor: a graph of 3 step_policy launches (dynamic LDS with
    the staging) replayed 3 times, the env against the oracle after each replay. Every 5th row is all
    zero: a uniform draw over 13,729 ids, almost surely illegal, so those envs lose and reset while
    the others advance."""
    from blokus_rl_amd.vector_env import BlokusVectorEnv

    E, N = 64, 14
    env = BlokusVectorEnv(E, N, 5, policy_draw="all")
    ref = VecEnvOracle(E, N, 5)
    env.reset(seed=4)
    ref.reset(seed=4)
    x = _policy_logits(E, env.eng.A, 1, np.random.default_rng(4))
    logits = torch.from_numpy(x).to(env.device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(3):
            env.step_policy(logits)
    torch.cuda.synchronize()
    ended, advanced = np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64)
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        for _ in range(3):
            ra, rlp = ref.sample_policy(x)
            last = [ref.step(e, int(ra[e])) for e in range(E)]
            ended += np.array([d for _, d in last])
            advanced += np.array([1 - d for _, d in last])
        assert (env.actions.cpu().numpy() == ra).all(), r
        assert (env.logp.cpu().numpy().view(np.uint32) == rlp.view(np.uint32)).all(), r
        _assert_env_is(env, _snapshot(ref), N, r)
        assert env.reward.cpu().numpy().tolist() == [x_ for x_, _ in last], r
        assert env.done.cpu().numpy().tolist() == [d for _, d in last], r
    assert (ended[::5] > 0).all() and advanced[np.arange(E) % 5 != 0].min() > 0, (ended, advanced)


def test_wave_draw_logprob_vs_torch():
    """One 14x14 state three plies in, zero_masked off: log-probs against log_softmax of the masked
    logits (float64) at the tolerance of the 7x7 check (rtol = atol = 2e-6), every drawn id legal."""
    from blokus_rl_amd.vector_env import BlokusVectorEnv

    E = 64
    env = BlokusVectorEnv(E, 14, 5, policy_draw="all")
    env.reset(seed=1)
    for _ in range(3):
        env.step_raw(None)
    assert int(env.done.sum()) == 0
    x = (torch.randn(E, env.eng.A, generator=torch.Generator().manual_seed(0)) * 1.5).to(env.device)
    legal = env.valid_mask()
    want_all = torch.log_softmax(env.masked_logits(x).double(), dim=1)
    for _ in range(4):  # four draws from the same state (the stream advances)
        a, lp = env.sample_policy(x, zero_masked=False)
        assert bool(legal.gather(1, a.long().view(-1, 1)).all())
        want = want_all.gather(1, a.long().view(-1, 1)).view(-1).float()
        print("max |logp - log_softmax|:", float((lp - want).abs().max()))
        torch.testing.assert_close(lp, want, rtol=2e-6, atol=2e-6)


def test_policy_draw_option():
    """The default env keeps `policy_kernels` False and the refusal on the generic presets;
    policy_draw="all" (by argument or BK_VEC_POLICY) turns the kernels on; anything else is a ValueError."""
    from blokus_rl_amd.vector_env import BlokusVectorEnv

    env = BlokusVectorEnv(2, 14, 5)
    assert env.policy_kernels is False
    env.reset(seed=0)
    with pytest.raises(ValueError, match="board_size=14, max_piece_cells=5"):
        env.step_policy(torch.zeros(2, env.eng.A, device=env.device))
    assert BlokusVectorEnv(2, 14, 5, policy_draw="classic").policy_kernels is False
    for N, cells in ((5, 5), (7, 3), (8, 5), (14, 5), (20, 5), (7, 4)):
        assert BlokusVectorEnv(2, N, cells, policy_draw="all").policy_kernels is True
    for bad in ("", "ALL", "7x7", "on"):
        with pytest.raises(ValueError, match="policy_draw"):
            BlokusVectorEnv(2, 7, 4, policy_draw=bad)


def test_policy_draw_option_from_the_environment(monkeypatch):
    from blokus_rl_amd.vector_env import BlokusVectorEnv

    monkeypatch.setenv("BK_VEC_POLICY", "all")
    assert BlokusVectorEnv(2, 8, 5).policy_kernels is True
    assert BlokusVectorEnv(2, 8, 5, policy_draw="classic").policy_kernels is False
    monkeypatch.setenv("BK_VEC_POLICY", "every")
    with pytest.raises(ValueError, match="policy_draw"):
        BlokusVectorEnv(2, 8, 5)
    monkeypatch.delenv("BK_VEC_POLICY")
    assert BlokusVectorEnv(2, 8, 5).policy_kernels is False
