"""Batched Arena: `play_match` (blokus_rl/alphazero/arena.py:10-87) for
MCTSPlayer seats (players/mcts_player.py:8-28), every game of the match played at once on the
batched engine.

Reference semantics kept exactly:
  * game i seats the players in order matches[i % len(matches)] (all permutations of the
    player list when permute, else the identity); colour c is played by player order[c];
  * each player owns its own MCTS, fresh at the start of every game (player.reset()) and kept
    across that player's moves of the game;
  * a move = `simulations` MCTS.simulate calls from the current state, then the T=0
    distribution's argmax (first max N) — deterministic given the priors;
  * scores[order] += the game's -1 / 3 / 1 one-hot (get_game_ended).

Layout: one tree per (game, player) — T = games x P trees in one BatchedMCTS; at each ply only
the tree of the player to move is active in each game. The G leaves of a simulation step are
gathered into one [G, 2P, N, N] batch; each distinct net evaluates it once (the arena compare
has two: the new net and the previous one) and rows are picked per game by the seat's net.
DumbNet seats (the "uninformed MCTS" player) get the uniform log-prior and zero values.

path="graph" (or BK_ARENA=graph; default "eager", the loop above): a ply's simulations are one
captured, linear graph of select_rows + max_sims x {leafnet_x3_rows, leaf_step_rows}
(bk_arena_sims): one workgroup per game finds its tree, its net and its budget in three device
tables, so an N-net match evaluates one net per leaf, with the sparse policy head, and the ply's
tail is arena_move, next_state, game_ended and arena_finish with no host sync (the host reads the
count of running games every 8 plies). Net seats need the packed-state split-f16 leaf net
(LeafResNet.takes_states) and nets of one shape; otherwise the arena plays the eager path and
says why in path_reason. The sparse head's logits differ from the dense head's in the last bits,
so games with net seats may diverge between the two paths (both fp32-class); uninformed seats
are exact.
"""
from __future__ import annotations

import os
from itertools import permutations

import numpy as np
import torch

from ..engine import Engine
from .batched_mcts import BatchedMCTS
from .selfplay import LeafEvaluator


class ArenaSeat:
    """One arena player: a net (None / DumbNet = uninformed MCTS) and its simulation count."""

    def __init__(self, model: torch.nn.Module | None, simulations: int):
        self.model = model
        self.simulations = int(simulations)


def seat_of(player) -> ArenaSeat:
    """An MCTSPlayer of the drop-in API (players.MCTSPlayer) -> its seat."""
    nn = getattr(player, "nn", None)
    if nn is None or not hasattr(player, "simulations"):
        raise TypeError(f"the batched arena plays MCTSPlayer seats only, got {player}")
    model = getattr(nn, "model", nn)
    return ArenaSeat(model, player.simulations)


def arena_finish_np(to_move, ended, scores, status, orders, seat_net, seat_sims, over, final, illegal=0):
    """bk_arena_finish restated in NumPy (the tests' oracle): from the next states' to_move [R],
    game_ended's ended [R] / scores [R, P], next_state's status [R], and the running over [R] /
    final [R, P] / illegal -> (tree_of_row, net_of_row, sims_of_row, over, final, illegal, running)."""
    to_move, ended, status = np.asarray(to_move), np.asarray(ended) != 0, np.asarray(status)
    orders, over = np.asarray(orders), np.asarray(over) != 0
    R, P = orders.shape
    illegal = int(bool(illegal) or bool(((status != 0) & ~over).any()))
    final = np.where((ended & ~over)[:, None], np.asarray(scores, dtype=np.float64), np.asarray(final, dtype=np.float64))
    over = over | ended
    player = orders[np.arange(R), to_move]
    tree = np.where(over, -1, np.arange(R) * P + player).astype(np.int32)
    net = np.asarray(seat_net)[player].astype(np.int32)
    sims = np.asarray(seat_sims)[player].astype(np.int32)
    return tree, net, sims, over.astype(np.uint8), final, illegal, int((~over).sum())


class BatchedArena:
    def __init__(self, eng: Engine, seats: list, cpuct: float = 1.0, node_cap: int | None = None,
                 child_cap_per_tree: int | None = None, nn_dtype: torch.dtype = torch.float32,
                 path: str | None = None, record_actions: bool = False, x3_boards: str | None = None):
        self.eng = eng
        self.seats = [s if isinstance(s, ArenaSeat) else seat_of(s) for s in seats]
        if len(self.seats) != eng.P:
            raise ValueError(f"{eng.P} players expected, got {len(self.seats)}")
        self.cpuct = cpuct
        if node_cap is None:
            # a seat's tree lives for the whole game and grows by <= sims nodes on each of its
            # player's plies (at most num_pieces of them)
            node_cap = max(s.simulations for s in self.seats) * eng.num_pieces + 1
        self.node_cap = node_cap
        self.child_cap_per_tree = child_cap_per_tree or node_cap * (256 if eng.N >= 14 else 64)
        self.nn_dtype = nn_dtype
        self.path = path if path is not None else os.environ.get("BK_ARENA", "eager")
        if self.path not in ("eager", "graph"):
            raise ValueError(f"path / BK_ARENA must be eager or graph, got {self.path!r}")
        self.path_reason = ""       # why a requested graph path fell back to eager ("" = it did not)
        self.path_used = None       # the path the last play() took
        self.record_actions = record_actions
        self.last_actions = None    # record_actions (graph path): [plies, G] int32, -1 = no move
        self.counters = None        # graph path: the search's counters after the last play()
        self.x3_boards = x3_boards  # the leaf net's board coverage (None: each model's own / BK_X3_BOARDS)
        # distinct nets (by identity) -> evaluator index; seat -> net index
        self._models: list = []
        self.seat_net = []
        for s in self.seats:
            m = s.model
            if m is not None and m.__class__.__name__ == "DumbNet":
                m = None
            for i, mm in enumerate(self._models):
                if mm is m:
                    self.seat_net.append(i)
                    break
            else:
                self._models.append(m)
                self.seat_net.append(len(self._models) - 1)

    def play(self, games_num: int, permute: bool = False, max_plies: int = 10_000):
        """-> (scores float64[P] accumulated per player, per-game score rows [G][P], final states)."""
        self.path_used = "eager"
        if self.path == "graph":
            evals = self._graph_evaluators()
            if evals is not None:
                self.path_used = "graph"
                return self._play_graph(games_num, permute, max_plies, evals)
        eng, P, G = self.eng, self.eng.P, games_num
        dev = eng.device
        matches = list(permutations(range(P))) if permute else [tuple(range(P))]
        orders = torch.tensor([matches[i % len(matches)] for i in range(G)], dtype=torch.int64, device=dev)  # [G,P]
        T = G * P
        mcts = BatchedMCTS(eng, T, node_cap=self.node_cap, child_cap=T * self.child_cap_per_tree)
        evals = [LeafEvaluator(m, eng, G, self.nn_dtype, use_graph=m is not None, sparse_policy=False)
                 for m in self._models]
        seat_net = torch.tensor(self.seat_net, dtype=torch.int64, device=dev)
        seat_sims = torch.tensor([s.simulations for s in self.seats], dtype=torch.int64, device=dev)
        max_sims = max(s.simulations for s in self.seats)
        states = eng.init_states(G)
        logp = torch.zeros((T, eng.A), dtype=torch.float32, device=dev)
        vals = torch.zeros((T, P), dtype=torch.float32, device=dev)
        garange = torch.arange(G, device=dev)
        over = torch.zeros(G, dtype=torch.bool, device=dev)
        final = torch.zeros((G, P), dtype=torch.float64, device=dev)
        for _ in range(max_plies):
            to_move = Engine.to_move(states).long()
            pidx = orders.gather(1, to_move.view(-1, 1)).view(-1)     # player index at each game's turn
            tree = garange * P + pidx                                    # its tree
            roots = states.repeat_interleave(P, dim=0)
            net_row = seat_net[pidx]
            sims_row = seat_sims[pidx]
            for s in range(max_sims):
                act_g = (~over) & (sims_row > s)
                active = torch.zeros(T, dtype=torch.int32, device=dev)
                active[tree] = act_g.to(torch.int32)
                _, obs, _ = mcts.select(roots, active, self.cpuct)
                obs_g = obs.index_select(0, tree)
                lp_g = None
                v_g = None
                for n, ev in enumerate(evals):
                    lp, v = ev(obs_g)
                    if len(evals) == 1:
                        lp_g, v_g = lp, v
                        break
                    pick = (net_row == n).view(-1, 1)
                    lp_g = lp if lp_g is None else torch.where(pick, lp, lp_g)
                    v_g = v if v_g is None else torch.where(pick, v, v_g)
                logp.index_copy_(0, tree, lp_g.expand(G, -1) if lp_g.shape[0] != G else lp_g)
                vals.index_copy_(0, tree, v_g.expand(G, -1) if v_g.shape[0] != G else v_g)
                mcts.expand_backup(logp, vals, prior_mode=0)
            act_t = torch.zeros(T, dtype=torch.int32, device=dev)
            act_t[tree] = (~over).to(torch.int32)
            ids, pi, counts = mcts.root_policy(roots, act_t, 0.0)
            ids_g, pi_g = ids.index_select(0, tree), pi.index_select(0, tree)
            k = counts.index_select(0, tree)
            if bool(((k < 0) & ~over).any()):
                raise RuntimeError("arena: a root had more children than the root_policy cap")
            k = k.clamp(min=0)
            col = torch.arange(pi_g.shape[1], device=dev).unsqueeze(0)
            pi_g = torch.where(col < k.unsqueeze(1), pi_g, torch.full_like(pi_g, -1.0))
            best = pi_g.argmax(dim=1)  # first max, as np.argmax over the one-hot distribution
            action = ids_g.gather(1, best.view(-1, 1)).view(-1)
            action = torch.where(over | (k == 0), torch.full_like(action, -1), action).to(torch.int32)
            states, _, status = eng.next_state(states, action.contiguous())
            if bool((status != 0).any()):
                raise RuntimeError("arena: an MCTS move was illegal")
            ended, scores = eng.game_ended(states)
            newly = ended.bool() & ~over
            final = torch.where(newly.view(-1, 1), scores.to(torch.float64), final)
            over |= ended.bool()
            if bool(over.all()):
                break
        mcts.check()
        return self._totals(final, orders, states)

    def _totals(self, final, orders, states):
        P = self.eng.P
        per_game = final.cpu().numpy()
        ords = orders.cpu().numpy()
        total = np.zeros(P)
        for g in range(per_game.shape[0]):
            total[list(ords[g])] += per_game[g]
        return total, per_game, states

    # ------------------------------------------------------------------ path="graph"
    def _graph_evaluators(self):
        """One sparse LeafEvaluator per distinct net seat, or None (and path_reason) when the graph
        path cannot take these seats."""
        from ..engine import ARENA_MAX_NETS

        self.path_reason = ""
        models = [m for m in self._models if m is not None]
        if len(models) > ARENA_MAX_NETS:
            self.path_reason = f"{len(models)} distinct nets, the net table holds {ARENA_MAX_NETS}"
            return None
        evals = []
        for m in models:
            ev = LeafEvaluator(m, self.eng, 1, self.nn_dtype, use_graph=False, sparse_policy=True,
                               x3_boards=self.x3_boards if self.x3_boards is not None else getattr(m, "x3_boards", None))
            # (the net table is the ResNet's: a DCNNet that takes states has no bk_leafnet_args form)
            if not (ev.takes_states and getattr(ev.model, "pipelines", False)):
                self.path_reason = (f"{type(m).__name__} seat: no packed-state split-f16 leaf net for it "
                                    f"({self.eng.N}x{self.eng.N}, {self.eng.P} players, x3_boards / BK_NET_MATH)")
                return None
            evals.append(ev)
        if evals:
            from ..nets import leafnet_x3_table
            try:  # the shapes only; the real table is built on the match's buffers
                dev = self.eng.device
                F = 2 * self.eng.N * self.eng.N
                leafnet_x3_table([ev.model for ev in evals], torch.empty((1, F), device=dev),
                                 torch.empty((1, self.eng.P), device=dev), torch.empty((1, 384), dtype=torch.uint8, device=dev),
                                 torch.zeros(1, dtype=torch.int32, device=dev))
            except (ValueError, AssertionError) as e:
                self.path_reason = f"the nets do not fit one table: {e}"
                return None
        return evals

    def _play_graph(self, games_num: int, permute: bool, max_plies: int, evals: list):
        from ..engine import arena_heads, arena_rows
        from ..nets import leafnet_x3_table

        eng, P, G = self.eng, self.eng.P, games_num
        dev = eng.device
        i32 = dict(dtype=torch.int32, device=dev)
        matches = list(permutations(range(P))) if permute else [tuple(range(P))]
        orders = torch.tensor([matches[i % len(matches)] for i in range(G)], **i32)  # [G,P]
        T = G * P
        mcts = BatchedMCTS(eng, T, node_cap=self.node_cap, child_cap=T * self.child_cap_per_tree)
        # seat -> index into the table of net seats, -1 = uninformed
        informed = [i for i, m in enumerate(self._models) if m is not None]
        seat_net = torch.tensor([informed.index(n) if n in informed else -1 for n in self.seat_net], **i32)
        seat_sims = torch.tensor([s.simulations for s in self.seats], **i32)
        max_sims = max(s.simulations for s in self.seats)
        pf = torch.zeros((T, 2 * eng.N * eng.N), dtype=torch.float32, device=dev)
        vout = torch.zeros((T, P), dtype=torch.float32, device=dev)
        table = leafnet_x3_table([ev.model for ev in evals], pf, vout, mcts.leaf_states_ptr, mcts.status) if evals else None
        heads = arena_heads([(ev.policy_w, ev.policy_b) for ev in evals])
        roots = eng.init_states(G)
        nxt = eng.empty_states(G)
        tabs = [torch.full((G,), -1, **i32) for _ in range(3)]
        rows = arena_rows(*tabs, T)
        over = torch.zeros(G, dtype=torch.uint8, device=dev)
        final = torch.zeros((G, P), dtype=torch.float64, device=dev)
        ended = torch.zeros(G, **i32)
        scores = torch.zeros((G, P), dtype=torch.float64, device=dev)
        status = torch.zeros(G, **i32)
        nplayer = torch.zeros(G, **i32)
        action = torch.full((G,), -1, **i32)
        illegal = torch.zeros(1, **i32)
        running = torch.zeros(1, **i32)
        # every row is dead here: one uncaptured pass that launches everything and touches nothing
        mcts.arena_sims(table, rows, max_sims, heads, pf, vout, roots, self.cpuct)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            mcts.arena_sims(table, rows, max_sims, heads, pf, vout, roots, self.cpuct)
        # the first ply's tables from the initial states (nothing ended, nothing illegal)
        eng.arena_finish(roots, ended, scores, status, orders, seat_net, seat_sims, *tabs, over, final, illegal, running)
        acts = [] if self.record_actions else None
        for ply in range(max_plies):
            graph.replay()
            mcts.arena_move(rows, roots, action)
            if acts is not None:
                acts.append(action.clone())
            eng.next_state_into(roots, action, nxt, nplayer, status)
            eng.game_ended_into(nxt, ended, scores)
            eng.arena_finish(nxt, ended, scores, status, orders, seat_net, seat_sims, *tabs, over, final, illegal,
                             running)
            roots.copy_(nxt)
            if ply % 8 == 7 and int(running.item()) == 0:
                break
        if acts is not None:
            a = torch.stack(acts).cpu().numpy() if acts else np.zeros((0, G), dtype=np.int32)
            live = (a >= 0).any(axis=1)
            self.last_actions = a[: int(np.nonzero(live)[0].max()) + 1] if live.any() else a[:0]
        if int(illegal.item()):
            raise RuntimeError("arena: an MCTS move was illegal")
        self.counters = mcts.check()
        return self._totals(final, orders.long(), roots)


def play_match_batched(game, players: list, games_num: int, permute: bool = False, cpuct: float = 1.0,
                       node_cap: int | None = None, path: str | None = None):
    """play_match(game, players, games_num, permute) (arena.py:10-32) for MCTSPlayer seats,
    batched: -> (scores, items) with items[i] = {"scores": game i's one-hot, "frames": []}."""
    arena = BatchedArena(game.engine, players, cpuct=cpuct, node_cap=node_cap, path=path)
    scores, per_game, _ = arena.play(games_num, permute)
    return scores, [{"scores": per_game[i], "frames": []} for i in range(games_num)]
