"""Shared helpers of the arena rows tests (no tests here): the per-stage reference of a ply's
search — the existing whole-batch entries, once per net — the rows drivers, and the arena's Python
bookkeeping. Trees are independent, so running the nets' trees one net after the other leaves the
trees of the rows entries, which run them side by side."""
import math
from itertools import permutations

import torch


def leaf_net(eng, seed, blocks=1):
    from blokus_rl_amd.nets import LeafResNet, ResNet

    torch.manual_seed(seed)
    net = ResNet(eng.N, eng.P, eng.A, blocks).to(eng.device).eval()
    leaf = LeafResNet(net, normalize=False, features=True, x3_boards="all").eval()
    assert leaf.takes_states()
    return net, leaf


def head_of(leaf):
    po = leaf.f.policy_out
    return po.weight.detach().float().contiguous(), po.bias.detach().float().contiguous()


def orders_of(G, P, permute, device):
    matches = list(permutations(range(P))) if permute else [tuple(range(P))]
    return torch.tensor([matches[i % len(matches)] for i in range(G)], dtype=torch.int64, device=device)


def tables_of(eng, states, orders, seat_net, seat_sims, over):
    """BatchedArena.play's per-ply bookkeeping: (tree, net, sims) int32[G], tree -1 where over."""
    from blokus_rl_amd.engine import Engine

    G, P = orders.shape
    to_move = Engine.to_move(states).long()
    pidx = orders.gather(1, to_move.view(-1, 1)).view(-1)
    tree = torch.arange(G, device=states.device) * P + pidx
    tree = torch.where(over, torch.full_like(tree, -1), tree)
    i32 = lambda t: t.to(torch.int32).contiguous()  # noqa: E731
    return i32(tree), i32(seat_net[pidx]), i32(seat_sims[pidx])


class PerStage:
    """One ply's simulations with the per-stage entries, once per net: select with active = 1
    exactly on that net's live trees (every other tree gets status 0), forward_states, leaf_logits
    with that net's head, expand_backup(None, v, 2); the uninformed seat: expand_backup(const, 0, 0)."""

    def __init__(self, eng, mcts, leaves, cpuct):
        self.eng, self.mcts, self.leaves, self.cpuct = eng, mcts, leaves, cpuct
        self.heads = [head_of(m) for m in leaves]
        T = mcts.T
        self.const_logp = torch.full((T, eng.A), -math.log(float(eng.A)), dtype=torch.float32, device=eng.device)
        self.zero_v = torch.zeros((T, eng.P), dtype=torch.float32, device=eng.device)

    def ply(self, roots, tree, net_row, sims_row, max_sims):
        eng, m = self.eng, self.mcts
        roots_t = roots.repeat_interleave(eng.P, dim=0)
        for s in range(max_sims):
            live = (tree >= 0) & (sims_row > s)
            for k in range(-1, len(self.leaves)):
                sel = live & (net_row == k)
                if not bool(sel.any()):
                    continue
                active = torch.zeros(m.T, dtype=torch.int32, device=eng.device)
                active[tree[sel].long()] = 1
                m.select(roots_t, active, self.cpuct)
                if k < 0:
                    m.expand_backup(self.const_logp, self.zero_v, 0)
                    continue
                states, _ = m.leaf_info()
                pf, v = self.leaves[k].forward_states(states, m.status)
                m.leaf_logits(pf.contiguous(), *self.heads[k])
                m.expand_backup(None, v.contiguous(), 2)

    def move(self, roots, tree):
        """root_policy(T = 0) + argmax on the live rows' trees (BatchedArena.play's move)."""
        eng, m = self.eng, self.mcts
        dev = eng.device
        over = tree < 0
        tr = tree.clamp(min=0).long()
        roots_t = roots.repeat_interleave(eng.P, dim=0)
        act_t = torch.zeros(m.T, dtype=torch.int32, device=dev)
        act_t[tr[~over]] = 1
        ids, pi, counts = m.root_policy(roots_t, act_t, 0.0)
        ids_g, pi_g, k = ids.index_select(0, tr), pi.index_select(0, tr), counts.index_select(0, tr).clamp(min=0)
        col = torch.arange(pi_g.shape[1], device=dev).unsqueeze(0)
        pi_g = torch.where(col < k.unsqueeze(1), pi_g, torch.full_like(pi_g, -1.0))
        action = ids_g.gather(1, pi_g.argmax(dim=1).view(-1, 1)).view(-1)
        return torch.where(over | (k == 0), torch.full_like(action, -1), action).to(torch.int32).contiguous()


class Rows:
    """The same ply through the rows entries, launch by launch or as one bk_arena_sims call
    (optionally captured once and replayed). The tables and roots are fixed buffers."""

    def __init__(self, eng, mcts, leaves, G, max_sims, cpuct, mode):
        from blokus_rl_amd.engine import arena_heads, arena_rows
        from blokus_rl_amd.nets import leafnet_x3_table

        self.eng, self.mcts, self.cpuct, self.mode, self.max_sims = eng, mcts, cpuct, mode, max_sims
        dev = eng.device
        T = mcts.T
        self.pf = torch.zeros((T, 2 * eng.N * eng.N), dtype=torch.float32, device=dev)
        self.vout = torch.zeros((T, eng.P), dtype=torch.float32, device=dev)
        self.tabs = [torch.full((G,), -1, dtype=torch.int32, device=dev) for _ in range(3)]
        self.rows = arena_rows(*self.tabs, T)
        self.roots = eng.init_states(G)
        self.leaves = leaves
        self.table = leafnet_x3_table(leaves, self.pf, self.vout, mcts.leaf_states_ptr, mcts.status) if leaves else None
        self.heads = arena_heads([head_of(m) for m in leaves])
        self.graph = None
        if mode == "graph":
            self._sims()  # every row dead: launches everything once, touches nothing
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._sims()

    def _sims(self):
        self.mcts.arena_sims(self.table, self.rows, self.max_sims, self.heads, self.pf, self.vout, self.roots,
                             self.cpuct)

    def ply(self, roots, tree, net_row, sims_row):
        from blokus_rl_amd.nets import leafnet_x3_rows

        for dst, src in zip(self.tabs, (tree, net_row, sims_row)):
            dst.copy_(src)
        self.roots.copy_(roots)
        if self.mode == "graph":
            self.graph.replay()
        elif self.mode == "sims":
            self._sims()
        else:
            m = self.mcts
            m.select_rows(self.rows, self.roots, self.cpuct)
            for s in range(self.max_sims):
                leafnet_x3_rows(self.table, self.rows, s, self.eng.device)
                m.leaf_step_rows(self.rows, s, self.pf, self.heads, self.vout,
                                 self.roots if s + 1 < self.max_sims else None, self.cpuct)

    def move(self):
        return self.mcts.arena_move(self.rows, self.roots)


def compare_trees(m1, m2, roots_t, seen):
    """root_stats (ids, N, Q, P, counts) of every tree used so far at its latest root, and the
    counters: equal bitwise."""
    for x, y in zip(m1.root_stats(roots_t, seen), m2.root_stats(roots_t, seen)):
        assert torch.equal(x, y)
    c1, c2 = m1.counters(), m2.counters()
    assert c1 == c2, (c1, c2)
    return c1
