"""Batched MCTS: T trees on one GPU, one simulation in flight per tree (bk_mcts_* C-ABI).

A simulation of the reference `MCTS.simulate` (blokus_rl/alphazero/mcts.py:13-71) is
`select()` -> one batched net forward over every tree's leaf -> `expand_backup()`. Because each
tree keeps exactly one simulation in flight, each tree's sequence of visits is the one the
reference's sequential recursion produces for the same priors and values.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ..engine import Engine, EngineError, _check, _ptr


_OWN_OBS = object()  # leaf_step(obs=...): the default, BatchedMCTS.obs


class BatchedMCTS:
    def __init__(self, eng: Engine, trees: int, node_cap: int = 8192, child_cap: int | None = None):
        self.eng = eng
        self.lib = eng.lib
        self.T = trees
        self.node_cap = node_cap
        if child_cap is None:
            # ~ node_cap nodes x mean branching; 20x20 trajectories average K ~ 211
            per_node = 256 if eng.N >= 14 else 64
            child_cap = trees * node_cap * per_node
        self.child_cap = child_cap
        h = ctypes.c_void_p()
        with torch.cuda.device(eng.device):
            _check(self.lib.bk_mcts_create(eng.h, trees, node_cap, ctypes.c_int64(child_cap), ctypes.byref(h)))
        self.h = h
        dev = eng.device
        self.status = torch.zeros(trees, dtype=torch.int32, device=dev)
        self.obs = torch.zeros((trees,) + eng.obs_shape, dtype=torch.float32, device=dev)
        self.leaf_mask = torch.zeros((trees, eng.W), dtype=torch.int64, device=dev)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.bk_mcts_destroy(self.h)
                self.h = None
        except Exception:  # pragma: no cover
            pass

    def _s(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.eng.device).cuda_stream)

    def reset(self, flags: torch.Tensor | None = None):
        _check(self.lib.bk_mcts_reset(self.h, _ptr(flags), self._s()))

    def select(self, roots: torch.Tensor, active: torch.Tensor | None, cpuct: float = 1.0, root_eps: float = 1e-6):
        """Descend every active tree to a leaf; returns (status[T], obs[T,2P,N,N], mask[T,W]).
        root_eps: the root's term under the square root of mcts.py:43 (1e-6 = epsilon_fix, 0 = not)."""
        if root_eps == 1e-6:
            _check(self.lib.bk_mcts_select(self.h, _ptr(roots), _ptr(active), float(cpuct), _ptr(self.status),
                                           _ptr(self.obs), _ptr(self.leaf_mask), self._s()))
        else:
            _check(self.lib.bk_mcts_select_eps(self.h, _ptr(roots), _ptr(active), float(cpuct), float(root_eps),
                                               _ptr(self.status), _ptr(self.obs), _ptr(self.leaf_mask), self._s()))
        return self.status, self.obs, self.leaf_mask

    def expand_backup(self, logp: torch.Tensor | None, values: torch.Tensor, prior_mode: int = 0):
        """prior_mode 0: dense logits/log-probs [T, A]; 1: priors at the legal ids (test hook);
        2: the sparse logits of leaf_logits() (logp None)."""
        assert values.dtype == torch.float32 and values.shape == (self.T, self.eng.P)
        if prior_mode != 2:
            assert logp.dtype == torch.float32 and logp.shape == (self.T, self.eng.A)
        _check(self.lib.bk_mcts_expand_backup(self.h, _ptr(logp), _ptr(values), prior_mode, self._s()))

    def leaf_logits(self, feat: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor):
        """Policy logits of each leaf's legal ids only (bk_mcts_leaf_logits): feat [T, F] f32,
        weight [A, F], bias [A] — the policy head's last Linear — for expand_backup(mode 2)."""
        assert feat.dtype == torch.float32 and feat.shape[0] == self.T and feat.stride(1) == 1
        assert weight.is_contiguous() and weight.shape == (self.eng.A, feat.shape[1]) and bias.shape == (self.eng.A,)
        _check(self.lib.bk_mcts_leaf_logits(self.h, ctypes.c_void_p(feat.data_ptr()), feat.stride(0), feat.shape[1],
                                            _ptr(weight), _ptr(bias), self._s()))

    def leaf_step(self, feat: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, values: torch.Tensor,
                  roots: torch.Tensor | None = None, active: torch.Tensor | None = None, cpuct: float = 1.0,
                  want_mask: bool = True, obs=_OWN_OBS):
        """leaf_logits(feat, weight, bias) + expand_backup(None, values, 2) and, when roots is given,
        the next select(roots, active, cpuct) in one launch (bk_mcts_leaf_step; the same trees
        bitwise). Returns select's (status, obs, mask) or None. want_mask=False: the next leaves'
        bitmasks are not copied out (the engine keeps its own for the next step; self-play's
        captured graph reads only status and obs), and the returned mask is stale. obs: the buffer
        the next leaves' observation planes go to (default: self.obs), or None to write none (a net
        that reads leaf_states_ptr and status needs none); the returned obs is then None."""
        assert feat.dtype == torch.float32 and feat.shape[0] == self.T and feat.stride(1) == 1
        assert weight.is_contiguous() and weight.shape == (self.eng.A, feat.shape[1]) and bias.shape == (self.eng.A,)
        assert values.dtype == torch.float32 and values.shape == (self.T, self.eng.P)
        sel = roots is not None
        if obs is _OWN_OBS:
            obs = self.obs
        if obs is not None:
            assert obs.dtype == torch.float32 and obs.shape == self.obs.shape and obs.device == self.obs.device
        _check(self.lib.bk_mcts_leaf_step(self.h, ctypes.c_void_p(feat.data_ptr()), feat.stride(0), feat.shape[1],
                                          _ptr(weight), _ptr(bias), _ptr(values), int(sel), _ptr(roots),
                                          _ptr(active), float(cpuct), _ptr(self.status) if sel else None,
                                          _ptr(obs) if sel else None,
                                          _ptr(self.leaf_mask) if sel and want_mask else None,
                                          self._s()))
        return (self.status, obs, self.leaf_mask) if sel else None

    def select_range(self, t0: int, n: int, roots: torch.Tensor, active: torch.Tensor | None, cpuct: float = 1.0):
        """select() on the trees [t0, t0 + n) only (bk_mcts_select_range); the buffers are the whole
        batch's and rows outside the range keep their contents."""
        _check(self.lib.bk_mcts_select_range(self.h, int(t0), int(n), _ptr(roots), _ptr(active), float(cpuct),
                                             _ptr(self.status), _ptr(self.obs), _ptr(self.leaf_mask), self._s()))
        return self.status, self.obs, self.leaf_mask

    def leaf_step_range(self, t0: int, n: int, feat: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                        values: torch.Tensor, roots: torch.Tensor | None = None, active: torch.Tensor | None = None,
                        cpuct: float = 1.0):
        """leaf_step() on the trees [t0, t0 + n) only (bk_mcts_leaf_step_range): feat and values are
        the whole batch's [T, ...] buffers, of which the range's rows are read."""
        assert feat.dtype == torch.float32 and feat.shape[0] == self.T and feat.stride(1) == 1
        assert weight.is_contiguous() and weight.shape == (self.eng.A, feat.shape[1]) and bias.shape == (self.eng.A,)
        assert values.dtype == torch.float32 and values.shape == (self.T, self.eng.P)
        sel = roots is not None
        _check(self.lib.bk_mcts_leaf_step_range(self.h, int(t0), int(n), ctypes.c_void_p(feat.data_ptr()),
                                                feat.stride(0), feat.shape[1], _ptr(weight), _ptr(bias), _ptr(values),
                                                int(sel), _ptr(roots), _ptr(active), float(cpuct),
                                                _ptr(self.status) if sel else None, _ptr(self.obs) if sel else None,
                                                _ptr(self.leaf_mask) if sel else None, self._s()))
        return (self.status, self.obs, self.leaf_mask) if sel else None

    def sims_pipelined(self, net_args, n_sims: int, groups: int, weight: torch.Tensor, bias: torch.Tensor,
                       roots: torch.Tensor, active: torch.Tensor | None, cpuct: float = 1.0,
                       obs: torch.Tensor | None = None, ring: int = 1):
        """n_sims simulations of every tree as `groups` staggered chains of select, n_sims x {leaf
        net, leaf step} on contiguous tree ranges (bk_mcts_sims_pipelined): the trees of the same
        launches on the whole batch, bitwise. net_args: nets.leafnet_x3_args (its status must be
        self.status); obs: the planes buffer the search writes, None when the net reads states.
        ring: the scheduling edges between the groups' steps (0 none, 1 every simulation, 2 the first
        only). n_sims = 0 only creates the group streams (call it once before capturing)."""
        assert weight.is_contiguous() and bias.shape == (self.eng.A,)
        assert weight.shape == (self.eng.A, 2 * self.eng.N * self.eng.N)
        _check(self.lib.bk_mcts_sims_pipelined(self.h, ctypes.byref(net_args), int(n_sims), int(groups), int(ring),
                                               _ptr(weight), _ptr(bias), _ptr(roots), _ptr(active), float(cpuct),
                                               _ptr(self.status), _ptr(obs), self._s()))

    # ---- the arena's rows entries: one workgroup per game, tree / net / budget from device tables
    # (engine.arena_rows); roots is [R, 384], indexed by row
    def select_rows(self, rows, roots: torch.Tensor, cpuct: float = 1.0):
        """The descent of simulation 0 for every live row (bk_mcts_select_rows): leaf states and
        status only, no observation planes, no mask copy."""
        assert roots.shape[0] == rows.R
        _check(self.lib.bk_mcts_select_rows(self.h, ctypes.byref(rows), _ptr(roots), float(cpuct), _ptr(self.status),
                                            self._s()))
        return self.status

    def leaf_step_rows(self, rows, sim: int, feat: torch.Tensor, heads, values: torch.Tensor,
                       roots: torch.Tensor | None = None, cpuct: float = 1.0):
        """leaf_step() for every row live at `sim` with the policy head of the row's net
        (engine.arena_heads; net -1: zero logits and values); with roots, also the next descent of
        the rows whose budget is not exhausted (bk_mcts_leaf_step_rows). feat [T, F], values [T, P]."""
        assert feat.dtype == torch.float32 and feat.shape[0] == self.T and feat.stride(1) == 1
        assert values.dtype == torch.float32 and values.shape == (self.T, self.eng.P)
        sel = roots is not None
        _check(self.lib.bk_mcts_leaf_step_rows(self.h, ctypes.byref(rows), int(sim), ctypes.c_void_p(feat.data_ptr()),
                                               feat.stride(0), feat.shape[1], ctypes.byref(heads), _ptr(values),
                                               int(sel), _ptr(roots), float(cpuct),
                                               _ptr(self.status) if sel else None, self._s()))

    def arena_move(self, rows, roots: torch.Tensor, action: torch.Tensor | None = None) -> torch.Tensor:
        """The T = 0 move of every live row straight from its tree (bk_arena_move): the id of the
        first child with maximal N, -1 for a dead row or a root without children."""
        if action is None:
            action = torch.empty(rows.R, dtype=torch.int32, device=self.eng.device)
        assert action.dtype == torch.int32 and action.shape == (rows.R,) and roots.shape[0] == rows.R
        _check(self.lib.bk_arena_move(self.h, ctypes.byref(rows), _ptr(roots), _ptr(action), self._s()))
        return action

    def arena_sims(self, net_table, rows, max_sims: int, heads, pf: torch.Tensor, vout: torch.Tensor,
                   roots: torch.Tensor, cpuct: float = 1.0):
        """A whole ply's search on the current stream, no forked branches (bk_arena_sims): select_rows,
        then max_sims x {leafnet_x3_rows, leaf_step_rows}. net_table: nets.leafnet_x3_table (or None:
        uninformed seats only); pf [T, F] / vout [T, P] are the nets' outputs."""
        n = 0 if net_table is None else len(net_table)
        assert pf.shape == (self.T, 2 * self.eng.N * self.eng.N) and vout.shape == (self.T, self.eng.P)
        _check(self.lib.bk_arena_sims(self.h, net_table, n, ctypes.byref(rows), int(max_sims), ctypes.byref(heads),
                                      _ptr(pf), _ptr(vout), _ptr(roots), float(cpuct), _ptr(self.status), self._s()))

    @property
    def leaf_states_ptr(self) -> int:
        """Device address of the search's own [T, 384] leaf-state buffer (bk_mcts_leaf_states): the
        row of a tree whose status is 1 is its current leaf, other rows are stale. It does not move
        while this object lives, so a captured graph can hold it (nets.leafnet_x3_states takes it)."""
        p = ctypes.c_void_p()
        _check(self.lib.bk_mcts_leaf_states(self.h, ctypes.byref(p)))
        return int(p.value)

    def root_policy(self, roots: torch.Tensor, active: torch.Tensor | None, temperature: float, cap: int = 2048,
                    zero: bool = True):
        """ids/pi rows of every root (k_root); zero=False leaves the entries past each row's count
        unwritten (bk_ply_policy reads only the first counts[t])."""
        alloc = torch.zeros if zero else torch.empty
        ids = alloc((self.T, cap), dtype=torch.int32, device=self.eng.device)
        pi = alloc((self.T, cap), dtype=torch.float64, device=self.eng.device)
        counts = alloc(self.T, dtype=torch.int32, device=self.eng.device)
        _check(self.lib.bk_mcts_root_policy(self.h, _ptr(roots), _ptr(active), float(temperature), _ptr(ids),
                                            _ptr(pi), cap, _ptr(counts), self._s()))
        return ids, pi, counts

    def root_stats(self, roots: torch.Tensor, active: torch.Tensor | None = None, cap: int = 2048):
        dev = self.eng.device
        ids = torch.zeros((self.T, cap), dtype=torch.int32, device=dev)
        n = torch.zeros((self.T, cap), dtype=torch.int32, device=dev)
        q = torch.zeros((self.T, cap), dtype=torch.float64, device=dev)
        p = torch.zeros((self.T, cap), dtype=torch.float32, device=dev)
        counts = torch.zeros(self.T, dtype=torch.int32, device=dev)
        _check(self.lib.bk_mcts_root_stats(self.h, _ptr(roots), _ptr(active), _ptr(ids), _ptr(n), _ptr(q), _ptr(p),
                                           cap, _ptr(counts), self._s()))
        return ids, n, q, p, counts

    def leaf_info(self):
        states = torch.empty((self.T, 384), dtype=torch.uint8, device=self.eng.device)
        depths = torch.empty(self.T, dtype=torch.int32, device=self.eng.device)
        _check(self.lib.bk_mcts_leaf_info(self.h, _ptr(states), _ptr(depths), self._s()))
        return states, depths

    def counters(self) -> dict:
        out = np.zeros(8, dtype=np.int64)
        _check(self.lib.bk_mcts_counters(self.h, out.ctypes.data_as(ctypes.c_void_p), self._s()))
        keys = ["nodes", "children", "levels", "expanded", "terminal", "errors", "scanned", "leaf_children"]
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def check(self):
        c = self.counters()
        if c["errors"]:
            raise EngineError(f"MCTS capacity/consistency error flags {c['errors']:#x} (counters {c})")
        return c


def smoke_search(eng: Engine, oracle) -> None:
    """Tiny search on cuda:0 (used by __graft_entry__.smoke): 4 trees x 8 simulations with a
    uniform prior, checked for tree growth, visit accounting and legal root children."""
    T = 4
    m = BatchedMCTS(eng, T, node_cap=64, child_cap=T * 64 * 700)
    roots = eng.init_states(T)
    logp = torch.zeros((T, eng.A), dtype=torch.float32, device=eng.device)
    vals = torch.zeros((T, eng.P), dtype=torch.float32, device=eng.device)
    for _ in range(8):
        m.select(roots, None, 1.0)
        m.expand_backup(logp, vals)
    c = m.check()
    assert c["expanded"] == T * 8, c
    ids, n, q, p, counts = m.root_stats(roots)
    K = int(counts[0])
    ref_ids = oracle.legal_ids(roots[0].cpu().numpy())
    assert K == len(ref_ids) and (ids[0, :K].cpu().numpy() == ref_ids).all()
    assert int(n[0, :K].sum()) == 7  # first simulation expands the root
    assert abs(float(p[0, :K].sum()) - 1.0) < 1e-5
