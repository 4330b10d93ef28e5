"""Shared helper of the rules tests (no tests here): a NumPy brute force of the placement rules.

A second restatement next to oracle/blokus_oracle.c, for checking the oracle at presets that no
recording of the reference pins. It keeps its own board ([N, N] colours, 0 = empty, q + 1 =
colour q) and its own used-piece sets, and takes from the oracle only the two tables
`action_cells()` and `action_table()[:, 0]` (the piece of every id): never its legality, next
state or game end.

An id is legal for colour q iff its piece is unused by q, all its cells are empty, none of its
cells is edge-adjacent to a cell of q, and it covers q's start corner while q has no cell on the
board, else one of its cells is diagonal to a cell of q. Start corners: (0,0), (N-1,N-1) for two
players; (0,0), (0,N-1), (N-1,0), (N-1,N-1) for four."""
import numpy as np


def start_corners(N: int, P: int):
    if P == 2:
        return [(0, 0), (N - 1, N - 1)]
    return [(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)]


class BruteRules:
    def __init__(self, N: int, P: int, action_cells: np.ndarray, piece_of: np.ndarray):
        self.N, self.P = N, P
        cells = np.asarray(action_cells, dtype=np.int64)
        self.valid = cells >= 0
        r, c = np.where(self.valid, cells // N, 0), np.where(self.valid, cells % N, 0)
        self.S = N + 2  # the board sits inside a one-cell empty border
        self.pidx = (r + 1) * self.S + (c + 1)
        self.cells = cells
        self.piece_of = np.asarray(piece_of, dtype=np.int64)
        self.corner = [(cr + 1) * self.S + (cc + 1) for cr, cc in start_corners(N, P)]
        self.board = np.zeros((N, N), dtype=np.int8)
        self.used = [set() for _ in range(P)]

    def _padded(self, inner: np.ndarray) -> np.ndarray:
        g = np.zeros((self.S, self.S), dtype=bool)
        g[1:-1, 1:-1] = inner
        return g

    def legal_ids(self, q: int, edge_rule: bool = True) -> np.ndarray:
        """edge_rule=False drops the edge-adjacency term (only to show that the tests notice)."""
        own = self._padded(self.board == q + 1)
        occ = self._padded(self.board != 0)
        # the border ring is empty, so a roll never carries a cell across the board
        edge = np.zeros_like(own)
        for d, ax in ((1, 0), (-1, 0), (1, 1), (-1, 1)):
            edge |= np.roll(own, d, axis=ax)
        diag = np.zeros_like(own)
        for dr in (1, -1):
            for dc in (1, -1):
                diag |= np.roll(np.roll(own, dr, axis=0), dc, axis=1)
        v = self.valid
        ok = ~np.isin(self.piece_of, list(self.used[q]))
        ok &= ~(occ.ravel()[self.pidx] & v).any(axis=1)
        if edge_rule:
            ok &= ~(edge.ravel()[self.pidx] & v).any(axis=1)
        if own.any():
            ok &= (diag.ravel()[self.pidx] & v).any(axis=1)
        else:
            ok &= ((self.pidx == self.corner[q]) & v).any(axis=1)
        return np.nonzero(ok)[0]

    def play(self, q: int, a: int):
        cells = self.cells[a][self.valid[a]]
        flat = self.board.reshape(-1)
        assert (flat[cells] == 0).all() and int(self.piece_of[a]) not in self.used[q]
        flat[cells] = q + 1
        self.used[q].add(int(self.piece_of[a]))

    def square_counts(self) -> np.ndarray:
        return np.array([(self.board == q + 1).sum() for q in range(self.P)], dtype=np.int32)

    def scores(self) -> np.ndarray:
        """The wrapper's end-of-game conversion: most squares wins, 3 alone, 1 shared, else -1."""
        sq = self.square_counts()
        win = sq == sq.max()
        return np.where(win, 3.0 if win.sum() == 1 else 1.0, -1.0)
