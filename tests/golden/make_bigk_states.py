"""Packed states with a prescribed number of legal moves K, far above what random playouts reach.

Run: `python tests/golden/make_bigk_states.py`. Deterministic, uses only oracle/. Output:
tests/golden/bigk_states.npz with, per entry, `preset` (N, P, max piece cells), `K` and the
384-byte `state` (player 0 to move, no flags).

Construction. A sparse lattice of single cells of the mover (rows and columns = a mod step) and
a sparser one of the next player, both hands full: every lattice cell offers four diagonal
anchors to all 21 pieces, so K runs into the thousands (20x20, step 5: 5056). A hill-climb then
walks K down to the target: a step either gives one empty cell to a player who is not the mover
(2 players: the opponent; 4 players: colours 3 and 4, so that the next player's cells stay
scattered) or takes one piece out of the mover's hand, and is kept when target <= K' < K. Small
targets start from a hand of the smallest pieces, where one blocked cell costs few moves. For
targets above 768 the state is kept only if some child position has more than 768 legal moves
too (the next player: scattered cells, full hand), so that a search meets large nodes below the
root. The positions are not reachable by play (single cells of a colour with its whole hand left):
the rules, search and policy kernels read occupancy, hands and the side to move, nothing else.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.oracle import Oracle  # noqa: E402

OUT = os.path.join(HERE, "bigk_states.npz")
BIG = 768  # kSelB * 64: above it select_child takes its two-pass branch
MAX = -1   # target: the lattice itself, whatever K it has

# preset, (mover's lattice step and offset, next player's step and offset), targets
PLAN = [
    ((20, 2, 5), (5, 1, 7, 4), [1, 2, 63, 64, 65, 768, 769, 1023, 1024, 1025, 1087, 1088, 2047, 2048, 2049, MAX]),
    ((20, 4, 5), (5, 1, 7, 4), [769, 1025, 2048]),
    ((14, 2, 5), (5, 0, 7, 3), [769, 1025, 2048, MAX]),
    ((7, 2, 5), (6, 0, 10, 3), [1, 64, 65, MAX]),
]


def piece_cells(o: Oracle) -> np.ndarray:
    """Cells of each piece, from the action table (piece of an action) and its cell list."""
    tab, cells = o.action_table(), o.action_cells()
    n = np.zeros(o.num_pieces, dtype=np.int64)
    for piece in range(o.num_pieces):
        a = int(np.nonzero(tab[:, 0] == piece)[0][0])
        n[piece] = int((cells[a] >= 0).sum())
    return n


def lattice(o: Oracle, step: int, a: int, step2: int, b: int) -> np.ndarray:
    cells = np.zeros((o.N, o.N), dtype=np.int8)
    cells[b::step2, b::step2] = 2
    cells[a::step, a::step] = 1
    return cells


def count(o: Oracle, cells, hands) -> int:
    return o.legal_mask(o.make_state(cells, hands, 0, 0))[1]


def climb(o: Oracle, cells, hands, target: int, rng) -> bool:
    """Walk K down to exactly `target` in place; False when the walk gets stuck above it."""
    blockers = [2] if o.P == 2 else [3, 4]
    K = count(o, cells, hands)
    for _ in range(20000):
        if K == target:
            return True
        if K < target:
            return False
        if rng.integers(8) == 0 and bin(int(hands[0])).count("1") > 1:
            have = [p for p in range(o.num_pieces) if (int(hands[0]) >> p) & 1]
            piece = have[int(rng.integers(len(have)))]
            hands[0] ^= np.uint32(1 << piece)
            K2 = count(o, cells, hands)
            if target <= K2 < K:
                K = K2
            else:
                hands[0] ^= np.uint32(1 << piece)
        else:
            r, c = (int(x) for x in rng.integers(o.N, size=2))
            if cells[r, c]:
                continue
            cells[r, c] = blockers[int(rng.integers(len(blockers)))]
            K2 = count(o, cells, hands)
            if target <= K2 < K:
                K = K2
            else:
                cells[r, c] = 0
    return False


def big_child(o: Oracle, st: np.ndarray) -> bool:
    ids = o.legal_ids(st)
    for a in ids[:: max(1, len(ids) // 16)]:
        nxt, _ = o.next_state(st, int(a))
        if o.game_ended(nxt) is None and o.legal_mask(nxt)[1] > BIG:
            return True
    return False


def make_state(o: Oracle, lat, target: int, ncell: np.ndarray) -> np.ndarray:
    full = np.uint32((1 << o.num_pieces) - 1)
    for seed in range(64):
        rng = np.random.default_rng([o.N, o.P, target & 0xFFFF, seed])
        cells = lattice(o, *lat)
        hands = np.array([full] * o.P + [0] * (4 - o.P), dtype=np.uint32)
        if target != MAX:
            if target < 200:  # the smallest pieces that reach the target: a blocked cell costs few moves
                for size in range(1, 6):
                    hands[0] = np.uint32(sum(1 << p for p in range(o.num_pieces) if ncell[p] <= size))
                    if count(o, cells, hands) >= target:
                        break
            if not climb(o, cells, hands, target, rng):
                continue
        st = o.make_state(cells, hands, 0, 0)
        K = o.legal_mask(st)[1]
        assert o.game_ended(st) is None and (target == MAX or K == target)
        if K > BIG and not big_child(o, st):
            continue
        return st
    raise RuntimeError(f"no state with K = {target} on {(o.N, o.P, o.maxc)}")


def generate():
    presets, Ks, states = [], [], []
    for preset, lat, targets in PLAN:
        o = Oracle(*preset)
        ncell = piece_cells(o)
        for target in targets:
            st = make_state(o, lat, target, ncell)
            presets.append(preset)
            Ks.append(o.legal_mask(st)[1])
            states.append(st)
    return {"preset": np.array(presets, dtype=np.int32), "K": np.array(Ks, dtype=np.int32),
            "state": np.stack(states).astype(np.uint8)}


def npz_bytes(arrays: dict) -> bytes:
    """An .npz np.load reads, with fixed member dates (np.savez stamps the current time)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name, arr in arrays.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(arr), version=(1, 0), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue())
    return buf.getvalue()


def main():
    data = npz_bytes(generate())
    with open(OUT, "wb") as f:
        f.write(data)
    z = np.load(OUT)
    for preset, K in zip(z["preset"], z["K"]):
        print(tuple(int(x) for x in preset), int(K))
    print(f"wrote {OUT} ({len(data)} bytes)")


if __name__ == "__main__":
    main()
