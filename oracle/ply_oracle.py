"""TEST INFRASTRUCTURE ONLY — NumPy restatement of the self-play ply tail
(blokus_rl_amd/csrc/ply.hip: k_ply_policy, k_ply_finish; contract in include/blokus_engine.h).

The tail's random numbers are counter-based (splitmix64 of seed, ply, game and draw index), so
every draw is predicted here instead of being tested statistically:

* `ply_rng` / `u01`: the draw of (seed, ply, game, draw index) and its map to (0, 1];
* `gamma_draw`: Gamma(alpha, 1) with the kernel's draw slots (entry idx owns slots idx * 128 ...:
  the alpha < 1 boost first, then per Marsaglia-Tsang round two slots for the normal and, when
  the candidate is positive, one for the acceptance test; 32 rounds);
* `ply_policy`: the first-ply Dirichlet mix in float64, the float32 pi, the record fields and the
  sampled action;
* `draw_index`: the action's law in its plainest form — a sequential float64 cumulative sum of
  the float32 probabilities, the first positive entry whose running sum exceeds (1 - u) * total —
  with the draw's margin (distance of the target to the nearest CDF boundary over the total).
  The kernel sums in another association (256 chunks, a scan, a walk), restated independently in
  `draw_index_chunked`; the two agree whenever the margin is far above float64 rounding, which
  tests/test_ply_oracle.py pins on the corpus the GPU test uses;
* `ply_finish`: a plain loop over the slots.
"""
from __future__ import annotations

import numpy as np

from .vecenv_oracle import mix64 as mix64_int

U64 = np.uint64
GOLDEN = U64(0x9E3779B97F4A7C15)
DRAW_ACTION = 0x7FFFFFFF  # the draw slot of the action's uniform
GAMMA_SLOTS = 128  # draw slots per noise entry
GAMMA_ROUNDS = 32
PLY_THREADS = 256  # chunks of the kernel's inverse CDF
MARGIN_MIN = 2.0 ** -40  # draws nearer than this to a CDF boundary may depend on the association


def mix64(x):
    """splitmix64 finalizer of x + golden (common.h mix64) on uint64 arrays (wrapping)."""
    with np.errstate(over="ignore"):
        z = np.asarray(x, dtype=U64) + GOLDEN
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def ply_rng(seed: int, ply: int, game, draw):
    """mix64(mix64(seed ^ mix64(ply)) + (uint32(game) << 24) + uint32(draw)); game and draw
    broadcast (int arrays or scalars, taken modulo 2^32 like the kernel's casts)."""
    base = mix64_int((int(seed) ^ mix64_int(int(ply))) & 0xFFFFFFFFFFFFFFFF)
    g = (np.asarray(game, dtype=np.int64) & 0xFFFFFFFF).astype(U64)
    d = (np.asarray(draw, dtype=np.int64) & 0xFFFFFFFF).astype(U64)
    with np.errstate(over="ignore"):
        return mix64(U64(base) + (g << U64(24)) + d)


def unmix64(z: int) -> int:
    """The inverse of mix64 (a bijection of 64-bit words), on Python ints."""
    m = (1 << 64) - 1
    z ^= (z >> 31) ^ (z >> 62)
    z = (z * pow(0x94D049BB133111EB, -1, 1 << 64)) & m
    z ^= (z >> 27) ^ (z >> 54)
    z = (z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & m
    z ^= (z >> 30) ^ (z >> 60)
    return (z - int(GOLDEN)) & m


def seed_for_draw(x: int, ply: int, game: int, draw: int) -> int:
    """The seed under which ply_rng(seed, ply, game, draw) == x: puts one chosen draw at a value
    no seed search would reach (u01's ends)."""
    m = (1 << 64) - 1
    inner = (unmix64(x) - ((game & 0xFFFFFFFF) << 24) - (draw & 0xFFFFFFFF)) & m
    return unmix64(inner) ^ mix64_int(int(ply))


def u01(x):
    """Uniform in (0, 1] from the top 53 bits."""
    return ((np.asarray(x, dtype=U64) >> U64(11)).astype(np.float64) + 1.0) * 2.0 ** -53


def gamma_draw(alpha: float, seed: int, ply: int, game, idx):
    """Gamma(alpha, 1) of noise entry idx of a game (arrays broadcast). alpha = 1: -log(u) of
    slot idx * 128. Otherwise Marsaglia-Tsang with d = a - 1/3, c = 1 / sqrt(9 d), a = alpha (+ 1
    and a u^(1/alpha) boost when alpha < 1), normals by Box-Muller, at most 32 rounds."""
    game, idx = np.broadcast_arrays(np.asarray(game, dtype=np.int64), np.asarray(idx, dtype=np.int64))
    shape = idx.shape
    game, idx = game.ravel(), idx.ravel()
    k = idx * GAMMA_SLOTS
    alpha = float(alpha)
    if alpha == 1.0:
        return (-np.log(u01(ply_rng(seed, ply, game, k)))).reshape(shape)
    boost = np.ones(idx.shape, dtype=np.float64)
    a = alpha
    if a < 1.0:
        boost = np.power(u01(ply_rng(seed, ply, game, k)), 1.0 / a)
        k = k + 1
        a += 1.0
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out = d * boost  # 32 rejections in a row
    todo = np.ones(idx.shape, dtype=bool)
    for _ in range(GAMMA_ROUNDS):
        if not todo.any():
            break
        u1 = u01(ply_rng(seed, ply, game, k))
        u2 = u01(ply_rng(seed, ply, game, k + 1))
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
        v = 1.0 + c * x
        pos = v > 0.0
        u = u01(ply_rng(seed, ply, game, k + 2))  # drawn only where the candidate is positive
        k = k + np.where(todo, np.where(pos, 3, 2), 0)
        v = v * v * v
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = (u < 1.0 - 0.0331 * x * x * x * x) | (np.log(u) < 0.5 * x * x + d * (1.0 - v + np.log(v)))
        acc = todo & pos & ok
        out = np.where(acc, d * v * boost, out)
        todo &= ~acc
    return out.reshape(shape)


def dirichlet_noise(alpha: float, seed: int, ply: int, game: int, K: int):
    """The kernel's Dir(alpha) over K legal ids: Gamma draws over their sum (floored at 1e-300)."""
    x = gamma_draw(alpha, seed, ply, game, np.arange(K))
    gs = float(np.sum(x))
    return x / (gs if gs > 1e-300 else 1e-300)


def draw_target(total, seed: int, ply: int, game):
    """(1 - u) * total in [0, total) with u from the action's draw slot."""
    return (1.0 - u01(ply_rng(seed, ply, game, DRAW_ACTION))) * total


def draw_index(p32_row, K: int, seed: int, ply: int, game: int):
    """-> (index, margin). Sequential float64 running sum of the row's first K float32
    probabilities; the first positive entry whose running sum exceeds the target, else (the
    target within rounding of the total) the last positive entry; -1 for a row without one.
    margin: min |target - boundary| / total over the boundaries 0 and every running sum."""
    p = np.asarray(p32_row[:K], dtype=np.float32)
    cs = np.cumsum(p.astype(np.float64))  # np.add.accumulate: strictly left to right
    total = float(cs[-1])
    target = float(draw_target(total, seed, ply, game))
    pos = p > 0
    if not pos.any():
        return -1, 0.0
    hit = np.nonzero(pos & (cs > target))[0]
    index = int(hit[0]) if len(hit) else int(np.nonzero(pos)[0][-1])
    margin = min(float(np.abs(cs - target).min()), target) / total
    return index, margin


def draw_index_chunked(p32_row, K: int, seed: int, ply: int, game: int):
    """The same draw in the kernel's association, restated on its own: 256 contiguous chunks of
    ceil(K / 256) entries, an exclusive scan of the chunk sums, and a walk from the scanned offset
    inside the chunk whose interval [offset, offset + sum) holds the target; the chunk's last
    positive entry when the walk's own rounding stays at or below the target; the row's last
    positive entry when no chunk claims the target. -> index."""
    p = np.asarray(p32_row[:K], dtype=np.float32).astype(np.float64)
    C = -(-K // PLY_THREADS)
    padded = np.zeros(PLY_THREADS * C)
    padded[:K] = p
    sums = np.cumsum(padded.reshape(PLY_THREADS, C), axis=1)[:, -1]  # each chunk left to right
    offs = np.concatenate([[0.0], np.cumsum(sums)])
    total = float(offs[-1])
    target = float(draw_target(total, seed, ply, game))
    best = -1
    for t in range(PLY_THREADS):
        lo, hi = t * C, min(t * C + C, K)
        if hi <= lo or not (offs[t] <= target < offs[t] + sums[t]):
            continue
        acc, last, at = float(offs[t]), -1, -1
        for i in range(lo, hi):
            acc += p[i]
            if p[i] > 0:
                last = i
                if acc > target:
                    at = i
                    break
        best = max(best, at if at >= 0 else last)
    if best < 0:
        nz = np.nonzero(p > 0)[0]
        best = int(nz[-1]) if len(nz) else 0
    return best


def ply_policy(ids, pi, counts, active, first_ply, cap: int, weight: float, alpha: float, seed: int, ply: int,
               to_move):
    """bk_ply_policy on the host. ids [G, cap] int32, pi [G, cap] float64 (entries at and beyond a
    row's count are never read), counts / active [G], first_ply [G], to_move [G].
    -> dict(ids16, pi32, act_mask, player, action, index, margin); index / margin: the drawn
    position in the row (-1 for games that take no action) and its margin."""
    ids = np.asarray(ids)
    pi = np.asarray(pi, dtype=np.float64)
    G = len(counts)
    ids16 = np.zeros((G, cap), dtype=np.int16)
    pi32 = np.zeros((G, cap), dtype=np.float32)
    act_mask = np.zeros(G, dtype=np.uint8)
    action = np.full(G, -1, dtype=np.int32)
    index = np.full(G, -1, dtype=np.int64)
    margin = np.full(G, np.inf)
    for g in range(G):
        K = max(int(counts[g]), 0)  # counts < 0: the root had more than cap children
        act = bool(active[g]) and K > 0
        act_mask[g] = act
        if K == 0:
            continue
        v = pi[g, :K].copy()
        if act and first_ply[g]:
            v = v * (1.0 - weight) + dirichlet_noise(alpha, seed, ply, g, K) * weight
        pi32[g, :K] = v.astype(np.float32)
        ids16[g, :K] = ids[g, :K].astype(np.int16)
        if act:
            index[g], margin[g] = draw_index(pi32[g], K, seed, ply, g)
            action[g] = ids[g, index[g]]
    return dict(ids16=ids16, pi32=pi32, act_mask=act_mask, player=np.asarray(to_move, dtype=np.int32).copy(),
                action=action, index=index, margin=margin)


def ply_finish(G: int, P: int, ended, scores, counts, act_mask, game_id, roots, init_state, continuous: bool,
               num_sims: int, active, first_ply, z_table, z_known, zcap: int, next_gid: int, fin_count: int,
               sims_count: int, cap_overflow: int):
    """bk_ply_finish on the host: a loop over the slots in order. The in/out arrays (active,
    first_ply, z_table, z_known) are copied, not written. -> dict of every output array and the
    four scalars."""
    active = np.array(active, dtype=np.int32)
    first_ply = np.array(first_ply, dtype=np.uint8)
    z_table = np.array(z_table, dtype=np.float32)
    z_known = np.array(z_known, dtype=np.uint8)
    roots = np.asarray(roots)
    reset_flags = np.zeros(G, dtype=np.int32)
    game_id_out = np.zeros(G, dtype=np.int64)
    roots_out = roots.copy()
    gid0, finished, moved, over = int(next_gid), 0, 0, False
    for g in range(G):
        act = active[g] != 0
        done = bool(act and ended[g] != 0)
        over |= bool(act and counts[g] < 0)
        moved += 1 if act_mask[g] else 0
        gid = int(game_id[g])
        if done and 0 <= gid < zcap:
            z_table[gid] = np.asarray(scores[g], dtype=np.float64).astype(np.float32)
            z_known[gid] = 1
        reset_flags[g] = 1 if done else 0
        first_ply[g] = 1 if ((first_ply[g] and not act_mask[g]) or (continuous and done)) else 0
        if continuous and done:
            roots_out[g] = np.asarray(init_state).reshape(-1)
            game_id_out[g] = gid0 + finished
        else:
            game_id_out[g] = gid
            if done:
                active[g] = 0
        finished += 1 if done else 0
    return dict(active=active, first_ply=first_ply, reset_flags=reset_flags, game_id_out=game_id_out,
                roots_out=roots_out, z_table=z_table, z_known=z_known,
                next_gid=gid0 + finished if continuous else gid0, fin_count=int(fin_count) + finished,
                sims_count=int(sims_count) + int(num_sims) * moved, cap_overflow=1 if over else int(cap_overflow))


# ---- the rows the draw tests use (tests/test_ply_oracle.py pins their margins on the host,
# tests/test_ply_gpu.py runs them through bk_ply_policy); one batch, so a row's game index — part
# of its draw's counter — is the same in both
CORPUS_K = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 2049, 4095, 4096)
CORPUS_CAP = 4096
CORPUS_SEED = 5
CORPUS_PLIES = (0, 7)


def corpus_rows(K: int, rng, per_kind: int = 16):
    """Rows of K probabilities (float64, each with a positive entry): per_kind each of Dirichlet
    rows, rows with 70% exact zeros, rows whose first half is zero and unnormalised rows (total
    ~1.5 K); then the structural rows: one-hot at 0, K - 1, C - 1 and C for the chunk size
    C = ceil(K / 256), one positive entry in the middle with zeros to the end, and a positive
    first half followed by zeros to the end."""
    rows = []
    for _ in range(per_kind):
        rows.append(rng.dirichlet(np.full(K, 0.3)))
    for _ in range(per_kind):
        r = rng.dirichlet(np.ones(K))
        r[rng.random(K) < 0.7] = 0.0
        if not r.any():
            r[rng.integers(K)] = 1.0
        rows.append(r / r.sum())
    for _ in range(per_kind):
        r = rng.dirichlet(np.ones(K))
        r[:K // 2] = 0.0
        rows.append(r / r.sum())
    for _ in range(per_kind):
        rows.append(rng.random(K) * 3.0 + 1e-3)
    C = -(-K // PLY_THREADS)
    for at in (0, K - 1, min(C - 1, K - 1), min(C, K - 1), K // 2):
        r = np.zeros(K)
        r[at] = 1.0
        rows.append(r)
    r = rng.random(K) + 1e-3
    r[K // 2 + 1:] = 0.0
    rows.append(r / r.sum())
    return rows


def draw_corpus(row_seed: int = 1234, cap: int = CORPUS_CAP):
    """-> (pi [G, cap] float64, NaN at and beyond each row's count; counts [G] int32)."""
    rng = np.random.default_rng(row_seed)
    rows = [r for K in CORPUS_K for r in corpus_rows(K, rng)]
    pi = np.full((len(rows), cap), np.nan)
    for g, r in enumerate(rows):
        pi[g, :len(r)] = r
    return pi, np.array([len(r) for r in rows], dtype=np.int32)
