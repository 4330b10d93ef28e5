"""The big-K fixture (tests/golden/bigk_states.npz, made by tests/golden/make_bigk_states.py): packed
states whose number of legal moves K is prescribed, up to thousands."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bigk_states.npz")


def load():
    """[(preset, K, state[384] uint8)] in file order."""
    z = np.load(PATH)
    return [(tuple(int(x) for x in p), int(k), s.copy()) for p, k, s in zip(z["preset"], z["K"], z["state"])]


def states_of(preset):
    """(K list, states [n, 384]) of one preset, in file order (K ascending)."""
    rows = [(k, s) for p, k, s in load() if p == tuple(preset)]
    return [k for k, _ in rows], np.stack([s for _, s in rows])


def state_named(preset, K):
    Ks, st = states_of(preset)
    return st[Ks.index(K)]
