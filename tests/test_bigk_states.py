"""The big-K fixture against the CPU oracle: every stored state has exactly its recorded number of
legal moves and is not over, the K every GPU test relies on are present, the roots above 768 have a
child above 768, and the generator reproduces the committed file byte for byte."""
import importlib.util
import os

import numpy as np

import bigk_util
from oracle.oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))


def test_states_have_their_recorded_k():
    rows = bigk_util.load()
    assert len(rows) == 27
    oracles = {}
    for preset, K, st in rows:
        o = oracles.setdefault(preset, Oracle(*preset))
        assert st.dtype == np.uint8 and st.shape == (384,)
        assert len(o.legal_ids(st)) == K == o.legal_mask(st)[1], (preset, K)
        assert o.game_ended(st) is None
        if K > 768:
            ids = o.legal_ids(st)
            assert max(o.legal_mask(o.next_state(st, int(a))[0])[1] for a in ids[:: len(ids) // 16]) > 768


def test_every_threshold_is_straddled():
    assert bigk_util.states_of((20, 2, 5))[0] == [1, 2, 63, 64, 65, 768, 769, 1023, 1024, 1025, 1087, 1088, 2047,
                                                 2048, 2049, 5056]
    assert bigk_util.states_of((20, 4, 5))[0] == [769, 1025, 2048]
    assert bigk_util.states_of((14, 2, 5))[0] == [769, 1025, 2048, 2374]
    assert bigk_util.states_of((7, 2, 5))[0] == [1, 64, 65, 400]


def test_generator_reproduces_the_file():
    spec = importlib.util.spec_from_file_location("make_bigk_states", os.path.join(HERE, "golden", "make_bigk_states.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(bigk_util.PATH, "rb") as f:
        assert gen.npz_bytes(gen.generate()) == f.read()
