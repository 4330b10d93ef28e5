"""The arena ply's tail (bk_arena_finish) restated in NumPy (batched_arena.arena_finish_np, the
oracle of tests/test_arena_graph_gpu.py) against the bookkeeping BatchedArena.play does in tensor
code today: the three row tables, over and final, over several plies of random inputs — all games
over, and a game that ends on the first ply checked."""
import numpy as np
import pytest
import torch

from blokus_rl_amd.alphazero.batched_arena import arena_finish_np


def play_bookkeeping(to_move, ended, scores, status, orders, seat_net, seat_sims, over, final):
    """The lines of BatchedArena.play (the eager path) after next_state / game_ended, and the
    tables its next ply derives from the new states, in torch on the CPU."""
    orders, over, final = torch.as_tensor(orders), torch.as_tensor(over).bool(), torch.as_tensor(final)
    ended, scores = torch.as_tensor(ended), torch.as_tensor(scores)
    G, P = orders.shape
    illegal = bool((torch.as_tensor(status) != 0).any())
    newly = ended.bool() & ~over
    final = torch.where(newly.view(-1, 1), scores.to(torch.float64), final)
    over = over | ended.bool()
    pidx = orders.gather(1, torch.as_tensor(to_move).long().view(-1, 1)).view(-1)
    tree = torch.arange(G) * P + pidx
    net_row = torch.as_tensor(seat_net)[pidx]
    sims_row = torch.as_tensor(seat_sims)[pidx]
    return tree, net_row, sims_row, over, final, illegal


def random_inputs(rng, R, P, p_end):
    orders = np.stack([rng.permutation(P) for _ in range(R)]).astype(np.int64)
    to_move = rng.integers(0, P, R)
    ended = (rng.random(R) < p_end).astype(np.int32)
    scores = np.where(ended[:, None] != 0, rng.choice([-1.0, 1.0, 3.0], (R, P)), 0.0)
    return orders, to_move, ended, scores


@pytest.mark.parametrize("R,P", [(1, 2), (37, 4), (300, 3), (24, 4)])
def test_numpy_tail_equals_play_bookkeeping(R, P):
    rng = np.random.default_rng(100 * R + P)
    seat_net = rng.integers(-1, 3, P)
    seat_sims = rng.integers(1, 50, P)
    over = np.zeros(R, dtype=bool)
    final = np.zeros((R, P))
    illegal = 0
    saw_first_ply_end = saw_all_over = latched = False
    for ply, p_end in enumerate([0.3, 0.0, 0.2, 0.5, 1.0, 0.4]):
        orders, to_move, ended, scores = random_inputs(rng, R, P, p_end)
        if ply == 0:
            ended[0], scores[0] = 1, 3.0  # a game that ends on the first ply checked
            saw_first_ply_end = True
        status = np.zeros(R, dtype=np.int32)
        if ply == 2 and (~over).any():
            status[np.nonzero(~over)[0][0]] = 1  # next_state refused a live row's move
        want = play_bookkeeping(to_move, ended, scores, status, orders, seat_net, seat_sims, over, final)
        tree, net, sims, over_n, final_n, illegal, running = arena_finish_np(
            to_move, ended, scores, status, orders, seat_net, seat_sims, over, final, illegal)
        w_tree, w_net, w_sims, w_over, w_final, w_illegal = want
        w_over = w_over.numpy()
        # the eager loop masks an over game out of every launch (act_g, act_t): tree -1 here
        np.testing.assert_array_equal(tree, np.where(w_over, -1, w_tree.numpy()))
        np.testing.assert_array_equal(net, w_net.numpy())
        np.testing.assert_array_equal(sims, w_sims.numpy())
        np.testing.assert_array_equal(over_n.astype(bool), w_over)
        np.testing.assert_array_equal(final_n, w_final.numpy())
        assert running == int((~w_over).sum())
        latched |= w_illegal
        assert illegal == int(latched)
        assert tree.dtype == net.dtype == sims.dtype == np.int32 and over_n.dtype == np.uint8
        over, final = over_n.astype(bool), final_n
        saw_all_over |= bool(over.all())
    assert saw_first_ply_end and saw_all_over and final[0].tolist() == [3.0] * P
    assert illegal == int(R > 1)  # latched at ply 2 and kept (R = 1: its only game was over by then)


def test_status_of_an_over_game_is_not_illegal():
    """An over game's row carries action -1; whatever status it reports is not a live row's."""
    P = 2
    orders = np.array([[0, 1], [1, 0]])
    out = arena_finish_np([0, 1], [0, 0], np.zeros((2, P)), [0, 7], orders, [0, -1], [5, 3],
                          [False, True], np.zeros((2, P)))
    tree, net, sims, over, final, illegal, running = out
    assert tree.tolist() == [0, -1] and net.tolist() == [0, 0] and sims.tolist() == [5, 5]
    assert illegal == 0 and running == 1 and over.tolist() == [0, 1]
    assert arena_finish_np([0, 1], [0, 0], np.zeros((2, P)), [3, 0], orders, [0, -1], [5, 3],
                           [False, True], np.zeros((2, P)))[5] == 1
