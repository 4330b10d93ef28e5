"""bk_leafnet_x3_np / bk_leafnet_x3_np_states (leafnet_np.hip): the one-launch split-f16 leaf net
for 2-player stems and 7x7 boards, one board (Q = 1) or four 7x7 boards (Q = 4) per workgroup.

Accuracy: the bar of tests/test_leafnet_gpu.py ("fp32-class": within 4x the f32 kernels' error
against an fp64 forward, or 2e-6 of the output scale; the tower output within 2e-6). The f32 path
is the same LeafResNet with the knob off. Invariance: a board's outputs are a function of that
board alone, bitwise, across Q, batch size, position and neighbours."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _net(N, P, nblocks, seed, A=60):
    from blokus_rl_amd.nets import ResNet

    torch.manual_seed(seed)
    net = ResNet(N, P, A, nblocks).cuda().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.1, 0.1)
    return net


def _leaf(net, knob="all"):
    from blokus_rl_amd.nets import LeafResNet

    return LeafResNet(net, normalize=False, features=True, x3_boards=knob).eval()


def _ref64(net, obs):
    """fp64 forward of the BN-folded net: (policy features, values, tower output)."""
    from blokus_rl_amd.nets import FusedResNet

    with torch.no_grad():
        fd = FusedResNet(net).double().eval()
        x = torch.relu(fd.stem(obs.double()))
        h = x
        for c1, c2 in fd.blocks:
            h = c2(torch.relu(c1(h)))
        xt = torch.relu(x + h)
        pf = torch.relu(fd.policy_conv(xt)).flatten(1)
        v = torch.tanh(fd.value_fc2(torch.relu(fd.value_fc1(torch.relu(fd.value_conv(xt)).flatten(1)))))
    return pf, v, xt


def _rel(a, ref):
    return float((a.double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


def _obs(B, P, N, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "binary":
        return (torch.rand((B, 2 * P, N, N), device="cuda", generator=g) < 0.3).float()
    scale = {"dense": 1.0, "tiny": 1e-3, "huge": 1e3}[kind]
    return torch.randn((B, 2 * P, N, N), device="cuda", generator=g) * scale


def _run(leaf, obs, q, monkeypatch, want_out=False):
    from blokus_rl_amd.nets import leafnet_x3

    monkeypatch.setenv("BK_X3_PACK", str(q))
    return leafnet_x3(obs.contiguous(), leaf, want_out=want_out)


@pytest.mark.parametrize("N,P,B,nblocks,kind,Q", [
    (7, 2, 37, 2, "binary", 1), (7, 2, 37, 2, "binary", 4), (7, 2, 5, 1, "dense", 4), (7, 2, 3, 1, "tiny", 1),
    (7, 2, 6, 2, "huge", 4), (7, 4, 9, 1, "binary", 4), (14, 2, 5, 2, "binary", 0), (20, 2, 3, 1, "dense", 0)])
def test_leafnet_np_is_fp32_class(N, P, B, nblocks, kind, Q, monkeypatch):
    net = _net(N, P, nblocks, seed=B + N + nblocks + P)
    obs = _obs(B, P, N, kind, seed=B * 3 + N)
    leaf, leaf32 = _leaf(net), _leaf(net, "classic")
    assert leaf.x3 and leaf.x3_entry(N) == "np" and leaf32.x3_entry(N) is None
    pf, v, out = _run(leaf, obs, Q, monkeypatch, want_out=True)
    pf32, v32 = leaf32(obs)  # the knob-off path: the f32 MFMA kernels
    torch.cuda.synchronize()
    pf_ref, v_ref, xt_ref = _ref64(net, obs)
    assert torch.isfinite(pf).all() and torch.isfinite(v).all()
    e_x3, e_32 = _rel(pf, pf_ref), _rel(pf32, pf_ref)
    ev_x3, ev_32 = float((v.double() - v_ref).abs().max()), float((v32.double() - v_ref).abs().max())
    e_out = _rel(out, xt_ref)
    print(f"pf {e_x3:.3g} (f32 {e_32:.3g})  v {ev_x3:.3g} (f32 {ev_32:.3g})  tower {e_out:.3g}")
    assert e_x3 <= max(4 * e_32, 2e-6), (e_x3, e_32)
    assert ev_x3 <= max(4 * ev_32, 2e-6), (ev_x3, ev_32)
    assert e_out <= 2e-6
    # LeafResNet.forward takes the same route
    pff, vf = leaf(obs)
    assert torch.equal(pff, pf) and torch.equal(vf, v)


@pytest.fixture(scope="module")
def mixed():
    """37 boards of a 7x7 2-player net: dense boards whose scales cycle through 1e-3, 1, 1e3 (every
    quad of a Q = 4 workgroup mixes them), every fifth board binary; and its Q = 1 outputs."""
    from blokus_rl_amd.nets import leafnet_x3

    net = _net(7, 2, 2, seed=41)
    leaf = _leaf(net)
    g = torch.Generator(device="cuda").manual_seed(7)
    obs = torch.randn((37, 4, 7, 7), device="cuda", generator=g)
    obs *= torch.tensor([1e-3, 1.0, 1e3], device="cuda")[torch.arange(37, device="cuda") % 3].view(-1, 1, 1, 1)
    binary = (torch.rand((37, 4, 7, 7), device="cuda", generator=g) < 0.3).float()
    obs[4::5] = binary[4::5]
    old = os.environ.get("BK_X3_PACK")
    os.environ["BK_X3_PACK"] = "1"
    try:
        ref = leafnet_x3(obs, leaf, want_out=True)
    finally:
        if old is None:
            del os.environ["BK_X3_PACK"]
        else:
            os.environ["BK_X3_PACK"] = old
    torch.cuda.synchronize()
    return leaf, obs, ref


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_one_and_four_boards_per_workgroup_are_bitwise_equal(mixed, monkeypatch):
    leaf, obs, ref = mixed
    assert _same(_run(leaf, obs, 4, monkeypatch, want_out=True), ref)
    assert _same(_run(leaf, obs, 0, monkeypatch, want_out=True), ref)


@pytest.mark.parametrize("Q", [1, 4])
def test_a_board_alone_equals_its_batch_row(mixed, Q, monkeypatch):
    leaf, obs, ref = mixed
    for b in (0, 17, 36):
        one = _run(leaf, obs[b:b + 1], Q, monkeypatch, want_out=True)
        assert _same(one, [t[b:b + 1] for t in ref]), b


@pytest.mark.parametrize("Q", [1, 4])
def test_a_permuted_batch_permutes_the_outputs(mixed, Q, monkeypatch):
    leaf, obs, ref = mixed
    perm = torch.randperm(37, generator=torch.Generator().manual_seed(3)).cuda()
    got = _run(leaf, obs[perm], Q, monkeypatch, want_out=True)
    assert _same(got, [t[perm] for t in ref])


def _np_call(leaf, obs, pf, v, out, q):
    """bk_leafnet_x3_np on the caller's output buffers (B = obs.shape[0])."""
    from blokus_rl_amd.engine import _ptr, _stream, load_library

    B, cin, N, _ = obs.shape
    h = leaf.x3_heads
    return load_library().bk_leafnet_x3_np(
        ctypes.c_void_p(obs.data_ptr()), B, N, cin, _ptr(leaf.x3_wstem), _ptr(leaf.x3_sstem), _ptr(h[0]),
        2 * len(leaf.f.blocks), _ptr(leaf.x3_wtower), _ptr(leaf.x3_stower), _ptr(leaf.b_tower), _ptr(leaf.x3_bounds),
        *[_ptr(t) for t in h[1:]], cin // 2, _ptr(pf), _ptr(v), ctypes.c_void_p(out.data_ptr()), q,
        _stream(obs.device))


@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_tail_workgroups_write_only_their_boards(mixed, B):
    """Q = 4 with B mod 4 != 0: two guard rows of a sentinel after pf, v and out stay untouched,
    and the B rows are the Q = 1 rows."""
    leaf, obs, ref = mixed
    sent = -12345.0
    pf = torch.full((B + 2, 2 * 49), sent, device="cuda")
    v = torch.full((B + 2, 2), sent, device="cuda")
    out = torch.full((B + 2, 49, 64), sent, device="cuda")
    assert _np_call(leaf, obs[:B].contiguous(), pf, v, out, 4) == 0
    torch.cuda.synchronize()
    for t in (pf, v, out):
        assert bool((t[B:] == sent).all())
    assert torch.equal(pf[:B], ref[0][:B]) and torch.equal(v[:B], ref[1][:B])
    assert torch.equal(out[:B].view(B, 7, 7, 64).permute(0, 3, 1, 2), ref[2][:B])


@pytest.mark.parametrize("N,B,Q", [(7, 37, 1), (7, 37, 4), (14, 5, 0), (20, 5, 0)])
def test_states_form_equals_planar_form(N, B, Q, monkeypatch):
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import leafnet_x3_states

    eng = Engine(N, 2, 5)
    leaf = _leaf(_net(N, 2, 1, seed=N, A=eng.A))
    states = random_boards(eng, B, seed0=9, max_plies=12)
    obs = eng.observe(states)
    assert obs.shape == (B, 4, N, N)
    monkeypatch.setenv("BK_X3_PACK", str(Q))
    assert leaf.takes_states()
    got = leafnet_x3_states(states, None, leaf, want_out=True)
    assert _same(got, _run(leaf, obs, Q, monkeypatch, want_out=True))
    pfs, vs = leaf.forward_states(states)
    assert torch.equal(pfs, got[0]) and torch.equal(vs, got[1])


@pytest.mark.parametrize("Q", [1, 4])
def test_states_form_skips_boards_that_are_no_leaves(Q, monkeypatch):
    """Boards whose status is not 1 are the all-zero observation and their state bytes are not
    read (here 0xFF): one quad with a single dead board, one whole quad dead, one quad with a
    single live board, and a tail."""
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import leafnet_x3_states

    B = 14
    eng = Engine(7, 2, 5)
    leaf = _leaf(_net(7, 2, 1, seed=23, A=eng.A))
    states = random_boards(eng, B, seed0=4, max_plies=12)
    status = torch.ones(B, dtype=torch.int32, device="cuda")
    status[1] = 0
    status[4:8] = torch.tensor([0, 2, 0, 3], dtype=torch.int32)
    status[8:12] = torch.tensor([0, 0, 1, 2], dtype=torch.int32)
    status[13] = 0
    obs = eng.observe(states) * (status == 1).view(-1, 1, 1, 1).float()
    dirty = states.clone()
    dirty[status != 1] = 0xFF
    monkeypatch.setenv("BK_X3_PACK", str(Q))
    got = leafnet_x3_states(dirty, status, leaf, want_out=True)
    assert _same(got, _run(leaf, obs, Q, monkeypatch, want_out=True))


def test_np_argument_checks():
    """Every out-of-range call is refused on the host, with a message, before any launch."""
    from blokus_rl_amd import engine

    lib = engine.load_library()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    ops = [p] * 3 + [2] + [p] * 4 + [p] * 8  # wstem sstem bstem nlayers wtower stower btower bounds, heads

    def planar(N, P, q):
        return lib.bk_leafnet_x3_np(p, 1, N, 2 * P, *ops, P, p, p, None, q, None)

    def states(N, P, q, ptr=p):
        return lib.bk_leafnet_x3_np_states(ptr, None, 1, N, P, *ops, p, p, None, q, None)

    assert lib.bk_leafnet_x3_np_supported(7, 2) and lib.bk_leafnet_x3_np_supported(20, 4)
    assert not lib.bk_leafnet_x3_np_supported(21, 2) and not lib.bk_leafnet_x3_np_supported(7, 5)
    for fn in (planar, states):
        assert fn(21, 2, 0) == -1 and b"N must be 7, 14 or 20" in lib.bk_last_error(), lib.bk_last_error()
        assert fn(7, 5, 0) == -1 and b"P must be" in lib.bk_last_error(), lib.bk_last_error()
        assert fn(7, 1, 0) == -1 and b"P must be" in lib.bk_last_error(), lib.bk_last_error()
        assert fn(20, 2, 4) == -1 and b"boards_per_wg" in lib.bk_last_error(), lib.bk_last_error()
        assert fn(7, 2, 2) == -1 and b"boards_per_wg" in lib.bk_last_error(), lib.bk_last_error()
    assert states(7, 2, 0, ctypes.c_void_p(buf.data_ptr() + 2)) == -1 and b"4-byte aligned" in lib.bk_last_error()
    # the classic entries still refuse the new shapes
    rc = lib.bk_leafnet_x3_states(p, None, 1, 7, 2, *ops, p, p, None, None)
    assert rc == -1 and b"P must be 4" in lib.bk_last_error()
    rc = lib.bk_leafnet_x3(p, 1, 7, 4, *ops, 2, p, p, None, None)
    assert rc == -1 and lib.bk_last_error()
