"""bk_leafnet_x3_run, the one entry behind bk_leafnet_x3, bk_leafnet_x3_states, bk_leafnet_x3_np
and bk_leafnet_x3_np_states: a row range writes its rows only, bitwise the whole batch's rows; the
four positional entries and nets.leafnet_x3 / leafnet_x3_states are that entry; its argument
checks. Shapes: the classic kernel at N = 14, P = 4, B = 5 and the np kernel at N = 7, P = 2,
B = 7 with np = 5 (four boards per workgroup: a range starting at row 1 packs other quads than the
whole batch does) and np = 2 (one board per workgroup). Last, the np kernel with one board per
workgroup against the classic kernel at N = 14 and 20, P = 4, B = 3: bitwise the same outputs."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
CONFIGS = [("classic", 0), ("np", 5), ("np", 2)]  # (kernel family, the struct's np)
FORMS = ["planar", "states"]


@functools.lru_cache(maxsize=None)
def _case(family):
    """(leaf net of one block, states [B, 384], their planes [B, 2P, N, N], status [B] with one
    row that is no leaf) of the family's shape."""
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import LeafResNet, ResNet

    N, P, B = (14, 4, 5) if family == "classic" else (7, 2, 7)
    eng = Engine(N, P, 5)
    torch.manual_seed(10 * N + P)
    net = ResNet(N, P, eng.A, 1).cuda().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.1, 0.1)
    leaf = LeafResNet(net, normalize=False, features=True, x3_boards="all" if family == "np" else "classic").eval()
    assert leaf.x3_entry(N) == family and leaf.takes_states()
    states = random_boards(eng, B, seed0=3, max_plies=3 * P).contiguous()
    status = torch.ones(B, dtype=torch.int32, device="cuda")
    status[2] = 0
    return leaf, states, eng.observe(states).contiguous(), status


def _buffers(leaf, B):
    """Sentinel-filled pf, vout and tower output of B + 2 rows."""
    N, P = leaf.board_size, leaf.f.value_fc2.out_features
    return [torch.full(shape, SENTINEL, device="cuda") for shape in ((B + 2, 2 * N * N), (B + 2, P), (B + 2, N * N, 64))]


def _args(leaf, form, np_, pf, v, monkeypatch, status="case", states=None):
    """The struct of the family's case in `form` writing the first B rows of pf and v."""
    from blokus_rl_amd.nets import leafnet_x3_args

    _, st, obs, stat = _case("np" if np_ else "classic")
    B = st.shape[0]
    monkeypatch.setenv("BK_X3_PACK", str(max(np_ - 1, 0)))
    if form == "planar":
        a = leafnet_x3_args(leaf, pf[:B], v[:B], obs=obs)
    else:
        a = leafnet_x3_args(leaf, pf[:B], v[:B], states=st if states is None else states,
                            status=stat if status == "case" else status, need_status=False)
    assert a.np == np_
    return a


def _run(a, t0, n, out):
    from blokus_rl_amd.engine import load_library

    optr = None if out is None else ctypes.c_void_p(out.data_ptr())
    rc = load_library().bk_leafnet_x3_run(ctypes.byref(a), t0, n, optr, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family,np_", CONFIGS)
def test_a_row_range_writes_its_rows_only_and_bitwise(family, np_, form, monkeypatch):
    leaf, states, _, _ = _case(family)
    B = states.shape[0]
    whole, part = _buffers(leaf, B), _buffers(leaf, B)
    assert _run(_args(leaf, form, np_, whole[0], whole[1], monkeypatch), 0, B, whole[2]) == 0
    assert _run(_args(leaf, form, np_, part[0], part[1], monkeypatch), 1, 3, part[2]) == 0
    for w, p in zip(whole, part):
        assert bool((w[B:] == SENTINEL).all()) and bool((w[:B] != SENTINEL).any(dim=-1).all())
        assert bool((p[0] == SENTINEL).all()) and bool((p[4:] == SENTINEL).all())
        assert torch.equal(p[1:4], w[1:4])


def _positional(leaf, form, np_, obs, states, status, outs):
    """The positional entry of `form` for the struct's np (0: the classic kernel, else the np
    kernel with boards_per_wg = np - 1) on every row of obs / states, writing outs = (pf, v, tower
    output)."""
    from blokus_rl_amd.engine import _ptr, load_library

    N, P = leaf.board_size, leaf.f.value_fc2.out_features
    h = leaf.x3_heads
    net = [_ptr(leaf.x3_wstem), _ptr(leaf.x3_sstem), _ptr(h[0]), 2 * len(leaf.f.blocks), _ptr(leaf.x3_wtower),
           _ptr(leaf.x3_stower), _ptr(leaf.b_tower), _ptr(leaf.x3_bounds)] + [_ptr(t) for t in h[1:]]
    outs = [_ptr(t) for t in outs]
    bpw = [np_ - 1] if np_ else []
    lib = load_library()
    if form == "planar":
        fn = lib.bk_leafnet_x3_np if np_ else lib.bk_leafnet_x3
        rc = fn(_ptr(obs), obs.shape[0], N, 2 * P, *net, P, *outs, *bpw, None)
    else:
        fn = lib.bk_leafnet_x3_np_states if np_ else lib.bk_leafnet_x3_states
        rc = fn(_ptr(states), _ptr(status), states.shape[0], N, P, *net, *outs, *bpw, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family,np_", CONFIGS)
def test_the_positional_entries_and_nets_are_the_entry(family, np_, form, monkeypatch):
    from blokus_rl_amd.nets import leafnet_x3, leafnet_x3_states

    leaf, states, obs, status = _case(family)
    B, N = states.shape[0], leaf.board_size
    ref = _buffers(leaf, B)
    assert _run(_args(leaf, form, np_, ref[0], ref[1], monkeypatch), 0, B, ref[2]) == 0
    ref = [t[:B] for t in ref]
    # the positional entry of the form
    got = _buffers(leaf, B)
    assert _positional(leaf, form, np_, obs, states, status, got) == 0
    for g, r in zip(got, ref):
        assert torch.equal(g[:B], r) and bool((g[B:] == SENTINEL).all())

    # nets.py (BK_X3_PACK as _args left it); the tower output comes back as [B, 64, N, N]
    def same(res):
        pf, v, out = res
        return torch.equal(pf, ref[0]) and torch.equal(v, ref[1]) and torch.equal(
            out.permute(0, 2, 3, 1).reshape(B, N * N, 64), ref[2])

    if form == "planar":
        assert same(leafnet_x3(obs, leaf, want_out=True))
        return
    assert same(leafnet_x3_states(states, status, leaf, want_out=True))
    assert same(leafnet_x3_states(states.data_ptr(), status, leaf, want_out=True))  # a raw address
    # status=None: every row a leaf
    ref = _buffers(leaf, B)
    assert _run(_args(leaf, form, np_, ref[0], ref[1], monkeypatch, status=None), 0, B, ref[2]) == 0
    ref = [t[:B] for t in ref]
    assert same(leafnet_x3_states(states, None, leaf, want_out=True))
    assert not torch.equal(ref[0][2], got[0][2])  # the row whose status was 0 is evaluated now


def test_argument_checks(monkeypatch):
    """Every bad call returns -1 with a message that names the entry, before any launch (the
    outputs keep their sentinel); n = 0 returns 0 without one."""
    from blokus_rl_amd.engine import load_library

    lib = load_library()
    bufs = {}

    def args(family, np_, form, **fields):
        leaf, states, _, _ = _case(family)
        pf, v, _ = bufs.setdefault(family, _buffers(leaf, states.shape[0]))
        a = _args(leaf, form, np_, pf, v, monkeypatch)
        for k, val in fields.items():
            setattr(a, k, val)
        return a

    def refused(a, t0=0, n=1):
        rc = lib.bk_leafnet_x3_run(None if a is None else ctypes.byref(a), t0, n, None, None)
        return rc == -1 and b"bk_leafnet_x3_run" in lib.bk_last_error()

    _, st14, obs14, _ = _case("classic")
    _, st7, _, _ = _case("np")
    assert refused(None)
    assert refused(args("classic", 0, "states"), t0=-1)
    assert refused(args("classic", 0, "states"), n=-1)
    assert refused(args("classic", 0, "states", obs=obs14.data_ptr()))  # both inputs
    assert refused(args("classic", 0, "states", states=None))           # neither
    for np_ in (-1, 3, 4, 6):
        assert refused(args("np", 2, "states", np=np_)), np_
    assert refused(args("classic", 0, "states", np=5)) and b"boards_per_wg" in lib.bk_last_error()  # np = 5, N = 14
    assert refused(args("classic", 0, "states", P=2)) and b"P must be 4" in lib.bk_last_error()
    assert refused(args("np", 2, "states", np=0)) and b"P must be 4" in lib.bk_last_error()
    assert refused(args("np", 2, "planar", np=0)) and b"N must be 14 or 20" in lib.bk_last_error()  # np = 0, N = 7
    assert refused(args("np", 2, "states", N=21)) and b"N must be 7, 14 or 20" in lib.bk_last_error()
    assert refused(args("np", 2, "states", P=5)) and b"P must be" in lib.bk_last_error()
    assert refused(args("classic", 0, "planar", nlayers=0))
    assert refused(args("np", 5, "states", nlayers=0))
    assert refused(args("classic", 0, "states", states=st14.data_ptr() + 2)) and b"4-byte aligned" in lib.bk_last_error()
    assert refused(args("np", 2, "states", states=st7.data_ptr() + 2)) and b"4-byte aligned" in lib.bk_last_error()
    a = args("classic", 0, "planar")
    assert refused(args("classic", 0, "planar", wtower=a.wtower + 8))
    assert refused(args("np", 5, "planar", wp=a.wp + 8))
    # a misaligned tower output
    rc = lib.bk_leafnet_x3_run(ctypes.byref(a), 0, 1, ctypes.c_void_p(bufs["classic"][2].data_ptr() + 8), None)
    assert rc == -1 and b"bk_leafnet_x3_run" in lib.bk_last_error()
    # n = 0: validated, nothing launched
    assert lib.bk_leafnet_x3_run(ctypes.byref(a), 0, 0, None, None) == 0
    assert lib.bk_leafnet_x3_run(ctypes.byref(args("np", 5, "states")), 3, 0, None, None) == 0
    assert refused(args("np", 5, "states", N=14), n=0)  # also with n = 0
    torch.cuda.synchronize()
    for family in bufs:
        assert all(bool((t == SENTINEL).all()) for t in bufs[family])


@functools.lru_cache(maxsize=None)
def _one_board_case(N):
    """(leaf net of one block, planes [3, 8, N, N]: the all-zero observation, a binary board, dense
    floats of magnitudes 1e-3..1e3; the first two as states [2, 384] with status (0, 1): a row
    that is no leaf is the all-zero observation) on the N x N board, P = 4."""
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import LeafResNet, ResNet

    eng = Engine(N, 4, 5)
    torch.manual_seed(100 + N)
    net = ResNet(N, 4, eng.A, 1).cuda().eval()
    leaf = LeafResNet(net, normalize=False, features=True, x3_boards="all").eval()
    states = random_boards(eng, 2, seed0=5, max_plies=12).contiguous()
    status = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    obs = torch.zeros(3, 8, N, N, device="cuda")
    obs[1] = eng.observe(states)[1]
    g = torch.Generator(device="cuda").manual_seed(N)
    sign = torch.randint(0, 2, (8, N, N), device="cuda", generator=g).float() * 2 - 1
    obs[2] = sign * 10.0 ** (torch.rand(8, N, N, device="cuda", generator=g) * 6 - 3)
    return leaf, obs.contiguous(), states, status


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", [14, 20])
def test_np_with_one_board_per_workgroup_is_the_classic_kernel(N, form):
    """bk_leafnet_x3_np with boards_per_wg = 1 and bk_leafnet_x3 (as launched by default) are the
    same function where both apply (8 planes, 14x14 and 20x20): pf, v and the tower output of a
    one-block net (one inner conv epilogue and the last one) agree bitwise."""
    leaf, obs, states, status = _one_board_case(N)
    B = obs.shape[0] if form == "planar" else states.shape[0]
    classic, np1 = _buffers(leaf, B), _buffers(leaf, B)
    assert _positional(leaf, form, 0, obs, states, status, classic) == 0
    assert _positional(leaf, form, 2, obs, states, status, np1) == 0
    assert bool((obs[1] != 0).any()) and bool((classic[0][:B] != SENTINEL).all())
    for c, p in zip(classic, np1):
        assert torch.equal(p, c)
