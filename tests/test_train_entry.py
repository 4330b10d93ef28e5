"""train_conv.train_entry, the one eligibility rule of the learner's device convolutions, and the
Learner's head choice on a CPU model (no GPU needed)."""
import types

import pytest
import torch


@pytest.mark.parametrize("supported", [True, False])
def test_train_entry_table(monkeypatch, supported):
    from blokus_rl_amd.alphazero import train_conv as tc

    asked = []

    def np_supported(N):
        asked.append(N)
        return int(supported and N in (7, 14))

    monkeypatch.setattr(tc, "load_library", lambda: types.SimpleNamespace(bk_conv_x3_np_supported=np_supported))
    for mode in ("classic", "all"):
        for N in (7, 14, 20, 10):
            for ch in (64, 32):
                want = None
                if ch == 64 and N == 20:
                    want = "x3"
                elif ch == 64 and N in (7, 14) and mode == "all" and supported:
                    want = "np"
                assert tc.train_entry(N, ch, mode) == want, (N, ch, mode)
    assert set(asked) <= {7, 14}  # the library is asked about the np boards under "all" only


def test_train_entry_bad_mode():
    from blokus_rl_amd.alphazero.train_conv import train_entry

    for mode in ("some", "", None, "ALL"):
        with pytest.raises(ValueError):
            train_entry(20, 64, mode)


def test_prepare_model_keeps_its_mode(monkeypatch):
    from blokus_rl_amd.alphazero.train_conv import TrainResNet, X3Conv2d, prepare_model
    from blokus_rl_amd.nets import ResNet

    monkeypatch.delenv("BK_X3_BOARDS", raising=False)
    model = prepare_model(ResNet(7, 2, 50, 1), x3_boards="all")
    assert isinstance(model, TrainResNet) and model.x3_boards == "all"
    convs = [m for m in model.modules() if isinstance(m, X3Conv2d)]
    assert len(convs) == 2 and all(m.x3_boards == "all" for m in convs)
    prepare_model(model)  # prepared once: the environment's default does not undo it
    assert model.x3_boards == "all" and all(m.x3_boards == "all" for m in convs)
    prepare_model(model, x3_boards="classic")
    assert model.x3_boards == "classic" and all(m.x3_boards == "classic" for m in convs)
    monkeypatch.setenv("BK_X3_BOARDS", "all")
    assert prepare_model(ResNet(7, 2, 50, 1)).x3_boards == "all"
    with pytest.raises(ValueError):
        prepare_model(ResNet(7, 2, 50, 1), x3_boards="some")
    # a CPU forward is PyTorch's own in either mode
    model = prepare_model(ResNet(7, 2, 50, 1), x3_boards="all").train()
    p, v = model(torch.zeros(2, 4, 7, 7))
    assert p.shape == (2, 50) and v.shape == (2, 2)


def test_learner_on_cpu_model():
    from blokus_rl_amd.alphazero.learner import Learner
    from blokus_rl_amd.nets import ResNet

    for kw in ({}, {"x3_boards": "all"}):
        L = Learner(ResNet(7, 2, 50, 1), batch_size=1024, **kw)
        assert L.device_path is False and L.sparse_head is False
