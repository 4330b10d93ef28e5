"""nets.dcnn_leaf_mode: the DCNNet leaf knob's values (no device)."""
import pytest


def test_dcnn_leaf_mode_accepts_fused(monkeypatch):
    from blokus_rl_amd.nets import dcnn_leaf_mode

    monkeypatch.delenv("BK_DCNN_LEAF", raising=False)
    assert dcnn_leaf_mode() == "torch"
    for m in ("torch", "x3", "fused"):
        assert dcnn_leaf_mode(m) == m
        monkeypatch.setenv("BK_DCNN_LEAF", m)
        assert dcnn_leaf_mode() == m
    # the argument wins over the environment
    assert dcnn_leaf_mode("x3") == "x3"
    for bad in ("mfma", "Fused", ""):
        with pytest.raises(ValueError):
            dcnn_leaf_mode(bad)
        monkeypatch.setenv("BK_DCNN_LEAF", bad)
        with pytest.raises(ValueError):
            dcnn_leaf_mode()
