"""pack_x3_stem: the split-f16 stem pack of a net with fewer than 8 observation planes is the
8-channel pack of the same weights with zero input channels appended (bk_leafnet_x3_np's wstem)."""
import pytest
import torch


@pytest.mark.parametrize("cin", [4, 6])
def test_padded_stem_pack_is_the_pack_of_the_padded_weights(cin):
    from blokus_rl_amd.nets import pack_x3, pack_x3_stem

    g = torch.Generator().manual_seed(cin)
    w = torch.randn((64, cin, 3, 3), generator=g) * torch.rand((64, 1, 1, 1), generator=g) * 3
    b = torch.randn(64, generator=g)
    packed, inv, bound = pack_x3_stem(w, b)
    w8 = torch.cat([w, torch.zeros(64, 8 - cin, 3, 3)], dim=1)
    packed8, inv8, bound8 = pack_x3(w8, b)
    assert packed.dtype == torch.uint8 and packed.shape == packed8.shape
    assert torch.equal(packed, packed8)
    assert torch.equal(inv, inv8) and torch.equal(bound, bound8)
    # the scales and the bound are those of the unpadded weights: zeros change no row maximum or L1 norm
    mx = w.double().abs().amax(dim=(1, 2, 3))
    assert torch.equal(inv.double(), torch.pow(2.0, -(15 - torch.frexp(mx)[1]).double()))
    assert float(bound[0]) >= float(w.double().abs().sum(dim=(1, 2, 3)).max())


def test_eight_plane_stem_pack_is_unchanged():
    from blokus_rl_amd.nets import pack_x3, pack_x3_stem

    g = torch.Generator().manual_seed(8)
    w, b = torch.randn((64, 8, 3, 3), generator=g), torch.randn(64, generator=g)
    for x, y in zip(pack_x3_stem(w, b), pack_x3(w, b)):
        assert torch.equal(x, y)
