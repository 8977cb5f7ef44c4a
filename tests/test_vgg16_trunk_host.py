"""The VGG16 trunk that the VGG loss and LPIPS share (`vfi_amd/vgg16.py`), without a GPU: the layout of its two slices, the
state-dict keys of the two owners, the loader's refusals as each owner words them, and the key of the pack cache."""
import re

import pytest
import torch
import torch.nn as nn

from vfi_amd import vgg16
from vfi_amd.adacof.losses import vgg
from vfi_amd.evaluation import lpips

CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)            # torchvision's vgg16.features, written out
WIDTHS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
# the texts of vgg.py and lpips.py before the trunk was shared
FORMAT = {10: "a torchvision vgg16 state dict (the file vgg16-397923af.pth of torchvision.models.vgg16, or any dict / "
              "torch.save file with the keys features.{0,2,5,7,10,12,14,17,19,21}.{weight,bias})",
          13: "a torchvision vgg16 state dict (the file vgg16-397923af.pth of torchvision.models.vgg16, or any dict / "
              "torch.save file with the keys features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias})"}
OWNERS = [(vgg.load_vgg16_features, 10, "the VGG loss", "the VGG loss needs weights"),
          (lpips.load_vgg16_features, 13, "LPIPS", "LPIPS needs the VGG16 weights")]


def _state(n_convs, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, idx in enumerate(CONVS[:n_convs]):
        sd[f"features.{idx}.weight"] = torch.randn((WIDTHS[i + 1], WIDTHS[i], 3, 3), generator=g) * (2.0 / (9 * WIDTHS[i])) ** 0.5
        sd[f"features.{idx}.bias"] = torch.randn((WIDTHS[i + 1],), generator=g) * 0.05
    return sd


def _heads():
    return [torch.rand(c) for c in (64, 128, 256, 512, 512)]


@pytest.mark.parametrize("n_convs,relu_last,layers,pools", [(10, False, 22, (1, 3, 6)), (13, True, 30, (1, 3, 6, 9))])
def test_trunk_layout(n_convs, relu_last, layers, pools):
    seq = vgg16.sequential(n_convs, relu_last)
    assert len(seq) == layers
    assert tuple(k for k, m in enumerate(seq) if isinstance(m, nn.Conv2d)) == CONVS[:n_convs]
    assert vgg16.pool_after(n_convs) == pools
    assert tuple(k - 2 for k, m in enumerate(seq) if isinstance(m, nn.MaxPool2d)) == tuple(CONVS[i] for i in pools)
    assert isinstance(seq[-1], nn.ReLU if relu_last else nn.Conv2d)
    assert [(m.in_channels, m.out_channels) for m in seq if isinstance(m, nn.Conv2d)] == list(zip(WIDTHS, WIDTHS[1:n_convs + 1]))
    # one table: the ten-convolution names are a prefix of the thirteen
    assert vgg16.CONV_INDICES == CONVS and vgg16.CHANNELS == WIDTHS
    assert vgg.CONV_INDICES == CONVS[:10] and vgg.CHANNELS == WIDTHS[:11]
    assert lpips.CONV_INDICES is vgg16.CONV_INDICES and lpips.CHANNELS is vgg16.CHANNELS
    assert lpips.TAP_CHANNELS == (64, 128, 256, 512, 512)
    assert len(vgg._sequential()) == 22


def test_state_dict_keys_stay_the_references():
    a = vgg.VGG(_state(10))
    assert sorted(a.state_dict()) == sorted(f"vgg16_conv_4_3.{i}.{k}" for i in CONVS[:10] for k in ("weight", "bias"))
    b = lpips.LPIPS(_state(13), _heads())
    assert sorted(b.state_dict()) == sorted([f"features.{i}.{k}" for i in CONVS for k in ("weight", "bias")]
                                            + [f"weights.{l}" for l in range(5)])
    assert isinstance(b.weights, nn.ParameterList)
    assert [n for n, _ in a.named_children()] == ["vgg16_conv_4_3"] and [n for n, _ in b.named_children()] == ["features", "weights"]
    assert not any(p.requires_grad for m in (a, b) for p in m.parameters())
    # a VGG and an LPIPS term share nothing
    assert a.vgg16_conv_4_3[0].weight is not b.features[0].weight


@pytest.mark.parametrize("load,n_convs,who,missing", OWNERS)
def test_loader_refusals(load, n_convs, who, missing, tmp_path):
    fmt = re.escape(FORMAT[n_convs])
    with pytest.raises(ValueError, match=re.escape(missing + ": pass --vgg_weights (or set VFI_VGG16_WEIGHTS) to ") + fmt):
        load(None)
    with pytest.raises(FileNotFoundError, match=re.escape(f"missing.pth: not found; {who} needs ") + fmt):
        load(str(tmp_path / "missing.pth"))
    last = CONVS[n_convs - 1]
    short = _state(n_convs)
    del short[f"features.{last}.bias"]
    with pytest.raises(KeyError, match=re.escape(f"features.{last}.bias is missing: {who} needs ") + fmt):
        load(short)
    wrong = _state(n_convs)
    wrong["features.5.weight"] = torch.zeros(128, 32, 3, 3)
    with pytest.raises(ValueError, match=re.escape(f"features.5.weight has shape (128, 32, 3, 3), not (128, 64, 3, 3): {who} needs ")
                       + fmt):
        load(wrong)
    # no dict and no path: a TypeError that names the type (the VGG loss used to pass on os.fspath's)
    with pytest.raises(TypeError, match="list"):
        load([1, 2])
    if who == "LPIPS":
        with pytest.raises(TypeError, match="list: LPIPS needs " + fmt):
            load([1, 2])
    # what it accepts: the dict, or its file, with keys beyond its own ignored
    full = _state(13)
    torch.save(full, tmp_path / "vgg16.pth")
    for given in (full, str(tmp_path / "vgg16.pth")):
        got = load(given)
        assert list(got) == [f"{i}.{k}" for i in CONVS[:n_convs] for k in ("weight", "bias")]
        assert all(torch.equal(v, full["features." + k]) for k, v in got.items())


def test_pack_cache_key():
    trunk = vgg16.Trunk(10, False, vgg.load_vgg16_features(_state(10)))
    key = trunk.pack_key()
    assert key[0] == torch.device("cpu") and len(key) == 1 + 20
    float(trunk.seq[21].weight.sum())                     # reading changes nothing
    trunk.seq.state_dict()
    assert trunk.pack_key() == key
    with torch.no_grad():
        trunk.seq[21].bias.mul_(1.0)                      # a write in place, even of the same values
    assert trunk.pack_key() != key and trunk.pack_key()[:-1] == key[:-1]
    key = trunk.pack_key()
    trunk.seq.load_state_dict(trunk.seq.state_dict())
    assert all(a > b for a, b in zip(trunk.pack_key()[1:], key[1:]))
    # the owners' caches are their trunks'
    node = vgg.VGG(_state(10))
    assert node._trunk.seq is node.vgg16_conv_4_3 and node._trunk.pack_key()[0] == torch.device("cpu")
