"""LPIPS without a GPU: the weight loaders and their refusals, the plain-torch face against the
thirteen layers written out (tests/lpips_ref.py), the `Loss` grammar, and the new command-line flags."""
import importlib
import types

import pytest
import torch

import lpips_ref as LR
from vfi_amd.evaluation import lpips


@pytest.fixture(scope="module")
def vgg_state():
    return LR.vgg16_state(11)


@pytest.fixture(scope="module")
def heads():
    return LR.head_weights(11)


def test_head_weight_formats(vgg_state, heads, tmp_path):
    flat = [w.reshape(-1) for w in heads]
    for given in (heads, tuple(heads), flat, LR.head_weights_dict(11)):
        got = lpips.load_head_weights(given)
        assert [tuple(t.shape) for t in got] == [(64,), (128,), (256,), (512,), (512,)]
        assert all(torch.equal(a, b) for a, b in zip(got, flat))
    # files of either format, and of the vgg16 state dict
    torch.save(heads, tmp_path / "piq.pt")
    torch.save(LR.head_weights_dict(11), tmp_path / "lpips.pth")
    torch.save({k: v.clone() for k, v in vgg_state.items() if k.startswith("features.")}, tmp_path / "vgg16.pth")
    for name in ("piq.pt", "lpips.pth"):
        net = lpips.LPIPS(str(tmp_path / "vgg16.pth"), tmp_path / name)
        assert all(torch.equal(p, w) for p, w in zip(net.weights, flat))
        assert all(not p.requires_grad for p in net.parameters()) and len(list(net.parameters())) == 26 + 5
        assert list(net.features.state_dict()) == [f"{i}.{k}" for i in LR.CONVS for k in ("weight", "bias")]
        assert torch.equal(net.features[28].weight, vgg_state["features.28.weight"])
    assert some_zero(flat)


def some_zero(flat):
    return all(bool((w == 0).any()) and bool((w > 0).any()) for w in flat)


def test_refusals(vgg_state, heads, tmp_path):
    with pytest.raises(ValueError, match="--vgg_weights.*VFI_VGG16_WEIGHTS.*torchvision vgg16 state dict"):
        lpips.LPIPS(None, heads)
    with pytest.raises(ValueError, match="--lpips_weights.*VFI_LPIPS_WEIGHTS.*five tensors"):
        lpips.LPIPS(vgg_state, None)
    with pytest.raises(FileNotFoundError, match="missing.pth.*torchvision vgg16 state dict"):
        lpips.LPIPS(str(tmp_path / "missing.pth"), heads)
    with pytest.raises(FileNotFoundError, match="missing.pt.*lin.0..4..model.1.weight"):
        lpips.LPIPS(vgg_state, str(tmp_path / "missing.pt"))
    # the ten-convolution dict of the VGG loss is not enough
    short = {k: v for k, v in vgg_state.items() if not k.startswith("features.28")}
    with pytest.raises(KeyError, match="features.28.weight is missing"):
        lpips.LPIPS(short, heads)
    wrong = dict(vgg_state)
    wrong["features.24.weight"] = torch.zeros(512, 256, 3, 3)
    with pytest.raises(ValueError, match=r"features.24.weight has shape \(512, 256, 3, 3\)"):
        lpips.LPIPS(wrong, heads)
    with pytest.raises(TypeError, match="vgg16 state dict"):
        lpips.load_vgg16_features([1, 2])
    with pytest.raises(ValueError, match="4 tensors, not 5"):
        lpips.load_head_weights(heads[:4])
    with pytest.raises(ValueError, match=r"head weight 2 is \(1, 128, 1, 1\), not 256 elements"):
        lpips.load_head_weights([heads[0], heads[1], heads[1], heads[3], heads[4]])
    with pytest.raises(ValueError, match="head weight 0 is float"):
        lpips.load_head_weights([1.0] + heads[1:])
    d = LR.head_weights_dict(11)
    del d["lin3.model.1.weight"]
    with pytest.raises(KeyError, match="lin3.model.1.weight is missing"):
        lpips.load_head_weights(d)
    with pytest.raises(TypeError, match="five tensors"):
        lpips.load_head_weights(torch.zeros(5))
    with pytest.raises(ValueError, match="reduction"):
        lpips.LPIPS(vgg_state, heads, reduction="median")


@pytest.mark.parametrize("h,w", [(16, 16), (17, 23), (32, 16)])
def test_plain_torch_face_is_the_thirteen_layers_written_out(h, w, vgg_state, heads):
    g = torch.Generator().manual_seed(h + w)
    x = torch.rand((2, 3, h, w), generator=g, dtype=torch.float64)
    y = (x + 0.1 * torch.randn((2, 3, h, w), generator=g, dtype=torch.float64)).clamp(0, 1)
    net = lpips.LPIPS(vgg_state, heads)
    xg = x.clone().requires_grad_(True)
    got = net(xg, y)
    want = LR.lpips_plain(vgg_state, heads, x, y)
    assert got.shape == (2,) and got.dtype == torch.float64 and float(want.min()) > 0
    assert float(((got.detach() - want).abs() / want).max()) <= 1e-12
    got.sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    assert torch.equal(net(x, x), torch.zeros(2, dtype=torch.float64))
    assert lpips.LPIPS(vgg_state, heads, reduction="sum")(x, y).dim() == 0
    with pytest.raises(ValueError, match="at least 16"):
        net(x[:, :, :8], y[:, :, :8])
    with pytest.raises(ValueError, match="must be equal"):
        net(x, y[:1])


def test_head_restatement_at_zero_pixels():
    """value and gradient of the plain-torch head are finite at pixels that are zero in x, in y or in both"""
    x, y, w = LR.head_inputs(2, 6, 5)
    xg = x.double().requires_grad_(True)
    v = lpips.head_torch(xg, y.double(), w)
    v.sum().backward()
    assert torch.allclose(v, LR.head(x.double(), y.double(), w), rtol=1e-14, atol=0)
    assert bool(torch.isfinite(xg.grad).all()) and bool((xg.grad[:, :, 0] == 0).all()) and bool((xg.grad[:, :, 2] == 0).all())
    assert float(xg.grad[:, :, 1].abs().max()) > 0


def test_loss_grammar(vgg_state, heads, capsys):
    from vfi_amd.adacof import losses
    from vfi_amd.adacof.losses.vgg import VGG
    crit = losses.Loss(types.SimpleNamespace(loss='1*Charb+0.1*LPIPS+0.2*VGG+0.01*g_Spatial', vgg_weights=vgg_state,
                                             lpips_weights=heads))
    assert [(l['type'], l['weight']) for l in crit.loss] == [('Charb', 1.0), ('LPIPS', 0.1), ('VGG', 0.2)]
    assert isinstance(crit.loss_module[1], lpips.LPIPS) and crit.loss_module[1].reduction == 'mean'
    assert isinstance(crit.loss_module[2], VGG) and [r['type'] for r in crit.regularize] == ['g_Spatial']
    assert "0.100 * LPIPS" in capsys.readouterr().out
    with pytest.raises(ValueError, match="--lpips_weights"):
        losses.Loss(types.SimpleNamespace(loss='1*LPIPS', vgg_weights=vgg_state, lpips_weights=None))
    # on the host the term is the plain-torch face
    g = torch.Generator().manual_seed(1)
    frame, gt = torch.rand((1, 3, 16, 16), generator=g), torch.rand((1, 3, 16, 16), generator=g)
    only = losses.Loss(types.SimpleNamespace(loss='0.5*LPIPS', vgg_weights=vgg_state, lpips_weights=heads))
    got = only({'frame1': frame}, gt, None)
    assert torch.equal(got, 0.5 * lpips.LPIPS(vgg_state, heads)(frame, gt).mean())


def test_command_line_flags(monkeypatch):
    from vfi_amd.adacof import train as adacof_train
    from vfi_amd.evaluation import evaluate
    from vfi_amd.fusion_net import train as fusion_train
    mods = (evaluate, adacof_train, fusion_train)
    try:
        monkeypatch.setenv("VFI_VGG16_WEIGHTS", "/w/vgg16.pth")
        monkeypatch.setenv("VFI_LPIPS_WEIGHTS", "/w/heads.pt")
        for m in mods:
            a = importlib.reload(m).parser.parse_args([])
            assert (a.vgg_weights, a.lpips_weights) == ("/w/vgg16.pth", "/w/heads.pt"), m.__name__
            a = m.parser.parse_args(["--vgg_weights", "a.pth", "--lpips_weights", "b.pt"])
            assert (a.vgg_weights, a.lpips_weights) == ("a.pth", "b.pt")
        assert fusion_train.parser.parse_args([]).lpips_weight == 0.0
        assert fusion_train.parser.parse_args(["--lpips_weight", "0.25"]).lpips_weight == 0.25
        monkeypatch.delenv("VFI_VGG16_WEIGHTS")
        monkeypatch.delenv("VFI_LPIPS_WEIGHTS")
        for m in mods:
            a = importlib.reload(m).parser.parse_args([])
            assert a.vgg_weights is None and a.lpips_weights is None
    finally:
        monkeypatch.undo()
        for m in mods:
            importlib.reload(m)


def test_evaluate_builds_no_module_without_both_files(capsys):
    from vfi_amd.evaluation import evaluate
    assert evaluate.build_lpips(types.SimpleNamespace(vgg_weights="x.pth", lpips_weights=None, gpu_id=0)) is None
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "--lpips_weights" in out and "NaN" in out
