"""The training loops: vfi_amd/train/trainer.py, vfi_amd/fusion_net/trainer.py, their command lines,
fed by TripletLoader from tiny seeded Vimeo-shaped datasets (train_batch_ref.write_triplets).

A Trainer's epoch is compared bit for bit with the loop written out in the test over the same loader and seed: every
training path is order-fixed and both run the same calls, so the loss history and every parameter
agree exactly or something differs in what was called."""
import math
import os
import random
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import phasenet_fusion_ref as FR
import train_batch_ref as TR
from conftest import PKG_DIR
from oracle import pipeline_cpu
from vfi_amd.adacof.models import Model
from vfi_amd.fusion_net.fusion_net import FusionNet
from vfi_amd.fusion_net.train_batch import fusion_net_inputs
from vfi_amd.fusion_net.trainer import Trainer as FusionNetTrainer
from vfi_amd.phase_net.architecture import PhaseNet as ArchPhaseNet
from vfi_amd.phase_net.phase_net import PhaseNet
from vfi_amd.train.datareader import DBreader_Vimeo90k, TripletLoader
from vfi_amd.train.loss import get_loss
from vfi_amd.train.pyramid import Pyramid
from vfi_amd.train.trainer import Trainer
from vfi_amd.train.utils import calc_pyr_height

pytestmark = pytest.mark.gpu


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _height(h, w):
    return calc_pyr_height(torch.empty(3, h, w, device="meta"))


def _args(**kw):
    base = dict(mode="phase", model=0, high_level=False, epochs=1, gpu_id=0, fixed_stats=False, test_paths=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _pyr(height, device):
    return Pyramid(height=height, nbands=4, scale_factor=np.sqrt(2), device=device)


def _arch(height, device, num_img=2):
    net = ArchPhaseNet(height, device, num_img=num_img)
    net.core.load_state_dict(FR.net_state(41, num_img))
    return net


def _adacof():
    adacof = Model(types.SimpleNamespace(model="vfi_amd.fusion_net.fusion_adacofnet", kernel_size=5, dilation=1, gpu_id=0))
    adacof.load(pipeline_cpu.seeded_weights(0)["adacof"])
    adacof.eval()
    return adacof


@pytest.fixture(scope="module")
def small_set(tmp_path_factory):
    """6 triplets of 40x56"""
    return TR.write_triplets(str(tmp_path_factory.mktemp("vimeo_small")), 6, 40, 56, seed=1, smooth=True)


@pytest.fixture(scope="module")
def wide_set(tmp_path_factory):
    """4 triplets of 72x104"""
    return TR.write_triplets(str(tmp_path_factory.mktemp("vimeo_wide")), 4, 72, 104, seed=2, smooth=True)


def _phase_loader(root, device):
    return TripletLoader(DBreader_Vimeo90k(root, random_crop=(32, 48)), 2, shuffle=True, workers=2, device=device, rgb=False)


def test_phase_epoch_is_the_manual_loop_bit_for_bit_and_its_checkpoint_loads(small_set, tmp_path, device):
    height, m, lr = _height(32, 48), 3, 1e-3
    out = str(tmp_path / "out")
    net = _arch(height, device)
    _seed(7)
    trainer = Trainer(_args(), _phase_loader(small_set, device), net, _pyr(height, device), lr=lr, out_dir=out, m=m, m_update=500)
    assert net.core.fine_tuning and net.core.batch_stats and not net.training        # the reference trains in train() mode
    assert trainer.max_step == 3 and not trainer.terminate()
    trainer.train()
    assert trainer.current_epoch == 1 and trainer.terminate() and trainer.m == m
    history = list(trainer.loss_history)
    assert len(history) == 3 and all(isinstance(v, float) and math.isfinite(v) for v in history)
    for f in ("checkpoint/model_0_0.pt", "log_train.txt", "log.txt"):
        assert os.path.exists(os.path.join(out, f)), f
    assert np.loadtxt(os.path.join(out, "log_train.txt")).reshape(-1).tolist() == history[:1]     # written at batch 0

    # the same epoch by hand
    ref = _arch(height, device)
    pyr = _pyr(height, device)
    _seed(7)
    loader = _phase_loader(small_set, device)
    ref.fine_tune(True, batch_stats=True)
    opt = torch.optim.Adam(ref.parameters(), lr=lr, weight_decay=0.0)
    manual = []
    for batch in loader:
        assert batch.rgb is None and batch.lab.shape == (3, 6, 32, 48)
        prediction, vals_pred, vals_target = ref(batch.img_batch_phase, m=m)
        loss = get_loss(vals_pred, vals_target, prediction, batch.lab_target, pyr)[0]
        opt.zero_grad()
        loss.backward()
        opt.step()
        manual.append(float(loss))
    print("loss history:", history, "by hand:", manual)
    assert history == manual
    moved = 0
    for (k, p), (k2, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert k == k2 and torch.equal(p, q), k
    for k, v in FR.net_state(41, 2).items():
        moved += int(not torch.equal(dict(net.core.state_dict())[k].cpu(), v))
    assert moved > 0
    for (k, p), (k2, q) in zip(net.named_buffers(), ref.named_buffers()):
        assert k == k2 and torch.equal(p, q), k

    # the end-of-epoch checkpoint of the command line loads into a new model, which computes the same bits.  The call is the
    # training call's shape, 18 images: a pyramid plan batches its small levels by its capacity, so
    # bits are compared between plans of one capacity, here 16 on both sides
    path = os.path.join(out, f"checkpoint/model_{trainer.current_epoch}.pt")
    torch.save(net.state_dict(), path)
    again = ArchPhaseNet(height, device)
    again.load_state_dict(torch.load(path, map_location="cpu"))
    for (k, v), (k2, v2) in zip(net.state_dict().items(), again.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k
    img_batch = next(iter(_phase_loader(small_set, device))).img_batch_phase
    net.fine_tune(False)
    a, b = net(img_batch, m=m)[0], again(img_batch, m=m)[0]
    assert a.grad_fn is None and a.shape == (6, 32, 48) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    trainer.close()


def test_m_schedule(small_set, tmp_path, device):
    height = _height(32, 48)
    net = _arch(height, device)
    _seed(3)
    trainer = Trainer(_args(fixed_stats=True), _phase_loader(small_set, device), net, _pyr(height, device), lr=1e-4,
                      out_dir=str(tmp_path / "out"), m=3, m_update=1)
    assert net.core.fine_tuning and not net.core.batch_stats                          # --fixed_stats
    used = []
    predict = trainer.predict

    def recording(*a, **kw):
        used.append(trainer.m)
        return predict(*a, **kw)
    trainer.predict = recording
    trainer.train()
    # batch_idx % m_update == 0 and batch_idx > 0: m steps after batches 1 and 2
    assert used == [3, 3, 4] and trainer.m == 5
    assert all(math.isfinite(v) for v in trainer.loss_history) and len(trainer.loss_history) == 3
    trainer.close()


@pytest.mark.parametrize("model,num_img", [(0, 4), (1, 3)])
def test_fusion_mode_step(model, num_img, wide_set, tmp_path, device):
    h, w = 64, 96
    height = _height(h, w)
    m = height - 2
    net = _arch(height, device, num_img=num_img)
    adacof = _adacof()
    _seed(5)
    ds = DBreader_Vimeo90k(wide_set, random_crop=(h, w))
    ds.triplet_list = ds.triplet_list[:2]
    ds.file_len = 2
    loader = TripletLoader(ds, 2, shuffle=True, workers=2, device=device)
    trainer = Trainer(_args(mode="fusion", model=model), loader, net, _pyr(height, device), lr=1e-4, out_dir=str(tmp_path / "out"),
                      m=m, m_update=500, adacof_model=adacof)
    assert trainer.max_step == 1
    trainer.train()
    loss = trainer.loss_history
    assert len(loss) == 1 and math.isfinite(loss[0]) and loss[0] > 0
    with_grad = 0
    for k, p in net.core.named_parameters():
        if p.grad is not None:
            with_grad += 1
            assert bool(torch.isfinite(p.grad).all()), k
    # the loss sees blocks 0 .. m - 2, eight tensors each (tests/test_phasenet_batch_train_gpu.py)
    print(f"fusion mode, {num_img} images: loss {loss[0]:.6f}, {with_grad} tensors with a gradient")
    assert with_grad == 8 * (m - 1)
    assert all(p.grad is None for p in adacof.parameters())
    trainer.close()


def test_test_writes_a_picture_and_leaves_the_model_as_it_found_it(tmp_path, device):
    from PIL import Image
    height = _height(32, 48)
    d = DBreader_Vimeo90k(TR.write_triplets(str(tmp_path / "pictures"), 1, 32, 48, seed=8, smooth=True)).triplet_list[0]
    paths = [f"{d}/im1.png", f"{d}/im2.png", f"{d}/im3.png"]
    for stats in (True, False):
        net = _arch(height, device)
        out = str(tmp_path / f"out{int(stats)}")
        trainer = Trainer(_args(fixed_stats=not stats), [], net, _pyr(height, device), out_dir=out, m=3)
        before = {k: v.clone() for k, v in net.core.named_buffers()}
        assert (net.core.fine_tuning, net.core.batch_stats) == (True, stats)
        trainer.test(idx=4, paths=paths, name="basketball")
        assert (net.core.fine_tuning, net.core.batch_stats) == (True, stats)
        assert all(blk.batch_stats == stats for blk in net.core.layers)
        for k, v in net.core.named_buffers():
            assert torch.equal(v, before[k]), k                                      # no running statistic moved
        img = Image.open(os.path.join(out, "result/basketball_0_4.png"))
        assert img.size == (48, 32) and img.mode == "RGB"
        trainer.test(paths=paths, name="x")
        assert os.path.exists(os.path.join(out, "result/x_0.png"))
        # no paths, or a missing file: silently nothing
        trainer.test(idx=0, paths=None, name="none")
        trainer.test(idx=0, paths=paths[:2] + [str(tmp_path / "missing.png")], name="none")
        assert sorted(os.listdir(os.path.join(out, "result"))) == ["basketball_0_4.png", "x_0.png"]
        trainer.close()


def _fusion_models(device, h, w):
    weights = pipeline_cpu.seeded_weights(0)
    fusion = FusionNet().to(device)
    fusion.load_state_dict(weights["fusionnet"])
    pyr = _pyr(_height(h, w), device)
    phase_net = PhaseNet(pyr, device, num_img=2)
    phase_net.load_state_dict(weights["phasenet"])
    return _adacof(), fusion, pyr, phase_net


def test_fusion_net_epoch_is_the_manual_loop_bit_for_bit(wide_set, tmp_path, device):
    h, w, lr = 64, 96, 1e-4
    loader = lambda: TripletLoader(DBreader_Vimeo90k(wide_set, random_crop=(h, w)), 2, shuffle=True, workers=2, device=device)
    adacof, fusion, pyr, phase_net = _fusion_models(device, h, w)
    out = str(tmp_path / "out")
    _seed(9)
    trainer = FusionNetTrainer(_args(save=False), loader(), fusion, phase_net, adacof, my_pyr=pyr, lr=lr, out_dir=out)
    assert fusion.training and trainer.max_step == 2
    trainer.train()
    history = list(trainer.loss_history)
    assert len(history) == 2 and all(math.isfinite(v) for v in history) and trainer.terminate()
    assert os.path.exists(os.path.join(out, "checkpoint/model_0_0.pt")) and os.path.exists(os.path.join(out, "log_train.txt"))
    assert all(p.grad is None for p in adacof.parameters()) and all(p.grad is None for p in phase_net.parameters())

    adacof2, ref, pyr2, phase_net2 = _fusion_models(device, h, w)
    ref.train()
    _seed(9)
    opt = torch.optim.Adam(ref.parameters(), lr=lr, weight_decay=0.0)
    manual = []
    for batch in loader():
        inputs = fusion_net_inputs(adacof2, phase_net2, pyr2, batch.lab_frame1, batch.lab_frame2, batch.rgb_frame1, batch.rgb_frame2)
        final = ref(*inputs, variant=0)
        loss = torch.nn.L1Loss()(batch.rgb_target, torch.clip(final, 0, 1))
        opt.zero_grad()
        loss.backward()
        opt.step()
        manual.append(float(loss))
    print("loss history:", history, "by hand:", manual)
    assert history == manual
    changed = 0
    start = pipeline_cpu.seeded_weights(0)["fusionnet"]
    for (k, p), (k2, q) in zip(fusion.named_parameters(), ref.named_parameters()):
        assert k == k2 and torch.equal(p, q), k
        changed += int(not torch.equal(p.detach().cpu(), start[k]))
    assert changed > 0
    with pytest.raises(NotImplementedError):
        FusionNetTrainer(_args(save=True), [], fusion, phase_net, adacof, my_pyr=pyr, out_dir=out)
    trainer.close()


def _run_cli(module, argv, out):
    env = dict(os.environ)
    env["PYTHONPATH"] = PKG_DIR + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", module] + argv + ["--out_dir", out, "--epochs", "1", "--batch_size", "2",
                                                                "--gpu_id", "0", "--workers", "2"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for f in ("checkpoint/model_1.pt", "log.txt", "config.txt"):
        assert os.path.exists(os.path.join(out, f)), f
    assert not os.path.exists(os.path.join(out, "log_train.txt"))
    log = np.loadtxt(os.path.join(out, "log.txt")).reshape(-1)
    assert log.shape == (2,) and bool(np.isfinite(log).all()), log
    assert "batch_size: 2" in open(os.path.join(out, "config.txt")).read()
    return r


def test_phase_command_line(tmp_path, device):
    four = TR.write_triplets(str(tmp_path / "vimeo4"), 4, 40, 56, seed=4, smooth=True)
    out = str(tmp_path / "out")
    r = _run_cli("vfi_amd.train.train", ["--train", four, "--crop", "32", "48", "--height", str(_height(32, 48)), "--m", "3",
                                         "--m_update", "1"], out)
    assert "Train Epoch:" in r.stdout
    again = ArchPhaseNet(_height(32, 48), device)
    again.load_state_dict(torch.load(os.path.join(out, "checkpoint/model_1.pt"), map_location="cpu"))


def test_fusion_net_command_line(wide_set, tmp_path, device):
    weights = pipeline_cpu.seeded_weights(0)
    ck_phase, ck_adacof = str(tmp_path / "phase_net.pt"), str(tmp_path / "ckpt.pth")
    torch.save(weights["phasenet"], ck_phase)
    torch.save({"state_dict": weights["adacof"]}, ck_adacof)
    out = str(tmp_path / "out")
    r = _run_cli("vfi_amd.fusion_net.train", ["--train", wide_set, "--crop", "64", "96", "--height", str(_height(64, 96)),
                                              "--phasenet_checkpoint", ck_phase, "--adacof_checkpoint", ck_adacof], out)
    assert "Train Epoch:" in r.stdout
    again = FusionNet()
    again.load_state_dict(torch.load(os.path.join(out, "checkpoint/model_1.pt"), map_location="cpu"))
