"""The AdaCoF training loop: vfi_amd/adacof/trainer.py, TestModule.py and the command line, fed
from a tiny seeded Vimeo-shaped dataset (train_batch_ref.write_triplets) and a Middlebury-shaped tree the test writes
(adacof_loss_ref.write_middlebury).

An epoch of the Trainer is compared bit for bit with the loop written out here over the same loader and seed: every training
path is order-fixed (section 12.1) and both run the same calls, so the loss history and every parameter agree exactly or
something differs in what was called."""
import math
import os
import random
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image
from torch.utils.data import DataLoader

import adacof_loss_ref as LR
import train_batch_ref as TR
from conftest import PKG_DIR
from oracle import nets_cpu
from vfi_amd.adacof import losses, train, utility
from vfi_amd.adacof.datareader import DBreader_Vimeo90k, TripletLoader
from vfi_amd.adacof.models import Model
from vfi_amd.adacof.TestModule import Middlebury_other
from vfi_amd.adacof.trainer import Trainer

pytestmark = pytest.mark.gpu

DEFAULT = '1*Charb+0.01*g_Spatial+0.005*g_Occlusion'


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _args(out_dir, loss=DEFAULT, **kw):
    base = dict(model="vfi_amd.adacof.models.adacofnet", kernel_size=5, dilation=1, gpu_id=0, out_dir=out_dir, epochs=1,
                loss=loss, optimizer='ADAMax', lr=1e-3, weight_decay=0, decay_type='step', lr_decay=20, gamma=0.5)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _model(args, sd):
    model = Model(args)
    model.load(sd)
    return model


@pytest.fixture(scope="module")
def small_set(tmp_path_factory):
    """6 triplets of 40x56"""
    return TR.write_triplets(str(tmp_path_factory.mktemp("vimeo_small")), 6, 40, 56, seed=1, smooth=True)


@pytest.fixture(scope="module")
def middlebury(tmp_path_factory):
    """the 12 names, 40x56 -> (input_dir, gt_dir)"""
    return LR.write_middlebury(str(tmp_path_factory.mktemp("middlebury")), 40, 56, seed=3)


@pytest.fixture(scope="module")
def state():
    return nets_cpu.adacofnet_random_state_dict(12, kernel_size=5)


def _loader(root, device):
    return TripletLoader(DBreader_Vimeo90k(root, random_crop=(32, 48)), 2, shuffle=True, workers=2, device=device, rgb=True, lab=False)


def _check_log_and_pictures(out, epoch_lines, model, db, name):
    """log.txt against float64 on the model's prediction, the PNGs against the quantisation rule"""
    lines = open(os.path.join(out, "log.txt")).read().split("\n")
    blocks = [i for i, l in enumerate(lines) if l.startswith("Epoch: ")]
    assert [lines[i] for i in blocks] == epoch_lines
    at = blocks[-1]
    model.eval()
    total = 0.0
    for idx, item in enumerate(LR.MIDDLEBURY):
        with torch.no_grad():
            pred = model(db.input0_list[idx], db.input1_list[idx])
        assert pred.grad_fn is None and pred.shape == (1, 3, 40, 56)
        want = -10 * math.log10(float(((db.gt_list[idx].double() - pred.double()) ** 2).mean()))
        total += want
        line = lines[at + 1 + idx]
        assert line.startswith('{:<15s}'.format(item + ': ')) and abs(float(line[15:]) - want) <= 1e-4, (line, want)
        p32 = pred[0].permute(1, 2, 0).cpu().numpy()
        rule = np.clip(p32 * np.float32(255) + np.float32(0.5), np.float32(0), np.float32(255)).astype(np.uint8)
        assert np.array_equal(np.array(Image.open(os.path.join(out, "result", item, name))), rule), item
    line = lines[at + 13]
    assert line.startswith('Average:       ') and abs(float(line[15:]) - total / 12) <= 1e-4


@pytest.mark.parametrize("loss", [DEFAULT, DEFAULT + '+0.1*VGG'])
def test_epoch_is_the_manual_loop_bit_for_bit(loss, small_set, middlebury, state, tmp_path, device, capsys):
    out = str(tmp_path / "out")
    vgg_state = LR.vgg16_state(7)
    args = _args(out, loss, vgg_weights=vgg_state)
    db = Middlebury_other(*middlebury, device=device)
    model = _model(args, state)
    crit = losses.Loss(args)
    trainer = Trainer(args, _loader(small_set, device), db, model, crit)
    assert trainer.max_step == 3 and not trainer.terminate() and not model.training           # the initial test: eval mode
    for d in ("result", "checkpoint"):
        assert os.path.isdir(os.path.join(out, d))
    _seed(7)
    trainer.train()
    assert model.training and trainer.current_epoch == 1 and trainer.terminate()
    assert trainer.scheduler.last_epoch == 1                                                  # stepped once per epoch
    history = list(trainer.loss_history)
    assert len(history) == 3 and all(isinstance(v, float) and math.isfinite(v) for v in history)
    printed = capsys.readouterr().out
    assert '{:<13s}{:<14s}{:<6s}{:<16s}{:<12s}{:<20.16f}'.format('Train Epoch: ', '[0/1]', 'Step: ', '[0/3]', 'train loss: ',
                                                                 history[0]) in printed         # trainer.py:52
    assert printed.count('Train Epoch: ') == 1
    trainer.test()
    trainer.logfile.flush()

    # the same epoch by hand
    ref = _model(args, state)
    ref.train()
    opt = torch.optim.Adamax(ref.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)
    charb = utility.Module_CharbonnierLoss()
    perceptual = crit.loss_module[1] if 'VGG' in loss else None
    _seed(7)
    manual = []
    for batch in _loader(small_set, device):
        assert batch.lab is None and batch.rgb.shape == (3, 2, 3, 32, 48)
        opt.zero_grad()
        o = ref(batch.rgb_frame1, batch.rgb_frame2)
        value = 1.0 * charb(o["frame1"], batch.rgb_target)
        if perceptual is not None:
            value = value + 0.1 * perceptual(o["frame1"], batch.rgb_target)
        value = value + 0.01 * o["g_Spatial"] + 0.005 * o["g_Occlusion"]
        value.backward()
        opt.step()
        manual.append(float(value.detach()))
    print("loss history:", history, "by hand:", manual)
    assert history == manual
    moved = 0
    for (k, p), (k2, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert k == k2 and torch.equal(p, q), k
        moved += int(not torch.equal(p.detach().cpu(), state[k[len("model."):]]))
    assert moved > 0
    if perceptual is not None:
        assert all(p.grad is None for p in perceptual.parameters())

    # the log, the pictures and the checkpoint
    _check_log_and_pictures(out, ['Epoch: 0  ', 'Epoch: 1  '], model, db, "001.png")
    assert os.path.exists(os.path.join(out, "result", "Walking", "000.png"))
    ckpt = torch.load(os.path.join(out, "checkpoint", "model_epoch001.pth"), map_location="cpu")
    assert sorted(ckpt) == ['epoch', 'state_dict'] and ckpt['epoch'] == 1
    fresh = Model(args)
    fresh.load(ckpt['state_dict'])
    for (k, p), (k2, q) in zip(model.named_parameters(), fresh.named_parameters()):
        assert k == k2 and torch.equal(p, q), k
    trainer.close()
    assert trainer.logfile.closed


def test_load_resumes_at_the_checkpoints_epoch(small_set, middlebury, state, tmp_path, device):
    ck = str(tmp_path / "model_epoch001.pth")
    torch.save({'epoch': 1, 'state_dict': state}, ck)
    out = str(tmp_path / "resumed")
    train.main(["--train", small_set, "--test_input", middlebury[0], "--gt", middlebury[1], "--out_dir", out, "--epochs", "1",
                "--batch_size", "2", "--patch_size", "32", "--workers", "2", "--load", ck])
    # epoch 1 of 1: the initial test of the loaded weights, and nothing trained
    args = _args(out)
    _check_log_and_pictures(out, ['Epoch: 1  '], _model(args, state), Middlebury_other(*middlebury, device=device), "001.png")
    assert os.listdir(os.path.join(out, "checkpoint")) == []
    config = open(os.path.join(out, "config.txt")).read()
    assert f"load: {ck}" in config and "vgg_weights: " in config and "workers: 2" in config


def test_stock_dataloader_step(small_set, middlebury, state, tmp_path, device):
    args = _args(str(tmp_path / "out"))
    ds = DBreader_Vimeo90k(small_set, random_crop=(32, 48))
    ds.triplet_list = ds.triplet_list[:2]
    ds.file_len = 2
    _seed(3)
    loader = DataLoader(dataset=ds, batch_size=2, shuffle=True, num_workers=0)                # train.py:55 of the reference
    model = _model(args, state)
    trainer = Trainer(args, loader, Middlebury_other(*middlebury, device=device), model, losses.Loss(args))
    assert trainer.max_step == 1
    trainer.train()
    loss = trainer.loss_history
    assert len(loss) == 1 and math.isfinite(loss[0]) and loss[0] > 0
    assert any(not torch.equal(p.detach().cpu(), state[k[len("model."):]]) for k, p in model.named_parameters())
    trainer.close()
    with pytest.raises(ValueError, match="rgb=True"):
        t2 = Trainer(args, TripletLoader(ds, 2, device=device, rgb=False, lab=True), trainer.test_loader, model, trainer.loss)
        t2.train()


def test_command_line(small_set, middlebury, tmp_path, device):
    out = str(tmp_path / "cli")
    env = dict(os.environ)
    env["PYTHONPATH"] = PKG_DIR + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "vfi_amd.adacof.train", "--train", small_set, "--test_input", middlebury[0],
                        "--gt", middlebury[1], "--out_dir", out, "--epochs", "1", "--batch_size", "2", "--patch_size", "32",
                        "--workers", "2", "--gpu_id", "0"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for f in ("checkpoint/model_epoch001.pth", "log.txt", "config.txt", "result/Venus/000.png", "result/Venus/001.png"):
        assert os.path.exists(os.path.join(out, f)), f
    assert "Train Epoch: [0/1]" in r.stdout and "1.000 * Charb" in r.stdout and "Average: " in r.stdout
    log = open(os.path.join(out, "log.txt")).read()
    assert log.count("Epoch: ") == 2 and log.count("Average: ") == 2 and all(n + ": " in log for n in LR.MIDDLEBURY)
    config = open(os.path.join(out, "config.txt")).read()
    assert "batch_size: 2" in config and "loss: " + DEFAULT in config
    ckpt = torch.load(os.path.join(out, "checkpoint/model_epoch001.pth"), map_location="cpu")
    assert ckpt["epoch"] == 1
    Model(_args(out)).load(ckpt["state_dict"])
