"""Training from clips on the device: `ClipTripletLoader` over a 64x96 `C420jpeg` clip of 7 frames the
test writes, against `ops.yuv_triplet_batch_prepare` on the same bytes and parameters, and two steps of each of the three
trainers fed through their command line's own flags (`--train_clips`, `--clip_stride 2`: 3 samples, 2 steps at batch 2)."""
import math
import os
import random
import types

import numpy as np
import pytest
import torch

import adacof_loss_ref as LR
import phasenet_fusion_ref as FR
from oracle import nets_cpu, pipeline_cpu
from vfi_amd import ops
from vfi_amd.adacof import losses
from vfi_amd.adacof import train as adacof_train
from vfi_amd.adacof.models import Model
from vfi_amd.adacof.TestModule import Middlebury_other
from vfi_amd.adacof.trainer import Trainer as AdaCoFTrainer
from vfi_amd.fusion_net import train as fusion_train
from vfi_amd.fusion_net.fusion_net import FusionNet
from vfi_amd.fusion_net.trainer import Trainer as FusionNetTrainer
from vfi_amd.phase_net.architecture import PhaseNet as ArchPhaseNet
from vfi_amd.phase_net.phase_net import PhaseNet
from vfi_amd.train import clipreader as C
from vfi_amd.train import train as phase_train
from vfi_amd.train.datareader import TripletBatch
from vfi_amd.train.pyramid import Pyramid
from vfi_amd.train.trainer import Trainer
from vfi_amd.train.utils import calc_pyr_height

pytestmark = pytest.mark.gpu

H, W, FRAMES = 64, 96, 7


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _height(h, w):
    return calc_pyr_height(torch.empty(3, h, w, device="meta"))


@pytest.fixture(scope="module")
def clip_dir(tmp_path_factory):
    """one clip: a smooth picture that moves a little from frame to frame (something a network can take a step on)"""
    root = tmp_path_factory.mktemp("clips")
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with open(root / "clip.y4m", "wb") as f:
        f.write(b"YUV4MPEG2 W96 H64 F25:1 Ip C420jpeg\n")
        for k in range(FRAMES):
            y = 128 + 90 * np.sin((xx + 1.5 * k) * 0.21) * np.cos((yy - k) * 0.17)
            cb = 128 + 60 * np.sin((xx[::2, ::2] + k) * 0.11)
            cr = 128 + 60 * np.cos((yy[::2, ::2] - k) * 0.13)
            f.write(b"FRAME\n" if k % 2 else b"FRAME Xk=%d\n" % k)
            for plane in (y, cb, cr):
                f.write(np.clip(plane, 16, 235).round().astype(np.uint8).tobytes())
    return str(root)


def _batches(loader):
    return [(b.rgb.clone() if b.rgb is not None else None, b.lab.clone() if b.lab is not None else None, b.params.clone(), list(b.paths))
            for b in loader]


def _by_hand(ds, batch_size, device, rgb=True, lab=True):
    """What ClipTripletLoader yields, assembled here: the permutation, the draws in sample order, the frames' bytes, one
    `ops.yuv_triplet_batch_prepare` per batch.  Consumes the generators as the loader does."""
    order = torch.randperm(len(ds)).tolist()
    out = []
    for a in range(0, len(order), batch_size):
        idx = order[a:a + batch_size]
        params = torch.tensor([ds.draw(ds.height, ds.width) for _ in idx], dtype=torch.int32)
        src = torch.from_numpy(np.stack([np.stack(ds.raw(i)) for i in idx])).to(device)
        r, l = ops.yuv_triplet_batch_prepare(src, ds.fmt, params, ds.crop_size(ds.height, ds.width), (ds.height, ds.width), rgb=rgb, lab=lab)
        out.append(TripletBatch(l, r, params, [ds.paths[i] for i in idx]))
    return out


def test_loader_batches_are_the_ops_bits_whatever_the_workers(clip_dir, device):
    ds = C.DBreader_Y4M(clip_dir, random_crop=(32, 48))
    assert len(ds) == 5 and (ds.height, ds.width) == (H, W) and ds.fmt.yuv == (0, 0, 0, 0)
    runs = []
    for workers in (1, 4, 1):                                         # the third pass: one seed, the same batches again
        _seed(21)
        loader = C.ClipTripletLoader(ds, 2, shuffle=True, workers=workers, device=device)
        assert len(loader) == 3
        runs.append(_batches(loader))
    _seed(21)
    hand = _by_hand(ds, 2, device)
    assert [tuple(r[0].shape) for r in runs[0]] == [(3, 2, 3, 32, 48), (3, 2, 3, 32, 48), (3, 1, 3, 32, 48)]      # a short last batch
    assert len({tuple(p) for r in runs[0] for p in r[2].tolist()}) > 1
    for run in runs:
        for (rgb, lab, params, paths), want in zip(run, hand):
            assert torch.equal(params, want.params) and paths == want.paths
            assert torch.equal(rgb, want.rgb) and torch.equal(lab, want.lab)
            assert bool(torch.isfinite(rgb).all()) and float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0
    assert sorted(p for r in runs[0] for p in r[3]) == sorted(ds.paths)
    # rgb=False as the phase trainer asks
    _seed(3)
    b = next(iter(C.ClipTripletLoader(ds, 2, workers=2, device=device, rgb=False)))
    assert b.rgb is None and b.lab.shape == (3, 6, 32, 48) and b.img_batch_phase.shape == (18, 32, 48)


def test_clip_stride_2_gives_3_samples(clip_dir):
    args = phase_train.parser.parse_args(["--train_clips", clip_dir, "--clip_stride", "2", "--crop", "32", "48"])
    ds, loader = C.training_input(args, tuple(args.crop), "cpu")
    assert len(ds) == 3 and ds.paths == [os.path.join(clip_dir, "clip.y4m") + f"#{k}" for k in range(3)]
    assert isinstance(loader, C.ClipTripletLoader)


def _phase_run(clip_dir, out, device, by_hand):
    height = _height(32, 48)
    args = phase_train.parser.parse_args(["--train_clips", clip_dir, "--clip_stride", "2", "--crop", "32", "48", "--batch_size", "2",
                                          "--workers", "2", "--epochs", "1", "--gpu_id", "0"])
    net = ArchPhaseNet(height, device, num_img=2)
    net.core.load_state_dict(FR.net_state(41, 2))
    _seed(7)
    if by_hand:
        ds = C.DBreader_Y4M(clip_dir, random_crop=(32, 48), stride=2)
        loader = _by_hand(ds, 2, device, rgb=False)
    else:
        ds, loader = C.training_input(args, tuple(args.crop), device, rgb=False)
        assert isinstance(loader, C.ClipTripletLoader) and len(loader) == 2
    trainer = Trainer(args, loader, net, Pyramid(height=height, nbands=4, scale_factor=np.sqrt(2), device=device), lr=1e-3,
                      out_dir=out, m=3, m_update=500)
    trainer.train()
    history = list(trainer.loss_history)
    trainer.close()
    return history, net


def test_phase_trainer_takes_two_steps_from_train_clips_and_equals_hand_made_batches(clip_dir, tmp_path, device):
    history, net = _phase_run(clip_dir, str(tmp_path / "a"), device, by_hand=False)
    assert len(history) == 2 and all(math.isfinite(v) for v in history)
    start = FR.net_state(41, 2)
    assert sum(int(not torch.equal(v.cpu(), start[k])) for k, v in net.core.state_dict().items() if k in start) > 0
    manual, ref = _phase_run(clip_dir, str(tmp_path / "b"), device, by_hand=True)
    print("loss history:", history, "hand-made batches:", manual)
    assert history == manual
    for (k, p), (k2, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert k == k2 and torch.equal(p, q), k


def test_fusion_net_trainer_takes_two_steps_from_train_clips(clip_dir, tmp_path, device):
    h, w = 64, 96
    args = fusion_train.parser.parse_args(["--train_clips", clip_dir, "--clip_stride", "2", "--crop", str(h), str(w), "--batch_size", "2",
                                           "--workers", "2", "--epochs", "1", "--gpu_id", "0"])
    weights = pipeline_cpu.seeded_weights(0)
    fusion = FusionNet().to(device)
    fusion.load_state_dict(weights["fusionnet"])
    pyr = Pyramid(height=_height(h, w), nbands=4, scale_factor=np.sqrt(2), device=device)
    phase_net = PhaseNet(pyr, device, num_img=2)
    phase_net.load_state_dict(weights["phasenet"])
    adacof = Model(types.SimpleNamespace(model="vfi_amd.fusion_net.fusion_adacofnet", kernel_size=5, dilation=1, gpu_id=0))
    adacof.load(weights["adacof"])
    adacof.eval()
    _seed(9)
    ds, loader = C.training_input(args, tuple(args.crop), device)
    assert isinstance(ds, C.DBreader_Y4M) and len(loader) == 2
    trainer = FusionNetTrainer(args, loader, fusion, phase_net, adacof, my_pyr=pyr, lr=1e-4, out_dir=str(tmp_path / "out"))
    trainer.train()
    history = list(trainer.loss_history)
    trainer.close()
    assert len(history) == 2 and all(math.isfinite(v) for v in history)
    assert sum(int(not torch.equal(p.detach().cpu(), weights["fusionnet"][k])) for k, p in fusion.named_parameters()) > 0


def test_adacof_trainer_takes_two_steps_from_train_clips(clip_dir, tmp_path, device):
    middlebury = LR.write_middlebury(str(tmp_path / "middlebury"), 40, 56, seed=3)
    args = adacof_train.parser.parse_args(["--train_clips", clip_dir, "--clip_stride", "2", "--patch_size", "32", "--batch_size", "2",
                                           "--workers", "2", "--epochs", "1", "--gpu_id", "0", "--out_dir", str(tmp_path / "out"),
                                           "--test_input", middlebury[0], "--gt", middlebury[1]])
    args.model = "vfi_amd.adacof.models." + args.model
    state = nets_cpu.adacofnet_random_state_dict(12, kernel_size=5)
    model = Model(args)
    model.load(state)
    _seed(7)
    ds, loader = C.training_input(args, (args.patch_size, args.patch_size), device, rgb=True, lab=False)
    assert isinstance(ds, C.DBreader_Y4M) and ds.random_crop == (32, 32) and len(loader) == 2
    first = next(iter(loader))
    assert first.lab is None and first.rgb.shape == (3, 2, 3, 32, 32)
    trainer = AdaCoFTrainer(args, loader, Middlebury_other(*middlebury, device=device), model, losses.Loss(args))
    trainer.train()
    history = list(trainer.loss_history)
    trainer.close()
    assert len(history) == 2 and all(math.isfinite(v) for v in history)
    assert any(not torch.equal(p.detach().cpu(), state[k[len("model."):]]) for k, p in model.named_parameters())
