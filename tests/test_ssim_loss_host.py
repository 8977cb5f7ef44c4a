"""SSIM as a loss, what needs no GPU: the batch restatement against scoring_ref.ssim_ref, the closed
form of the gradient against float64 autograd, the plain-torch face of vfi_amd.evaluation.ssim against both, the loss
grammar, the command-line flag, the refusals of the module and of the two entries."""
import ctypes
import types

import pytest
import torch

import scoring_ref as SR
import ssim_loss_ref as R
from vfi_amd.evaluation import ssim as ssim_mod

IDS = [R.case_id(c) for c in R.ENTRY_CASES]


def test_batch_restatement_is_ssim_ref():
    """image by image the batch expression is scoring_ref.ssim_ref: equal maps, bit for bit, in both dtypes"""
    for i in (0, 1, 4):
        c = SR.ssim_case(i)
        for dtype in (torch.float64, torch.float32):
            s, m = SR.ssim_ref(c["x"], c["y"], dtype)
            got = R.ssim_map(c["x"].to(dtype)[None], c["y"].to(dtype)[None])
            assert torch.equal(got[0], m)
            assert abs(float(R.ssim_batch(c["x"].to(dtype)[None], c["y"].to(dtype)[None])[0]) - s) <= 1e-6
    c = SR.ssim_case(5)                                          # 384 x 385, f = 2
    s, m = SR.ssim_ref(c["x"], c["y"], torch.float64)
    assert torch.equal(R.ssim_map(c["x"].double()[None], c["y"].double()[None], factor=c["f"])[0], m)


@pytest.mark.parametrize("case", R.ENTRY_CASES, ids=IDS)
def test_closed_form_gradient_is_autograd(case):
    """the A, B, Cm form the backward kernel evaluates, in float64, against float64 autograd of the restatement"""
    shape, ks, sigma = case
    c = R.case(shape, ks, sigma)
    got = R.closed_form_grad_x(c["x"].double(), c["y"].double(), c["up"], ks, sigma)
    err = float((got - c["gx64"]).abs().max() / c["gx64"].abs().max())
    print(f"{R.case_id(case)}: closed form against autograd, of the largest entry: {err:.2e}")
    assert err <= 1e-12
    swapped = R.closed_form_grad_x(c["y"].double(), c["x"].double(), c["up"], ks, sigma)       # the target's gradient
    assert float((swapped - c["gy64"]).abs().max() / c["gy64"].abs().max()) <= 1e-12


@pytest.mark.parametrize("dtype,rtol", [(torch.float64, 1e-13), (torch.float32, 1e-6)])
@pytest.mark.parametrize("case", R.ENTRY_CASES, ids=IDS)
def test_plain_torch_face(case, dtype, rtol):
    """CPU arguments: the module is the restatement and its autograd, in the arguments' dtype"""
    shape, ks, sigma = case
    c = R.case(shape, ks, sigma)
    x, y = c["x"].to(dtype).clone().requires_grad_(True), c["y"].to(dtype).clone().requires_grad_(True)
    loss = ssim_mod.SSIMLoss(kernel_size=ks, kernel_sigma=sigma, reduction='none')(x, y)
    assert loss.dtype == dtype and loss.shape == (shape[0],)
    (loss * c["up"].to(dtype)).sum().backward()
    v, _, gx, gy = R.evaluate(c["x"], c["y"], c["up"], dtype, ks, sigma)
    assert torch.allclose(loss.detach(), v, rtol=rtol, atol=0)
    assert torch.allclose(x.grad, gx, rtol=0, atol=rtol * float(gx.abs().max()))
    assert torch.allclose(y.grad, gy, rtol=0, atol=rtol * float(gy.abs().max()))
    with torch.no_grad():
        s = ssim_mod.ssim(x, y, kernel_size=ks, kernel_sigma=sigma)
        assert torch.allclose(s, 1 - v, rtol=rtol, atol=0)
        for red, want in (('mean', v.mean()), ('sum', v.sum())):
            got = ssim_mod.SSIMLoss(kernel_size=ks, kernel_sigma=sigma, reduction=red)(x, y)
            assert got.dim() == 0 and torch.allclose(got, want, rtol=rtol, atol=0)


def test_plain_torch_face_pools_and_scales():
    """f = 2 on a 384 x 385 image against ssim_ref; data_range r on r * images is the data_range 1 value"""
    c = SR.ssim_case(5)
    x, y = c["x"].double()[None], c["y"].double()[None]
    assert abs(float(ssim_mod.ssim(x, y)[0]) - c["ref64"]) <= 1e-13
    c = SR.ssim_case(9)                                         # the same shape, downsample=False
    x, y = c["x"].double()[None], c["y"].double()[None]
    assert abs(float(ssim_mod.ssim(x, y, downsample=False)[0]) - c["ref64"]) <= 1e-13
    small = SR.ssim_case(4)
    x, y = small["x"].double()[None], small["y"].double()[None]
    assert abs(float(ssim_mod.ssim(255 * x, 255 * y, data_range=255.0)[0]) - small["ref64"]) <= 1e-12




def test_refusals_of_the_module():
    """every refusal is a ValueError raised by the argument check, which runs before either path is chosen.

    On 384 x 20: piq takes the pooling factor from the short side, f = max(1, round(min(H, W) / 256)), so a plane whose
    short side is below 128 is never pooled, and one that is pooled keeps at least 192 pixels on its short side: "too small
    after pooling" cannot arise.  384 x 20 has f = 1 and a 374 x 10 map; piq accepts it and so does the module (checked
    against float64 below).  The refusal with a long side of 384 is 384 x 10."""
    z = lambda *s: torch.zeros(s)
    with pytest.raises(ValueError, match="smaller than the 11-tap window"):
        ssim_mod.SSIMLoss()(z(1, 3, 10, 40), z(1, 3, 10, 40))
    with pytest.raises(ValueError, match="smaller than the 11-tap window"):
        ssim_mod.SSIMLoss()(z(1, 1, 384, 10), z(1, 1, 384, 10))
    assert ssim_mod.pool_factor(384, 20) == 1 == SR.pool_factor(384, 20)
    x, y = R.batch_inputs((1, 1, 384, 20), 77)
    got = ssim_mod.ssim(x.double(), y.double())
    assert abs(float(got[0]) - SR.ssim_ref(x[0], y[0], torch.float64)[0]) <= 1e-13
    with pytest.raises(ValueError, match="kernel_size"):
        ssim_mod.SSIMLoss(kernel_size=10)
    with pytest.raises(ValueError, match="kernel_size"):
        ssim_mod.ssim(z(1, 1, 40, 40), z(1, 1, 40, 40), kernel_size=13)
    with pytest.raises(ValueError, match="kernel_size"):
        ssim_mod.ssim(z(1, 1, 40, 40), z(1, 1, 40, 40), kernel_size=4)
    with pytest.raises(ValueError, match="reduction"):
        ssim_mod.SSIMLoss(reduction='batchmean')
    with pytest.raises(ValueError, match="must be equal"):
        ssim_mod.SSIMLoss()(z(1, 3, 40, 40), z(1, 3, 40, 41))
    with pytest.raises(ValueError, match="must be equal"):
        ssim_mod.SSIMLoss()(z(3, 40, 40), z(3, 40, 40))
    with pytest.raises(ValueError, match="kernel_sigma"):
        ssim_mod.ssim(z(1, 1, 40, 40), z(1, 1, 40, 40), kernel_sigma=0.0)
    assert ssim_mod.pool_factor(384, 385) == 2 and ssim_mod.pool_factor(641, 643) == 3
    for h, w in ((384, 385), (641, 643), (767, 390), (896, 899), (128, 32), (640, 2000)):
        assert ssim_mod.pool_factor(h, w) == SR.pool_factor(h, w)


def test_entries_refuse_bad_arguments_without_a_device():
    """the library's status codes, returned before anything is enqueued (no GPU here): -1 VFI_ERR_INVALID_ARG, -2 VFI_ERR_SHAPE"""
    import vfi_amd
    h = vfi_amd.lib()
    p = ctypes.c_void_p(16)
    f32 = ctypes.c_float
    fwd = lambda n, c, hh, ww, ks, sg=1.5, xs=1 << 30, x=p: h.vfi_ssim_loss_forward(x, xs, p, 1 << 30, p, p, n, c, hh, ww, ks, f32(sg), f32(1e-4),
                                                                              f32(9e-4), None)
    bwd = lambda n, c, hh, ww, ks, sg=1.5, gs=1 << 30, up=p: h.vfi_ssim_loss_backward(p, 1 << 30, p, 1 << 30, up, p, gs, n, c, hh, ww, ks,
                                                                                f32(sg), f32(1e-4), f32(9e-4), None)
    for f in (fwd, bwd):
        assert f(1, 3, 10, 40, 11) == -2 and b"smaller than the 11-tap window" in h.vfi_last_error()
        assert f(1, 3, 40, 10, 11) == -2 and f(1, 1, 192, 10, 11) == -2 and f(1, 1, 6, 6, 7) == -2
        assert f(1, 3, 40, 40, 10) == -1 and b"kernel_size" in h.vfi_last_error()
        assert f(1, 3, 40, 40, 13) == -1 and f(1, 3, 40, 40, 1) == -1 and f(1, 3, 40, 40, -3) == -1
        assert f(0, 3, 40, 40, 11) == -1 and f(1, 0, 40, 40, 11) == -1 and f(-1, 3, 40, 40, 11) == -1
        assert f(1, 3, 40, 40, 11, 0.0) == -1 and f(1, 3, 40, 40, 11, float("nan")) == -1
    assert fwd(2, 3, 40, 40, 11, xs=3 * 40 * 40 - 1) == -1 and b"batch stride" in h.vfi_last_error()
    assert bwd(2, 3, 40, 40, 11, gs=3 * 40 * 40 - 1) == -1 and b"batch stride" in h.vfi_last_error()
    assert fwd(1, 3, 40, 40, 11, x=None) == -1 and bwd(1, 3, 40, 40, 11, up=None) == -1
    assert h.vfi_avg_pool_backward(None, p, 1, 8, 8, 2, None) == -1 and h.vfi_avg_pool_backward(p, p, 1, 8, 8, 0, None) == -1
    assert h.vfi_avg_pool_backward(p, p, 0, 8, 8, 2, None) == -1 and h.vfi_avg_pool_backward(p, p, 1, 2, 8, 3, None) == -1


def test_loss_grammar(capsys):
    from vfi_amd.adacof import losses
    crit = losses.Loss(types.SimpleNamespace(loss='1*Charb+0.1*SSIM+0.01*g_Spatial'))
    assert [(l['type'], l['weight']) for l in crit.loss] == [('Charb', 1.0), ('SSIM', 0.1)]
    term = crit.loss_module[1]
    assert isinstance(term, ssim_mod.SSIMLoss) and term.reduction == 'mean' and term.downsample is True
    assert (term.kernel_size, term.kernel_sigma, term.k1, term.k2, term.data_range) == (11, 1.5, 0.01, 0.03, 1.0)
    assert [r['type'] for r in crit.regularize] == ['g_Spatial'] and "0.100 * SSIM" in capsys.readouterr().out
    assert len(list(crit.parameters())) == 0
    # the refusals stay as they were
    with pytest.raises(NotImplementedError):
        losses.Loss(types.SimpleNamespace(loss='1*Charb+0.005*GAN'))
    with pytest.raises(ValueError, match="unknown loss type"):
        losses.Loss(types.SimpleNamespace(loss='1*MS-SSIM'))
    # on the host the term is the plain-torch face
    frame, gt = R.batch_inputs((2, 3, 16, 20), 5)
    only = losses.Loss(types.SimpleNamespace(loss='0.5*SSIM'))
    got = only({'frame1': frame}, gt, None)
    assert torch.equal(got, 0.5 * ssim_mod.SSIMLoss()(frame, gt)) and 0 < float(got) < 0.5


def test_command_line_flag():
    from vfi_amd.fusion_net import train as fusion_train
    assert fusion_train.parser.parse_args([]).ssim_weight == 0.0
    a = fusion_train.parser.parse_args(["--ssim_weight", "0.25"])
    assert a.ssim_weight == 0.25 and a.lpips_weight == 0.0
