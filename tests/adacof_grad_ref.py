"""Differentiable torch restatement of the AdaCoF forward (reference src/adacof/cupy_module/adacof.py:6-65), used by
the backward tests: its autograd gradients are what FunctionAdaCoF.backward must reproduce.

Semantics as the reference's kernel: A = (int)alpha truncates toward zero and carries no gradient, each of the four
corners is clamped to the input on its own, the bilinear weights come from the un-clamped fractions, and the channel
sum runs over all C channels.  Runs on whatever device / dtype the arguments have (the tests use float64 on the CPU).
"""
import torch


def adacof_restated(input, weight, offset_i, offset_j, dilation, y0=0):
    """out[n, c, y, x] = sum_{k,l} w * bilinear(input[n, c], y0 + y + k*d + alpha, x + l*d + beta).

    `weight`, `offset_i`, `offset_j` are (N, F*F, H, W) and may be a band of rows starting at output row `y0` of a
    larger image; `input` is always the full (padded) frame, since a band's taps reach rows outside it."""
    n, c, hin, win = input.shape
    ff, h, w = weight.shape[1:]
    f = int(round(ff ** 0.5))
    dev = input.device
    rows = (torch.arange(h, device=dev) + y0).view(1, h, 1)
    cols = torch.arange(w, device=dev).view(1, 1, w)
    flat = input.reshape(n, c, hin * win)
    out = input.new_zeros((n, c, h, w))
    for k in range(f):
        for l in range(f):
            t = k * f + l
            alpha, beta = offset_i[:, t], offset_j[:, t]
            A, B = alpha.detach().trunc(), beta.detach().trunc()
            fa, fb = alpha - A, beta - B
            r = rows + k * dilation + A.long()
            q = cols + l * dilation + B.long()
            i0, i1 = r.clamp(0, hin - 1), (r + 1).clamp(0, hin - 1)
            j0, j1 = q.clamp(0, win - 1), (q + 1).clamp(0, win - 1)

            def gather(i, j):
                idx = (i * win + j).reshape(n, 1, h * w).expand(n, c, h * w)
                return flat.gather(2, idx).reshape(n, c, h, w)

            ga, gb = (1 - fa).unsqueeze(1), (1 - fb).unsqueeze(1)
            fa, fb = fa.unsqueeze(1), fb.unsqueeze(1)
            v = gather(i0, j0) * ga * gb + gather(i1, j0) * fa * gb + gather(i0, j1) * ga * fb + gather(i1, j1) * fa * fb
            out = out + weight[:, t].unsqueeze(1) * v
    return out


def restated_grads(input, weight, offset_i, offset_j, dilation, grad_output, y0=0):
    """float64 autograd gradients (weight, offset_i, offset_j) of adacof_restated for upstream `grad_output`."""
    leaves = [torch.as_tensor(x).detach().double().cpu().requires_grad_() for x in (weight, offset_i, offset_j)]
    out = adacof_restated(torch.as_tensor(input).detach().double().cpu(), *leaves, dilation, y0)
    return torch.autograd.grad(out, leaves, torch.as_tensor(grad_output).detach().double().cpu())
