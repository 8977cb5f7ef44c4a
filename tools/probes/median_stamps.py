"""Probe: where the waves of median_walk_kernel spend their cycles at 1080p, S = 50 (library built with -DMEDIAN_STAMPS on
vfi_image.hip, selected by VFI_HIP_LIBRARY): s_memtime per phase, summed over every wave of one launch."""
import ctypes, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd")]
from vfi_amd import ops, _lib
dev = torch.device("cuda:0")
h, w = 1080, 1920
yy, xx = np.meshgrid(np.linspace(0, 6, h), np.linspace(0, 9, w), indexing="ij")
smooth = torch.from_numpy((np.sin(yy) * np.cos(xx) + 0.1 * np.sin(7 * xx)).astype(np.float32)[None]).to(dev)
noise = torch.randn((1, h, w), device=dev)
lib = _lib.lib()
buf = (ctypes.c_ulonglong * 8)()
names = ["load", "key mask", "radix passes", "rank build", "fill + first cursor", "slide + cursor walk"]
for name, x in (("smooth", smooth), ("noise", noise)):
    for _ in range(2):
        ops.median_filter(x, 50)
    torch.cuda.synchronize()
    assert lib.vfi_debug_median_stamps(buf, 1) == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); ops.median_filter(x, 50); e1.record(); torch.cuda.synchronize()
    assert lib.vfi_debug_median_stamps(buf, 0) == 0
    a = np.frombuffer(buf, dtype=np.uint64).astype(np.float64)
    waves, passes = a[6], a[7]
    tiles = waves / 16
    print(f"median50 1080p {name}: {e0.elapsed_time(e1):.3f} ms (stamped build); {tiles:.0f} tiles, {passes / tiles:.1f} radix passes per tile")
    tot = a[:6].sum()
    for k, nm in enumerate(names):
        print(f"  {nm:22s} {a[k] / waves:9.0f} cycles per wave  {100 * a[k] / tot:5.1f} %")
