"""Per-call timing of the deterministic vs atomic weight-gradient convs at config-3 map sizes (4 x 720p): five alternating runs of
20 calls per arm, median [range] in microseconds.  Includes the wrapper's output zeroing and slab allocation."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import statistics, torch
from transformerupscaler_amd import ops
dev = "cuda"; g = torch.Generator(device=dev).manual_seed(0)
B, H, W = 4, 720, 1280
x64 = torch.randn((B, H, W, 64), generator=g, device=dev).bfloat16()
gm = torch.randn((B, H, W, 64), generator=g, device=dev).bfloat16()
gpl = torch.randn((B, 3, H, W), generator=g, device=dev)
x3 = torch.randn((B, 3, H, W), generator=g, device=dev)
g2 = torch.randn((B, 3, 2 * H, 2 * W), generator=g, device=dev)
cases = {"c64 (decoder_conv1)": lambda: ops.conv_c64_wgrad(x64, gm, 1), "thin (decoder_conv2)": lambda: ops.conv_thin_wgrad(x64, gpl, True),
         "planar r=1": lambda: ops.conv_planar_wgrad(x3, gpl, 1), "planar r=2": lambda: ops.conv_planar_wgrad(x3, g2, 2)}
def t(fn, n=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize(); return e0.elapsed_time(e1) / n * 1000
for name, fn in cases.items():
    res = {False: [], True: []}
    for arm in (False, True): ops.deterministic = arm; fn(); torch.cuda.synchronize()
    for _ in range(5):
        for arm in (False, True):
            ops.deterministic = arm; res[arm].append(t(fn))
    print(f"{name}: atomic median {statistics.median(res[False]):.1f} us [{min(res[False]):.1f}-{max(res[False]):.1f}], "
          f"det median {statistics.median(res[True]):.1f} us [{min(res[True]):.1f}-{max(res[True]):.1f}]")
ops.deterministic = False
