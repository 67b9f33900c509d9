"""Per-call timing of the deterministic vs atomic weight-gradient convs, weight-gradient GEMMs, column sums and LayerNorm backward
at config-3 sizes (4 x 720p: 61,440 token rows): five alternating runs of 20 calls per arm, median [range] in microseconds
(DESIGN 7d).  Includes the wrapper's output zeroing and slab allocation (the token-path forms reuse one cached slab)."""
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
M = 61440
tok = {n: torch.randn((M, n), generator=g, device=dev).bfloat16() for n in (192, 576, 768)}
t32 = torch.randn((M, 192), generator=g, device=dev)
mean, rstd, gamma = t32.mean(1).contiguous(), t32.var(1).rsqrt().contiguous(), torch.ones(192, device=dev)
for ni, nj in ((576, 192), (192, 192), (768, 192), (192, 768)):
    cases[f"gemm_wgrad_bias {ni}x{nj}"] = lambda ni=ni, nj=nj: ops.gemm_wgrad_bias(tok[ni], tok[nj])
cases.update({"patch_wgrad wide (patch_unembed)": lambda: ops.patch_wgrad(t32, gm, False),
              "colsum 61440x192 fp32": lambda: ops.colsum(t32), "colsum 3.7Mx64 bf16": lambda: ops.colsum(gm.view(-1, 64)),
              "layernorm_bwd (+dropout)": lambda: ops.layernorm_bwd(tok[192], t32, mean, rstd, gamma, gres=t32, drop=(0.1, 7))})
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
