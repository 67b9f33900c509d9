#!/usr/bin/env python3
"""Build-time guard for the kernels whose LDS-DMA hand-off is ordered by hand-counted `s_waitcnt vmcnt(N)`.

Scratch (register spill) loads and stores count on the same `vmcnt` as the LDS-DMA pieces those waits count, so a build of
such a kernel with scratch > 0 can pass a barrier before its weights have landed: wrong results at full size, masked at small
sizes (DESIGN 5b records exactly that for the whole-block kernel).  The Makefile compiles every object with
`-Rpass-analysis=kernel-resource-usage`, keeps the remarks in build/<file>.remarks and runs this script before linking:

    check_resources.py build/*.remarks  ->  build/resource_usage.json, exit 1 if a guarded kernel reports scratch

Diagnostic instantiations (the `STAMPS = true` builds, which spill by design and are never launched by the product path)
are exempt.  A GUARDED name or a REG_BUDGET fragment that matches no kernel of its source file (a rename that left the entry
behind) fails the same way, for the source files that are part of the invocation.  The JSON also records the compiler version, which bench.py copies into its line.
"""
import json
import os
import re
import subprocess
import sys

# (source file, kernel function names) -> every instantiation must have ScratchSize == 0
GUARDED = [
    ("fused_attn.hip", ["fused_qkv_attn_kernel"]),
    ("block_stream.hip", ["blocks_stream_kernel"]),
    ("conv3x3_c64.hip", ["conv_c64_persistent_kernel", "bra_rows_persistent_kernel", "conv3_thin_rows_kernel"]),
    ("conv_thin.hip", ["conv3x3_c3_persistent_kernel"]),
    ("decoder_fused.hip", ["decoder_fused_kernel"]),
    ("conv12_fused.hip", ["conv12_fused_kernel"]),
    ("gemm_tokens.hip", ["gemm_panel2_kernel", "patch_embed_kernel"]),
    # no counted hand-off here: guarded because the unrolled halo-row loops sit at 240 / 202 registers and a build that hoists their
    # read addresses out of the tile loop spills (seen twice while they were written)
    ("conv_bwd.hip", ["conv3x3_wgrad_c64_kernel", "conv3x3_wgrad_thin_kernel", "conv3x3_wgrad_c64_det_kernel", "conv3x3_wgrad_thin_det_kernel"]),
    ("branch_a_train.hip", ["bra_wgrad_kernel"]),
    # counted vmcnt between its LDS-DMA stages, asm fragment reads with counted lgkmcnt
    ("gemm_wgrad.hip", ["gemm_wgrad_wide_kernel"]),
    # the deterministic forms of the token-path reductions: no counted hand-off in these, guarded so that a DET epilogue that starts
    # to spill (a slower twin of a kernel tuned to stay under its register budget) fails the build instead of shipping
    # (the DET = true instantiations: mangled ...Lb1EEEv...; the wide kernel's is covered by its entry above)
    ("gemm_wgrad.hip", ["gemm_wgrad_kernelILi0ELi0ELb1E", "gemm_wgrad_kernelILi0ELi1ELb1E", "gemm_wgrad_kernelILi1ELi0ELb1E",
                        "gemm_wgrad_kernelILi1ELi1ELb1E", "gemm_wgrad_kernelILi1ELi2ELb1E", "colsum_kernelILb0ELb1E", "colsum_kernelILb1ELb1E"]),
    ("attention_bwd.hip", ["layernorm_bwd_kernelILi2ELb1E", "layernorm_bwd_kernelILi3ELb1E"]),
    # no counted hand-off: four register rings (7 rows of 5 moment sums, of 3 coefficient sums, of x and y) indexed by the unrolled
    # row loop; a build that indexes them dynamically puts them in scratch
    ("quality_loss.hip", ["quality_loss_bwd_kernel"]),
    # no counted hand-off: a streaming kernel at 12 B per element; scratch traffic would be a large share of what it moves
    ("grad_accumulate.hip", ["grad_accumulate_kernel"]),
    # no counted hand-off: streaming kernels at 4 B (norm pass) and 28 B (step) per element, same reasoning
    ("step_guard.hip", ["grad_sumsq_kernel", "guard_finish_kernel", "adam_guarded_kernel"]),
    # ... and the step with the weight average at 36 B per element (an entry of its own: the line above is quoted by a test)
    ("step_guard.hip", ["adam_ema_kernel"]),
    # no counted hand-off: byte work at ~15 B of memory traffic per HR pixel whose tap loops index small LDS tiles; scratch would add
    # memory traffic to a kernel that exists to remove it
    ("patch_pairs.hip", ["patch_pairs_kernel"]),
    # no counted vmcnt here, but the kernel lives on three waves per SIMD with every row's loads requested a row ahead: scratch reloads
    # queue behind those loads (seen in round 3).  All four instances (RESIZE x PARTS) sit at 133-152 registers of 168
    ("tail_stream.hip", ["tail_stream_r2_kernel"]),
    # no counted hand-off: the YUV 4:2:0 frame templates of yuv420_kernels.h, byte work at 13.5 B (NV12, image_io.hip) and 15 B (P010,
    # p010.hip) of memory traffic per pixel whose small per-lane tables (3 x 3 chroma pairs, 2 x 3 x 5 quantised codes) are indexed by
    # unrolled loops; a build that indexes them dynamically puts them in scratch
    ("image_io.hip", ["yuv420_to_f32chw_kernel", "f32chw_to_yuv420_kernel"]),
    ("p010.hip", ["yuv420_to_f32chw_kernel", "f32chw_to_yuv420_kernel"]),
    # no counted hand-off: four 8-point DCT passes hold 8 values a lane in unrolled arrays; a build that indexes them dynamically spills
    ("degrade.hip", ["degrade_lr_kernel"]),
    # ... and the launch that also knows the 4:2:0 round trip (an entry of its own: the line above is quoted by a test): the same DCT
    # passes, and staging that holds 17 loads a lane in an unrolled array
    ("degrade420.hip", ["degrade_sub_kernel"]),
    # no counted hand-off: the DCT passes hold 8 values a lane in unrolled arrays, and the coder's zigzag walk is a loop over LDS; scratch
    # would put memory traffic into the one stage that bounds the kernel
    ("jpeg_encode.hip", ["jpeg_segment_kernel", "jpeg_scan_kernel"]),
    # no counted hand-off: the one lane that walks the Huffman codes bounds the decoder, and its reader state, predictors and the IDCT's
    # 8 values a lane must stay in registers and LDS; scratch would put memory latency into every symbol
    ("jpeg_decode.hip", ["jpeg_index_kernel", "jpeg_blocks_kernel", "jpeg_finish_kernel"]),
    # no counted hand-off: 256 lanes walk the Huffman codes of their subsequences out of LDS, several times over; their reader state and
    # counts must stay in registers, scratch would put memory latency into every symbol of every lane
    ("jpeg_sync.hip", ["jpeg_sync_index_kernel"]),
    # no counted hand-off: the Huffman builder, the header's run-length coder and the byte walks index LDS arrays only; a build that moves
    # one of them into a private array puts scratch latency into the one lane the whole workgroup waits for
    ("png_encode.hip", ["png_filter_kernel", "png_block_kernel", "png_scan_kernel"]),
    # ... and the same templates (png_kernels.h) instantiated for the two-byte samples of 16-bit files
    ("png16_encode.hip", ["png_filter_kernel", "png_block_kernel"]),
    # no counted hand-off: one wave walks a zlib stream with its reader state, tables, input window and output ring in registers and LDS;
    # scratch would put memory latency into every token.  The unfilter pass carries three pixels a lane through 64-step chunks
    ("png_decode.hip", ["png_inflate_kernel", "png_finish_kernel"]),
]
# (source file, mangled-name fragment, registers): instantiations that must also stay within a register budget (VGPRs + AGPRs)
REG_BUDGET = [
    # patch_unembed's 8-wave form, __launch_bounds__(512, 1): two waves per SIMD is all its one workgroup per CU asks for, so the
    # compiler would hand it 512 registers; it must stay what the 4-wave form is, wave for wave (<= 256)
    ("gemm_tokens.hip", "gemm_panel2_kernelILi0ELi4ELi8E", 256),
    ("gemm_tokens.hip", "gemm_panel2_kernelILi1ELi4ELi8E", 256),
]
# diagnostic template instantiations, never launched by the product path: fused_qkv_attn_kernel<STAMPS = true, TGN>, blocks_stream_kernel<true>
EXEMPT = re.compile(r"fused_qkv_attn_kernel<true, \d>|fused_qkv_attn_kernelILb1ELi\d+E|blocks_stream_kernel<true>|blocks_stream_kernelILb1E")

FIELDS = {
    "sgprs": r"TotalSGPRs: (\d+)", "vgprs": r" VGPRs: (\d+)", "agprs": r"AGPRs: (\d+)",
    "scratch_bytes_per_lane": r"ScratchSize \[bytes/lane\]: (\d+)", "waves_per_simd": r"Occupancy \[waves/SIMD\]: (\d+)",
    "sgpr_spill": r"SGPRs Spill: (\d+)", "vgpr_spill": r"VGPRs Spill: (\d+)",
}


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except Exception:                       # noqa: BLE001 -- no demangler: patterns below are tried on the mangled name too
        return {n: n for n in names}


def parse(path):
    txt = open(path, errors="replace").read()
    parts = re.split(r"remark: Function Name: (\S+)", txt)
    recs = {}
    for name, body in zip(parts[1::2], parts[2::2]):
        rec = {}
        for k, pat in FIELDS.items():
            m = re.search(pat, body)
            if m:
                rec[k] = int(m.group(1))
        recs[name] = rec
    return recs


def main(argv):
    out_path = None
    files = []
    for a in argv:
        if a.startswith("--out="):
            out_path = a[6:]
        else:
            files.append(a)
    report, bad, over, seen_budget, seen_guarded = {}, [], [], set(), set()
    for f in sorted(files):
        src = os.path.basename(f).replace(".remarks", ".hip")
        recs = parse(f)
        names = demangle(list(recs))
        for mangled, rec in recs.items():
            nice = names.get(mangled, mangled)
            rec["source"] = src
            matched = {(gsrc, fn) for gsrc, fns in GUARDED for fn in fns if src == gsrc and fn in mangled}
            seen_guarded |= matched
            guarded = bool(matched) and not (EXEMPT.search(nice) or EXEMPT.search(mangled))
            rec["guarded_no_scratch"] = bool(guarded)
            report[nice] = rec
            if guarded and rec.get("scratch_bytes_per_lane", 0) > 0:
                bad.append((src, nice, rec["scratch_bytes_per_lane"]))
            for bsrc, frag, budget in REG_BUDGET:
                if src == bsrc and frag in mangled:
                    seen_budget.add(frag)
                    rec["register_budget"] = budget
                    if rec.get("vgprs", 0) + rec.get("agprs", 0) > budget:
                        over.append((src, nice, rec.get("vgprs", 0) + rec.get("agprs", 0), budget))
    try:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout
        m = re.search(r"HIP version: (\S+)", ver)
        c = re.search(r"clang version (\S+)", ver)
        compiler = {"hip_version": m.group(1) if m else None, "clang_version": c.group(1) if c else None}
    except Exception:                       # noqa: BLE001
        compiler = {"hip_version": None, "clang_version": None}
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"compiler": compiler, "kernels": report}, fh, indent=1, sort_keys=True)
    if bad:
        for src, nice, sc in bad:
            sys.stderr.write(f"check_resources: {src}: {nice} uses {sc} B/lane of scratch; its hand-counted vmcnt waits "
                             "would be wrong (scratch traffic counts on vmcnt). Reduce register pressure; do not ship this build.\n")
        return 1
    for src, nice, regs, budget in over:
        sys.stderr.write(f"check_resources: {src}: {nice} uses {regs} registers, its budget is {budget}. Do not ship this build.\n")
    srcs = {os.path.basename(f).replace(".remarks", ".hip") for f in files}
    missing = [frag for bsrc, frag, _ in REG_BUDGET if bsrc in srcs and frag not in seen_budget]
    for frag in missing:
        sys.stderr.write(f"check_resources: no kernel matches the register-budget entry {frag}; correct the entry.\n")
    stale = [(gsrc, fn) for gsrc, fns in GUARDED for fn in fns if gsrc in srcs and (gsrc, fn) not in seen_guarded]
    for gsrc, fn in stale:
        sys.stderr.write(f"check_resources: no kernel of {gsrc} matches the guarded entry {fn}; correct the entry.\n")
    if over or missing or stale:
        return 1
    n_guard = sum(1 for r in report.values() if r["guarded_no_scratch"])
    print(f"check_resources: {len(report)} kernels, {n_guard} guarded (scratch 0), compiler {compiler}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
