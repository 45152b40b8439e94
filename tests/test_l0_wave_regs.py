"""smooth_grad_lean_wave is built for five wavefronts per SIMD (KLT_L0_WAVE_PER_SIMD): its four instantiations fit 96 VGPRs without
scratch, from a fresh device-only compile (tools/kernel_regs.py; hipcc cross-compiles gfx950 without a GPU)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# instantiations that profiles/README.md records as left at four wavefronts per SIMD (<= 104 VGPRs): none
KEPT_AT_FOUR = ()


def test_wave_kernels_fit_five_wavefronts_per_simd():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_regs
    regs = kernel_regs.kernel_regs("pyramid_kernels.hip", "smooth_grad_lean_wave")
    assert len(regs) == 4, sorted(regs)
    assert sorted(n.split("smooth_grad_lean_wave")[1][:7] for n in regs) == ["IfLi5EE", "IfLi9EE", "IhLi5EE", "IhLi9EE"], sorted(regs)
    for n, r in sorted(regs.items()):
        print(n, r)
        assert r["scratch"] == 0, (n, r)
        assert r["vgpr"] <= (104 if any(k in n for k in KEPT_AT_FOUR) else 96), (n, r)
