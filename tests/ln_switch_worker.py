"""Child process of tests/test_ln_routes_gpu.py::test_switch_child.  MVLT_LN_BWD2 and MVLT_LN_BWD2_PF are read once per
process by the library; the parent sets exactly one of them.  MVLT_LN_BWD2=0: every backward takes the general kernel in
8-wave blocks (4 at C = 2048, where the LDS clamp halves them) and dy_parts is refused.  MVLT_LN_BWD2_PF=1: the
low-footprint kernel keeps two row groups in flight for NV <= 3; the row counts give its waves 1, 2 and 3 passes, so
both exits of its loop are taken.  Either way: the bf16 backward cases of the parent file, same reference, same bound."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    off = os.environ.get("MVLT_LN_BWD2") == "0"
    pf = os.environ.get("MVLT_LN_BWD2_PF") == "1"
    assert off != pf, "the parent sets exactly one of MVLT_LN_BWD2=0 / MVLT_LN_BWD2_PF=1"
    import mvlt_amd  # noqa: F401
    from mvlt_amd import _lib as L, ops
    import test_ln_routes_gpu as T
    L.lib()
    label = "MVLT_LN_BWD2=0" if off else "MVLT_LN_BWD2_PF=1"
    if off:
        # 8-wave blocks: twice the rows per block, so half the partial rows (4 waves once the LDS clamp bites)
        assert L.lib().mvlt_layernorm_bwd_nparts(64, 768) == 8 and L.lib().mvlt_layernorm_bwd_nparts(64, 2048) == 16
    else:
        assert L.lib().mvlt_layernorm_bwd_nparts(64, 768) == 16
    T.bf16_backward_cases(L, ops, label, parts=not off)
    if off:
        import torch
        T.test_backward_parts_refused(L, ops, 384, torch.bfloat16)
    T.report()
    assert T.WORST and all(v <= 1.0 for v in T.WORST.values())
    print("LN-SWITCH-OK")


if __name__ == "__main__":
    main()
