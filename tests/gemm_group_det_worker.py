"""Child process of tests/test_gemm_engines_gpu.py::test_gemm_group_deterministic_child.  MVLT_DETERMINISTIC=1 (read once
per process by the library, set by the parent) forbids the atomic k-slices; a group with few tiles and a long reduction
must then run on the 8-wave engine, cut into slices that meet through slabs: twice the same bits, inside the bound."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert os.environ.get("MVLT_DETERMINISTIC") == "1"
    import mvlt_amd  # noqa: F401
    from mvlt_amd import _lib as L, ops
    import test_gemm_engines_gpu as T

    class Req:          # what Group.run_and_check needs of a pytest request
        class node:
            name = "deterministic-child"
    L.lib()
    g = T.Group(L, ops, torch.bfloat16, T.SMALL, 4000 - 24, no_colsum=(1,))
    name, slices = g.route()
    print(f"route {name} x {slices}")
    assert name.startswith("GROUP_G8_") and slices > 1, (name, slices)
    g.run_and_check(Req)
    first = [(it[4].clone(), None if it[5] is None else it[5].clone()) for it in g.items]
    for it in g.items:          # the second run starts from NaN again
        it[4].fill_(float("nan"))
        if it[5] is not None:
            it[5].fill_(float("nan"))
    g.launch()
    for (dw, cs), it in zip(first, g.items):
        assert torch.equal(dw[:-1, :it[3].shape[1]], it[4][:-1, :it[3].shape[1]]), "dW differs between two runs"
        assert cs is None or torch.equal(cs[:-1], it[5][:-1]), "bias gradient differs between two runs"
    # the atomic form must be unreachable in this process, whatever MVLT_G8 says
    os.environ["MVLT_G8"] = "0"
    name0, slices0 = T.Group(L, ops, torch.bfloat16, T.SMALL, 2100).route()
    assert name0 != "GROUP_ATOMIC" and slices0 == 1, (name0, slices0)
    print("DETERMINISTIC-GROUP-OK")


if __name__ == "__main__":
    main()
