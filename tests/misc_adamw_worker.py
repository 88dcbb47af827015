"""Child process of tests/test_misc_routes_gpu.py::test_adamw_grid_does_not_matter.  MVLT_ADAMW_BLOCKS is read once per
process by the library; the parent sets it to 3, so n = 10007 (2501 vectors and a tail of three) takes four trips of the
grid-stride loop.  The same three checked steps as the parent runs on the default grid; the results go to the file named
on the command line."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert os.environ.get("MVLT_ADAMW_BLOCKS") == "3", "the parent sets MVLT_ADAMW_BLOCKS=3"
    import torch
    import mvlt_amd  # noqa: F401
    from mvlt_amd import ops
    import test_misc_routes_gpu as T
    torch.save(T.adamw_grid_run(ops), sys.argv[1])
    assert T.WORST and all(v <= 1.0 for v in T.WORST.values())
    print("ADAMW-GRID-OK")


if __name__ == "__main__":
    main()
