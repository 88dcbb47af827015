"""Child process of tests/test_param_groups_gpu.py::test_grid_does_not_matter.  MVLT_ADAMW_BLOCKS is read once per process by the
library; the parent sets it to 3, so n = 524288 + 64 takes 171 trips of the grid-stride loop.  The same three steps as the parent
runs on the default grid; the results go to the file named on the command line."""
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
    import test_param_groups_gpu as T
    torch.save(T.grid_run(ops), sys.argv[1])
    print("ADAMW-GROUPS-GRID-OK")


if __name__ == "__main__":
    main()
