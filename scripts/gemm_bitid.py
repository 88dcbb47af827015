#!/usr/bin/env python3
"""Bit identity of two builds of libmvlt_hip.so on the GEMM routes: did a refactor change a single output bit?

    python scripts/gemm_bitid.py --lib old/libmvlt_hip.so > old.txt
    python scripts/gemm_bitid.py                          > new.txt          (the package's own library)
    diff old.txt new.txt

Runs the rows of the route table of tests/test_gemm_routes_gpu.py and of the 8-wave and grouped tables of
tests/test_gemm_engines_gpu.py through the tests' own code (same seeds, same buffers, route assertions included) and prints
one line per checked buffer -- output, saved pre-activation, column sums / bias gradients -- with the sha256 of its bytes;
the per-element bound is checked as in the tests.  The atomic k-slice rows are left out: their addition order is not fixed.
One process per library (it is loaded once); run both on the same machine.
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


class Env:
    """the part of pytest's monkeypatch the tests use (nothing to undo: the process ends with the table)"""
    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=True):
        os.environ.pop(k, None)


class Request:
    class node:
        name = ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="library to load instead of the package's own")
    args = ap.parse_args()
    import torch
    from mvlt_amd import _lib, ops
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    _lib.lib()
    import gemm_ref
    import test_gemm_engines_gpu as E
    import test_gemm_routes_gpu as T

    row, count = [""], [0]
    real_check = gemm_ref.check_bound

    def hashing_check(out, ref, bound, what="", heads=None):
        data = out.detach().contiguous().cpu()
        digest = hashlib.sha256(data.view(-1).view(dtype=torch.uint8).numpy().tobytes()).hexdigest()
        print(f"{row[0]} | {what} | {tuple(data.shape)} | {digest}", flush=True)
        count[0] += 1
        real_check(out, ref, bound, what, heads)

    T.check_bound = E.check_bound = hashing_check
    T._note = E._note = lambda *a, **k: None
    env, req = Env(), Request()
    for prm in T.ROUTES:
        row[0] = "routes::" + prm.id
        T.test_gemm_route(ops, prm.values[0], req)
    for prm in E.G8_ROWS:
        row[0] = "gemm8::" + prm.id
        E.test_gemm8_route(_lib, ops, env, req, prm.values[0])
    for prm in E.GROUP_ROWS:
        if prm.values[0]["want"][0] == "GROUP_ATOMIC":
            continue
        row[0] = "group::" + prm.id
        E.test_gemm_group_route(_lib, ops, env, req, prm.values[0])
    print(f"# {count[0]} buffers", flush=True)


if __name__ == "__main__":
    main()
