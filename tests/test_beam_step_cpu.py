"""mvlt_beam_step without a GPU: the built library exports it, the ctypes mirror of its parameter struct has the size the library
was compiled with, the ABI constants agree at 16; and the host driver of tests/beam_step_ref.py (what the GPU tests compare the
kernel with) gives the result worked out by hand for a three-step stream, and its streams cover what they are there for."""
import ctypes
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_step_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_beam_step():
    from mvlt_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mvlt_beam_step")
    assert "mvlt_beam_step" in _lib.SYMBOLS


def test_beam_step_struct_size_matches_the_mirror():
    from mvlt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    sid = int(re.search(r"MVLT_STRUCT_BEAM_STEP\s*=\s*(\d+)", hdr).group(1))
    assert _lib.STRUCTS[sid] is _lib.MvltBeamStep
    assert _lib.lib().mvlt_sizeof(sid) == ctypes.sizeof(_lib.MvltBeamStep) > 0


def test_abi_constants_agree_at_16():
    from mvlt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip.h")).read()
    macro = int(re.search(r"#define\s+MVLT_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert macro == _lib.ABI_VERSION == _lib.lib().mvlt_version() == 17


def test_driver_on_a_hand_written_stream():
    """num_beams 2, one sample, max_length 4.  Step 0: [END] at rank 1 -> the hypothesis [MASK] at -2 / 1.  Step 1: [END] at rank 1
    from row 1 ([6]) at -2 / 1: the pool is full, worst -2.  Step 2: [END] at rank 0 from row 1 ([5, 4]) at -2 / 2 = -1 beats worst
    and evicts the tied entry inserted first ([MASK]); [END] at rank 2 is skipped.  finalize offers [5, 8, 2] at -2.5 / 3 (taken,
    evicts [6]) and [5, 4, 1] at -7 / 3 (refused): the best hypothesis is [5, 8, 2], closed with [END]."""
    from mvlt_amd.decode import BeamScorer
    E = R.EOS
    stream = [
        ([[-1.0, -2.0, -3.0, -4.0]], [[0, 0, 0, 0]], [[5, E, 6, 9]]),
        ([[-1.5, -2.0, -3.5, -4.5]], [[0, 1, 0, 1]], [[8, E, 4, 9]]),
        ([[-2.0, -2.5, -6.0, -7.0]], [[1, 0, 0, 1]], [[E, 2, E, 1]]),
    ]
    res = R.drive(BeamScorer, stream, 1, 2, 4, E)
    assert res["steps"][0][:3] == ([-1.0, -3.0], [5, 6], [0, 0])
    assert res["steps"][1][:3] == ([-1.5, -3.5], [8, 4], [0, 0])
    assert res["steps"][2][:3] == ([-2.5, -7.0], [2, 1], [0, 1])
    assert [st[3] for st in res["steps"]] == [[False]] * 3
    assert res["pools"] == [[(-2.0, [6]), (-1.0, [5, 4])]] and res["worst"] == [-2.0]
    assert res["seqs"] == [[5, 8, 2], [5, 4, 1]]
    assert res["final"] == [[5, 8, 2, E]]


def test_streams_cover_what_they_are_for():
    from mvlt_amd.decode import BeamScorer
    R.coverage(BeamScorer)
    shapes = {(len(plans), nb, ml) for _, plans, nb, ml, _, _ in R.cases()}
    assert {g for g, _, _ in shapes} == {1, 3} and {nb for _, nb, _ in shapes} == {1, 2, 5, 8} and {ml for _, _, ml in shapes} == {4, 12}
