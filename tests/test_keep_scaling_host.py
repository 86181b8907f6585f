"""CPU: what of mpcqp_update_matrices / setKeepScaling can be checked without a GPU -- the entry is declared, exported and bound, the facades carry the
switch (off by default), the C++ program of tests/test_gpu_update_matrices.py builds against cpp/CuCaQP.hpp, and the kernel's translation unit is in the library."""
import ctypes as C
import os
import re
import subprocess

from optimal_control_problem_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "support", "cucaqp_keep_scaling_test")


def test_entry_point_is_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    decl = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mpcqp_update_matrices\(([^;]*)\);", hdr, re.S)
    assert decl, "mpcqp_update_matrices is not declared"
    assert "CuCaQP.cpp:106-116,129-140" in decl.group(1) and "MPCQP_ERR_LIMIT" in decl.group(1) and "MPCQP_ERR_STATE" in decl.group(1)
    args = lambda name: re.sub(r"\s+", " ", re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1))
    assert args("mpcqp_update_matrices") == args("mpcqp_update")          # the same signature
    assert "mpcqp_update_matrices" in _lib.EXPORTS
    L = _lib.lib()
    assert L.mpcqp_update_matrices.argtypes == L.mpcqp_update.argtypes
    assert L.mpcqp_update_matrices(None, None, 0, None, 0, None, 0, None, 0, None, 0, 0) == _lib.ERR_ARG      # null handle


def test_facades_carry_the_switch_off_by_default():
    from optimal_control_problem_amd.batch_qp import BatchQP
    from optimal_control_problem_amd.cucaqp import CuCaQP
    assert callable(BatchQP.update_matrices)
    qp = CuCaQP()
    assert qp._keep_scaling is False
    qp.setKeepScaling(True)
    assert qp._keep_scaling is True
    for name in ("CuCaQP.hpp", "StageSQP.hpp"):
        src = open(os.path.join(ROOT, "optimal_control_problem_amd", "cpp", name)).read()
        assert "void setKeepScaling(bool" in src and "keepScaling_ = false" in src and "mpcqp_update_matrices(" in src, name


def test_cpp_program_builds_and_refuses_without_a_system(built):
    """(no file argument: the facade, with the switch on, refuses a solve() before initSolver() like the reference, CuCaQP.cpp:200-203)"""
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr)
    assert "not initialized" in r.stderr


def test_library_holds_the_rescale_kernels(built):
    """both instances' kernel names are in the library's gfx950 code object (the symbol names of the device functions are kept as strings in the fat binary)"""
    blob = open(_lib.SO_PATH, "rb").read()
    assert blob.count(b"mpcqp_oc_rescale_kernelILi4ELb1EE") > 0 and blob.count(b"mpcqp_oc_rescale_kernelILi4ELb0EE") > 0
    assert C.CDLL(_lib.SO_PATH) is not None
