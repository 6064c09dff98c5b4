"""CPU-side checks of the GEMM launch tables (csrc/gemm_forms.h): which kernel instantiations exist, how operands select one, and
that a call whose operands select none is refused before anything is launched."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT


def test_form_tables_and_operand_mapping(tmp_path):
    """tests/gemm_forms_check.cpp: the 28 instantiations of gemm_nt_g3_kernel, every combination of operands against them (host
    program with its own main, under the address and undefined-behaviour sanitizers)."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'gemm_forms_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                    os.path.join(ROOT, 'tests', 'gemm_forms_check.cpp')], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert '28 forms reached, 0 failures' in run.stdout, run.stdout


def test_p4_a_operand_with_a_form_that_has_no_instantiation_is_refused():
    """vqcpc_gemm_nt_g3_pl with a pre-split A and add + add2, or add2 == C: no gemm_nt_g3_kernel<.., PL = 3> of these forms exists,
    so the call is refused with a message (it used to launch PL = 2, which reads the P4 image of A as fp32).  Dummy addresses,
    never dereferenced: host-only, as test_abi.py::test_argument_validation_without_gpu."""
    if torch.cuda.is_available():
        pytest.skip('host-only: a missing refusal must not become a launch on dummy addresses')
    from vqcpc_bach_amd import build, hip
    if not os.path.exists(hip.LIB_PATH):
        build.build(verbose=False)
    lib = hip.load()
    p = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # 16-byte aligned
    a, b, c, add, add2, st, amax_a, amax_b = p
    M = N = 256
    K = 32
    for add2_ in (add2, c):                                            # add + add2; add2 == C (same leading dimension)
        rc = lib.vqcpc_gemm_nt_g3_pl(a, K, b, K, c, N, M, N, K, None, 0, 0.0, 0, add, N, add2_, N, None, 1.0, None, st, amax_a, amax_b,
                                     None)
        assert rc != 0 and b'gemm_nt_g3_pl' in lib.vqcpc_last_error(), (rc, lib.vqcpc_last_error())
