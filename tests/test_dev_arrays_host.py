"""csrc/dev_arrays.h, the owner of every plan's device arrays, without a GPU.
tests/c_host/dev_arrays_host.cpp defines the header's three seam functions over malloc
(with a table of live pointers and switches that fail the k-th malloc or the k-th copy)
and checks inside the program: a mixed alloc / upload / adopt / release sequence frees
everything exactly once at scope exit, also with a failure at every position; upload
frees its own array when the copy fails; take and move construction move every pointer;
n == 0 gives a one-element array; release(nullptr) does nothing.  The program is an
ordinary executable built with the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, REPO

SRC = os.path.join(REPO, 'tests', 'c_host', 'dev_arrays_host.cpp')
ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')


def _compiler():
    for cxx in ('g++', 'clang++', os.path.join(ROCM, 'llvm', 'bin', 'clang++')):
        path = shutil.which(cxx)
        if path:
            return path
    pytest.skip('cannot build the C++ host here: no g++ or clang++')


def test_dev_arrays_own_and_free_on_every_path(tmp_path):
    exe = str(tmp_path / 'dev_arrays_host')
    # (-static-libasan: the sanitizer's runtime is part of the program, so the run does not
    # depend on the order in which the loader brings in shared libraries)
    cmd = [_compiler(), '-std=c++17', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=undefined', '-static-libasan', '-I' + os.path.join(PKG, 'csrc'), SRC, '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and 'dev_arrays_host ok' in res.stdout, res.stdout + res.stderr
