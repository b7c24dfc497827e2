"""The handle's host-side table code on a CPU: tests/host_tables_main.cc drives
csrc/dtrecords.h (every refusal of the five record uploads, whole texts) and
csrc/dtdevbuf.h (the two upload rules, each HIP call failing in turn) over
stand-ins for the HIP calls, built with AddressSanitizer + UBSan and linked
against no HIP library.  Run as a child process: a failed check, a sanitizer
report or a leaked allocation is a non-zero exit status."""
import os
import re
import subprocess

import pytest

from conftest import REPO


def _clangxx():
    with open(os.path.join(REPO, 'Makefile')) as f:
        return re.search(r'^CLANG \?= (\S+)', f.read(), re.M).group(1) + '++'


def test_records_and_device_buffers_under_asan_and_ubsan(tmp_path):
    cxx = _clangxx()
    if not os.path.exists(cxx):
        pytest.skip('no ' + cxx)
    exe = str(tmp_path / 'host_tables')
    r = subprocess.run([cxx, '-std=c++17', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include',
                        '-Iinclude', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-g', '-O1',
                        os.path.join('tests', 'host_tables_main.cc'), '-o', exe],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-6000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
