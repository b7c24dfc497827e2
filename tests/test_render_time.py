"""The per-decision step counters' C-ABI boundary (no GPU): dt_step_many_time,
dt_copy_time and dt_render_group are declared, exported and bound with the
header's argument lists, at the ABI version the library already had."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

NEW = ('dt_step_many_time', 'dt_copy_time', 'dt_render_group')


@pytest.fixture(scope='module')
def libpath():
    from aido1_amd import _lib
    return _lib.build()


def test_new_entry_points_are_declared_and_exported(libpath):
    from aido1_amd import _lib
    declared = _lib.exported_symbols()
    for name in NEW:
        assert name in declared, name
    nm = subprocess.run(['nm', '-D', '--defined-only', libpath], capture_output=True,
                        text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if ' T ' in line}
    for name in NEW:
        assert name in exported, name


def test_abi_version_stays_14(libpath):
    from aido1_amd import _lib
    assert _lib.ABI_VERSION == 14 and _lib.lib().dt_abi_version() == 14
    with open(os.path.join(REPO, 'include', 'dtsim.h')) as f:
        assert re.search(r'^#define DT_ABI_VERSION 14\b', f.read(), re.M)


def header_args(name):
    """(pointer arguments, int32_t arguments) of `name`'s declaration in dtsim.h."""
    with open(os.path.join(REPO, 'include', 'dtsim.h')) as f:
        src = f.read()
    m = re.search(r'^int\s+%s\s*\(([^)]*)\)\s*;' % name, src, re.M)
    assert m, name
    args = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
    ptrs = [a for a in args if '*' in a]
    ints = [a for a in args if '*' not in a]
    assert all(re.match(r'int32_t\s+\w+$', a) for a in ints), ints
    return len(ptrs), len(ints)


@pytest.mark.parametrize('name', NEW + ('dt_step_many', 'dt_copy_pose', 'dt_render3'))
def test_bound_argument_lists_match_the_header(libpath, name):
    """Every new entry point (and the three they extend, as a check of the
    check): as many void* and int32 arguments bound as the header declares, in
    a position-independent count, and an int status."""
    from aido1_amd import _lib
    fn = getattr(_lib.lib(), name)
    assert fn.restype is ctypes.c_int
    bound = (sum(a is ctypes.c_void_p for a in fn.argtypes),
             sum(a is ctypes.c_int32 for a in fn.argtypes))
    assert sum(bound) == len(fn.argtypes)
    assert bound == header_args(name), (name, bound, header_args(name))


def test_step_many_time_is_step_many_plus_one_pointer():
    assert header_args('dt_step_many_time') == (header_args('dt_step_many')[0] + 1, 1)
    assert header_args('dt_copy_time') == header_args('dt_copy_pose')


def test_a_null_handle_is_an_argument_error(libpath):
    """No device work: each new entry point refuses a NULL handle first."""
    from aido1_amd import _lib
    L = _lib.lib()
    assert L.dt_step_many_time(None, 1, None, None, None, None, None, None, None, None) == -1
    assert L.dt_copy_time(None, None, None) == -1
    assert L.dt_render_group(None, None, None, 1, None) == -1


def test_host_api_takes_time():
    """The host functions grew a `time` argument, default None (today's calls)."""
    import inspect
    from aido1_amd import render
    from aido1_amd.vec_env import VecEnv
    fns = [render.render_into, render.bind_render, render.render_group_into,
           render.bind_render_group, render.render2_into, render.bind_render2,
           VecEnv.step_many_into, VecEnv.bind_step_many, VecEnv.copy_pose,
           VecEnv.bind_copy_pose, VecEnv.render_into]
    for fn in fns:
        p = inspect.signature(fn).parameters
        assert 'time' in p and p['time'].default is None, fn.__qualname__
