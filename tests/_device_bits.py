"""What the GPU tests of the policy, the population, the evolution strategy and the observation statistics share: a device array
brought to the host, equality of bits, and the C consumers of tests/c_abi built against the library under test.  TEST CODE."""
import ctypes
import os
import subprocess

import numpy as np

from basilisk_env_amd import _hip, _lib


def download(ptr, dtype, count):
    out = np.empty(count, dtype=dtype)
    _hip.check(_hip.runtime().hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), out.nbytes, _hip.hipMemcpyDeviceToHost), "hipMemcpy")
    return out


def bits(a):
    """a float array as integers: equality of bits, NaN payloads and signed zeros included"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def build_c_consumer(tmp_path, name):
    """tests/c_abi/<name>.c compiled as plain C99 with warnings as errors and linked against the library under test -> the
    executable's path"""
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / name
    libdir = os.path.dirname(_lib.lib_path())
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.join(root_dir, "include"),
                           os.path.join(root_dir, "tests", "c_abi", name + ".c"), "-L", libdir, "-lbskgpu", "-L", rocm,
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + rocm, "-o", str(exe)])
    return exe
