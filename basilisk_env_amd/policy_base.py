"""What every ctypes binding of the policy subsystem is built on (``policy.py``: the policy, the population, the evolution strategy,
the observation statistics; ``policy_fit.py``: the fit): a handle of the library on one GPU - create, close, the closed-handle
refusal, ``sync``, use as a context manager - and the host block an argument is turned into.  A module of its own so that both
files import it and neither imports the other first."""
import ctypes as C
import sys

import numpy as np

from . import _hip, _lib
from ._lib import check
from .policy_spec import c_spec


def _host_block(values, n, dtype=np.float32, rows=0, what="parameters"):
    """Host values -> a contiguous ``dtype`` array: ``n`` elements flattened (``rows=0``), or blocks of ``n`` as the rows of a 2-D
    array - exactly ``rows`` of them, any number from one on with ``rows=None``.  Anything else is a ``ValueError``."""
    p = np.ascontiguousarray(values, dtype=dtype)
    if rows == 0:
        p = p.reshape(-1)
        if p.size != n:
            raise ValueError("expected %d %s, got %d" % (n, what, p.size))
    elif p.ndim != 2 or p.shape[1] != n or p.shape[0] < 1 or (rows is not None and p.shape[0] != rows):
        raise ValueError("expected %s of shape (%s, %d), got %r" % (what, "P" if rows is None else rows, n, p.shape))
    return p


class _DeviceObject(object):
    """A handle of the library on one GPU, made by ``bsk_<_kind>_create(spec, ..., device, &handle)`` (an object without a
    ``spec``: without that argument).  ``_out`` holds the
    ``_hip.DeviceBuffer``s the object owns, by name (None: none yet), ``_source`` the device array a queued launch still reads,
    ``_stats`` the ``ObsStats`` attached to it."""
    _kind = None              # policy / population / es / obs_stats: the C functions are bsk_<_kind>_*
    _what = None              # what the object is called in a message

    def _c(self, name):
        return getattr(self._lib, "bsk_%s_%s" % (self._kind, name))

    def _create(self, device, *args):
        self._lib = _lib.load()
        self.device = int(device)
        h = C.c_void_p()
        if getattr(self, "spec", None) is not None:
            self._cs = c_spec(self.spec)
            args = (C.byref(self._cs),) + args
        check(self._c("create")(*args, self.device, C.byref(h)))
        self._p = h
        self._out = self._source = None

    def close(self):
        if getattr(self, "_p", None):
            self._c("destroy")(self._p)
            self._p = None
        for b in (getattr(self, "_out", None) or {}).values():
            b.free()
        self._out = self._source = self._stats = self._outcomes = None

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _handle(self):
        if not self._p:
            raise RuntimeError("%s is closed" % self._what)
        return self._p

    def sync(self):
        """Waits for everything queued on the object's device (it keeps no stream of its own)."""
        with _hip.device_guard(self.device):
            _hip.check(_hip.runtime().hipDeviceSynchronize(), "hipDeviceSynchronize")

    def _device_pointer(self, src, itemsize, refuse):
        """``src``: a raw device pointer - returned as it is, with no element count - or anything with
        ``__cuda_array_interface__``, read into typestr, shape, element count and whether its strides (where it gives any) are those
        of a dense array of ``itemsize``-byte elements.  ``refuse(typestr, shape, size, dense)`` -> the text of the ``ValueError`` or
        None; an array it lets pass is kept alive in ``_source``, for the launch reads it after the call has returned.
        -> (pointer, element count or None)"""
        cai = getattr(src, "__cuda_array_interface__", None)
        if cai is None:
            return src, None
        shape, strides = tuple(cai["shape"]), cai.get("strides")
        size = int(np.prod(shape)) if len(shape) else 1
        dense = tuple(itemsize * int(np.prod(shape[k + 1:], dtype=np.int64)) for k in range(len(shape)))
        dense = strides is None or tuple(strides) == dense
        why = refuse(cai["typestr"], cai["shape"], size, dense)
        if why:
            raise ValueError(why)
        self._source = src
        return cai["data"][0], size
