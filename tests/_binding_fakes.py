"""The fakes behind the binding pins (tests/test_policy_binding_host.py, tests/test_fit_binding_host.py): a C library, a HIP runtime
and a device allocator that record every call with its arguments and return 0.  Scalars are recorded as values; a pointer as None,
as the name of what it points to where a fake handed it out (a handle, a device buffer, a stream: "buf#7" in one call and in a later
one is the same buffer), as the element type, count and CRC-32 of the host array it has to point to where the ABI fixes that, and as
"ptr" otherwise.  With ``Recorder(offsets=True)`` an address inside something a fake handed out is recorded as "buf#3+5120"."""
import ctypes as C
import types
import zlib

import numpy as np

# per C function, what each argument is: v a scalar; p a pointer; s the policy spec; S a BskFitSchedule by reference; o an
# out-parameter the fake fills; F / G / T host float32 of n_params / P * n_params / n_params elements read by the call; D / B host
# float64 of n_params / 2 elements read by the call; f / d / b host float32 n_params / float64 n_params / float64 2 the call fills;
# w host uint64 8 the call fills
KINDS = {
    "bsk_policy_create": "sFvo", "bsk_policy_set_params": "pF", "bsk_policy_destroy": "p", "bsk_policy_set_rng": "pvv",
    "bsk_policy_get_rng": "poo", "bsk_policy_act": "ppvvvvppppvp", "bsk_policy_rollout": "ppvvvpppppp",
    "bsk_population_create": "svGvo", "bsk_population_destroy": "p", "bsk_population_set_rng": "pvv", "bsk_population_get_rng": "poo",
    "bsk_population_set_params": "pG", "bsk_population_set_params_device": "ppvvp", "bsk_population_get_member": "pvf",
    "bsk_population_act": "ppvvvvvppppvp", "bsk_population_rollout": "ppvvvvpppppppppp",
    "bsk_es_create": "svFvvvvvo", "bsk_es_destroy": "p", "bsk_es_ask": "ppp", "bsk_es_tell": "ppp", "bsk_es_get_state": "pdo",
    "bsk_es_set_state": "pDv", "bsk_es_generation_device": "po", "bsk_es_set_optimizer": "pvvvvv", "bsk_es_get_moments": "pddb",
    "bsk_es_set_moments": "pDDB",
    "hipGetDevice": "o", "hipSetDevice": "v", "hipDeviceSynchronize": "", "hipMemcpyAsync": "ppvvp",
    # the fit, the free functions of the policy-gradient loop, and what the loop asks of the policy and the statistics
    "bsk_fit_create": "pvvvvvvo", "bsk_fit_destroy": "p", "bsk_fit_accumulate": "ppvvppppvp", "bsk_fit_accumulate_pg": "ppvvpppvvpppvp",
    "bsk_fit_accumulate_ppo": "ppvvpppvvppvppvpp", "bsk_fit_step": "pp", "bsk_fit_apply_obs_norm": "ppvp", "bsk_fit_stats_device": "po",
    "bsk_fit_pg_stats_device": "po", "bsk_fit_vclip_stats_device": "po", "bsk_fit_grad_norm_device": "po",
    "bsk_fit_schedule_device": "po", "bsk_fit_get_state": "pdddbo", "bsk_fit_set_state": "pDDDBv", "bsk_fit_set_lr": "pv",
    "bsk_fit_set_max_grad_norm": "pv", "bsk_fit_set_schedule": "pS", "bsk_fit_schedule_begin": "pp", "bsk_fit_kl_gate": "ppvp",
    "bsk_fit_schedule_end": "ppvp", "bsk_fit_get_schedule_state": "pw", "bsk_fit_set_schedule_state": "pv",
    "bsk_gae": "ppppvvvvvppp", "bsk_adv_normalize": "ppvvvvppp", "bsk_reward_norm": "ppvvvvvvvppppp",
    "bsk_pg_gather": "pvvvvvpppppppvppppppp", "bsk_pg_shuffle_advance": "pp", "bsk_pg_episodes": "pppppvvvppppvpp",
    "bsk_pg_log_update": "pvpvpvpp", "bsk_pg_log_advance": "pvpp",
    "bsk_policy_value": "ppvvpp", "bsk_policy_set_obs_stats": "pp", "bsk_obs_stats_create": "vvo", "bsk_obs_stats_destroy": "p",
    "hipMemsetAsync": "pvvp", "hipMemcpy": "ppvv", "hipMemcpy2DAsync": "pvpvvvvp",
}
OUT = {"bsk_policy_get_rng": (11, 22), "bsk_population_get_rng": (33, 44), "bsk_es_get_state": (55,), "hipGetDevice": (0,),
       "bsk_fit_get_state": (66,)}
HOST = {"F": (np.float32, "np"), "G": (np.float32, "Pnp"), "D": (np.float64, "np"), "B": (np.float64, 2),
        "f": (np.float32, "np"), "d": (np.float64, "np"), "b": (np.float64, 2), "w": (np.uint64, 8)}
BASE, APART = 0x7000000000, 0x100000           # the fake addresses: where they start and how far apart they are
D2H, H2D = 2, 1                                # hipMemcpyDeviceToHost, hipMemcpyHostToDevice


def _out_name(name):
    """what the pointer an out-parameter of ``name`` receives is called"""
    if name.endswith("generation_device"):
        return "generation"
    if name.startswith("bsk_fit_") and name.endswith("_device"):
        return name[len("bsk_"):-len("_device")]
    return "obs_stats" if name.startswith("bsk_obs_stats") else name.split("_")[1]


class Recorder(object):
    """The log, the names of the pointers the fakes hand out, and the fakes themselves."""

    def __init__(self, offsets=False):
        self.log, self.errors, self.names, self.count, self.sizes = [], [], {}, {}, {}
        self.offsets = offsets
        self.fail_next = None                      # name of the C function whose next call returns BSK_EINVAL
        self.lib, self.rt = types.SimpleNamespace(), types.SimpleNamespace()
        for name, kinds in KINDS.items():
            setattr(self.rt if name.startswith("hip") else self.lib, name, self._function(name, kinds))
        self.lib.bsk_last_error = lambda: b"fake"
        rec = self

        class DeviceBuffer(object):
            def __init__(self, nbytes, device):
                self.ptr, self.nbytes, self.device = rec.pointer("buf"), int(nbytes), int(device)
                self.name = rec.names[self.ptr]
                rec.log.append(["DeviceBuffer", self.name, nbytes, device])

            def free(self):
                if self.ptr:
                    rec.log.append(["DeviceBuffer.free", self.name])
                    self.ptr = None
        self.DeviceBuffer = DeviceBuffer

    def pointer(self, what):
        """a new fake address, known by the name what#k from here on"""
        self.count[what] = k = self.count.get(what, 0) + 1
        addr = BASE + APART * len(self.names)
        self.names[addr] = "%s#%d" % (what, k)
        return addr

    def name_of(self, a):
        if isinstance(a, C.c_void_p):
            a = a.value
        if hasattr(a, "_obj"):                     # (byref)
            a = C.addressof(a._obj)
        if not a:
            return None
        a = int(a)
        base = a - (a - BASE) % APART
        if self.offsets and a != base and base in self.names:
            return "%s+%d" % (self.names[base], a - base)
        return self.names.get(a, "ptr")

    def _host(self, kind, addr, fill):
        dt, count = HOST[kind]
        count = self.sizes.get(count, count)
        arr = np.ctypeslib.as_array((C.c_byte * (count * np.dtype(dt).itemsize)).from_address(addr)).view(dt)
        if fill:
            arr[:] = np.arange(count) * 0.5 + 1.0
            return "%s[%d] filled" % (np.dtype(dt).str, count)
        return "%s[%d] crc %08x" % (np.dtype(dt).str, count, zlib.crc32(arr.tobytes()))

    def _copy(self, name, args, row):
        """a copy between the host and the device: what goes up is recorded by its CRC-32, what comes down is zeros"""
        addr = lambda a: a.value if isinstance(a, C.c_void_p) else a      # noqa: E731
        if name == "hipMemcpy" and args[3] == H2D:
            row[1] = "host crc %08x" % zlib.crc32(C.string_at(addr(args[1]), args[2]))
        elif name in ("hipMemcpy", "hipMemcpyAsync") and args[3] == D2H and row[0] == "ptr":
            C.memset(addr(args[0]), 0, args[2])

    def _function(self, name, kinds):
        def call(*args):
            assert len(args) == len(kinds), (name, len(args))
            row, outs = [], list(OUT.get(name, ()))
            for kind, a in zip(kinds, args):
                if kind == "v":
                    assert isinstance(a, (int, float)), (name, a)
                    row.append(a)
                elif kind == "p":
                    row.append(self.name_of(a))
                elif kind == "s":
                    s = a._obj
                    row.append(["spec", s.abi_version, s.struct_size, s.n_hidden, list(s.hidden), s.activation, s.has_value, s.v_n_hidden,
                                list(s.v_hidden), s.v_activation])
                elif kind == "S":
                    s = a if a is None else a._obj
                    row.append(s and ["schedule", list(s.lr), list(s.clip), list(s.clip_vf), list(s.ent_coef), s.total, s.kl_stop])
                elif kind == "o":
                    if a is None:
                        row.append(None)
                        continue
                    a._obj.value = outs.pop(0) if outs else self.pointer(_out_name(name))
                    row.append("out")
                else:
                    addr = a.value if isinstance(a, C.c_void_p) else a
                    row.append(None if not addr else self._host(kind, int(addr), kind in "fdbw"))
            self._copy(name, args, row)
            self.log.append([name] + row)
            if self.fail_next == name:
                self.fail_next = None
                return -1
            return 0
        return call

    def note(self, *what):
        self.log.append(["--"] + list(what))

    def raises(self, fn, *args, **kw):
        try:
            fn(*args, **kw)
        except Exception as e:      # noqa: BLE001 - the type is what gets recorded
            self.errors.append([type(e).__name__, str(e)])
            self.log.append(["raised", type(e).__name__, str(e)])
        else:
            raise AssertionError("nothing raised")


class FakeArray(object):
    def __init__(self, ptr, shape, typestr, strides=None, with_strides=True):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}
        if with_strides:
            self.__cuda_array_interface__["strides"] = strides


class FakePropagator(object):
    def __init__(self, rec, n_envs, device, env_base=None):
        self.rec, self.n_envs, self.device = rec, n_envs, device
        if env_base is not None:
            self.env_base = env_base
        self._h, self._stream, self._obs = rec.pointer("prop"), rec.pointer("stream"), rec.pointer("obs")

    def device_views(self):
        return {"obs": FakeArray(self._obs, (5, self.n_envs), "<f8"), "stride": self.n_envs + 64}

    def stream_ptr(self):
        return self._stream

    def _handle(self):
        return C.c_void_p(self._h)

    def sync(self):
        self.rec.log.append(["prop.sync", self.rec.names[self._h]])

    def reset_from_pool_shared(self, envs_per_member, epoch):
        self.rec.log.append(["prop.reset_from_pool_shared", envs_per_member, self.rec.name_of(epoch)])

    def reset_from_pool_device(self, slots):
        self.rec.log.append(["prop.reset_from_pool_device", slots])


def _block(n, dtype=np.float32, at=0.0):
    return (np.arange(n) * 0.25 + at).astype(dtype)
