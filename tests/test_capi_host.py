"""CPU: what the translation units of the C-ABI share (csrc/bsk_capi.hpp) as far as a machine without a GPU can reach it - the
admission of a device, written once (csrc/bsk_capi.hip: open_device) behind everything the library creates on one."""
import pytest

from basilisk_env_amd import _hip
from helpers import create_each


def test_every_create_refuses_alike_without_a_device():
    """With valid arguments otherwise, all four create entry points end in the same admission: BSK_ENODEV, *out left NULL, one
    text - and the text is bsk_last_error's, whichever translation unit's entry point wrote it."""
    if _hip.device_count() > 0:
        pytest.skip("a HIP device is visible (tests/test_gpu_policy.py holds the four calls to a device_id past the last one)")
    got = create_each(0, hidden=(16,), n_members=2, n_envs=64)
    assert [name for name, _, _, _ in got] == ["bsk_create", "bsk_policy_create", "bsk_population_create", "bsk_es_create"]
    for name, rc, out, text in got:
        assert rc == -2 and out is None                    # BSK_ENODEV, (name, rc, out, text)
    assert len({text for _, _, _, text in got}) == 1 and got[0][3] == "no HIP device visible: libbskgpu has no CPU fallback", got
